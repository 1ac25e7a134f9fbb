"""ctypes binding of libalpharat_hip.so (include/alpharat_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950). There is no CPU
fallback: if the library is missing, or no HIP device is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import os

PKG = Path(__file__).resolve().parent
# AR_LIB: another build of the same library (A/B measurements of two builds); never a different backend
LIB_PATH = Path(os.environ["AR_LIB"]) if os.environ.get("AR_LIB") else PKG / "libalpharat_hip.so"

AR_OK, AR_E_INVALID, AR_E_BACKEND, AR_E_IO, AR_E_DEVICE, AR_E_NOMEM = 0, -1, -2, -3, -4, -5


class ArSearchConfig(C.Structure):
    _fields_ = [
        ("c_puct", C.c_float), ("fpu_reduction", C.c_float), ("force_k", C.c_float),
        ("noise_epsilon", C.c_float), ("noise_concentration", C.c_float),
        ("collision_limit_min", C.c_uint32), ("collision_limit_max", C.c_uint32),
        ("collision_scaling_start", C.c_uint32), ("collision_scaling_end", C.c_uint32),
        ("collision_scaling_power", C.c_float),
    ]


class ArGameSpec(C.Structure):
    _fields_ = [
        ("width", C.c_uint8), ("height", C.c_uint8), ("max_turns", C.c_uint16), ("turn", C.c_uint16),
        ("p1_x", C.c_uint8), ("p1_y", C.c_uint8), ("p2_x", C.c_uint8), ("p2_y", C.c_uint8),
        ("p1_mud", C.c_uint8), ("p2_mud", C.c_uint8), ("p1_score", C.c_float), ("p2_score", C.c_float),
        ("cost", C.c_void_p), ("cheese", C.c_void_p),
    ]


class ArSearchResult(C.Structure):
    _fields_ = [
        ("policy_p1", C.c_float * 5), ("policy_p2", C.c_float * 5), ("value_p1", C.c_float), ("value_p2", C.c_float),
        ("visit_counts_p1", C.c_float * 5), ("visit_counts_p2", C.c_float * 5),
        ("prior_p1", C.c_float * 5), ("prior_p2", C.c_float * 5),
        ("total_visits", C.c_uint32), ("nn_evals", C.c_uint32), ("terminals", C.c_uint32), ("collisions", C.c_uint32),
    ]


class ArLeaf(C.Structure):
    _fields_ = [
        ("p1_x", C.c_uint8), ("p1_y", C.c_uint8), ("p2_x", C.c_uint8), ("p2_y", C.c_uint8),
        ("p1_mud", C.c_uint8), ("p2_mud", C.c_uint8), ("turn", C.c_uint16),
        ("p1_score", C.c_float), ("p2_score", C.c_float), ("cheese_bits", C.c_uint64 * 4),
    ]


ArPredictFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(ArLeaf), C.c_uint32, C.POINTER(C.c_float),
                          C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float))


class ArSelfPlayParams(C.Structure):
    _fields_ = [
        ("width", C.c_uint8), ("height", C.c_uint8), ("cheese_count", C.c_uint16), ("max_turns", C.c_uint16),
        ("num_games", C.c_uint32), ("cheese_symmetric", C.c_int), ("maze_type", C.c_char_p), ("positions", C.c_char_p),
        ("wall_density", C.c_float), ("mud_density", C.c_float), ("maze_symmetric", C.c_int),
        ("simulations", C.c_uint32), ("batch_size", C.c_uint32), ("search", ArSearchConfig),
        ("num_threads", C.c_uint32), ("output_dir", C.c_char_p), ("max_games_per_bundle", C.c_uint32),
        ("weights_path", C.c_char_p), ("device", C.c_char_p), ("mux_max_batch_size", C.c_uint32),
        ("cache_size", C.c_uint64), ("has_seed", C.c_int), ("game_seed_base", C.c_uint64),
        ("rng_seed_base", C.c_uint64), ("first_game_index", C.c_uint32), ("concurrent_games", C.c_uint32),
        ("device_index", C.c_int),
    ]


class ArSelfPlayStats(C.Structure):
    _fields_ = [
        ("total_games", C.c_uint32), ("total_positions", C.c_uint64), ("total_simulations", C.c_uint64),
        ("elapsed_secs", C.c_double), ("p1_wins", C.c_uint32), ("p2_wins", C.c_uint32), ("draws", C.c_uint32),
        ("total_cheese_collected", C.c_float), ("total_cheese_available", C.c_uint32),
        ("min_turns", C.c_uint32), ("max_turns", C.c_uint32),
        ("total_nn_evals", C.c_uint64), ("total_terminals", C.c_uint64), ("total_collisions", C.c_uint64),
        ("cache_hits", C.c_uint64), ("cache_misses", C.c_uint64),
        ("gather_node_visits", C.c_uint64), ("backup_node_visits", C.c_uint64), ("new_nodes", C.c_uint64),
        ("device_secs", C.c_double), ("steps", C.c_uint64),
        ("gather_secs", C.c_double), ("gather_launches", C.c_uint64),
    ]


class ArSessionInfo(C.Structure):
    _fields_ = [
        ("resident_games", C.c_uint32), ("groups", C.c_uint32), ("gather_kind", C.c_uint32), ("gather_pass_limit", C.c_uint32),
        ("tree_region_bytes", C.c_uint64), ("host_grown_arenas", C.c_uint64), ("idle_slots", C.c_uint32),
        ("tree_pages_per_game", C.c_float),
    ]


class ArProgress(C.Structure):
    _fields_ = [
        ("games_completed", C.c_uint32), ("positions_completed", C.c_uint64),
        ("simulations_completed", C.c_uint64), ("nn_evals_completed", C.c_uint64),
    ]


class ArGameRecordView(C.Structure):
    _fields_ = [
        ("width", C.c_uint8), ("height", C.c_uint8), ("max_turns", C.c_uint16),
        ("game_index", C.c_uint32), ("n_positions", C.c_uint32),
        ("maze", C.POINTER(C.c_int8)), ("initial_cheese", C.POINTER(C.c_uint8)), ("cheese_outcomes", C.POINTER(C.c_uint8)),
        ("final_p1_score", C.c_float), ("final_p2_score", C.c_float), ("result", C.c_uint8),
        ("cheese_available", C.c_uint16),
        ("total_simulations", C.c_uint64), ("total_nn_evals", C.c_uint64), ("total_terminals", C.c_uint64),
        ("total_collisions", C.c_uint64),
        ("p1_pos", C.POINTER(C.c_uint8)), ("p2_pos", C.POINTER(C.c_uint8)),
        ("p1_score", C.POINTER(C.c_float)), ("p2_score", C.POINTER(C.c_float)),
        ("p1_mud", C.POINTER(C.c_uint8)), ("p2_mud", C.POINTER(C.c_uint8)),
        ("turn", C.POINTER(C.c_uint16)), ("cheese_mask", C.POINTER(C.c_uint8)),
        ("value_p1", C.POINTER(C.c_float)), ("value_p2", C.POINTER(C.c_float)),
        ("visit_counts_p1", C.POINTER(C.c_float)), ("visit_counts_p2", C.POINTER(C.c_float)),
        ("prior_p1", C.POINTER(C.c_float)), ("prior_p2", C.POINTER(C.c_float)),
        ("policy_p1", C.POINTER(C.c_float)), ("policy_p2", C.POINTER(C.c_float)),
        ("action_p1", C.POINTER(C.c_uint8)), ("action_p2", C.POINTER(C.c_uint8)),
    ]


ArGameSink = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(ArGameRecordView))


class ArMatchAgent(C.Structure):
    _fields_ = [
        ("weights_path", C.c_char_p), ("simulations", C.c_uint32), ("batch_size", C.c_uint32),
        ("search", ArSearchConfig), ("rng_seed_base", C.c_uint64), ("kind", C.c_uint32), ("temperature", C.c_float),
    ]


AR_AGENT_SEARCH, AR_AGENT_RANDOM, AR_AGENT_GREEDY = 0, 1, 2


class ArMatchParams(C.Structure):
    _fields_ = [
        ("width", C.c_uint8), ("height", C.c_uint8), ("cheese_count", C.c_uint16), ("max_turns", C.c_uint16),
        ("cheese_symmetric", C.c_int), ("maze_type", C.c_char_p), ("positions", C.c_char_p),
        ("wall_density", C.c_float), ("mud_density", C.c_float), ("maze_symmetric", C.c_int),
        ("num_games", C.c_uint32), ("first_game_index", C.c_uint32), ("has_seed", C.c_int),
        ("game_seed_base", C.c_uint64), ("swap_sides", C.c_int), ("concurrent_games", C.c_uint32),
        ("device", C.c_char_p), ("device_index", C.c_int), ("a", ArMatchAgent), ("b", ArMatchAgent),
    ]


class ArMatchSearchView(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_float)) for k in (
        "policy_p1", "policy_p2", "value_p1", "value_p2", "visit_counts_p1", "visit_counts_p2", "prior_p1", "prior_p2")
    ] + [(k, C.POINTER(C.c_uint32)) for k in ("total_visits", "nn_evals", "terminals", "collisions")]


class ArMatchGameView(C.Structure):
    _fields_ = [
        ("width", C.c_uint8), ("height", C.c_uint8), ("max_turns", C.c_uint16),
        ("game_index", C.c_uint32), ("n_positions", C.c_uint32), ("a_is_p1", C.c_uint8), ("result", C.c_uint8),
        ("final_p1_score", C.c_float), ("final_p2_score", C.c_float),
        ("p1_pos", C.POINTER(C.c_uint8)), ("p2_pos", C.POINTER(C.c_uint8)),
        ("p1_score", C.POINTER(C.c_float)), ("p2_score", C.POINTER(C.c_float)),
        ("p1_mud", C.POINTER(C.c_uint8)), ("p2_mud", C.POINTER(C.c_uint8)),
        ("turn", C.POINTER(C.c_uint16)), ("cheese_mask", C.POINTER(C.c_uint8)),
        ("action_p1", C.POINTER(C.c_uint8)), ("action_p2", C.POINTER(C.c_uint8)),
        ("a", ArMatchSearchView), ("b", ArMatchSearchView),
    ]


class ArMatchStats(C.Structure):
    _fields_ = [
        ("total_games", C.c_uint32), ("wins_a", C.c_uint32), ("wins_b", C.c_uint32), ("draws", C.c_uint32),
        ("cheese_a", C.c_float), ("cheese_b", C.c_float), ("total_positions", C.c_uint64),
        ("simulations_a", C.c_uint64), ("simulations_b", C.c_uint64), ("nn_evals_a", C.c_uint64),
        ("nn_evals_b", C.c_uint64), ("terminals_a", C.c_uint64), ("terminals_b", C.c_uint64),
        ("collisions_a", C.c_uint64), ("collisions_b", C.c_uint64), ("elapsed_secs", C.c_double),
    ]


ArMatchSink = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(ArMatchGameView))


class ArTrainRows(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2", "action_p1",
                                          "action_p2", "cheese_outcomes")]


class ArValSums(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_double * 2) for k in ("ce", "sq_err", "ent_pred", "ent_target")] + [
        (k, C.c_uint64 * 2) for k in ("top1", "top2")] + [
        (k, C.c_double * 2) for k in ("sum_pred", "sum_target", "sum_pred2", "sum_target2", "sum_pred_target")]


class ArValRows(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("logits_p1", "logits_p2", "value_p1", "value_p2")]


class ArOwnSums(C.Structure):
    _fields_ = [("n", C.c_uint64), ("cells", C.c_uint64), ("ce", C.c_double), ("batch_weighted", C.c_double),
                ("batch_rows", C.c_uint64)]


class ArOwnRows(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("ce", "cells", "value", "logits")]


MLP_TENSORS = ("trunk0_w", "trunk0_b", "bn1_w", "bn1_b", "trunk4_w", "trunk4_b", "bn2_w", "bn2_b", "p1_w", "p1_b", "p2_w", "p2_b",
               "value_w", "value_b")


class ArMlpTensors(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in MLP_TENSORS]


class ArMlpBnStats(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("mean1", "var1", "mean2", "var2")]


class ArTrainOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("losses", "logits_p1", "logits_p2", "value_p1", "value_p2")]


SYM_TENSORS = ("se0_w", "se0_b", "se1_w", "se1_b", "pe0_w", "pe0_b", "pe1_w", "pe1_b", "trunk0_w", "trunk0_b", "bn1_w", "bn1_b",
               "trunk4_w", "trunk4_b", "bn2_w", "bn2_b", "policy_w", "policy_b", "value_w", "value_b")


class ArSymTensors(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in SYM_TENSORS]


class ArSymBnStats(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("se_mean", "se_var", "pe_mean", "pe_var", "bn1_mean", "bn1_var", "bn2_mean",
                                          "bn2_var")]


LV_TENSORS = MLP_TENSORS + ("own0_w", "own0_b", "own2_w", "own2_b")


class ArLvTensors(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in LV_TENSORS]


class ArLvTrainOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("losses", "logits_p1", "logits_p2", "value_p1", "value_p2", "ownership_logits")]


class ArTrainDropout(C.Structure):
    _fields_ = [("p", C.c_float), ("seed", C.c_uint64), ("step", C.c_uint64)]


class ArCnnDims(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("channels", "player_dim", "hidden_dim", "n_blocks")]


# ArCnnTensors and ArCnnBnStats hold eight block slots each, as flat pointers: a model of B blocks fills the first B
CNN_MAX_BLOCKS = 8
CNN_BLOCK_TENSORS = ("bn1_w", "bn1_b", "conv1_w", "bn2_w", "bn2_b", "conv2_w")
CNN_TENSORS = (("stem_w", "stem_bn_w", "stem_bn_b") + tuple(f"b{b}_{k}" for b in range(CNN_MAX_BLOCKS) for k in CNN_BLOCK_TENSORS)
               + ("enc_w", "enc_b", "comb_w", "comb_b", "policy_w", "policy_b", "value_w", "value_b"))
CNN_BLOCK_STATS = ("bn1_mean", "bn1_var", "bn2_mean", "bn2_var")
CNN_STATS = ("stem_mean", "stem_var") + tuple(f"b{b}_{k}" for b in range(CNN_MAX_BLOCKS) for k in CNN_BLOCK_STATS)


class ArCnnTensors(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in CNN_TENSORS]


class ArCnnBnStats(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in CNN_STATS]


# ar_rows_grad_cnn_gpool: a block's gpool_channels (0: a ResBlock), its five further tensors and pool_bn's two statistics
CNN_POOL_BLOCK_TENSORS = ("pool_bn_w", "pool_bn_b", "pool_conv_w", "pool_linear_w", "pool_linear_b")
CNN_POOL_TENSORS = tuple(f"b{b}_{k}" for b in range(CNN_MAX_BLOCKS) for k in CNN_POOL_BLOCK_TENSORS)
CNN_POOL_STATS = tuple(f"b{b}_{k}" for b in range(CNN_MAX_BLOCKS) for k in ("pool_bn_mean", "pool_bn_var"))


class ArCnnPoolDims(C.Structure):
    _fields_ = [("gpool_channels", C.c_uint32 * CNN_MAX_BLOCKS)]


class ArCnnPoolTensors(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in CNN_POOL_TENSORS]


class ArCnnPoolStats(C.Structure):  # the eight blocks' ArCnnPoolStats, as flat pointers
    _fields_ = [(k, C.c_void_p) for k in CNN_POOL_STATS]


# every symbol include/alpharat_hip.h declares (checked by the CPU test-suite)
EXPORTS = {
    "ar_version": (C.c_char_p, []),
    "ar_last_error": (C.c_size_t, [C.c_char_p, C.c_size_t]),
    "ar_device_count": (C.c_int, []),
    "ar_generate_maze": (C.c_int, [C.c_uint8, C.c_uint8, C.c_float, C.c_float, C.c_int, C.c_uint64, C.c_void_p]),
    "ar_generate_cheese": (C.c_int, [C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint16, C.c_int, C.c_uint64,
                                    C.c_void_p]),
    "ar_device_sync": (C.c_int, [C.c_int]),
    "ar_release_device_memory": (C.c_int, [C.c_int]),
    "ar_net_load": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "ar_net_free": (None, [C.c_void_p]),
    "ar_net_evaluate": (C.c_int, [C.c_void_p, C.POINTER(ArGameSpec), C.c_uint32] + [C.c_void_p] * 6),
    "ar_encode": (C.c_int, [C.POINTER(ArGameSpec), C.c_uint32, C.c_int, C.c_void_p]),
    "ar_search": (C.c_int, [C.POINTER(ArGameSpec), C.POINTER(ArSearchConfig), C.c_uint32, C.c_uint32,
                            C.POINTER(C.c_uint64), ArPredictFn, C.c_void_p, C.c_void_p, C.c_int,
                            C.POINTER(ArSearchResult)]),
    "ar_search_many": (C.c_int, [C.POINTER(ArGameSpec), C.c_uint32, C.POINTER(ArSearchConfig), C.c_uint32, C.c_uint32,
                                 C.POINTER(C.c_uint64), C.c_void_p, C.c_int, C.POINTER(ArSearchResult)]),
    "ar_selfplay_run": (C.c_int, [C.POINTER(ArSelfPlayParams), C.POINTER(ArProgress), ArGameSink, C.c_void_p,
                                  C.POINTER(ArSelfPlayStats)]),
    "ar_selfplay_open": (C.c_int, [C.POINTER(ArSelfPlayParams), C.POINTER(ArProgress), ArGameSink, C.c_void_p,
                                   C.POINTER(C.c_void_p)]),
    "ar_selfplay_step": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(ArSelfPlayStats), C.POINTER(C.c_int)]),
    "ar_selfplay_close": (C.c_int, [C.c_void_p, C.POINTER(ArSelfPlayStats)]),
    "ar_selfplay_info": (C.c_int, [C.c_void_p, C.POINTER(ArSessionInfo)]),
    "ar_match_run": (C.c_int, [C.POINTER(ArMatchParams), ArMatchSink, C.c_void_p, C.POINTER(ArMatchStats)]),
    "ar_write_bundle": (C.c_int, [C.POINTER(ArGameRecordView), C.c_uint32, C.c_char_p]),
    "ar_rows_open": (C.c_int, [C.c_uint8, C.c_uint8, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]),
    "ar_rows_add_games": (C.c_int, [C.c_void_p, C.POINTER(ArGameRecordView), C.c_uint32]),
    "ar_rows_attach": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ar_rows_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "ar_rows_games": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ar_rows_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ArTrainRows)]),
    "ar_rows_build_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "ar_rows_order_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "ar_rows_build_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ArTrainRows), C.c_void_p]),
    "ar_rows_clear": (C.c_int, [C.c_void_p]),
    "ar_rows_close": (None, [C.c_void_p]),
    "ar_rows_validate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(ArValSums),
                                   C.POINTER(ArValRows)]),
    "ar_net_has_ownership": (C.c_int, [C.c_void_p]),
    "ar_rows_validate_lv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.POINTER(ArValSums), C.POINTER(ArOwnSums), C.POINTER(ArValRows),
                                      C.POINTER(ArOwnRows)]),
    "ar_rows_grad_mlp": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(ArMlpTensors),
                                   C.POINTER(ArMlpTensors), C.POINTER(ArMlpBnStats), C.c_float, C.c_float,
                                   C.POINTER(ArTrainOut), C.c_void_p]),
    "ar_rows_grad_symmetric": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(ArSymTensors),
                                         C.POINTER(ArSymTensors), C.POINTER(ArSymBnStats), C.c_float, C.c_float,
                                         C.POINTER(ArTrainOut), C.c_void_p]),
    "ar_rows_grad_local_value": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(ArLvTensors),
                                           C.POINTER(ArLvTensors), C.POINTER(ArMlpBnStats), C.c_float, C.c_float, C.c_float,
                                           C.POINTER(ArLvTrainOut), C.c_void_p]),
    "ar_rows_grad_mlp_dropout": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(ArMlpTensors),
                                           C.POINTER(ArMlpTensors), C.POINTER(ArMlpBnStats), C.c_float, C.c_float,
                                           C.POINTER(ArTrainOut), C.POINTER(ArTrainDropout), C.c_void_p]),
    "ar_rows_grad_symmetric_dropout": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(ArSymTensors),
                                                 C.POINTER(ArSymTensors), C.POINTER(ArSymBnStats), C.c_float, C.c_float,
                                                 C.POINTER(ArTrainOut), C.POINTER(ArTrainDropout), C.c_void_p]),
    "ar_rows_grad_local_value_dropout": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(ArLvTensors),
                                                   C.POINTER(ArLvTensors), C.POINTER(ArMlpBnStats), C.c_float, C.c_float,
                                                   C.c_float, C.POINTER(ArLvTrainOut), C.POINTER(ArTrainDropout), C.c_void_p]),
    "ar_rows_grad_cnn": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ArCnnDims), C.POINTER(ArCnnTensors),
                                   C.POINTER(ArCnnTensors), C.POINTER(ArCnnBnStats), C.c_float, C.c_float,
                                   C.POINTER(ArTrainOut), C.c_void_p]),
    "ar_rows_grad_cnn_gpool": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ArCnnDims), C.POINTER(ArCnnPoolDims),
                                         C.POINTER(ArCnnTensors), C.POINTER(ArCnnPoolTensors), C.POINTER(ArCnnTensors),
                                         C.POINTER(ArCnnPoolTensors), C.POINTER(ArCnnBnStats), C.POINTER(ArCnnPoolStats),
                                         C.c_float, C.c_float, C.POINTER(ArTrainOut), C.POINTER(ArTrainDropout), C.c_void_p]),
    "ar_train_dropout_mask": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p,
                                        C.c_void_p]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP library. Raises if it has not been built -- there is no other backend."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). alpharat_amd has no CPU fallback."
        )
    L = C.CDLL(str(LIB_PATH))
    for name, (res, args) in EXPORTS.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def last_error() -> str:
    buf = C.create_string_buffer(4096)
    load().ar_last_error(buf, 4096)
    return buf.value.decode(errors="replace")


def check(rc: int) -> None:
    """Map C-ABI error codes onto the exceptions the reference's PyO3 layer raises
    (crates/alpharat-sampling/src/bindings.rs:474-482, crates/alpharat-mcts/src/bindings.rs:300-303)."""
    if rc == AR_OK:
        return
    msg = last_error()
    if rc == AR_E_INVALID:
        raise ValueError(msg)
    if rc == AR_E_IO:
        raise OSError(msg)
    if rc == AR_E_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)
