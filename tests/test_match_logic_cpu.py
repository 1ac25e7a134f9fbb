"""Head-to-head matches on the CPU: the product's search headers and dev_match.h match_move (compiled for the CPU by
tests/hostsim_match, scheduled like the device: two slot sets, ticks, drains, refills) against the match restated on
the oracle (tests/_match.py oracle_game). Every position record must be equal bit for bit: positions, both actions,
both agents' policies, values, visit counts, priors and counters."""
import numpy as np
import pytest

import _hostsim as H
import _match as M
import _oracle as O

SEED_A, SEED_B = 0xA0000, 0xB0000


def _agents(width):
    """A: SmartUniform, 40 simulations, batch 8. B: the hashed evaluator, 100 simulations, batch 16, another c_puct."""
    a = M.Agent(O.make_config(), 40, 8, SEED_A)
    b = M.Agent(O.make_config(c_puct=0.9), 100, 16, SEED_B, backend=4, net=O.CallbackBackend(H.hashed_eval(width)))
    return a, b


def _games(w, h, cheese, max_turns, indices):
    return [O.Game(w, h, max_turns).random_cheese(cheese, True, i) for i in indices]


def test_twelve_games_both_orientations_match_the_oracle():
    a, b = _agents(5)
    idx = list(range(12))
    ogs = _games(5, 5, 5, 30, idx)
    # 12 games on 5 resident slot pairs: slots are refilled and the last generation is partial
    got, info = M.hostsim_match(ogs, idx, 30, M.ms_agent(a), M.ms_agent(b, evaluator=1), swap_sides=True, resident=5)
    assert {g["a_is_p1"] for g in got} == {True, False}
    for i, og in zip(idx, ogs):
        want = M.oracle_game(og, i, a, b, a_is_p1=i % 2 == 0)
        M.assert_same_game(got[i], want, f"game {i}")
    # the agents' searches end at different times: a move takes more ticks than either agent's search alone
    assert info["ticks"] > sum(g["n"] for g in got) / 5


def test_records_do_not_depend_on_slots_cuts_or_parked_gathers():
    a, b = _agents(5)
    idx = list(range(6))
    ogs = _games(5, 5, 5, 30, idx)
    base, _ = M.hostsim_match(ogs, idx, 30, M.ms_agent(a), M.ms_agent(b, evaluator=1), resident=6, visit_every=1)
    # other slot counts and visit periods; gathers cut off after 3 rounds and resumed; trees that stall and grow
    other, info = M.hostsim_match(ogs, idx, 30, M.ms_agent(a, gather_rounds=3, arena_nodes=16),
                                  M.ms_agent(b, evaluator=1, gather_rounds=5, arena_nodes=32), resident=2, visit_every=7)
    assert info["grows_a"] > 0 and info["grows_b"] > 0
    for i in idx:
        M.assert_same_game(other[i], base[i], f"game {i}")


def test_game_that_ends_at_the_turn_limit():
    a, b = _agents(5)
    og = O.Game(5, 5, 6).random_cheese(5, True, 3)
    got, _ = M.hostsim_match([og], [3], 6, M.ms_agent(a), M.ms_agent(b, evaluator=1), resident=1)
    want = M.oracle_game(og, 3, a, b, a_is_p1=False)  # (index 3 is odd: B plays P1)
    assert want["n"] == 6 and int(want["ints"][-1, 6]) == 5
    M.assert_same_game(got[0], want, "turn limit")


def test_board_above_64_cells():
    a, b = _agents(11)
    og = O.Game(11, 9, 12).random_cheese(9, True, 2)
    got, _ = M.hostsim_match([og], [2], 12, M.ms_agent(a), M.ms_agent(b, evaluator=1), resident=1)
    M.assert_same_game(got[0], M.oracle_game(og, 2, a, b, a_is_p1=True), "11x9")


def test_agent_a_alone_and_independent_of_b_seed():
    """A against A with swap_sides off: A's searches are those of A alone, whatever B's seed base is."""
    a = M.Agent(O.make_config(), 40, 8, SEED_A)
    idx = [0, 1, 2]
    ogs = _games(5, 5, 5, 30, idx)
    runs = []
    for seed_b in (SEED_B, SEED_B + 977):
        b = M.Agent(O.make_config(), 40, 8, seed_b)
        got, _ = M.hostsim_match(ogs, idx, 30, M.ms_agent(a), M.ms_agent(b), swap_sides=False, resident=3)
        for i, og in zip(idx, ogs):
            assert got[i]["a_is_p1"]
            M.assert_same_game(got[i], M.oracle_game(og, i, a, b, a_is_p1=True), f"game {i} seed_b {seed_b:#x}")
        runs.append(got)
    for i, og in zip(idx, ogs):
        alone = M.oracle_game(og, i, a, a, a_is_p1=True, only="a")
        for got in runs:
            assert got[i]["a"]["floats"][0].tobytes() == alone["a"]["floats"][0].tobytes(), i
            np.testing.assert_array_equal(got[i]["a"]["counts"][0], alone["a"]["counts"][0])
            assert got[i]["ints"][0, 7] == alone["ints"][0, 7]  # and A's first action (A is P1)
        # B's stream did change what B did
    assert any(runs[0][i]["b"]["floats"].tobytes() != runs[1][i]["b"]["floats"].tobytes()
               or not np.array_equal(runs[0][i]["ints"], runs[1][i]["ints"]) for i in idx)
