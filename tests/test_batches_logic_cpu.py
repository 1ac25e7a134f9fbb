"""The row of a position as either player sees it, on the CPU: rows_build_row_as of alpharat_amd/csrc/dev_rows.h (what
k_rows_batch runs, compiled for the CPU by tests/hostsim_batches) against swap_rows(stack_rows(games), mask) of the NumPy
restatements (tests/_rows_np.py, tests/_augment_np.py), on games played by the oracle. Equality of bytes."""
import numpy as np
import pytest

import _augment_np as A
import _batches as B
import _rows as T
import _rows_np as R


@pytest.fixture(scope="module", params=B.BOARDS, ids=lambda b: b[0])
def board(request):
    games = T.board_games(*request.param)
    return request.param, games, R.stack_rows(games)


def test_the_boards_cover_what_they_are_there_for():
    cells = {name: w * h for name, w, h, *_ in B.BOARDS}
    assert 64 < cells["9x8"] <= 128 and cells["16x16"] == 256    # cheese bits beyond one word; the largest board
    assert any(c % 4 for c in cells.values())                    # int8 rows that are no multiple of four bytes
    assert any(maze is not None for _, _, _, _, _, maze, *_ in B.BOARDS)  # mud (checked on the games in tests/test_rows_logic_cpu.py)


def test_rows_equal_the_swapped_restatement_byte_for_byte(board):
    (name, w, h, *_), games, plain = board
    n = len(plain["value_p1"])
    rng = np.random.default_rng(17)
    masks = dict(all=np.ones(n, bool), none=np.zeros(n, bool), random=rng.random(n) < 0.5)
    assert n == 1 or (masks["random"].any() and not masks["random"].all())
    orders = dict(identity=np.arange(n), permutation=rng.permutation(n), repeated=rng.integers(0, n, size=n + 3))
    for mname, mask in masks.items():
        want = A.swap_rows(plain, mask, w, h)
        for oname, rows in orders.items():
            got = [B.sim_batch(games, rows, mask[rows], reverse=rev) for rev in (False, True)]
            T.assert_rows_equal(got[0], R.take(want, rows), f"{name} mask={mname} order={oname}")
            T.assert_rows_equal(got[1], got[0], f"{name} mask={mname} order={oname}: lanes in reverse order")
    if name == "9x8":  # cheese on cells of the second 64-bit word
        assert any(np.asarray(g["cheese_mask"]).reshape(g["n"], -1)[:, 64:].any() for g in games)
    if n > 1:  # the swapped rows are other bytes
        assert A.swap_rows(plain, masks["all"], w, h)["observation"].tobytes() != plain["observation"].tobytes()


def test_without_a_mask_the_rows_are_rows_build_rows(board):
    (name, *_), games, plain = board
    n = len(plain["value_p1"])
    rows = np.random.default_rng(3).permutation(n)
    want = T.sim_build(games, rows)
    T.assert_rows_equal(B.sim_batch(games, rows, None), want, f"{name} no mask")
    T.assert_rows_equal(B.sim_batch(games, rows, np.zeros(n, np.uint8), reverse=True), want, f"{name} mask of zeros")


def test_mud_scores_and_every_outcome_are_exchanged():
    for game in (B.mud_game(), B.capture_game(), B.open_game()):
        w, h, n = game["width"], game["height"], game["n"]
        plain = R.game_rows(game)
        want = A.swap_rows(plain, np.ones(n, bool), w, h)
        for rev in (False, True):
            T.assert_rows_equal(B.sim_batch([game], np.arange(n), np.ones(n, np.uint8), reverse=rev), want, f"{w}x{h}")
    # the open game's first position: equal scores, swapped to -0.0
    assert want["observation"][0, w * h * 7].view(np.uint32) == 0x80000000
    assert set(np.unique(R.game_rows(B.capture_game())["cheese_outcomes"])) == {-1, 0, 1, 2, 3}
    mud = B.mud_game()
    assert (np.asarray(mud["p1_mud"]) != np.asarray(mud["p2_mud"])).any()


def test_row_index_out_of_range_is_refused():
    g = B.capture_game()
    keep: list = []
    gs = (T.RsGame * 1)(T._rs_game(g, keep))
    rows = np.array([g["n"]], np.uint64)
    out = T.empty_rows(1, 5, 5)
    assert B.sim().bs_build(gs, 1, rows.ctypes.data, None, 1, 0, *[out[k].ctypes.data for k in R.KEYS]) == -1


def test_the_benchmarks_record_sizes_are_the_headers():
    from tools.bench_batches import POSREC_BYTES

    assert POSREC_BYTES == {1: B.sim().bs_record_bytes(49), 4: B.sim().bs_record_bytes(65)}
