"""Bundle writer (ar_write_bundle, host only) against the reference's own known-answer bundle test:
the two games of crates/alpharat-sampling/src/bin/write_test_bundle.rs:24-168 (inputs, restated here as
data) and the assertions of tests/data/test_rust_bundle_parity.py:66-230 on what a reader must find,
plus the container contract of recording.rs / npz_writer.rs (26 arrays, dtypes, v1.0 headers padded to
256 bytes, deflate)."""
import ctypes as C

import numpy as np
import pytest

from _bundles import check_container, view_of
from alpharat_amd import _lib

UNCOLLECTED, P1WIN, SIMULTANEOUS = 2, 0, 1


def _game0():
    maze = np.ones(9 * 4, np.int8)
    for i in (2, 3, 9, 10, 24, 27, 32, 33):
        maze[i] = -1
    cheese = np.zeros(9, np.uint8)
    cheese[4] = 1
    out = np.full(9, UNCOLLECTED, np.uint8)
    out[4] = SIMULTANEOUS
    pos = dict(
        p1_pos=[[0, 0], [0, 1]], p2_pos=[[2, 2], [2, 1]], p1_score=[0, 0], p2_score=[0, 0], p1_mud=[0, 0], p2_mud=[0, 0],
        turn=[0, 1], cheese_mask=[cheese, cheese], value_p1=[0.75, 0.8], value_p2=[0.25, 0.2],
        visit_counts_p1=[[10, 5, 0, 0, 1], [4, 12, 0, 0, 0]], visit_counts_p2=[[0, 0, 6, 8, 2], [0, 0, 0, 12, 4]],
        prior_p1=[[.3, .3, .1, .1, .2], [.4, .4, .1, .05, .05]], prior_p2=[[.1, .1, .3, .3, .2], [.05, .05, .1, .4, .4]],
        policy_p1=[[.625, .3125, 0, 0, .0625], [.25, .75, 0, 0, 0]], policy_p2=[[0, 0, .375, .5, .125], [0, 0, 0, .75, .25]],
        action_p1=[0, 1], action_p2=[2, 3])
    return dict(width=3, height=3, max_turns=30, game_index=0, maze=maze, initial_cheese=cheese, cheese_outcomes=out,
                final=(0.5, 0.5), result=0, cheese_available=1, sims=32, pos=pos)


def _game1():
    cheese = np.zeros(9, np.uint8)
    cheese[[0, 8]] = 1
    out = np.full(9, UNCOLLECTED, np.uint8)
    out[0] = P1WIN
    pos = dict(
        p1_pos=[[1, 0]], p2_pos=[[1, 2]], p1_score=[0], p2_score=[0], p1_mud=[0], p2_mud=[3], turn=[0], cheese_mask=[cheese],
        value_p1=[1.2], value_p2=[0.8], visit_counts_p1=[[2, 2, 2, 6, 4]], visit_counts_p2=[[0, 0, 0, 0, 16]],
        prior_p1=[[.2] * 5], prior_p2=[[0, 0, 0, 0, 1]], policy_p1=[[.125, .125, .125, .375, .25]],
        policy_p2=[[0, 0, 0, 0, 1]], action_p1=[3], action_p2=[4])
    return dict(width=3, height=3, max_turns=20, game_index=1, maze=np.ones(36, np.int8), initial_cheese=cheese,
                cheese_outcomes=out, final=(1.0, 0.0), result=1, cheese_available=2, sims=16, pos=pos)


def _view(g, keep):
    """The nested layout above as the flat game dict tests/_bundles.py works on."""
    flat = dict(width=g["width"], height=g["height"], max_turns=g["max_turns"], game_index=g["game_index"],
                maze=g["maze"], initial_cheese=g["initial_cheese"], cheese_outcomes=g["cheese_outcomes"],
                final_p1_score=g["final"][0], final_p2_score=g["final"][1], result=g["result"],
                cheese_available=g["cheese_available"], total_simulations=g["sims"], **g["pos"])
    flat["cheese_mask"] = np.stack(flat["cheese_mask"])
    return view_of(flat, keep)


@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    lib = _lib.load()
    keep = []
    views = (_lib.ArGameRecordView * 2)(_view(_game0(), keep), _view(_game1(), keep))
    path = tmp_path_factory.mktemp("bundle") / "bundle_known_answer.npz"
    lib.ar_write_bundle.restype = C.c_int
    _lib.check(lib.ar_write_bundle(views, 2, str(path).encode()))
    return path


def test_container_contract(bundle):
    check_container(bundle)


def test_known_answers(bundle):
    z = np.load(bundle)
    assert z["game_lengths"].tolist() == [2, 1]
    assert z["max_turns"].tolist() == [30, 20] and z["result"].tolist() == [0, 1]
    np.testing.assert_allclose(z["final_p1_score"], [0.5, 1.0])
    np.testing.assert_allclose(z["final_p2_score"], [0.5, 0.0])
    maze = z["maze"]
    assert maze.shape == (2, 3, 3, 4)
    assert maze[0, 0, 0, 2] == -1 and maze[0, 0, 0, 3] == -1 and maze[0, 0, 0, 0] == 1 and maze[0, 0, 0, 1] == 1
    ic = z["initial_cheese"]
    assert ic.shape == (2, 3, 3) and ic[0, 1, 1] and ic[0].sum() == 1 and ic[1, 0, 0] and ic[1, 2, 2]
    co = z["cheese_outcomes"]
    assert co[0, 1, 1] == SIMULTANEOUS and co[0, 0, 0] == UNCOLLECTED and co[1, 0, 0] == P1WIN and co[1, 2, 2] == UNCOLLECTED
    assert z["p1_pos"].tolist() == [[0, 0], [0, 1], [1, 0]] and z["p2_pos"].tolist() == [[2, 2], [2, 1], [1, 2]]
    assert z["turn"].tolist() == [0, 1, 0] and z["p2_mud"].tolist() == [0, 0, 3]
    assert z["action_p1"].tolist() == [0, 1, 3] and z["action_p2"].tolist() == [2, 3, 4]
    np.testing.assert_allclose(z["value_p1"], [0.75, 0.8, 1.2], atol=1e-6)
    np.testing.assert_allclose(z["policy_p1"][0], [0.625, 0.3125, 0.0, 0.0, 0.0625], atol=1e-6)
    np.testing.assert_allclose(z["policy_p2"][0], [0.0, 0.0, 0.375, 0.5, 0.125], atol=1e-6)
    np.testing.assert_allclose(z["prior_p1"][0], [0.3, 0.3, 0.1, 0.1, 0.2], atol=1e-6)
    np.testing.assert_allclose(z["visit_counts_p2"][2], [0, 0, 0, 0, 16], atol=1e-6)
    assert z["cheese_mask"].shape == (3, 3, 3) and z["cheese_mask"][0, 1, 1] and z["cheese_mask"][2].sum() == 2
