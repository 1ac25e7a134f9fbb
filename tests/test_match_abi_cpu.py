"""CPU: the match entry point is declared, exported and bound; without a device it fails loudly; the Python result
carries the reference's field names (alpharat/eval/tournament.py:61-72 MatchupResult)."""
import dataclasses
import inspect
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from alpharat_amd import _lib

    return _lib.load()


def test_match_entry_point_is_declared_exported_and_bound(lib):
    from alpharat_amd import _lib

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    assert re.search(r"\bint\s+ar_match_run\s*\(", header)
    assert "ar_match_run" in _lib.EXPORTS
    assert lib.ar_match_run is not None
    for name in ("ArMatchAgent", "ArMatchParams", "ArMatchGameView", "ArMatchStats", "ArMatchSink"):
        assert name in header and hasattr(_lib, name), name
    # the ctypes mirrors have the fields the header declares, in its order
    for cls in (_lib.ArMatchAgent, _lib.ArMatchParams, _lib.ArMatchSearchView, _lib.ArMatchGameView, _lib.ArMatchStats):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cls.__name__, cls.__name__), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n for stmt in body.split(";") for n in re.findall(r"[\s*,](\w+)\s*(?=,|$)", " " + stmt.strip())]
        assert declared == [f[0] for f in cls._fields_], cls.__name__


def test_match_result_carries_the_reference_field_names():
    import alpharat_amd
    from alpharat_amd.match import MatchAgent, MatchResult, play_match

    assert alpharat_amd.play_match is play_match and alpharat_amd.MatchAgent is MatchAgent
    names = [f.name for f in dataclasses.fields(MatchResult)]
    assert names[:7] == ["agent_a", "agent_b", "wins_a", "draws", "wins_b", "avg_cheese_a", "avg_cheese_b"]
    for extra in ("simulations_a", "simulations_b", "nn_evals_a", "nn_evals_b", "terminals_a", "terminals_b",
                  "collisions_a", "collisions_b", "total_positions", "games"):
        assert extra in names, extra
    p = inspect.signature(play_match).parameters
    assert p["swap_sides"].default is True and p["keep_games"].default is False
    for name in ("width", "height", "cheese_count", "max_turns", "num_games"):
        assert p[name].default is inspect.Parameter.empty and p[name].kind is inspect.Parameter.KEYWORD_ONLY

    class Cfg:  # the attributes of RustMCTSConfig (alpharat/mcts/config.py:69-90)
        simulations, batch_size, c_puct, force_k, fpu_reduction = 500, 16, 0.512, 0.103, 0.459
        noise_epsilon, noise_concentration = 0.0, 10.83
        collision_limit_min, collision_limit_max, collision_scaling_start, collision_scaling_end = 1, 256, 800, 50000
        collision_scaling_power = 1.0

    a = MatchAgent.from_config(Cfg, checkpoint=None)
    assert (a.name, a.simulations, a.batch_size, a.c_puct, a.checkpoint) == ("mcts_500", 500, 16, 0.512, None)


def test_refusals_and_no_device(lib):
    import torch

    from alpharat_amd.match import MatchAgent, play_match

    # refusals come before any work, device or not
    with pytest.raises(ValueError, match="maze_type"):
        play_match(MatchAgent("a"), MatchAgent("b"), width=5, height=5, cheese_count=5, max_turns=30, num_games=2,
                   maze_type="hexagonal")
    with pytest.raises(ValueError, match="batch_size"):
        play_match(MatchAgent("a"), MatchAgent("b", batch_size=0), width=5, height=5, cheese_count=5, max_turns=30,
                   num_games=2)
    with pytest.raises(ValueError, match="256 cells"):
        play_match(MatchAgent("a"), MatchAgent("b"), width=20, height=20, cheese_count=5, max_turns=30, num_games=2)
    if not torch.cuda.is_available():  # in the GPU-less build container a valid match returns an error, never a result
        with pytest.raises(RuntimeError, match="no HIP device|hipGetDeviceCount"):
            play_match(MatchAgent("a", simulations=10), MatchAgent("b", simulations=20), width=5, height=5, cheese_count=5,
                       max_turns=30, num_games=2, seed=0)
