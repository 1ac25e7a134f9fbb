"""Head-to-head matches between two agents, played on the MI355X from the first move to the last.

The reference plays evaluation games on the CPU: ``alpharat/eval/tournament.py:329-373`` runs one game per worker
through ``alpharat/eval/game.py:47-87`` ``play_game``, whose agents (``alpharat/ai/searcher_agent.py:40-56``) search the
position on a fresh tree and sample their move from the policy of their side. ``play_match`` is that loop for two
agents over ``num_games`` games as ONE device run (``ar_match_run``): both agents' searches, the action samples and
the game steps stay on the device; the host only drains finished games.

Agent A plays P1 in even games and, with ``swap_sides``, P2 in odd ones (tournament.py:397). Each agent draws from
its own random stream per game (``seed + game index``), which continues from move to move.

Besides search agents there are the baselines of the reference's benchmark (``alpharat/eval/benchmark.py:78-125``):
``MatchAgent.random`` (``ai/random_agent.py``), ``MatchAgent.greedy`` (``ai/greedy_agent.py``) and ``MatchAgent.nn``
(``ai/config.py:88-106``: the network's policy alone, sampled at a temperature). ``standard_agents`` builds the
benchmark's set and ``play_round_robin`` plays every pair of a set; ratings and tables are left to the caller.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any

import numpy as np

from . import _lib

_KINDS = {"search": _lib.AR_AGENT_SEARCH, "random": _lib.AR_AGENT_RANDOM, "greedy": _lib.AR_AGENT_GREEDY}
_SEARCH_FIELDS = ("c_puct", "fpu_reduction", "force_k", "noise_epsilon", "noise_concentration", "collision_limit_min",
                  "collision_limit_max", "collision_scaling_start", "collision_scaling_end", "collision_scaling_power")


@dataclass
class MatchAgent:
    """One side of a match: a name, an evaluator (``checkpoint``: a ``.pt`` / ``.arnet`` path, None = smart-uniform
    priors), the search arguments of ``HipSearcher`` and the base of its per-game random streams. ``kind`` is
    ``"search"``, ``"random"`` or ``"greedy"``; the last two take no checkpoint and ignore the search arguments.
    ``temperature`` (search agents) is that of ``ai/utils.py:8-40``: 1.0 samples the policy, 0.0 takes its argmax."""

    name: str
    checkpoint: str | Path | None = None
    simulations: int = 100
    batch_size: int = 8
    c_puct: float = 1.5
    fpu_reduction: float = 0.2
    force_k: float = 2.0
    noise_epsilon: float = 0.0
    noise_concentration: float = 10.83
    collision_limit_min: int = 1
    collision_limit_max: int = 256
    collision_scaling_start: int = 800
    collision_scaling_end: int = 50_000
    collision_scaling_power: float = 1.0
    seed: int = 0
    kind: str = "search"
    temperature: float = 1.0

    @classmethod
    def random(cls, name: str = "random", seed: int = 0) -> "MatchAgent":
        """``RandomAgent``: a uniform draw over the five actions at every move."""
        return cls(name=name, kind="random", seed=seed)

    @classmethod
    def greedy(cls, name: str = "greedy") -> "MatchAgent":
        """``GreedyAgent``: the first step of the cheapest path to the nearest cheese."""
        return cls(name=name, kind="greedy")

    @classmethod
    def nn(cls, checkpoint: str | Path, temperature: float = 0.0, name: str | None = None, seed: int = 0) -> "MatchAgent":
        """``NNAgentConfig``: the network's policy without a search. One simulation on a fresh tree evaluates the root
        and visits no child, so the search returns the network's prior on the position's outcomes."""
        return cls(name=name if name is not None else "nn", checkpoint=checkpoint, simulations=1, batch_size=1,
                   noise_epsilon=0.0, seed=seed, temperature=temperature)

    @classmethod
    def from_config(cls, mcts_config: Any, checkpoint: str | Path | None = None, name: str | None = None,
                    seed: int = 0) -> "MatchAgent":
        """From a ``RustMCTSConfig`` (``alpharat/mcts/config.py:69-90``) or anything with the same attributes, as
        ``HipSearcher.from_config``. The temperature is 1.0 (searcher_agent.py:53-54)."""
        kw = {n: getattr(mcts_config, n) for n in ("simulations", "batch_size") + _SEARCH_FIELDS}
        return cls(name=name if name is not None else f"mcts_{kw['simulations']}", checkpoint=checkpoint, seed=seed, **kw)

    def _weights(self) -> bytes | None:
        if self.checkpoint is None:
            return None
        cp = Path(self.checkpoint)
        if cp.suffix != ".arnet":
            from .weights import checkpoint_to_blob

            cp = checkpoint_to_blob(cp)
        return str(cp).encode()

    def _c(self) -> _lib.ArMatchAgent:
        if self.kind not in _KINDS:
            raise ValueError(f"agent {self.name!r}: unknown kind {self.kind!r} (one of {', '.join(_KINDS)})")
        cfg = _lib.ArSearchConfig(*[getattr(self, n) for n in _SEARCH_FIELDS])
        return _lib.ArMatchAgent(self._weights(), int(self.simulations), int(self.batch_size), cfg,
                                 int(self.seed) & 0xFFFFFFFFFFFFFFFF, _KINDS[self.kind], float(self.temperature))


@dataclass
class MatchResult:
    """``MatchupResult`` of the reference (tournament.py:61-72) plus the search counters of both agents."""

    agent_a: str
    agent_b: str
    wins_a: int
    draws: int
    wins_b: int
    avg_cheese_a: float
    avg_cheese_b: float
    # extensions
    total_games: int = 0
    total_positions: int = 0
    simulations_a: int = 0
    simulations_b: int = 0
    nn_evals_a: int = 0
    nn_evals_b: int = 0
    terminals_a: int = 0
    terminals_b: int = 0
    collisions_a: int = 0
    collisions_b: int = 0
    elapsed_secs: float = 0.0
    games: list[dict] = field(default_factory=list)  # keep_games=True: one record per game, in finishing order

    @property
    def games_per_second(self) -> float:
        return self.total_games / self.elapsed_secs if self.elapsed_secs > 0 else 0.0


def _arr(ptr, shape, dtype):
    n = int(np.prod(shape))
    if n == 0:
        return np.zeros(shape, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True).reshape(shape)


def _search_to_dict(v: _lib.ArMatchSearchView, n: int) -> dict:
    d = {k: _arr(getattr(v, k), (n, 5), np.float32) for k in ("policy_p1", "policy_p2", "visit_counts_p1",
                                                              "visit_counts_p2", "prior_p1", "prior_p2")}
    d.update({k: _arr(getattr(v, k), (n,), np.float32) for k in ("value_p1", "value_p2")})
    d.update({k: _arr(getattr(v, k), (n,), np.uint32) for k in ("total_visits", "nn_evals", "terminals", "collisions")})
    return d


def match_record_to_dict(v: _lib.ArMatchGameView) -> dict:
    """Copy one finished game out of the sink callback (the view dies when the callback returns)."""
    n, hw = int(v.n_positions), int(v.width) * int(v.height)
    return dict(
        width=int(v.width), height=int(v.height), max_turns=int(v.max_turns), game_index=int(v.game_index), n=n,
        a_is_p1=bool(v.a_is_p1), result=int(v.result), final_p1_score=float(v.final_p1_score),
        final_p2_score=float(v.final_p2_score),
        p1_pos=_arr(v.p1_pos, (n, 2), np.uint8), p2_pos=_arr(v.p2_pos, (n, 2), np.uint8),
        p1_score=_arr(v.p1_score, (n,), np.float32), p2_score=_arr(v.p2_score, (n,), np.float32),
        p1_mud=_arr(v.p1_mud, (n,), np.uint8), p2_mud=_arr(v.p2_mud, (n,), np.uint8), turn=_arr(v.turn, (n,), np.uint16),
        cheese_mask=_arr(v.cheese_mask, (n, hw), np.uint8),
        action_p1=_arr(v.action_p1, (n,), np.uint8), action_p2=_arr(v.action_p2, (n,), np.uint8),
        a=_search_to_dict(v.a, n), b=_search_to_dict(v.b, n),
    )


def play_match(agent_a: MatchAgent, agent_b: MatchAgent, *, width: int, height: int, cheese_count: int, max_turns: int,
               num_games: int, swap_sides: bool = True, cheese_symmetric: bool = True, maze_type: str = "open",
               positions: str = "corners", wall_density: float = 0.7, mud_density: float = 0.1,
               maze_symmetric: bool = True, seed: int | None = None, first_game_index: int = 0,
               concurrent_games: int = 0, device: str = "auto", device_index: int | None = None,
               keep_games: bool = False, on_game: Any = None) -> MatchResult:
    """Play ``num_games`` games of ``agent_a`` against ``agent_b`` on one MI355X. Game arguments are those of
    ``rust_self_play``; ``seed`` fixes the games (``seed + index``) and, with the agents' own ``seed``, every draw --
    ``seed=None`` takes entropy for all of them, as the reference does. ``keep_games=True`` returns every game's
    record (positions, both actions and both agents' search outputs as numpy arrays) in ``MatchResult.games``;
    ``on_game(record)`` receives them as they finish."""
    L = _lib.load()
    if device_index is None:
        device_index = int(os.environ.get("LOCAL_RANK", "0")) if device in ("auto", "hip") else 0
    enc = lambda s: None if s is None else str(s).encode()  # noqa: E731
    p = _lib.ArMatchParams(
        width, height, cheese_count, max_turns, int(cheese_symmetric), enc(maze_type), enc(positions), wall_density,
        mud_density, int(maze_symmetric), num_games, first_game_index, int(seed is not None),
        (seed or 0) & 0xFFFFFFFFFFFFFFFF, int(swap_sides), concurrent_games, enc(device), device_index,
        agent_a._c(), agent_b._c())
    games: list[dict] = []
    sink = _lib.ArMatchSink()
    if keep_games or on_game is not None:
        def _sink(_u, v):
            rec = match_record_to_dict(v.contents)
            if keep_games:
                games.append(rec)
            if on_game is not None:
                on_game(rec)

        sink = _lib.ArMatchSink(_sink)
    out = _lib.ArMatchStats()
    _lib.check(L.ar_match_run(C.byref(p), sink, None, C.byref(out)))
    n = max(int(out.total_games), 1)
    return MatchResult(
        agent_a=agent_a.name, agent_b=agent_b.name, wins_a=int(out.wins_a), draws=int(out.draws), wins_b=int(out.wins_b),
        avg_cheese_a=float(out.cheese_a) / n, avg_cheese_b=float(out.cheese_b) / n, total_games=int(out.total_games),
        total_positions=int(out.total_positions), simulations_a=int(out.simulations_a), simulations_b=int(out.simulations_b),
        nn_evals_a=int(out.nn_evals_a), nn_evals_b=int(out.nn_evals_b), terminals_a=int(out.terminals_a),
        terminals_b=int(out.terminals_b), collisions_a=int(out.collisions_a), collisions_b=int(out.collisions_b),
        elapsed_secs=float(out.elapsed_secs), games=games)


def standard_agents(checkpoint: str | Path, mcts_config: Any, baseline_checkpoint: str | Path | None = None,
                    seed: int = 0) -> dict[str, MatchAgent]:
    """The agent set of ``build_standard_agents`` (benchmark.py:78-125) under its names: ``random``, ``greedy``, ``mcts``
    (the search without a network), ``nn`` (the network alone, temperature 1.0), ``mcts+nn``, and ``nn-prev`` /
    ``mcts+nn-prev`` for a ``baseline_checkpoint``. Dirichlet noise is stripped (``for_evaluation()``); every agent's
    stream base is ``seed`` plus its own offset, so no two agents share a stream."""
    import dataclasses

    def base(k: int) -> int:
        return (int(seed) + (k << 40)) & 0xFFFFFFFFFFFFFFFF

    def searcher(name: str, cp, k: int) -> MatchAgent:
        return dataclasses.replace(MatchAgent.from_config(mcts_config, checkpoint=cp, name=name, seed=base(k)), noise_epsilon=0.0)

    agents = {
        "random": MatchAgent.random(seed=base(1)),
        "greedy": dataclasses.replace(MatchAgent.greedy(), seed=base(0)),  # (a greedy agent draws nothing)
        "mcts": searcher("mcts", None, 2),
        "nn": MatchAgent.nn(checkpoint, temperature=1.0, name="nn", seed=base(3)),
        "mcts+nn": searcher("mcts+nn", checkpoint, 4),
    }
    if baseline_checkpoint is not None:
        agents["nn-prev"] = MatchAgent.nn(baseline_checkpoint, temperature=1.0, name="nn-prev", seed=base(5))
        agents["mcts+nn-prev"] = searcher("mcts+nn-prev", baseline_checkpoint, 6)
    return agents


def play_round_robin(agents: dict[str, MatchAgent], *, games_per_matchup: int, **game_and_run_arguments: Any
                     ) -> dict[tuple[str, str], MatchResult]:
    """One ``play_match`` per unordered pair of ``agents``, pairs in insertion order, ``games_per_matchup`` games each
    with ``swap_sides=True``; every pair plays the same games (the arguments of ``play_match`` are passed on as they
    are). Returns ``{(name_a, name_b): MatchResult}``."""
    for k in ("num_games", "swap_sides"):
        if k in game_and_run_arguments:
            raise TypeError(f"play_round_robin sets {k} itself")
    names = list(agents)
    out: dict[tuple[str, str], MatchResult] = {}
    for i, na in enumerate(names):
        for nb in names[i + 1:]:
            out[(na, nb)] = play_match(agents[na], agents[nb], num_games=games_per_matchup, swap_sides=True,
                                       **game_and_run_arguments)
    return out
