"""GPU: one engine walked through every kernel family of the search plan (alphazero_amd/csrc/az_search_plan.h):
plain -> playout cap -> cap + forced playouts -> forced playouts -> off -> Gumbel -> Gumbel full -> Gumbel with 2 walkers -> off ->
leaf_batch 4 -> plain.  After every switch a wave of az_engine_run is, bit for bit, the wave of a fresh engine created directly in
that mode: samples, lock-steps and graph replays.  A plan left over from the mode before, or a graph key shared by two families,
launches the other family's kernels and breaks this.  The fake evaluator, as in the whole-wave tests of every mode's own file."""
import numpy as np
import pytest

from alphazero_amd import engine as E

pytestmark = pytest.mark.gpu

N_SLOTS, N_SIM, N_GAMES = 32, 8, 40  # two blocks of slots; 8 slots are refilled
CAP, K_FORCED, M = (3, 0.5), 2.0, 4
KEYS = ("state", "pi", "visits", "z", "meta")
OFF = dict(cap=None, forced=None, gumbel=None, full=False, gumbel_batch=1, leaf_batch=1)
WALK = [("plain", {}), ("playout cap", {"cap": CAP}), ("cap + forced", {"cap": CAP, "forced": K_FORCED}), ("forced", {"forced": K_FORCED}),
        ("off", {}), ("gumbel", {"gumbel": M}), ("gumbel full", {"gumbel": M, "full": True}),
        ("gumbel batch 2", {"gumbel": M, "full": True, "gumbel_batch": 2}), ("off again", {}), ("leaf_batch 4", {"leaf_batch": 4}),
        ("plain again", {})]


def switch(eng, now, to):
    """from mode `now` to mode `to`: what goes off first (the setters refuse the combinations), then what comes on"""
    off_first = [k for k in OFF if now[k] != to[k] and to[k] == OFF[k]]
    for k in off_first + [k for k in OFF if now[k] != to[k] and k not in off_first]:
        {"cap": eng.set_playout_cap, "forced": eng.set_forced_playouts, "gumbel": eng.set_gumbel, "full": eng.set_gumbel_full,
         "gumbel_batch": eng.set_gumbel_batch, "leaf_batch": eng.set_leaf_batch}[k](to[k])


def wave(eng):
    """one run's samples sorted by (game id, move idx), its lock-steps and the graph replays it added"""
    before = eng.stats()["graph_replays"]
    a = {k: v.cpu().numpy() for k, v in eng.run(N_GAMES, first_game_id=5).items()}
    order = np.lexsort((a["meta"][:, 1], a["meta"][:, 0]))
    st = eng.stats()
    assert st["error_flags"] == 0 and st["games_done"] == N_GAMES
    return {k: v[order] for k, v in a.items()}, {"lockstep_iters": st["lockstep_iters"], "graph_replays": st["graph_replays"] - before,
                                                  "net_evals": st["net_evals"], "plies": st["plies"], "samples": st["samples"]}


def engine():
    return E.SelfPlayEngine(0, 4, 4, n_slots=N_SLOTS, n_sim=N_SIM, evaluator=E.EVAL_FAKE, seed=11, node_capacity=4096)


def test_a_walk_through_the_families_plays_each_modes_own_waves():
    walked, now, seen = engine(), dict(OFF), {}
    for name, mode in WALK:
        to = {**OFF, **mode}
        switch(walked, now, to)
        now = to
        got, st = wave(walked)
        fresh = engine()
        switch(fresh, dict(OFF), to)
        want, st_fresh = wave(fresh)
        fresh.close()
        for k in KEYS:
            assert got[k].shape == want[k].shape, (name, k)
            assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (name, k)
        assert st == st_fresh, name
        assert st["graph_replays"] > 0, name
        seen[name] = (got, st)
    walked.close()
    # the walk did change what is played: the modes' waves differ from the plain one, and coming back is the plain one again
    plain = seen["plain"]
    for name in ("off", "off again", "plain again"):
        assert seen[name][1] == plain[1] and all(np.array_equal(seen[name][0][k], plain[0][k]) for k in KEYS), name
    for name in ("playout cap", "cap + forced", "forced", "gumbel", "gumbel full", "gumbel batch 2", "leaf_batch 4"):
        assert seen[name][1] != plain[1] or any(not np.array_equal(seen[name][0][k], plain[0][k]) for k in KEYS), name
