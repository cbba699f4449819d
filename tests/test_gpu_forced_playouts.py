"""GPU: forced playouts and policy target pruning of the self-play wave (k_step_forced, k_step_cap_forced, move_policy;
az_engine_set_forced_playouts).  Comparisons are bit for bit on the byte views of the arrays.

  1. whole az_engine_run waves are the host model's (tests/forced_playouts_model.py): state, pi, visits, z, meta, net_evals and both
     counters, on three boards, both tie modes, hash noise, a fractional temperature schedule, a ragged block and slot refill;
  2. the same waves with the playout cap on: fast plies force and prune nothing; the cap's counters too;
  3. the same games under 1, 2 and 4 slot groups;
  4. set_roots / search / root_readout / advance: root statistics after every search call, a readout's pi and action are what the
     advance that follows records, the visits stay raw; again on the inherited tree;
  5. a root with more than 16 children: a forced pick in the second round of 16 lanes;
  6. production noise on the HIP network: k = 1e-12 is the mode off bit for bit, k = 2 grows every root by exactly n_sim visits, every
     recorded pi sums to 1 and is 0 wherever visits is 0;
  7. off is off: on, off, run -- the samples and the graph replays of an engine that never had it on;
  8. every refusal, in both directions; the setter waits for an open search;
  9. one trainer iteration with selfplay_forced_playouts, alone and with selfplay_playout_cap.
(tests/test_forced_playouts_host.py checks on the model that every wave played here has forced picks, pruned playouts and a pruned pi.)
"""
import numpy as np
import pytest
import torch

import forced_playouts_model as F
import playout_cap_model as PC
from alphazero_amd import _lib
from alphazero_amd import engine as E
from alphazero_amd.games.othello import OthelloNet
from leaf_batch_model import make_board
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

TIES = {"lowest": E.TIE_LOWEST, "random": E.TIE_RANDOM}
KEYS = ("state", "pi", "visits", "z", "meta")
OFF = {"forced_picks": 0, "pruned_playouts": 0}
_CACHE = {}


def fake_engine(tag, tie, n_slots, n_sim=None, **kw):
    _, gid, H, W = F.GAMES[tag]
    kw.setdefault("node_capacity", 8192)
    kw.setdefault("sample_capacity", 4096)  # TicTacToe: 28 games of up to 9 plies on 20 slots outgrow the default
    return E.SelfPlayEngine(gid, H, W, n_slots=n_slots, n_sim=n_sim or F.N_SIMS[tag], evaluator=E.EVAL_FAKE, tie_mode=TIES[tie],
                            noise_mode=E.NOISE_HASH, dirichlet_alpha=F.NOISE[0], dirichlet_epsilon=F.NOISE[1], temp_max_step=F.TMAX,
                            temp_min_step=F.TMIN, seed=F.SEED, **kw)


def ordered(smp):
    """samples as numpy arrays sorted by (game id, move idx)"""
    a = {k: v.cpu().numpy() for k, v in smp.items()}
    order = np.lexsort((a["meta"][:, 1], a["meta"][:, 0]))
    return {k: v[order] for k, v in a.items()}


def same_rows(got, want, what, keys=KEYS):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


# ------------------------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("cap", [None, F.CAP], ids=["cap off", "cap on"])
@pytest.mark.parametrize("tie", ["lowest", "random"])
@pytest.mark.parametrize("tag", ["othello6", "connect4", "tictactoe"])
def test_a_wave_is_the_host_models(tag, tie, cap):
    want, ctr = F.wave(tag, tie, cap)
    eng = fake_engine(tag, tie, F.N_SLOTS)  # 20 slots: a full block and a ragged one; 28 games: 8 slots are refilled
    if cap is not None:
        eng.set_playout_cap(cap)
    eng.set_forced_playouts(F.K)
    got = ordered(eng.run(F.N_GAMES, first_game_id=F.FIRST))
    same_rows(got, want, (tag, tie, cap))
    st = eng.stats()
    assert eng.forced_playouts_stats() == {"forced_picks": ctr["forced_picks"], "pruned_playouts": ctr["pruned_playouts"]}
    assert (st["samples"], st["plies"], st["games_done"], st["net_evals"]) == (ctr["samples"], ctr["plies"], F.N_GAMES, ctr["rows"])
    if cap is None:
        assert eng.playout_cap_stats() == {"full_plies": 0, "fast_plies": 0}
    else:
        assert eng.playout_cap_stats() == {"full_plies": ctr["full_plies"], "fast_plies": ctr["fast_plies"]}
    assert st["error_flags"] == 0 and st["graph_replays"] > 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("cap", [None, F.CAP], ids=["cap off", "cap on"])
def test_slot_groups_play_the_same_games(cap):
    n_games = 56
    outs = []
    for n in (1, 2, 4):
        eng = fake_engine("othello6", "random", 48)  # three blocks: groups of 48 | 32 + 16 | 16 + 16 + 16 + 0
        if cap is not None:
            eng.set_playout_cap(cap)
        eng.set_forced_playouts(F.K)
        eng.set_groups(n)
        assert eng.groups() == n
        got = ordered(eng.run(n_games, first_game_id=F.FIRST))
        st = eng.stats()
        assert st["error_flags"] == 0 and st["games_done"] == n_games
        outs.append((got, {k: st[k] for k in ("samples", "plies", "net_evals", "games_done")}, eng.forced_playouts_stats(), eng.playout_cap_stats()))
        eng.close()
    for got, st, fs, cs in outs[1:]:
        same_rows(got, outs[0][0], "groups")
        assert st == outs[0][1] and fs == outs[0][2] and cs == outs[0][3]
    got, st, fs, cs = outs[0]
    assert fs["forced_picks"] > 0 and fs["pruned_playouts"] > 0
    # the first 28 of these games are the wave of test 1: a game depends on (seed, game id) only
    want, _ = F.wave("othello6", "random", cap)
    first = got["meta"][:, 0] < F.FIRST + F.N_GAMES
    same_rows({k: v[first] for k, v in got.items()}, want, "groups against the model")


# ------------------------------------------------------------------------------------------------------------------ 4
def _roots(n):
    """Othello 6x6 positions after 0 .. n - 1 seeded random moves, each at its own ply"""
    rng, out = np.random.default_rng(4), []
    for plies in range(n):
        b = make_board("othello", 6, 6)
        for _ in range(plies):
            moves = sorted(b.get_moves(), key=lambda m: cf.move_to_action("othello", m, 6))
            b.play_move(moves[int(rng.integers(len(moves)))])
        assert not b.is_game_over()
        out.append(b)
    return out


def _compare(eng, slot, m, what):
    a, N, Q, P, rootn = eng.root_children(slot)
    want = m.root_children()
    assert list(a) == [c[0] for c in want] and list(N) == [c[1] for c in want] and rootn == m.root.N, (what, list(N), [c[1] for c in want])
    assert np.array_equal(np.asarray(Q).view(np.int64), np.array([c[2] for c in want], np.float64).view(np.int64)), what
    assert np.array_equal(np.asarray(P).view(np.int64), np.array([c[3] for c in want], np.float64).view(np.int64)), what
    assert eng.nodes_used(slot) == m.node_count(), what


def _readout_is_the_models(eng, models, fulls, k):
    """root_readout's pi, action and visits against the model's move_policy under the mode; returns the readout as numpy"""
    ro = {key: v.cpu().numpy() for key, v in eng.root_readout().items() if key in ("pi", "action", "visits", "root_N")}
    pruned_rows = 0
    for s, (m, full) in enumerate(zip(models, fulls)):
        temp = PC.linear_temp(m.ply, F.TMAX, F.TMIN)
        idx, pi, cut = F.move_policy(m, temp, k if full else None)
        assert np.array_equal(ro["pi"][s].view(np.uint32), pi.view(np.uint32)), ("readout pi", s)
        assert int(ro["action"][s]) == m.root.children[idx].act, ("readout action", s)
        vis = np.zeros(m.A, np.int32)
        for c in m.root.children:
            vis[c.act] = c.N
        assert np.array_equal(ro["visits"][s], vis) and int(ro["root_N"][s]) == m.root.N  # raw counts
        pruned_rows += 1 if cut > 0 else 0
    return ro, pruned_rows


@pytest.mark.parametrize("cap", [None, F.CAP], ids=["cap off", "cap on"])
def test_the_finer_grained_api(cap):
    n = 10
    roots = _roots(n)
    gids, plies = 300 + np.arange(n), np.arange(n)  # plies 0 .. 9: temperatures 1, fractional and 0
    eng = fake_engine("othello6", "random", n, n_sim=12)
    if cap is not None:
        eng.set_playout_cap(cap)
    eng.set_forced_playouts(F.K)
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8), game_ids=gids.astype(np.uint32),
                  plies=plies.astype(np.int32))
    models = [F.ForcedModel(b, K=1, noise=None, tie="random", seed=F.SEED, game_id=int(g), ply=int(p)) for b, g, p in zip(roots, gids, plies)]
    fulls = [PC.is_full(cap, F.SEED, int(g), int(p)) for g, p in zip(gids, plies)]
    assert cap is None or 2 <= sum(fulls) <= 8, fulls
    total = dict(OFF)
    for round_ in range(2):  # fresh roots, then the roots the move left: inherited counts
        for sims in (9, 3, 7):
            eng.search(sims)
            for s, m in enumerate(models):
                assert F.search_call(m, sims, F.K, cap, F.NOISE) is fulls[s]
                _compare(eng, s, m, ("search", round_, sims, s))
        assert sum(m.picks for m in models) > 0
        assert eng.forced_playouts_stats() == total  # a ply's picks are folded in by its move only
        ro, pruned_rows = _readout_is_the_models(eng, models, fulls, F.K)
        assert pruned_rows > 0
        before = eng.stats()["samples"]
        eng.advance()
        got = {k: v.cpu().numpy()[before:] for k, v in eng.samples().items()}  # this ply's rows
        rows = {int(g): i for i, g in enumerate(got["meta"][:, 0].view(np.uint32))}
        assert sorted(rows) == [int(g) for g, f in zip(gids, fulls) if f]
        picks = cut = 0
        for s, (m, full) in enumerate(zip(models, fulls)):
            smp, p, c = F.advance(m, F.TMAX, F.TMIN, full, F.K)
            picks, cut = picks + p, cut + c
            if not full:
                assert smp is None
                continue
            i = rows[int(gids[s])]
            for k in ("state", "pi", "visits", "meta"):
                same_rows({k: got[k][i]}, {k: np.asarray(smp[k]).reshape(got[k][i].shape)}, ("advance", round_, s, k), keys=(k,))
            # what the readout showed is what the advance recorded and played
            assert np.array_equal(got["pi"][i].view(np.uint32), ro["pi"][s].view(np.uint32)) and int(got["meta"][i, 3]) == int(ro["action"][s])
            assert np.array_equal(got["visits"][i], ro["visits"][s])
        assert picks > 0 and cut > 0
        total = {"forced_picks": total["forced_picks"] + picks, "pruned_playouts": total["pruned_playouts"] + cut}
        assert eng.forced_playouts_stats() == total
        fulls = [PC.is_full(cap, F.SEED, int(g), m.ply) for g, m in zip(gids, models)]
        assert not any(m.root.board.is_game_over() for m in models)
    assert eng.stats()["error_flags"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5
MANY_MOVES = np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                       [0, -1, -1, -1, 1, -1, -1, 0],
                       [0, 1, 1, 0, -1, 1, 0, 1],
                       [0, -1, -1, 1, 0, 0, -1, 0],
                       [0, 0, 1, 0, 1, 0, -1, 0],
                       [0, -1, 0, 0, -1, 1, 1, 1],
                       [0, -1, -1, 0, -1, 1, -1, 0],
                       [0, -1, 1, 0, 0, 0, 0, 0]], np.int8)  # Othello 8x8: 34 legal moves for player +1


@pytest.mark.parametrize("tie", ["lowest", "random"])
def test_a_root_with_more_than_16_children(tie):
    sims = 150
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=2, n_sim=sims, dirichlet_alpha=F.NOISE[0], dirichlet_epsilon=F.NOISE[1], temp_max_step=2, temp_min_step=7,
                           tie_mode=TIES[tie], noise_mode=E.NOISE_HASH, evaluator=E.EVAL_FAKE, seed=3, node_capacity=1 << 15)
    eng.set_forced_playouts(F.K)
    eng.set_roots(np.stack([MANY_MOVES, MANY_MOVES]), np.array([1, 1], np.int8), game_ids=np.array([5, 6], np.uint32))
    eng.search(sims)
    models = []
    for slot, gid in enumerate((5, 6)):
        m = F.ForcedModel(make_board("othello", 8, 8, grid=MANY_MOVES, player=1), K=1, noise=None, tie=tie, seed=3, game_id=gid)
        F.search_call(m, sims, F.K, None, F.NOISE)
        assert len(m.root.children) == 34
        assert m.high_picks > 0, "the model never took a forced pick of a child in the second or third round of 16 lanes"
        _compare(eng, slot, m, ("wide root", tie, slot))
        models.append(m)
    _readout_is_the_models(eng, models, [True, True], F.K)
    eng.advance()
    want = [F.advance(m, 2, 7, True, F.K) for m in models]
    assert eng.forced_playouts_stats() == {"forced_picks": sum(w[1] for w in want), "pruned_playouts": sum(w[2] for w in want)}
    assert eng.stats()["error_flags"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6
N_SIM_NET = 12


def othello6_net():
    if "net" not in _CACHE:
        net = OthelloNet(6, device="cuda")
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.tensor(v) for k, v in cf.closed_form_state_dict(shapes).items()})
        net.eval()
        _CACHE["net"] = net.to_hip(max_batch=64)
    return _CACHE["net"]


def net_run(k, n_games=32, seed=23):
    """32 games on 20 slots of a production engine (Philox Dirichlet noise, random ties, the HIP network)"""
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=20, n_sim=N_SIM_NET, net=othello6_net(), seed=seed, node_capacity=8192)
    if k is not None:
        eng.set_forced_playouts(k)
    got = ordered(eng.run(n_games, first_game_id=50))
    st, fs = eng.stats(), eng.forced_playouts_stats()
    assert st["error_flags"] == 0 and st["games_done"] == n_games
    eng.close()
    return got, st, fs


def test_production_noise_on_the_network():
    off, st_off, fs_off = net_run(None)
    assert fs_off == OFF
    tiny, st, fs = net_run(1e-12)  # the forced kernels and the pruning pass, with nothing to force and nothing to prune
    same_rows(tiny, off, "k = 1e-12")
    assert fs == OFF and (st["samples"], st["plies"], st["net_evals"]) == (st_off["samples"], st_off["plies"], st_off["net_evals"])
    got, st, fs = net_run(F.K)
    assert fs["forced_picks"] > 0 and fs["pruned_playouts"] > 0 and st["samples"] == st["plies"] == len(got["z"])
    meta, vsum = got["meta"], got["visits"].sum(axis=1)
    # every root grows by exactly n_sim visits: a fresh root (ply 0) holds n_sim; a root that was the child played on the ply before
    # had visits[action] there, one of them its own evaluation, and inherits visits[action] - 1
    for i in range(len(vsum)):
        g, p = int(meta[i, 0]), int(meta[i, 1])
        if p == 0:
            assert vsum[i] == N_SIM_NET, (g, p)
        else:
            assert meta[i - 1, 0] == g and meta[i - 1, 1] == p - 1
            assert vsum[i] == N_SIM_NET + got["visits"][i - 1, meta[i - 1, 3]] - 1, (g, p)
    # a recorded pi: every entry is a double p_i rounded to float32 (off by at most p_i 2^-24) and the p_i sum to 1 within a few
    # 2^-53, so the float32 row sums to 1 within 2^-23; pruning takes playouts away and never adds: 0 wherever visits is 0
    assert np.all(np.abs(got["pi"].astype(np.float64).sum(axis=1) - 1.0) <= 2.0 ** -23)
    assert np.all(got["pi"][got["visits"] == 0] == 0.0)
    assert np.any((got["pi"] == 0.0) & (got["visits"] > 0))  # and some visited child was pruned away


# ------------------------------------------------------------------------------------------------------------------ 7
def test_off_is_off():
    outs = []
    for detour in (False, True):
        eng = fake_engine("othello6", "random", F.N_SLOTS)
        if detour:
            eng.set_forced_playouts(F.K)
            eng.set_forced_playouts(F.K)  # the same setting again: nothing to do
            eng.set_forced_playouts(8)
            eng.set_forced_playouts(None)
            eng.set_forced_playouts(None)
        got = {k: v.cpu().numpy() for k, v in eng.run(F.N_GAMES, first_game_id=F.FIRST).items()}  # unsorted: the same launches, the same order
        st = eng.stats()
        assert eng.forced_playouts_stats() == OFF and st["samples"] == st["plies"]
        outs.append((got, st))
        eng.close()
    same_rows(outs[1][0], outs[0][0], "on, off, run")
    for k in ("samples", "plies", "net_evals", "lockstep_iters", "graph_replays", "games_done", "max_nodes_used"):
        assert outs[1][1][k] == outs[0][1][k], k
    assert outs[0][1]["graph_replays"] > 0


# ------------------------------------------------------------------------------------------------------------------ 8
def test_the_setter_waits_for_an_open_search():
    eng = fake_engine("othello6", "random", 4)
    b = make_board("othello", 6, 6)
    eng.set_roots(np.tile(b.grid.astype(np.int8)[None], (4, 1, 1)), np.full(4, b.player, np.int8))
    eng.search_begin(4)
    for k in (F.K, None):
        with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_set_forced_playouts: a search begun"):
            eng.set_forced_playouts(k)
    with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_forced_playouts_stats"):
        eng.forced_playouts_stats()
    eng.search_end()
    eng.set_forced_playouts(F.K)
    eng.search_begin(4)
    eng.search_end()
    assert eng.stats()["error_flags"] == 0
    eng.close()


def test_refusals_name_the_mode():
    eng = fake_engine("othello6", "random", 4)
    L = _lib.lib()
    for bad in (-1.0, 64.5, float("inf"), float("nan")):
        assert L.az_engine_set_forced_playouts(eng.h, bad) == _lib.AZ_EINVAL
        assert b"k must be finite and in [0, 64]" in L.az_last_error()
    eng.set_forced_playouts(64)
    eng.set_forced_playouts(None)
    eng.set_leaf_batch(2)
    with pytest.raises(ValueError, match=r"forced playouts are not served for leaf_batch > 1"):
        eng.set_forced_playouts(F.K)
    eng.set_leaf_batch(1)
    eng.set_gumbel(8)
    with pytest.raises(ValueError, match=r"forced playouts are not served for the Gumbel search"):
        eng.set_forced_playouts(F.K)
    eng.set_gumbel(None)
    eng.set_forced_playouts(F.K)  # and the other way round, while the mode is on
    with pytest.raises(ValueError, match=r"az_engine_set_leaf_batch: forced playouts are on"):
        eng.set_leaf_batch(2)
    with pytest.raises(ValueError, match=r"az_engine_set_gumbel: forced playouts are on"):
        eng.set_gumbel(8)
    eng.set_leaf_batch(1)
    eng.set_gumbel(None)
    eng.set_playout_cap(F.CAP)   # the playout cap combines, in either order
    eng.set_playout_cap(None)
    eng.close()
    net = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=N_SIM_NET, net=othello6_net(), seed=1)
    for sym, name in (("all", "the symmetry ensemble"), ("random", "the random symmetry mode")):
        net.set_symmetry(sym)
        with pytest.raises(ValueError, match=f"forced playouts are not served for {name}"):
            net.set_forced_playouts(F.K)
        net.set_symmetry(None)
    net.set_forced_playouts(F.K)
    with pytest.raises(ValueError, match=r"az_engine_set_symmetry: forced playouts are on"):
        net.set_symmetry("all")
    with pytest.raises(ValueError, match=r"az_engine_set_symmetry_random: forced playouts are on"):
        net.set_symmetry("random")
    net.close()
    for ev, name in ((E.EVAL_ROLLOUT, "AZ_EVAL_ROLLOUT"), (E.EVAL_EXTERNAL, "AZ_EVAL_EXTERNAL")):
        other = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=N_SIM_NET, evaluator=ev, seed=1)
        with pytest.raises(ValueError, match=f"forced playouts are not served for .*{name}"):
            other.set_forced_playouts(F.K)
        other.set_forced_playouts(None)  # off stays off everywhere
        other.close()


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("cap", [None, (4, 0.4)], ids=["alone", "with the playout cap"])
def test_one_trainer_iteration(tmp_path, cap):
    from alphazero_amd import base
    from alphazero_amd.games.othello import OthelloConfig
    from alphazero_amd.trainer import AlphaZeroTrainer
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    tr = AlphaZeroTrainer(verbose=False, engine_slots=16, seed=6, materialize_memory=True, selfplay_forced_playouts=2, selfplay_playout_cap=cap)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=8, episodes=16, epochs=1, batch_size=16, iterations=1, do_eval=False, device="cuda")
    torch.manual_seed(3)
    tr.setup()
    tr.self_play(0)
    fs, cs = tr._engine.forced_playouts_stats(), tr._engine.playout_cap_stats()
    got = {k: v.cpu().numpy() for k, v in tr.device_samples.items()}
    assert fs["forced_picks"] > 0 and fs["pruned_playouts"] > 0 and len(got["z"]) == tr._engine.stats()["samples"]
    assert (cs["fast_plies"] > 0) == (cap is not None)
    c = tr.config
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=16, n_sim=8, net=tr._hipnet, dirichlet_alpha=c.dirichlet_alpha, dirichlet_epsilon=c.dirichlet_epsilon,
                           temp_max_step=c.temp_max_step, temp_min_step=c.temp_min_step, seed=6, max_plies=72, sample_capacity=16 * 72)
    if cap is not None:
        eng.set_playout_cap(cap)
    eng.set_forced_playouts(2)
    want = ordered(eng.run(16, first_game_id=0))
    assert eng.forced_playouts_stats() == fs and eng.playout_cap_stats() == cs
    eng.set_forced_playouts(None)  # and the wave without the mode records other targets
    plain = ordered(eng.run(16, first_game_id=0))
    eng.close()
    same_rows(got, want, "trainer")
    assert plain["pi"].shape != want["pi"].shape or not np.array_equal(plain["pi"], want["pi"])
    tr.optimize_network(0)
    tr.update_network(0)
    assert tr.loss_values[0] and tr.sgd_backend_used is not None
