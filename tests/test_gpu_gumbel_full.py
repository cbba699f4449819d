"""GPU: the full Gumbel search (az_engine_set_gumbel_full) -- every evaluated node keeps its network value, v_mix is
the paper's at the root and below, and below the root the child is chosen deterministically by pi' - N / (1 + sum N).

  1. the engine equals the host model of the contract (tests/gumbel_full_model.py) bit for bit: root children, considered set, move,
     pi', visits, node count, collisions, network rows, lock-steps and the root's stored value -- over n_sim x m x K at gumbel_batch
     1 (k_step_gumbel) and above (k_step_gumbel_multi), through a move and a second search on the subtree the re-rooting kept (the
     values travelled with their nodes), several searches on one root, grown pools, the HIP network, a random symmetry;
  2. the self-play wave does not depend on slot count or refill and equals the model game by game; no draw is made below the root;
  3. off is off: an untouched engine, the switch set to False and a detour through True are the same bits and the same graph
     replays, with the Gumbel mode on and with it off; replayed graphs equal plain launches; refusals;
  4. the players and the trainer carry the option.
"""
from unittest import mock

import numpy as np
import pytest
import torch

from alphazero_amd import _lib, base
from alphazero_amd import engine as E
from alphazero_amd import gumbel as G
from alphazero_amd.games.othello import OthelloBoard, OthelloConfig, OthelloNet
from alphazero_amd.mcts import MCT
from alphazero_amd.players import BatchedAlphaZeroPlayer
from alphazero_amd.trainer import AlphaZeroTrainer
from gumbel_batch_model import wide_root
from gumbel_full_model import GumbelFullModel
from gumbel_model import pass_position, playout
from leaf_batch_model import make_board
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

GAMES = {"othello8": ("othello", 0, 8, 8), "othello4": ("othello", 0, 4, 4), "connect4": ("connect4", 1, 6, 7),
         "tictactoe": ("tictactoe", 2, 3, 3)}
QUIET = dict(tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, dirichlet_alpha=None, dirichlet_epsilon=None)
FIXED = dict(temp_max_step=-1, temp_min_step=0, node_capacity=8192, **QUIET)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """the cached roots and networks go with the module: the tests that follow find the device memory as they would without this file"""
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def roots_of(tag):
    if tag not in _CACHE:
        game, _, H, W = GAMES[tag]
        rng = np.random.default_rng(17)
        if tag == "othello8":  # the start (4 children), the 18-child midgame root, a forced pass (m0 = 1)
            roots = [make_board(game, H, W), wide_root(16), pass_position(8)]
        elif tag == "tictactoe":
            roots = []
            while len(roots) < 4:  # from ply 4: terminal leaves, K above the child count
                b = playout(game, H, W, rng, int(rng.integers(4, 7)))
                if b is not None and all((b.grid != r.grid).any() for r in roots):
                    roots.append(b)
        else:
            roots = [make_board(game, H, W), playout(game, H, W, rng, 9)]
        _CACHE[tag] = roots
    return _CACHE[tag]


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def f32bits(x):
    return int(np.asarray(x, np.float32).reshape(1).view(np.uint32)[0])


def compare(eng, slot, m, ro, what):
    a, N, Q, P, rootn = eng.root_children(slot)
    want = m.root_children()
    assert list(a) == [c[0] for c in want], what
    assert list(N) == [c[1] for c in want], (what, list(N), [c[1] for c in want])
    assert rootn == m.root.N, what
    assert np.array_equal(bits(Q), bits([c[2] for c in want])), what
    assert np.array_equal(bits(P), bits([c[3] for c in want])), what
    assert eng.nodes_used(slot) == m.node_count(), what
    assert eng.considered(slot) == m.considered(), (what, eng.considered(slot), m.considered())
    if m.root.evaluated:
        assert f32bits(eng.root_value(slot)) == f32bits(m.root_value()), (what, eng.root_value(slot), m.root_value())
    else:
        with pytest.raises(_lib.AzError, match="has not been evaluated"):
            eng.root_value(slot)
    if want:
        assert int(ro["action"][slot]) == m.move(), what
        assert np.array_equal(ro["pi"][slot].view(np.uint32), m.policy().view(np.uint32)), what
        assert np.array_equal(ro["visits"][slot], m.visits()), what


def readout(eng):
    return {k: v.cpu().numpy() for k, v in eng.root_readout().items()}


def run_case(eng, roots, spec, K, n_sims, tie, seed, what, net=None, between=None):
    """set_roots -> the searches of n_sims -> move -> the same searches on the kept subtree, on the engine and on one model per slot;
    the engine's collisions, network rows and lock-step count follow the models and the contract"""
    eng.set_gumbel(spec)
    eng.set_gumbel_batch(K)
    eng.set_gumbel_full(True)
    gids = 100 + np.arange(len(roots))
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8), game_ids=gids.astype(np.uint32))
    models = [GumbelFullModel(b, K=K, tie=tie, seed=seed, game_id=int(g), net=net, **spec) for b, g in zip(roots, gids)]
    coll0, live = eng.collisions(), list(range(len(roots)))
    for stage in ("first", "second"):
        for n in n_sims:
            iters, before = eng.stats()["lockstep_iters"], [m.root.N for m in models]
            eng.search(n)
            ro = readout(eng)
            assert eng.stats()["lockstep_iters"] - iters == (G.locksteps(n, spec["m"], K) if K > 1 else n) + 1, (what, spec, K, n)
            for s in live:
                models[s].search(n)
                assert models[s].root.N == before[s] + n and len(models[s].plan) <= G.locksteps(n, spec["m"], K)
                compare(eng, s, models[s], ro, (what, spec, K, n, s, stage))
            if between is not None:
                between(eng)
        assert eng.collisions() - coll0 == sum(models[s].dups for s in range(len(roots))), (what, spec, K, stage)
        if stage == "first":
            eng.advance()
            assert eng.stats()["net_evals"] == sum(m.rows for m in models), (what, spec, K)
            for m in models:
                m.advance()
            live = [s for s in live if not models[s].root.board.is_game_over()]
            for s in live:
                assert eng.considered(s) == []  # k_move cleared it
                if models[s].root.evaluated:  # the value travelled with its node into the other pool
                    assert f32bits(eng.root_value(s)) == f32bits(models[s].root_value()), (what, spec, K, s)
    assert eng.stats()["error_flags"] == 0
    return models


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("tag", ["othello8", "tictactoe", "connect4"])
def test_engine_equals_the_model(tag, K):
    game, gid, H, W = GAMES[tag]
    roots = roots_of(tag)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=3, **FIXED)
    deep = 0
    for m in (4, 16):
        for n_sim in (5, 16, 50):
            models = run_case(eng, roots, {"m": m}, K, (n_sim,), "lowest", 3, tag)
            deep = max(deep, max(x.max_path for x in models))
    if tag == "othello8":
        assert len(roots[0].get_moves()) == 4 and len(roots[1].get_moves()) >= 16 and len(roots[2].get_moves()) == 1
    assert deep >= 3, "no walk went below the root's children: the non-root selection was not exercised"
    eng.close()


def test_two_and_three_searches_on_one_root_and_grown_pools():
    game, gid, H, W = GAMES["othello8"]
    roots = roots_of("othello8")
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=3, **FIXED)
    run_case(eng, roots, {"m": 4}, 1, (8, 8), "lowest", 3, "twice 8")
    run_case(eng, roots, {"m": 16}, 16, (5, 16, 3), "lowest", 3, "5, 16, 3")
    caps = iter((12288, 16384, 20480, 24576))
    run_case(eng, roots, {"m": 16}, 4, (16, 16), "lowest", 3, "grown pools", between=lambda e: e.grow_pools(next(caps)))
    assert eng.cfg.node_capacity == 24576
    eng.close()


def othello8_net():
    if "net" not in _CACHE:
        net = OthelloNet(8, device="cuda")
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.tensor(v) for k, v in cf.closed_form_state_dict(shapes).items()})
        net.eval()
        _CACHE["net"] = (net, net.to_hip(max_batch=64))
    return _CACHE["net"]


def test_the_network_path_equals_the_model_on_the_networks_outputs():
    _, hip = othello8_net()
    roots = roots_of("othello8")[:2]

    def net(grid, player, A):
        x = torch.tensor((player * np.asarray(grid)).astype(np.float32).reshape(1, -1), device="cuda")
        p, v = hip.forward(x)
        return p[0].cpu().numpy(), float(v[0].cpu())
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=len(roots), n_sim=16, net=hip, seed=9, **FIXED)
    run_case(eng, roots, {"m": 16}, 16, (16,), "lowest", 9, "hip network, K 16", net=net)
    run_case(eng, roots, {"m": 4}, 1, (16,), "lowest", 9, "hip network, K 1", net=net)
    eng.close()


def test_with_a_random_symmetry_the_draws_follow_the_game_not_the_slot():
    _, hip = othello8_net()
    roots = roots_of("othello8")
    grids, players = np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8)
    gids = np.array([7, 8, 9], np.uint32)
    for K in (1, 4):
        outs = []
        for order in (np.arange(3), np.arange(3)[::-1].copy()):
            eng = E.SelfPlayEngine(0, 8, 8, n_slots=3, n_sim=16, net=hip, seed=9, **FIXED)
            eng.set_symmetry("random")
            eng.set_gumbel(16)
            eng.set_gumbel_batch(K)
            eng.set_gumbel_full(True)
            eng.set_roots(grids[order], players[order], game_ids=gids[order])
            eng.search(16)
            ro = readout(eng)
            ro["value"] = np.array([eng.root_value(s) for s in range(3)], np.float32)
            eng.advance()
            eng.search(16)
            ro.update({k + "2": v for k, v in readout(eng).items()})
            outs.append({k: v[np.argsort(order)] for k, v in ro.items()})
            assert eng.stats()["error_flags"] == 0
            eng.close()
        for k in outs[0]:
            assert np.array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8)), (K, k)
        assert (outs[0]["root_N"] == 16).all()


# ------------------------------------------------------------------------------------------------------------------ 2
def sort_samples(d):
    d = {k: v.cpu().numpy() for k, v in d.items()}
    order = np.lexsort((d["meta"][:, 1], d["meta"][:, 0]))
    return {k: v[order] for k, v in d.items()}


@pytest.mark.parametrize("tag", ["tictactoe", "othello4"])
def test_wave_is_slot_independent_and_equals_the_model(tag):
    game, gid, H, W = GAMES[tag]
    n_sim, n_games, K = 16, 37, 4
    runs = []
    for slots in (37, 17, 5):  # groups on both sides of a 16-game block boundary; 5 and 17 refill
        eng = E.SelfPlayEngine(gid, H, W, n_slots=slots, n_sim=n_sim, evaluator=E.EVAL_FAKE, seed=5, node_capacity=8192,
                               sample_capacity=n_games * 40, **QUIET)
        eng.set_gumbel(16)
        eng.set_gumbel_batch(K)
        eng.set_gumbel_full(True)
        runs.append(sort_samples(eng.run(n_games, first_game_id=900)))
        st = eng.stats()
        assert st["games_done"] == n_games and st["error_flags"] == 0
        eng.close()
    for other in runs[1:]:
        for k in ("state", "pi", "z", "meta", "visits"):
            assert np.array_equal(other[k], runs[0][k]), k
    r = runs[0]
    assert (r["visits"].sum(1) >= n_sim).all()  # every root grew by n_sim; a kept subtree brings visits of its own
    for g in (900, 917, 936):
        rows = np.flatnonzero(r["meta"][:, 0] == g)
        rec, winner = GumbelFullModel(make_board(game, H, W), K=K, m=16, seed=5, game_id=g).play_game(n_sim)
        assert len(rows) == len(rec), g
        for i, (state, pi, vis, action, player) in zip(rows, rec):
            assert np.array_equal(r["state"][i], state) and r["meta"][i, 3] == action and r["meta"][i, 2] == player, (g, i)
            assert np.array_equal(r["pi"][i].view(np.uint32), pi.view(np.uint32)), (g, i)
            assert np.array_equal(r["visits"][i], vis), (g, i)
            assert r["z"][i] == winner * player, (g, i)


@pytest.mark.parametrize("K", [1, 4])
def test_no_draw_is_made_below_the_root(K):
    """tie_mode random and lowest give equal trees with the switch on (without it the random mode draws among equal PUCT scores)"""
    game, gid, H, W = GAMES["tictactoe"]
    outs = []
    for tie in (E.TIE_RANDOM, E.TIE_LOWEST):
        eng = E.SelfPlayEngine(gid, H, W, n_slots=17, n_sim=16, evaluator=E.EVAL_FAKE, seed=77, node_capacity=8192, sample_capacity=37 * 12,
                               **dict(QUIET, tie_mode=tie))
        eng.set_gumbel(4)
        eng.set_gumbel_batch(K)
        eng.set_gumbel_full(True)
        outs.append(sort_samples(eng.run(37, first_game_id=0)))
        assert eng.stats()["error_flags"] == 0
        eng.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


# ------------------------------------------------------------------------------------------------------------------ 3
def six_rounds(gumbel, before=None, after=None):
    """six search / move rounds of 37 games; `before` runs ahead of set_roots, `after` behind it (on fresh roots)"""
    game, gid, H, W = GAMES["othello8"]
    n, n_sim = 37, 24
    start = make_board(game, H, W)
    grids, players = np.tile(start.grid.astype(np.int8)[None], (n, 1, 1)), np.full(n, start.player, np.int8)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=n, n_sim=n_sim, evaluator=E.EVAL_FAKE, seed=21, node_capacity=8192)  # random ties, Philox noise
    if gumbel is not None:
        eng.set_gumbel(gumbel)
    if before is not None:
        before(eng)
    eng.set_roots(grids, players, game_ids=np.arange(500, 500 + n, dtype=np.uint32))
    if after is not None:
        after(eng)
    reads = []
    for _ in range(6):
        eng.search(n_sim)
        reads.append(readout(eng))
        eng.advance()
    smp = {k: v.cpu().numpy() for k, v in eng.samples().items()}
    st = eng.stats()
    assert st["graph_replays"] > 0 and st["error_flags"] == 0
    eng.close()
    return reads, smp, st


def same_rounds(a, b):
    for x, y in zip(a[0], b[0]):
        for k in y:
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), k
    for k in b[1]:
        assert np.array_equal(a[1][k], b[1][k]), k
    for k in ("net_evals", "lockstep_iters", "graph_replays", "plies", "samples"):
        assert a[2][k] == b[2][k], k


def detour(e):
    e.set_gumbel_full(True)
    e.set_gumbel_full(False)


@pytest.mark.parametrize("gumbel", [16, None])
def test_off_is_off(gumbel):
    ref = six_rounds(gumbel)
    same_rounds(six_rounds(gumbel, before=lambda e: e.set_gumbel_full(False)), ref)
    same_rounds(six_rounds(gumbel, after=detour), ref)
    if gumbel is None:
        # with the mode off the switch is accepted and not in force: the plain search, launch for launch, and no value is kept
        def on(e):
            e.set_gumbel_full(True)
            with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_root_value"):
                e.root_value(0)
        same_rounds(six_rounds(None, after=on), ref)
    else:
        # ... and in force it is another search, in either order of the setters
        a = six_rounds(16, after=lambda e: e.set_gumbel_full(True))

        def early(e):
            e.set_gumbel(None)
            e.set_gumbel_full(True)
            e.set_gumbel(16)
        same_rounds(six_rounds(16, before=early), a)
        assert any(not np.array_equal(x["visits"], y["visits"]) for x, y in zip(a[0], ref[0]))
        assert a[2]["lockstep_iters"] == ref[2]["lockstep_iters"] == 6 * 25


@pytest.mark.parametrize("K", [1, 4])
def test_replayed_graphs_of_the_mode_equal_plain_launches(monkeypatch, K):
    game, gid, H, W = GAMES["othello4"]
    outs = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("AZ_ENGINE_GRAPHS", graphs)  # read when an engine is created
        eng = E.SelfPlayEngine(gid, H, W, n_slots=17, n_sim=16, evaluator=E.EVAL_FAKE, seed=5, node_capacity=8192, sample_capacity=37 * 40)
        eng.set_gumbel(4)
        eng.set_gumbel_batch(K)
        eng.set_gumbel_full(True)
        outs.append(sort_samples(eng.run(37, first_game_id=0)))
        st = eng.stats()
        assert (st["graph_replays"] > 0) == (graphs == "1") and st["error_flags"] == 0
        eng.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_refusals_name_their_cause():
    start = OthelloBoard(n=8)

    def fresh(eng, n=4):
        eng.set_roots(np.tile(start.grid.astype(np.int8)[None], (n, 1, 1)), np.full(n, start.player, np.int8))

    def works(eng, n=4):
        fresh(eng, n)
        eng.search(6)
        assert (eng.root_readout(temps=0)["root_N"].cpu().numpy() == 6).all()

    eng = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, evaluator=E.EVAL_FAKE, **FIXED)
    for bad in (1, 0, None, "on"):
        with pytest.raises(ValueError, match="gumbel_full must be True or False"):
            eng.set_gumbel_full(bad)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="gumbel_full must be 0 or 1"):
            _lib.check(_lib.lib().az_engine_set_gumbel_full(eng.h, bad))
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_root_value"):  # the switch is off
        eng.root_value(0)
    # the switch cannot come into force on trees that were evaluated without it: by its own setter ...
    eng.set_gumbel(4)
    works(eng)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_set_gumbel_full.*set_roots.*reset"):
        eng.set_gumbel_full(True)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_root_value"):
        eng.root_value(0)
    works(eng)  # ... and the refused call left the engine as it was
    fresh(eng)
    eng.set_gumbel_full(True)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*has not been evaluated"):
        eng.root_value(0)
    with pytest.raises(ValueError, match="slot"):
        eng.root_value(4)
    eng.search(6)
    assert all(abs(eng.root_value(s)) <= 1.0 for s in range(4))
    # ... nor with the mode: PUCT searches keep no value
    eng.set_gumbel(None)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_root_value"):
        eng.root_value(0)
    works(eng)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_set_gumbel:.*set_roots.*reset"):
        eng.set_gumbel(4)
    fresh(eng)
    eng.set_gumbel(4)
    eng.search(6)
    assert all(abs(eng.root_value(s)) <= 1.0 for s in range(4))
    # not while a search is open
    eng.search_begin(6)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_set_gumbel_full"):
        eng.set_gumbel_full(False)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_root_value"):
        eng.root_value(0)
    eng.search_end()
    eng.set_gumbel_full(False)
    works(eng)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4
def othello6_net():
    if "net6" not in _CACHE:
        torch.manual_seed(61)
        net = OthelloNet(6, device="cuda")
        net.eval()
        _CACHE["net6"] = net
    return _CACHE["net6"]


def test_batched_player_equals_single_trees():
    net = othello6_net()
    games, rng = [], np.random.default_rng(8)
    while len(games) < 8:
        b = OthelloBoard(n=6)
        for _ in range(len(games)):
            moves = b.get_moves()
            b.play_move(moves[int(rng.integers(len(moves)))])
        games.append(b)
    np.random.seed(11)  # the players draw their game ids from numpy's global stream
    base_id = int(np.random.randint(0, 2**31 - 1))
    np.random.seed(11)
    p = BatchedAlphaZeroPlayer(n_sim=16, nn=net, n_slots=8, gumbel=4, gumbel_full=True, seed=3)
    res = p.get_moves(games, temps=1)
    st = p._engine.stats()
    assert st["error_flags"] == 0 and st["lockstep_iters"] == 17
    values = [p._engine.root_value(i) for i in range(8)]
    p.close()
    for i, (b, (move, probs, counts, priors)) in enumerate(zip(games, res)):
        t = MCT(eval_method="neural", nn=net, seed=3, gumbel=4, gumbel_full=True)
        with mock.patch("numpy.random.randint", return_value=base_id + i):
            t.search(b, n_sim=16)
        assert t._engine_gf is True and t._engine.root_value(0) == values[i]
        best, c1 = t.get_action_probs(b, temp=0)
        assert list(best) == [move] and c1 == counts and sum(counts.values()) == 16, i
        pr, _ = t.get_action_probs(b, temp=1)
        tot = sum(probs.values())
        assert set(pr) == set(probs) and all(abs(pr[k] - probs[k] / tot) < 1e-12 for k in pr), i
        t._engine.close()


def test_trainer_self_play_with_the_full_gumbel_search(tmp_path):
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    tr = AlphaZeroTrainer(verbose=False, engine_slots=8, seed=4, materialize_memory=False, selfplay_gumbel=16, selfplay_gumbel_batch=4,
                          selfplay_gumbel_full=True)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=8, episodes=8, epochs=1, batch_size=32, iterations=1, do_eval=False, device="cuda")
    torch.manual_seed(2)
    tr.setup()
    tr.self_play(0)
    got = {k: v.cpu().numpy() for k, v in tr.device_samples.items()}
    c = tr.config
    outs = []
    for full in (True, False):
        eng = E.SelfPlayEngine(0, 6, 6, n_slots=8, n_sim=8, net=tr._hipnet, dirichlet_alpha=c.dirichlet_alpha, dirichlet_epsilon=c.dirichlet_epsilon,
                               temp_max_step=c.temp_max_step, temp_min_step=c.temp_min_step, seed=4, max_plies=72, sample_capacity=8 * 72)
        eng.set_gumbel(16)
        eng.set_gumbel_batch(4)
        eng.set_gumbel_full(full)
        outs.append(sort_samples(eng.run(8, first_game_id=0)))
        eng.close()
    for k in ("state", "pi", "z", "meta", "visits"):
        assert np.array_equal(got[k], outs[0][k]), k
    assert len(outs[0]["pi"]) != len(outs[1]["pi"]) or not np.array_equal(outs[0]["pi"], outs[1]["pi"])  # the switch reached the engine
