"""GPU: several Sequential Halving leaves per network call (k_step_gumbel_multi, az_engine_set_gumbel_batch).

  1. the engine equals the host model of the contract (tests/gumbel_batch_model.py) bit for bit: root children, considered set, move,
     pi', visits, node count, collisions, network rows -- over n_sim x m x K, roots with fewer children than m, with 16 and more (one
     lock-step), a forced pass, terminal leaves, a move and a second search on the kept subtree, roots with plans of different
     length in one engine, two searches on one root, random ties below the root, the HIP network, a random symmetry;
  2. the self-play wave does not depend on slot count or refill and equals the model game by game;
  3. off is off: at K = 1 and with the mode off nothing changes, graph replay included; refusals; replayed graphs equal plain launches;
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
from gumbel_batch_model import GumbelBatchModel, wide_root
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
        if tag == "othello8":  # m > nch; 16 children and more: a search of 16 is one lock-step; a forced pass: m0 = 1
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
    if want:
        assert int(ro["action"][slot]) == m.move(), what
        assert np.array_equal(ro["pi"][slot].view(np.uint32), m.policy().view(np.uint32)), what
        assert np.array_equal(ro["visits"][slot], m.visits()), what


def readout(eng):
    return {k: v.cpu().numpy() for k, v in eng.root_readout().items()}


def run_case(eng, roots, spec, K, n_sims, tie, seed, what, net=None):
    """set_roots -> the searches of n_sims -> move -> the same searches on the kept subtree, on the engine and on one model per slot;
    the engine's collisions and lock-step count follow the models and the contract"""
    eng.set_gumbel(spec)
    eng.set_gumbel_batch(K)
    gids = 100 + np.arange(len(roots))
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8), game_ids=gids.astype(np.uint32))
    models = [GumbelBatchModel(b, K=K, tie=tie, seed=seed, game_id=int(g), net=net, **spec) for b, g in zip(roots, gids)]
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
        assert eng.collisions() - coll0 == sum(models[s].dups for s in range(len(roots))), (what, spec, K, stage)
        if stage == "first":
            eng.advance()
            assert eng.stats()["net_evals"] == sum(m.rows for m in models), (what, spec, K)
            for m in models:
                m.advance()
            live = [s for s in live if not models[s].root.board.is_game_over()]
            for s in live:
                assert eng.considered(s) == []  # k_move cleared it
    assert eng.stats()["error_flags"] == 0
    return models


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("K", [2, 3, 4, 16])
@pytest.mark.parametrize("tag", ["othello8", "tictactoe", "connect4"])
def test_engine_equals_the_model(tag, K):
    game, gid, H, W = GAMES[tag]
    roots = roots_of(tag)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=3, **FIXED)
    dups = 0
    for m in (2, 4, 16):
        for n_sim in (5, 7, 16, 50):
            models = run_case(eng, roots, {"m": m}, K, (n_sim,), "lowest", 3, tag)
            dups += sum(x.dups for x in models)
    if tag == "othello8":
        assert len(roots[0].get_moves()) == 4 and len(roots[1].get_moves()) >= 16 and len(roots[2].get_moves()) == 1
    assert dups > 0 or K == 2, "no walker met a pending leaf: the collision policy was not exercised"
    eng.close()


def test_roots_with_plans_of_different_length_share_one_engine():
    game, gid, H, W = GAMES["othello8"]
    roots = [make_board(game, H, W), wide_root(16), wide_root(9, 9)]  # m0 = 4, 16, 9: two lock-steps, one, three of Lmax = 4
    plans = [G.lockstep_plan(16, min(16, len(b.get_moves())), 16) for b in roots]
    assert plans == [[(0, 8), (8, 8)], [(0, 16)], [(0, 9), (9, 4), (13, 3)]] and G.locksteps(16, 16, 16) == 4
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=3, **FIXED)
    models = run_case(eng, roots, {"m": 16}, 16, (16,), "lowest", 3, "three plans")  # every root grows by 16 and equals its model
    eng.close()
    assert all(m.root.N >= 16 for m in models)
    wide = GumbelBatchModel(roots[1], K=16, m=16, seed=3, game_id=101)
    wide.search(16)
    assert wide.plan == [(0, 16)] and wide.dups == 0 and wide.rows == 17


def test_two_searches_on_one_root_each_run_a_schedule():
    game, gid, H, W = GAMES["othello8"]
    roots = roots_of("othello8")
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=3, **FIXED)
    run_case(eng, roots, {"m": 4}, 4, (8, 8), "lowest", 3, "twice 8")
    run_case(eng, roots, {"m": 16}, 16, (5, 16, 3), "lowest", 3, "5, 16, 3")
    eng.close()


@pytest.mark.parametrize("tag", ["tictactoe", "othello4"])
def test_random_ties_below_the_root(tag):
    game, gid, H, W = GAMES[tag]
    roots = roots_of(tag)
    kw = dict(FIXED, tie_mode=E.TIE_RANDOM)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=77, **kw)
    for n, K in ((16, 4), (50, 3)):
        run_case(eng, roots, {"m": 4}, K, (n,), "random", 77, (tag, "random ties"))
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
    run_case(eng, roots, {"m": 16}, 16, (16,), "lowest", 9, "hip network", net=net)
    eng.close()


def test_with_a_random_symmetry_the_draws_follow_the_game_not_the_slot():
    _, hip = othello8_net()
    roots = roots_of("othello8")
    grids, players = np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8)
    gids = np.array([7, 8, 9], np.uint32)
    outs = []
    for order in (np.arange(3), np.arange(3)[::-1].copy()):
        eng = E.SelfPlayEngine(0, 8, 8, n_slots=3, n_sim=16, net=hip, seed=9, **FIXED)
        eng.set_symmetry("random")
        eng.set_gumbel(16)
        eng.set_gumbel_batch(4)
        eng.set_roots(grids[order], players[order], game_ids=gids[order])
        eng.search(16)
        ro = readout(eng)
        outs.append({k: v[np.argsort(order)] for k, v in ro.items()})
        assert eng.stats()["error_flags"] == 0
        eng.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8)), k
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
        rec, winner = GumbelBatchModel(make_board(game, H, W), K=K, m=16, seed=5, game_id=g).play_game(n_sim)
        assert len(rows) == len(rec), g
        for i, (state, pi, vis, action, player) in zip(rows, rec):
            assert np.array_equal(r["state"][i], state) and r["meta"][i, 3] == action and r["meta"][i, 2] == player, (g, i)
            assert np.array_equal(r["pi"][i].view(np.uint32), pi.view(np.uint32)), (g, i)
            assert np.array_equal(r["visits"][i], vis), (g, i)
            assert r["z"][i] == winner * player, (g, i)


# ------------------------------------------------------------------------------------------------------------------ 3
def six_rounds(setup, gumbel):
    game, gid, H, W = GAMES["othello8"]
    n, n_sim = 37, 24
    start = make_board(game, H, W)
    grids, players = np.tile(start.grid.astype(np.int8)[None], (n, 1, 1)), np.full(n, start.player, np.int8)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=n, n_sim=n_sim, evaluator=E.EVAL_FAKE, seed=21, node_capacity=8192)  # random ties, Philox noise
    if gumbel is not None:
        eng.set_gumbel(gumbel)
    setup(eng)
    eng.set_roots(grids, players, game_ids=np.arange(500, 500 + n, dtype=np.uint32))
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


def test_off_is_off():
    ref = six_rounds(lambda e: None, 16)
    same_rounds(six_rounds(lambda e: e.set_gumbel_batch(1), 16), ref)
    same_rounds(six_rounds(lambda e: (e.set_gumbel_batch(4), e.set_gumbel_batch(1)), 16), ref)
    # with the mode off the setting is accepted and not in force: the plain search, launch for launch
    plain = six_rounds(lambda e: None, None)
    same_rounds(six_rounds(lambda e: e.set_gumbel_batch(4), None), plain)
    # ... and it comes into force with the mode, in either order of the two setters
    a = six_rounds(lambda e: e.set_gumbel_batch(4), 16)

    def before(e):
        e.set_gumbel(None)
        e.set_gumbel_batch(4)
        e.set_gumbel(16)
    same_rounds(six_rounds(before, 16), a)
    assert a[2]["lockstep_iters"] == 6 * (G.locksteps(24, 16, 4) + 1) < ref[2]["lockstep_iters"] == 6 * 25


def test_replayed_graphs_of_the_mode_equal_plain_launches(monkeypatch):
    game, gid, H, W = GAMES["othello4"]
    outs = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("AZ_ENGINE_GRAPHS", graphs)
        eng = E.SelfPlayEngine(gid, H, W, n_slots=17, n_sim=16, evaluator=E.EVAL_FAKE, seed=5, node_capacity=8192, sample_capacity=37 * 40)
        eng.set_gumbel(4)
        eng.set_gumbel_batch(4)
        outs.append(sort_samples(eng.run(37, first_game_id=0)))
        st = eng.stats()
        assert (st["graph_replays"] > 0) == (graphs == "1") and st["error_flags"] == 0
        eng.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_refusals_name_their_cause():
    start = OthelloBoard(n=8)

    def works(eng, n=4):
        eng.set_roots(np.tile(start.grid.astype(np.int8)[None], (n, 1, 1)), np.full(n, start.player, np.int8))
        eng.search(6)
        assert (eng.root_readout(temps=0)["root_N"].cpu().numpy() == 6).all()

    eng = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, evaluator=E.EVAL_FAKE, **FIXED)
    for k in (0, 17, -3):
        with pytest.raises(ValueError, match=r"gumbel_batch must be in"):
            eng.set_gumbel_batch(k)
        with pytest.raises(ValueError, match=r"gumbel_batch must be in \[1, 16\]"):
            _lib.check(_lib.lib().az_engine_set_gumbel_batch(eng.h, k))
    # the leaf_batch x gumbel refusals stand, whatever the batch says
    eng.set_gumbel_batch(4)
    eng.set_leaf_batch(4)
    with pytest.raises(ValueError, match="az_engine_set_leaf_batch"):
        eng.set_gumbel(4)
    works(eng)
    eng.set_leaf_batch(1)
    eng.set_gumbel(4)
    with pytest.raises(ValueError, match="az_engine_set_gumbel"):
        eng.set_leaf_batch(4)
    works(eng)
    eng.search_begin(6)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_set_gumbel_batch"):
        eng.set_gumbel_batch(2)
    eng.search_end()
    eng.set_gumbel_batch(2)
    works(eng)
    eng.close()
    # the ensemble and gumbel_batch > 1 refuse each other, each naming the other setter; the random symmetry mode combines
    _, hip = othello8_net()
    net = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, net=hip, **FIXED)
    net.set_gumbel(4)
    net.set_symmetry("all")
    with pytest.raises(ValueError, match="az_engine_set_symmetry"):
        net.set_gumbel_batch(4)
    net.set_gumbel_batch(1)
    works(net)
    net.set_symmetry(None)
    net.set_gumbel_batch(4)
    with pytest.raises(ValueError, match="az_engine_set_gumbel_batch"):
        net.set_symmetry("all")
    net.set_symmetry("random")
    works(net)
    with pytest.raises(ValueError, match="max_batch"):  # 17 x 4 rows on a network of 64
        big = E.SelfPlayEngine(0, 8, 8, n_slots=17, n_sim=1, net=hip, **FIXED)
        big.set_gumbel(4)
        big.set_gumbel_batch(4)
    big.close()
    net.close()


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
    p = BatchedAlphaZeroPlayer(n_sim=16, nn=net, n_slots=8, gumbel=16, gumbel_batch=4, seed=3)
    res = p.get_moves(games, temps=1)
    st = p._engine.stats()
    assert st["error_flags"] == 0 and st["lockstep_iters"] == G.locksteps(16, 16, 4) + 1
    p.close()
    for i, (b, (move, probs, counts, priors)) in enumerate(zip(games, res)):
        t = MCT(eval_method="neural", nn=net, seed=3, gumbel=16, gumbel_batch=4)
        with mock.patch("numpy.random.randint", return_value=base_id + i):
            t.search(b, n_sim=16)
        assert t._engine_gb == 4
        best, c1 = t.get_action_probs(b, temp=0)
        assert list(best) == [move] and c1 == counts and sum(counts.values()) == 16, i
        pr, _ = t.get_action_probs(b, temp=1)
        tot = sum(probs.values())
        assert set(pr) == set(probs) and all(abs(pr[k] - probs[k] / tot) < 1e-12 for k in pr), i
        t._engine.close()


def test_trainer_self_play_with_the_batched_gumbel_search(tmp_path):
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    tr = AlphaZeroTrainer(verbose=False, engine_slots=8, seed=4, materialize_memory=False, selfplay_gumbel=16, selfplay_gumbel_batch=4)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=8, episodes=8, epochs=1, batch_size=32, iterations=1, do_eval=False, device="cuda")
    torch.manual_seed(2)
    tr.setup()
    tr.self_play(0)
    got = {k: v.cpu().numpy() for k, v in tr.device_samples.items()}
    c = tr.config
    assert tr._hipnet.max_batch == 32
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=8, n_sim=8, net=tr._hipnet, dirichlet_alpha=c.dirichlet_alpha, dirichlet_epsilon=c.dirichlet_epsilon,
                           temp_max_step=c.temp_max_step, temp_min_step=c.temp_min_step, seed=4, max_plies=72, sample_capacity=8 * 72)
    eng.set_gumbel(16)
    eng.set_gumbel_batch(4)
    ref = sort_samples(eng.run(8, first_game_id=0))
    for k in ("state", "pi", "z", "meta", "visits"):
        assert np.array_equal(got[k], ref[k]), k
    first = np.flatnonzero(ref["meta"][:, 1] == 0)
    assert ((ref["pi"][first] > 0).sum(1) == 4).all() and (ref["visits"][first].sum(1) == 8).all()
    eng.close()
