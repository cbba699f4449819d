"""GPU: the Gumbel root search (k_step_gumbel, az_engine_set_gumbel).

  1. the engine equals the host model of the contract (tests/gumbel_model.py) bit for bit: root children, considered set, move, pi',
     node count, network rows -- over n_sim x m, roots with fewer and more children than m, terminal children, a forced pass, a move
     and a second search on the kept subtree, two searches on one root, random ties below the root, the HIP network, a random symmetry;
  2. the self-play wave does not depend on slot count or refill and equals the model game by game;
  3. off is off: the untouched engine, set_gumbel(None) and a detour over 4 are bit-equal, graph replay included; refusals; replayed
     graphs of the mode equal plain launches;
  4. the players and the trainer carry the option.
"""
from unittest import mock

import numpy as np
import pytest
import torch

from alphazero_amd import _lib, base
from alphazero_amd import engine as E
from alphazero_amd.arena import Arena
from alphazero_amd.gumbel import locate
from alphazero_amd.games.othello import OthelloBoard, OthelloConfig, OthelloNet
from alphazero_amd.mcts import MCT, _action_of
from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer, GreedyPlayer
from alphazero_amd.trainer import AlphaZeroTrainer
from gumbel_model import GumbelModel, pass_position, playout
from leaf_batch_model import make_board
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

GAMES = {"othello8": ("othello", 0, 8, 8), "othello4": ("othello", 0, 4, 4), "connect4": ("connect4", 1, 6, 7),
         "tictactoe": ("tictactoe", 2, 3, 3)}
QUIET = dict(tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, dirichlet_alpha=None, dirichlet_epsilon=None)
FIXED = dict(temp_max_step=-1, temp_min_step=0, node_capacity=8192, **QUIET)
_CACHE = {}


def roots_of(tag):
    if tag not in _CACHE:
        game, _, H, W = GAMES[tag]
        rng = np.random.default_rng(17)
        if tag == "othello8":
            wide = None
            while wide is None or len(wide.get_moves()) < 9:  # more children than m = 4: halving drops candidates at once
                wide = playout(game, H, W, rng, int(rng.integers(10, 30)))
            roots = [make_board(game, H, W), wide, pass_position(8)]
        elif tag == "tictactoe":
            roots = []
            while len(roots) < 4:  # from ply 4: terminal root children and terminal leaves
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
    return {k: v.cpu().numpy() for k, v in eng.root_readout().items()}  # the scheduler's temperature: the mode ignores it


def run_case(eng, roots, spec, n_sims, tie, seed, what, net=None):
    """set_roots -> the searches of n_sims -> move -> the same searches on the kept subtree, on the engine and on one model per slot"""
    eng.set_gumbel(spec)
    gids = 100 + np.arange(len(roots))
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8), game_ids=gids.astype(np.uint32))
    models = [GumbelModel(b, tie=tie, seed=seed, game_id=int(g), net=net, **spec)
              for b, g in zip(roots, gids)]
    live = list(range(len(roots)))
    for stage in ("first", "second"):
        for n in n_sims:
            eng.search(n)
            ro = readout(eng)
            for s in live:
                models[s].search(n)
                compare(eng, s, models[s], ro, (what, spec, n, s, stage))
        if stage == "first":
            eng.advance()
            assert eng.stats()["net_evals"] == sum(m.rows for m in models), (what, spec)
            for s, m in enumerate(models):
                moved = m.advance()
                assert 0 <= moved < m.A
            live = [s for s in live if not models[s].root.board.is_game_over()]
            for s in live:
                assert eng.considered(s) == []  # k_move cleared it
    assert eng.stats()["error_flags"] == 0
    return models


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("tag", ["othello8", "tictactoe", "connect4"])
def test_engine_equals_the_model(tag):
    game, gid, H, W = GAMES[tag]
    roots = roots_of(tag)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=3, **FIXED)
    dropped = False
    for m in (1, 2, 4, 16):
        for n_sim in (1, 5, 16, 50):
            models = run_case(eng, roots, {"m": m}, (n_sim,), "lowest", 3, tag)
            dropped |= any(0 < len(x.considered()) < min(m, len(x.root.children)) for x in models)
    assert dropped, "no search halved its candidates: the test would prove little"
    if tag == "othello8":
        assert len(roots[1].get_moves()) >= 9 and len(roots[0].get_moves()) == 4 and len(roots[2].get_moves()) == 1
    # other constants, the deterministic search among them
    for spec in ({"m": 4, "gumbel_scale": 0.0}, {"m": 8, "c_visit": 10.0, "c_scale": 1.5, "gumbel_scale": 0.5}, {"m": 3, "c_scale": 0.0}):
        run_case(eng, roots, spec, (16,), "lowest", 3, tag)
    eng.close()


def test_two_searches_on_one_root_each_run_a_schedule():
    game, gid, H, W = GAMES["othello8"]
    roots = roots_of("othello8")
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=3, **FIXED)
    run_case(eng, roots, {"m": 4}, (8, 8), "lowest", 3, "twice 8")
    run_case(eng, roots, {"m": 16}, (5, 16, 3), "lowest", 3, "5, 16, 3")
    eng.close()


@pytest.mark.parametrize("tag", ["tictactoe", "othello4"])
def test_random_ties_below_the_root(tag):
    game, gid, H, W = GAMES[tag]
    roots = roots_of(tag)
    kw = dict(FIXED, tie_mode=E.TIE_RANDOM)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, seed=77, **kw)
    for n in (16, 50):
        run_case(eng, roots, {"m": 4}, (n,), "random", 77, (tag, "random ties"))
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
    run_case(eng, roots, {"m": 16}, (16,), "lowest", 9, "hip network", net=net)
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
        eng.set_gumbel(4)
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
    n_sim, n_games = 16, 37
    runs = []
    for slots in (37, 17, 5):  # groups on both sides of a 16-game block boundary; 5 and 17 refill
        eng = E.SelfPlayEngine(gid, H, W, n_slots=slots, n_sim=n_sim, evaluator=E.EVAL_FAKE, seed=5, node_capacity=8192,
                               sample_capacity=n_games * 40, **QUIET)  # the default temperature schedule: ignored
        eng.set_gumbel(16)
        runs.append(sort_samples(eng.run(n_games, first_game_id=900)))
        st = eng.stats()
        assert st["games_done"] == n_games and st["error_flags"] == 0
        eng.close()
    for other in runs[1:]:
        for k in ("state", "pi", "z", "meta", "visits"):
            assert np.array_equal(other[k], runs[0][k]), k
    r = runs[0]
    for g in (900, 917, 936):
        rows = np.flatnonzero(r["meta"][:, 0] == g)
        rec, winner = GumbelModel(make_board(game, H, W), m=16, seed=5, game_id=g).play_game(n_sim)
        assert len(rows) == len(rec), g
        for i, (state, pi, vis, action, player) in zip(rows, rec):
            assert np.array_equal(r["state"][i], state) and r["meta"][i, 3] == action and r["meta"][i, 2] == player, (g, i)
            assert np.array_equal(r["pi"][i].view(np.uint32), pi.view(np.uint32)), (g, i)
            assert np.array_equal(r["visits"][i], vis), (g, i)
            assert r["z"][i] == winner * player, (g, i)
    # the visits follow the schedule: a fresh root's children share exactly n_sim visits, dealt as the phases say (the survivors
    # of a phase enter the next with equal counts, so the counts do not depend on which children survive)
    nch = 4 if tag == "othello4" else 9
    want = [0] * nch
    for s in range(n_sim):
        _, mp, i = locate(s, n_sim, min(16, nch))
        want[i % mp] += 1
    for i in np.flatnonzero(r["meta"][:, 1] == 0):
        assert sorted(int(x) for x in r["visits"][i] if x > 0) == sorted(w for w in want if w > 0), i


# ------------------------------------------------------------------------------------------------------------------ 3
def test_off_is_off():
    game, gid, H, W = GAMES["othello8"]
    G, n_sim = 37, 24
    start = make_board(game, H, W)
    grids, players = np.tile(start.grid.astype(np.int8)[None], (G, 1, 1)), np.full(G, start.player, np.int8)
    outs = []
    for detour in ((), (None,), (4, None)):
        eng = E.SelfPlayEngine(gid, H, W, n_slots=G, n_sim=n_sim, evaluator=E.EVAL_FAKE, seed=21, node_capacity=8192)  # random ties, Philox noise
        for spec in detour:
            eng.set_gumbel(spec)
        eng.set_roots(grids, players, game_ids=np.arange(500, 500 + G, dtype=np.uint32))
        reads = []
        for _ in range(6):
            eng.search(n_sim)
            reads.append(readout(eng))
            eng.advance()
        smp = {k: v.cpu().numpy() for k, v in eng.samples().items()}
        st = eng.stats()
        assert st["graph_replays"] > 0 and all(eng.considered(s) == [] for s in (0, 36))
        outs.append((reads, smp, st))
        eng.close()
    ref = outs[0]
    for reads, smp, st in outs[1:]:
        for a, b in zip(reads, ref[0]):
            for k in b:
                assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        for k in ref[1]:
            assert np.array_equal(smp[k], ref[1][k]), k
        for k in ("net_evals", "lockstep_iters", "graph_replays", "plies", "samples"):
            assert st[k] == ref[2][k], k


def test_replayed_graphs_of_the_mode_equal_plain_launches(monkeypatch):
    game, gid, H, W = GAMES["othello4"]
    outs = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("AZ_ENGINE_GRAPHS", graphs)
        eng = E.SelfPlayEngine(gid, H, W, n_slots=17, n_sim=16, evaluator=E.EVAL_FAKE, seed=5, node_capacity=8192, sample_capacity=37 * 40)
        eng.set_gumbel(4)
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
    eng.set_leaf_batch(4)
    with pytest.raises(ValueError, match="az_engine_set_leaf_batch"):
        eng.set_gumbel(4)
    works(eng)
    eng.set_leaf_batch(1)
    eng.set_gumbel(4)
    with pytest.raises(ValueError, match="az_engine_set_gumbel"):
        eng.set_leaf_batch(4)
    eng.set_leaf_batch(1)
    works(eng)
    assert len(eng.considered(0)) == 2
    for m in (-1, 17):
        with pytest.raises(ValueError, match=r"m must be in \[0, 16\]"):
            _lib.check(_lib.lib().az_engine_set_gumbel(eng.h, m, 50.0, 0.5, 1.0))
    for bad in ((-1.0, 0.5, 1.0), (50.0, float("inf"), 1.0), (50.0, 0.5, float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            _lib.check(_lib.lib().az_engine_set_gumbel(eng.h, 4, *bad))
    eng.search_begin(6)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_set_gumbel"):
        eng.set_gumbel(None)
    eng.search_end()
    eng.set_gumbel(None)  # clears the candidate sets
    assert eng.considered(0) == []
    works(eng)

    def uniform(batch):
        batch.probs.fill_(1.0 / batch.A)
        batch.value.zero_()
    ext = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, evaluator=E.EVAL_EXTERNAL, **FIXED)
    ext.set_evaluator(uniform)
    with pytest.raises(ValueError, match="AZ_EVAL_EXTERNAL"):
        ext.set_gumbel(4)
    ext.set_gumbel(None)
    works(ext)
    roll = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, evaluator=E.EVAL_ROLLOUT, **FIXED)
    with pytest.raises(ValueError, match="rollout"):
        roll.set_gumbel(4)
    works(roll)
    for e in (eng, ext, roll):
        e.close()


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
    p = BatchedAlphaZeroPlayer(n_sim=16, nn=net, n_slots=8, gumbel=4, seed=3)
    res = p.get_moves(games, temps=1)
    assert p._engine.stats()["error_flags"] == 0 and len(p._engine.considered(0)) == 2
    p.close()
    for i, (b, (move, probs, counts, priors)) in enumerate(zip(games, res)):
        t = MCT(eval_method="neural", nn=net, seed=3, gumbel=4)
        with mock.patch("numpy.random.randint", return_value=base_id + i):
            t.search(b, n_sim=16)
        best, c1 = t.get_action_probs(b, temp=0)
        assert list(best) == [move] and c1 == counts and sum(counts.values()) == 16, i
        pr, _ = t.get_action_probs(b, temp=1)
        tot = sum(probs.values())
        assert set(pr) == set(probs) and all(abs(pr[k] - probs[k] / tot) < 1e-12 for k in pr), i
        assert abs(sum(pr.values()) - 1.0) < 1e-12
        t._engine.close()


def test_single_player_plays_a_whole_game_deterministically():
    net = othello6_net()
    np.random.seed(4)
    single = AlphaZeroPlayer(n_sim=8, nn=net, gumbel={"m": 4, "gumbel_scale": 0})
    res = Arena(single, GreedyPlayer(), OthelloBoard(n=6)).play_game(return_results=True)
    assert res["winner"] in (0, 1, 2)
    assert single.mct._engine is not None and single.mct._engine_gumbel == (4, 50.0, 0.5, 0.0)
    assert single.mct._engine.stats()["error_flags"] == 0


def test_trainer_self_play_with_the_gumbel_search(tmp_path):
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    tr = AlphaZeroTrainer(verbose=False, engine_slots=8, seed=4, materialize_memory=False, selfplay_gumbel=16)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=8, episodes=8, epochs=1, batch_size=32, iterations=1, do_eval=False, device="cuda")
    torch.manual_seed(2)
    tr.setup()
    tr.self_play(0)
    got = {k: v.cpu().numpy() for k, v in tr.device_samples.items()}
    c = tr.config
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=8, n_sim=8, net=tr._hipnet, dirichlet_alpha=c.dirichlet_alpha, dirichlet_epsilon=c.dirichlet_epsilon,
                           temp_max_step=c.temp_max_step, temp_min_step=c.temp_min_step, seed=4, max_plies=72, sample_capacity=8 * 72)
    eng.set_gumbel(16)
    ref = sort_samples(eng.run(8, first_game_id=0))
    for k in ("state", "pi", "z", "meta", "visits"):
        assert np.array_equal(got[k], ref[k]), k
    # pi is the improved policy, not the visit counts: full support over the legal moves of a fresh root
    first = np.flatnonzero(ref["meta"][:, 1] == 0)
    assert ((ref["pi"][first] > 0).sum(1) == 4).all() and (ref["visits"][first].sum(1) == 8).all()
    eng.close()
