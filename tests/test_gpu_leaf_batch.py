"""GPU: several leaves per slot and lock-step, kept apart by virtual loss (k_step_multi, az_engine_set_leaf_batch).

  1. leaf_batch 1 -- also after a detour over 4 -- is the plain search, bit for bit, graph replay included;
  2. the engine equals the host model of the contract (tests/leaf_batch_model.py): root children, node count, collisions, network rows,
     over ragged lock-steps, K above n_sim, terminal leaves, a forced pass, a move and a second search on the kept subtree;
  3. the same with random ties drawn from the kernel's Philox counters;
  4. production-mode invariants: reproducible, independent of slot count and refill, n_sim visits per search, arena sides;
  5. the HIP network under K = 8 equals the model fed with HipNet.forward's outputs;
  6. refusals name their cause, pool exhaustion stays an error code;
  7. the players play with the option and carry it through clone().
"""
from unittest import mock

import numpy as np
import pytest
import torch

from alphazero_amd import _lib
from alphazero_amd import engine as E
from alphazero_amd.arena import Arena
from alphazero_amd.games.othello import OthelloBoard, OthelloNet
from alphazero_amd.mcts import MCT, _move_of
from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer, GreedyPlayer
from leaf_batch_model import Model, make_board
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

GAMES = {"othello8": ("othello", 0, 8, 8), "othello4": ("othello", 0, 4, 4), "connect4": ("connect4", 1, 6, 7),
         "tictactoe": ("tictactoe", 2, 3, 3)}
FIXED = dict(temp_max_step=-1, temp_min_step=0, node_capacity=8192)
_CACHE = {}


def playout(game, H, W, rng, plies):
    """the position after `plies` seeded random legal moves from the start (None when the game ended before)"""
    b = make_board(game, H, W)
    for _ in range(plies):
        if b.is_game_over():
            return None
        moves = sorted(b.get_moves(), key=lambda m: cf.move_to_action(game, m, H))
        b.play_move(moves[int(rng.integers(len(moves)))])
    return None if b.is_game_over() else b


def positions(tag, count, seed, lo, hi):
    game, _, H, W = GAMES[tag]
    rng, out, seen = np.random.default_rng(seed), [], set()
    while len(out) < count:
        b = playout(game, H, W, rng, int(rng.integers(lo, hi + 1)))
        if b is not None and (b.grid.tobytes(), b.player) not in seen:
            seen.add((b.grid.tobytes(), b.player))
            out.append(b)
    return out


def pass_position(H, seed=5):
    """an Othello position whose side to move has no legal cell but whose game goes on: the root has the one child `pass`"""
    rng = np.random.default_rng(seed)
    for _ in range(4000):
        b = make_board("othello", H, H)
        while not b.is_game_over():
            moves = b.get_moves()
            if tuple(moves[0]) == tuple(b.pass_move):
                return b
            moves = sorted(moves)
            b.play_move(moves[int(rng.integers(len(moves)))])
    raise AssertionError("no forced pass found")


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def compare(eng, slot, m, what):
    a, N, Q, P, rootn = eng.root_children(slot)
    want = m.root_children()
    assert list(a) == [c[0] for c in want], what
    assert list(N) == [c[1] for c in want], (what, list(N), [c[1] for c in want])
    assert rootn == m.root.N, what
    assert np.array_equal(bits(Q), bits([c[2] for c in want])), what
    assert np.array_equal(bits(P), bits([c[3] for c in want])), what
    assert eng.nodes_used(slot) == m.node_count(), what


def run_case(eng, roots, K, n_sim, noise, tie, seed, what):
    """set_roots -> search -> move -> search on the engine and on one model per slot"""
    eng.set_leaf_batch(K)
    gids = 100 + np.arange(len(roots))
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8), game_ids=gids.astype(np.uint32))
    models = [Model(b, K=K, noise=noise, tie=tie, seed=seed, game_id=int(g)) for b, g in zip(roots, gids)]
    c0 = eng.collisions()
    eng.search(n_sim)
    for s, m in enumerate(models):
        m.search(n_sim)
        compare(eng, s, m, (what, K, n_sim, s, "first search"))
    assert eng.collisions() - c0 == sum(m.dups for m in models), (what, K, n_sim)
    eng.advance()
    assert eng.stats()["net_evals"] == sum(m.rows for m in models), (what, K, n_sim)  # rows, not simulations
    live = []
    for s, m in enumerate(models):
        m.advance()
        if not m.root.board.is_game_over():
            live.append(s)
    eng.search(n_sim)  # on the subtree k_reroot kept
    for s in live:
        models[s].search(n_sim)
        compare(eng, s, models[s], (what, K, n_sim, s, "second search"))
    assert eng.collisions() - c0 == sum(m.dups for m in models), (what, K, n_sim)
    return models


def case_roots(tag):
    if tag not in _CACHE:
        game, _, H, W = GAMES[tag]
        if tag == "tictactoe":
            roots = positions(tag, 6, 1, 4, 6)  # from ply 4: terminal leaves, several walkers on one of them, K above the child count
        elif tag == "othello4":
            roots = positions(tag, 5, 2, 2, 8) + [pass_position(4)]
        else:
            roots = positions(tag, 5, 3, 0, 30) + [pass_position(8)]
        _CACHE[tag] = roots
    return _CACHE[tag]


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("tag", ["othello8", "connect4", "tictactoe"])
def test_leaf_batch_one_is_the_plain_search(tag):
    game, gid, H, W = GAMES[tag]
    G, n_sim = 37, 24  # two full blocks of 16 games and a partial one
    start = make_board(game, H, W)
    grids, players = np.tile(start.grid.astype(np.int8)[None], (G, 1, 1)), np.full(G, start.player, np.int8)
    outs = []
    for detour in (None, (1,), (4, 1)):
        eng = E.SelfPlayEngine(gid, H, W, n_slots=G, n_sim=n_sim, evaluator=E.EVAL_FAKE, seed=21, node_capacity=8192)  # random ties, Philox noise
        for k in detour or ():
            eng.set_leaf_batch(k)
        eng.set_roots(grids, players, game_ids=np.arange(500, 500 + G, dtype=np.uint32))
        reads = []
        for _ in range(6):
            eng.search(n_sim)
            r = eng.root_readout()
            reads.append({k: v.cpu().numpy() for k, v in r.items()})
            eng.advance()
        smp = {k: v.cpu().numpy() for k, v in eng.samples().items()}
        st = eng.stats()
        assert st["graph_replays"] > 0 and eng.collisions() == 0
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


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("tag", ["othello8", "othello4", "tictactoe"])
def test_engine_equals_the_model(tag, noise):
    game, gid, H, W = GAMES[tag]
    roots = case_roots(tag)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, tie_mode=E.TIE_LOWEST,
                           noise_mode=E.NOISE_HASH if noise else E.NOISE_OFF, dirichlet_alpha=0.03 if noise else None,
                           dirichlet_epsilon=0.25 if noise else None, seed=3, **FIXED)
    dups = 0
    for K in (2, 3, 5, 8, 16):
        for n_sim in (7, 24):  # ragged last lock-steps; K = 8, 16 above n_sim = 7
            models = run_case(eng, roots, K, n_sim, (0.03, 0.25) if noise else None, "lowest", 3, (tag, noise))
            dups += sum(m.dups for m in models)
            if tag != "tictactoe":  # the forced pass: one child, every later walker of the first lock-step collides
                assert models[-1].dups >= min(K, n_sim) - 1
    assert dups > 0
    assert eng.stats()["error_flags"] == 0
    eng.close()


def test_paths_beyond_16_nodes_at_k4():
    """a late Connect4 position searched long enough that root..leaf paths pass 16 nodes: those positions carry no virtual count and
    are backed up by parent chasing"""
    game, gid, H, W = GAMES["connect4"]
    root = playout(game, H, W, np.random.default_rng(7), 16)
    m = Model(root, K=4)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=1, n_sim=1, evaluator=E.EVAL_FAKE, tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF,
                           dirichlet_alpha=None, dirichlet_epsilon=None, temp_max_step=-1, temp_min_step=0, node_capacity=1 << 16)
    eng.set_leaf_batch(4)
    eng.set_roots(root.grid.astype(np.int8)[None], np.array([root.player], np.int8), game_ids=np.array([0], np.uint32))
    n_sim = 6000
    m.search(n_sim)
    eng.search(n_sim)
    assert m.max_path > 16, "no deep path: the test would prove nothing"
    assert eng.stats()["max_path_len"] == m.max_path
    compare(eng, 0, m, "deep")
    assert eng.collisions() == m.dups
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("tag", ["tictactoe", "othello4"])
def test_random_ties_follow_the_kernels_counters(tag):
    game, gid, H, W = GAMES[tag]
    roots = case_roots(tag)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=len(roots), n_sim=1, evaluator=E.EVAL_FAKE, tie_mode=E.TIE_RANDOM, noise_mode=E.NOISE_OFF,
                           dirichlet_alpha=None, dirichlet_epsilon=None, seed=77, **FIXED)
    for n_sim in (7, 24):
        run_case(eng, roots, 4, n_sim, None, "random", 77, (tag, "random ties"))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4
def othello8_net(max_batch):
    key = ("net", max_batch)
    if key not in _CACHE:
        if "torch_net" not in _CACHE:
            net = OthelloNet(8, device="cuda")
            shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
            net.load_state_dict({k: torch.tensor(v) for k, v in cf.closed_form_state_dict(shapes).items()})
            net.eval()
            _CACHE["torch_net"] = net
        _CACHE[key] = _CACHE["torch_net"].to_hip(max_batch=max_batch)
    return _CACHE[key]


def sort_samples(d):
    d = {k: v.cpu().numpy() for k, v in d.items()}
    order = np.lexsort((d["meta"][:, 1], d["meta"][:, 0]))
    return {k: v[order] for k, v in d.items()}


def test_production_mode_invariants():
    G, n_sim, K = 37, 24, 4
    hip = othello8_net(4 * 37)
    kw = dict(n_sim=n_sim, net=hip, seed=5, node_capacity=8192, sample_capacity=G * 128)
    runs = []
    for slots in (G, G, 5):  # twice the same; then the same 37 games through 5 slots with refill
        eng = E.SelfPlayEngine(0, 8, 8, n_slots=slots, **kw)
        eng.set_leaf_batch(K)
        runs.append(sort_samples(eng.run(G, first_game_id=900)))
        st = eng.stats()
        assert st["games_done"] == G and st["error_flags"] == 0
        assert st["net_evals"] + eng.collisions() <= st["plies"] * (n_sim + 1)  # rows, not simulations
        eng.close()
    for other in runs[1:]:
        for k in ("state", "pi", "z", "meta", "visits"):
            assert np.array_equal(other[k], runs[0][k]), k
    # a fresh root's children share exactly n_sim visits; a kept root's share what they brought plus n_sim, and they brought at
    # most the root's visits less its own first one
    r = runs[0]
    vs, meta = r["visits"].sum(1), r["meta"]
    for i in range(len(vs)):
        if meta[i, 1] == 0:
            assert vs[i] == n_sim
        else:
            assert meta[i - 1, 0] == meta[i, 0] and meta[i - 1, 1] == meta[i, 1] - 1
            assert n_sim <= vs[i] <= r["visits"][i - 1, meta[i - 1, 3]] - 1 + n_sim, i
    # every search makes every root grow by exactly n_sim visits, the same total as leaf_batch 1
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=G, **kw)
    eng.set_leaf_batch(K)
    start = OthelloBoard(n=8)
    eng.set_roots(np.tile(start.grid.astype(np.int8)[None], (G, 1, 1)), np.full(G, start.player, np.int8),
                  game_ids=np.arange(900, 900 + G, dtype=np.uint32))
    brought = np.zeros(G, np.int64)
    for _ in range(5):
        eng.search(n_sim)
        ro = {k: v.cpu().numpy() for k, v in eng.root_readout().items()}
        assert np.array_equal(ro["root_N"], brought + n_sim)
        brought = ro["visits"][np.arange(G), ro["action"]].astype(np.int64)  # the child advance() re-roots at
        eng.advance()
    eng.close()


def test_sides_search_their_slots_alone():
    G, n_sim, K = 37, 24, 4
    hip = othello8_net(4 * 37)
    roots = positions("othello8", G, 9, 0, 9)
    grids, players = np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8)
    gids = np.arange(300, 300 + G, dtype=np.uint32)
    assert (players == 1).any() and (players == -1).any()
    kw = dict(n_sim=n_sim, net=hip, seed=6, node_capacity=8192)
    both = E.SelfPlayEngine(0, 8, 8, n_slots=G, **kw)
    both.set_leaf_batch(K)
    for side in (1, -1):
        both.set_roots(grids, players, game_ids=gids)
        both.set_sides(np.full(G, side, np.int8))
        both.search(n_sim)
        got = {k: v.cpu().numpy() for k, v in both.root_readout(temps=0).items()}
        mine = np.flatnonzero(players == side)
        alone = E.SelfPlayEngine(0, 8, 8, n_slots=len(mine), **kw)
        alone.set_leaf_batch(K)
        alone.set_roots(grids[mine], players[mine], game_ids=gids[mine])
        alone.search(n_sim)
        ref = {k: v.cpu().numpy() for k, v in alone.root_readout(temps=0).items()}
        for k in ("visits", "Q", "P", "child", "root_N", "action"):
            assert np.array_equal(got[k][mine].view(np.uint8), ref[k].view(np.uint8)), (side, k)
        others = np.flatnonzero(players != side)
        assert (got["root_N"][others] == 0).all() and (got["action"][others] == -1).all()
        alone.close()
    both.close()


# ------------------------------------------------------------------------------------------------------------------ 5
def test_the_network_path_equals_the_model_on_the_networks_outputs():
    hip = othello8_net(16)
    root = positions("othello8", 1, 13, 6, 6)[0]

    def net(grid, player, A):
        x = torch.tensor((player * np.asarray(grid)).astype(np.float32).reshape(1, -1), device="cuda")
        p, v = hip.forward(x)
        return p[0].cpu().numpy(), float(v[0].cpu())
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=1, n_sim=16, net=hip, tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, dirichlet_alpha=None,
                           dirichlet_epsilon=None, **FIXED)
    eng.set_leaf_batch(8)
    eng.set_roots(root.grid.astype(np.int8)[None], np.array([root.player], np.int8), game_ids=np.array([1], np.uint32))
    eng.search(16)
    m = Model(root, K=8, net=net)
    m.search(16)
    compare(eng, 0, m, "hip network")
    assert eng.collisions() == m.dups
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_refusals_name_their_cause():
    hip = othello8_net(16)
    start = OthelloBoard(n=8)
    kw = dict(tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, dirichlet_alpha=None, dirichlet_epsilon=None, **FIXED)

    def works(eng, n=4):
        eng.set_roots(np.tile(start.grid.astype(np.int8)[None], (n, 1, 1)), np.full(n, start.player, np.int8))
        eng.search(6)
        assert (eng.root_readout(temps=0)["root_N"].cpu().numpy() == 6).all()

    eng = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, net=hip, **kw)
    for k in (0, 17, -3):
        with pytest.raises(ValueError, match=r"leaf_batch must be in \[1, 16\]"):
            eng.set_leaf_batch(k)
    with pytest.raises(ValueError, match=r"32 rows.*max_batch is 16"):
        eng.set_leaf_batch(8)
    works(eng)
    eng.set_symmetry((0, 1))
    with pytest.raises(ValueError, match="symmetry"):
        eng.set_leaf_batch(2)
    eng.set_symmetry(None)
    eng.set_leaf_batch(4)  # 4 * 4 rows fit
    with pytest.raises(ValueError, match="leaf_batch"):
        eng.set_symmetry((0, 1))
    works(eng)
    eng.search_begin(6)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_set_leaf_batch"):
        eng.set_leaf_batch(1)
    eng.search_end()
    works(eng)

    def uniform(batch):
        batch.probs.fill_(1.0 / batch.A)
        batch.value.zero_()
    ext = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, evaluator=E.EVAL_EXTERNAL, **kw)
    ext.set_evaluator(uniform)
    with pytest.raises(ValueError, match="AZ_EVAL_EXTERNAL"):
        ext.set_leaf_batch(2)
    works(ext)
    roll = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, evaluator=E.EVAL_ROLLOUT, **kw)
    with pytest.raises(ValueError, match="rollout"):
        roll.set_leaf_batch(2)
    works(roll)
    # a node pool too small for the search is still an error code, not a fault
    small = E.SelfPlayEngine(0, 8, 8, n_slots=4, n_sim=1, evaluator=E.EVAL_FAKE, tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF,
                             dirichlet_alpha=None, dirichlet_epsilon=None, temp_max_step=-1, temp_min_step=0, node_capacity=160)
    small.set_leaf_batch(8)
    small.set_roots(np.tile(start.grid.astype(np.int8)[None], (4, 1, 1)), np.full(4, start.player, np.int8))
    with pytest.raises(_lib.AzError, match=r"\[-4\].*node pool"):
        small.search(400)
    for e in (eng, ext, roll, small):
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_players_play_with_leaf_batch():
    torch.manual_seed(31)
    net = OthelloNet(6, device="cuda")
    net.eval()
    np.random.seed(8)
    single = AlphaZeroPlayer(n_sim=24, nn=net, leaf_batch=8)
    res = Arena(single, GreedyPlayer(), OthelloBoard(n=6)).play_game(return_results=True)
    assert res["winner"] in (0, 1, 2)
    assert single.mct._engine is not None and single.mct._engine.stats()["error_flags"] == 0
    twin = single.clone()
    assert twin.leaf_batch == 8 and twin.mct.leaf_batch == 8
    # a compute_time search walks leaf_batch simulations per chunk
    timed = AlphaZeroPlayer(compute_time=0.02, nn=net, leaf_batch=4)
    timed.get_move(OthelloBoard(n=6))
    n_rollouts, _ = timed.mct.get_stats()
    assert n_rollouts >= 4 and n_rollouts % 4 == 0 and timed.mct._engine.root_children(0)[4] == n_rollouts
    timed.mct._engine.close()

    # a budget shorter than the engine's own construction still searches one chunk: the root has visits and get_move a move to return
    brief = AlphaZeroPlayer(compute_time=1e-9, nn=net, leaf_batch=4)
    move, probs, counts, _ = brief.get_move(OthelloBoard(n=6))
    assert brief.mct.get_stats()[0] == 4 and brief.mct._engine.root_children(0)[4] == 4 and len(counts) > 0 and probs == {move: 1}
    brief.mct._engine.close()

    # 20 boards at once == 20 single-board searches under the same seeds and game ids (random ties: the draws depend on both)
    rng = np.random.default_rng(17)
    boards = []
    while len(boards) < 20:
        b = playout("othello", 6, 6, rng, int(rng.integers(0, 10)))
        if b is not None:
            boards.append(b)
    many = BatchedAlphaZeroPlayer(n_sim=24, nn=net, n_slots=20, seed=99, leaf_batch=4)
    with mock.patch.object(np.random, "randint", return_value=4000):  # the base of the game ids: slot i searches game 4000 + i
        got = many.get_moves(boards, temps=0)
    assert many._hipnet.max_batch == 4 * 20
    for i, b in enumerate(boards):
        one = MCT(eval_method="neural", nn=net, seed=99, leaf_batch=4)
        with mock.patch.object(np.random, "randint", return_value=4000 + i):
            one.search(b, n_sim=24)
        _, counts = one.get_action_probs(b, 0)
        assert counts == got[i][2], i
        drawn = int(one._engine.root_readout(temps=0, n=1)["action"][0])  # the device's draw among equals: same seed, game id, ply
        assert _move_of(b, drawn) == got[i][0], i
        one._engine.close()
    many.close()
