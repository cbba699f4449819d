"""GPU: every leaf evaluated in ONE board symmetry drawn per evaluation (k_sym_pick / k_sym_twin / k_sym_unpick,
az_net_forward_sym_codes, az_engine_set_symmetry_random).

  5. forward_sym_codes == twin -> HipNet.forward -> mapped back, per row, bit for bit; one code everywhere == forward_sym of that code;
  6. the engine in random mode == the same composition through the external-evaluator route with the codes drawn on the host;
  7. the draw is keyed by the game, not the slot; another seed draws other codes;
  8. the identity-only mask is the plain search bit for bit;
  9. graph capture / replay, switching between off, ensemble and random, and a search continued on one root;
 10. with leaf_batch: the engine == the host model (tests/symmetry_random_model.py), both orders of the two setters;
 11. a self-play wave does not depend on the slot count;
 12. the players play with the option;
 13. the trainer's self-play wave == a bare engine in random mode;
 14. refusals leave the handles usable.
"""
import numpy as np
import pytest
import torch

from alphazero_amd import _lib, base
from alphazero_amd import engine as E
from alphazero_amd import symmetry as S
from alphazero_amd.arena import Arena
from alphazero_amd.games.connect4 import Connect4Board, Connect4Net
from alphazero_amd.games.othello import OthelloBoard, OthelloConfig, OthelloNet
from alphazero_amd.games.tictactoe import TicTacToeBoard, TicTacToeNet
from alphazero_amd.mcts import _action_of
from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer, GreedyPlayer
from alphazero_amd.trainer import AlphaZeroTrainer
from leaf_batch_model import make_board
from symmetry_random_model import RandomSymmetryModel
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

# tag: (game, id, H, W, A, network, board)
GAMES = {
    "othello6": ("othello", 0, 6, 6, 37, lambda: OthelloNet(6, device="cuda"), lambda: OthelloBoard(n=6)),
    "connect4": ("connect4", 1, 6, 7, 7, lambda: Connect4Net(7, 6, device="cuda"), lambda: Connect4Board(width=7, height=6)),
    "tictactoe": ("tictactoe", 2, 3, 3, 9, lambda: TicTacToeNet(device="cuda"), lambda: TicTacToeBoard()),
}
MAX_ROWS = 8 * 16  # the "all" engine of 16 slots; 130 rows of forward_sym_codes
_CACHE = {}
SEED = 5
FIXED = dict(tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, dirichlet_alpha=None, dirichlet_epsilon=None, node_capacity=8192, seed=SEED)


def setup(tag):
    """one random-init network per game and its HIP twin, shared by the tests and left unchanged"""
    if tag not in _CACHE:
        torch.manual_seed(sorted(GAMES).index(tag) + 60)
        net = GAMES[tag][5]()
        net.eval()
        _CACHE[tag] = (net, net.to_hip(max_batch=max(MAX_ROWS, 130)))
    return _CACHE[tag]


def boards(tag, B, seed):
    _, _, H, W, _, _, _ = GAMES[tag]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (B, H, W), generator=g).to(torch.float32).cuda()


def compose(hip, x, codes, game, H, W):
    """row r in the one orientation codes[r], from its parts: the twin in torch, the plain forward on as many rows as came in,
    the policy mapped back -- copies only"""
    codes = np.asarray(codes)
    tw = x.clone()
    for c in np.unique(codes):
        idx = torch.as_tensor(np.flatnonzero(codes == c), device=x.device)
        tw[idx] = S.twin_planes(x[idx], int(c))
    p, v = hip.forward(tw.reshape(x.shape[0], H * W))
    out = torch.empty_like(p)
    for c in np.unique(codes):
        idx = torch.as_tensor(np.flatnonzero(codes == c), device=x.device)
        out[idx] = S.untwin_probs(p[idx], int(c), game, H, W)
    return out, v


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("B", [1, 7, 130])
@pytest.mark.parametrize("tag", list(GAMES))
def test_forward_sym_codes_equals_its_composition(tag, B):
    game, gid, H, W, A, _, _ = GAMES[tag]
    _, hip = setup(tag)
    x = boards(tag, B, seed=B + 1)
    members = S.members(game, H, W, "all")
    codes = np.random.default_rng(B).choice(members, size=B)
    p, v = hip.forward_sym_codes(x, codes)
    rp, rv = compose(hip, x, codes, game, H, W)
    assert p.shape == (B, A) and v.shape == (B,)
    assert torch.equal(p, rp) and torch.equal(v, rv), (tag, B)
    p0, v0 = hip.forward(x)
    for c in members:  # every row on one code: the ensemble of that single member
        pc, vc = hip.forward_sym_codes(x, np.full(B, c))
        rp, rv = (p0, v0) if c == 0 else hip.forward_sym(x, [c])
        assert torch.equal(pc, rp) and torch.equal(vc, rv), (tag, B, c)
    if B > 1:  # the network is not equivariant: the codes are really in the loop
        assert not torch.equal(p, p0)
    for bad in [[9] * B, [-1] * B, [0.0] * B, [0] * (B + 1)] + ([[2] * B] if tag == "connect4" else []):
        with pytest.raises(ValueError):
            hip.forward_sym_codes(x, bad)


# ------------------------------------------------------------------------------------------------------------------ 6
def _random_positions(board, count, rng):
    """`count` random mid-game roots; the first is one move from the end of its game, and `finals` holds for every root a
    position one move from the end with that move (to put every slot's game over)"""
    def playout(stop_after):
        b = board.clone()
        b.reset()
        prev, last, plies = None, None, 0
        while not b.is_game_over() and (stop_after is None or plies < stop_after):
            moves = b.get_moves()
            m = moves[int(rng.integers(len(moves)))]
            prev, last = b.clone(), m
            b.play_move(m)
            plies += 1
        return b, prev, last
    grids, players, finals = [], [], []
    while len(finals) < count:
        _, prev, last = playout(None)
        finals.append((prev.grid.astype(np.int8), prev.player, _action_of(prev, last)))
    grids.append(finals[0][0])
    players.append(finals[0][1])
    while len(grids) < count:
        b, _, _ = playout(int(rng.integers(0, 12)))
        if not b.is_game_over():
            grids.append(b.grid.astype(np.int8))
            players.append(b.player)
    return np.array(grids), np.array(players, np.int8), finals


def _readout(eng, n=None):
    r = eng.root_readout(temps=0, n=n)
    return {k: r[k].cpu().numpy() for k in ("visits", "Q", "P", "child", "root_N")}


def _same(a, b, what=None):
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


GIDS = (1000 + 3 * np.arange(8)).astype(np.uint32)
PLIES = np.arange(8, dtype=np.int32)


class HostDraw:
    """the evaluator of an EVAL_EXTERNAL engine that restates the random mode: the code of every pending row drawn with
    symmetry.random_code from the row's slot, the known game ids / plies and its own call counter (call 0: the root-prior pass,
    then the simulations s0, s0 + 1, ...), then the composition of test 5"""

    def __init__(self, hip, tag, members, gids, plies, seed=SEED):
        self.hip, self.tag, self.members, self.gids, self.plies, self.seed = hip, tag, members, gids, plies, seed
        self.rows, self.calls, self.empty = [], 0, 0
        self.new_root()

    def new_root(self, s0=0, root_pass=True):
        self.next_s = S.ROOT_PASS if root_pass else s0
        self.s0 = s0

    def __call__(self, batch):
        game, _, H, W, _, _, _ = GAMES[self.tag]
        s = self.next_s
        self.next_s = self.s0 if s == S.ROOT_PASS else s + 1
        n = int(batch.count[0].item())
        self.calls += 1
        self.rows.append(n)
        if n == 0:
            self.empty += 1
            return
        slots = batch.slots[:n].cpu().numpy()
        codes = [S.random_code(self.seed, self.gids[g], self.plies[g], s, self.members) for g in slots]
        codes += [0] * (batch.cap - n)  # the network on the batch the engine's own call has; only the pending rows are written
        p, v = compose(self.hip, batch.x.reshape(batch.cap, H, W), codes, game, H, W)
        batch.probs[:n] = p[:n]
        batch.value[:n] = v[:n]


@pytest.mark.parametrize("tag", ["othello6", "connect4"])
def test_engine_random_equals_the_external_route(tag):
    game, gid, H, W, A, _, make = GAMES[tag]
    _, hip = setup(tag)
    members = S.members(game, H, W, "all")
    grids, players, finals = _random_positions(make(), 8, np.random.default_rng(3))
    a = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **FIXED)
    a.set_symmetry("random")
    ev = HostDraw(hip, tag, members, GIDS, PLIES)
    b = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, evaluator=E.EVAL_EXTERNAL, **FIXED)
    b.set_evaluator(ev)
    for eng in (a, b):
        eng.set_roots(grids, players, game_ids=GIDS, plies=PLIES)
        eng.search(24)
    ra, rb = _readout(a), _readout(b)
    _same(ra, rb, tag)
    assert (ra["root_N"] == 24).all() and ra["child"].any(axis=1).all()
    assert a.stats()["net_evals"] == b.stats()["net_evals"]
    assert ev.calls == 25 and min(ev.rows) < 8  # the root one move from the end: some lock-steps had fewer pending rows than slots
    # a plain engine and an ensemble engine on the same roots search differently: the draw is really in the loop
    for other in (None, "all"):
        eng = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **FIXED)
        eng.set_symmetry(other)
        eng.set_roots(grids, players, game_ids=GIDS, plies=PLIES)
        eng.search(24)
        assert not np.array_equal(_readout(eng)["P"], ra["P"]), other
        eng.close()

    # every slot's game over: no row is pending in any pass, nothing is evaluated and nothing written
    calls, empty = ev.calls, ev.empty
    for eng in (a, b):
        eng.set_roots(np.array([f[0] for f in finals]), np.array([f[1] for f in finals], np.int8), game_ids=GIDS, plies=PLIES)
        evals = eng.stats()["net_evals"]
        eng.play([f[2] for f in finals])
        assert eng.root_status()[1].all()
        eng.search(24)
        st = eng.stats()
        assert st["net_evals"] == evals and st["error_flags"] == 0
    assert ev.empty - empty == ev.calls - calls > 0
    ra, rb = _readout(a), _readout(b)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]) and not ra[k].any(), (tag, k)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_keyed_by_the_game_not_the_slot():
    game, gid, H, W, A, _, make = GAMES["othello6"]
    _, hip = setup("othello6")
    grids, players, _ = _random_positions(make(), 8, np.random.default_rng(4))

    def run(n_slots, order, seed=SEED):
        eng = E.SelfPlayEngine(gid, H, W, n_slots=n_slots, n_sim=1, net=hip, **{**FIXED, "seed": seed})
        eng.set_symmetry("random")
        o = np.asarray(order)
        eng.set_roots(grids[o], players[o], game_ids=GIDS[o], plies=PLIES[o])
        eng.search(24)
        r = _readout(eng, n=len(o))
        eng.close()
        return {k: v[np.argsort(o)] for k, v in r.items()}  # back to game order
    want = run(8, np.arange(8))
    _same(run(8, np.arange(8)[::-1]), want, "reversed slots")
    _same(run(16, np.arange(8)), want, "16 slots")
    _same(run(16, np.array([5, 2, 7, 0, 1, 6, 3, 4])), want, "16 slots, shuffled")
    assert not np.array_equal(run(8, np.arange(8), seed=SEED + 1)["P"], want["P"])


# ------------------------------------------------------------------------------------------------------------------ 8
def test_identity_only_mask_is_the_plain_search():
    game, gid, H, W, A, _, make = GAMES["othello6"]
    _, hip = setup("othello6")
    grids, players, _ = _random_positions(make(), 8, np.random.default_rng(6))
    kw = dict(FIXED, tie_mode=E.TIE_RANDOM, noise_mode=E.NOISE_PHILOX, dirichlet_alpha=0.3, dirichlet_epsilon=0.25)
    plain = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **kw)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **kw)
    eng.set_symmetry(("random", [0]))
    for e in (plain, eng):
        e.set_roots(grids, players, game_ids=GIDS, plies=PLIES)
    for rnd in range(3):
        for e in (plain, eng):
            e.search(24)
        _same(_readout(eng), _readout(plain), rnd)
        for e in (plain, eng):
            e.advance()
    sa, sb = eng.stats(), plain.stats()
    assert sa["net_evals"] == sb["net_evals"] and sa["error_flags"] == 0 and sa["graph_replays"] == sb["graph_replays"]
    plain.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 9
def test_graphs_and_mode_switches():
    game, gid, H, W, A, _, make = GAMES["othello6"]
    _, hip = setup("othello6")
    members = S.members(game, H, W, "all")
    grids, players, _ = _random_positions(make(), 8, np.random.default_rng(9))

    def rounds(eng, n):
        out = []
        for _ in range(n):
            eng.set_roots(grids, players, game_ids=GIDS, plies=PLIES)
            eng.search(24)
            out.append(_readout(eng))
        return out
    fresh = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **FIXED)
    want_plain = rounds(fresh, 1)[0]
    fresh.close()
    eng = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **FIXED)
    eng.set_symmetry("random")
    rnd = rounds(eng, 3)  # plain launches, capture, replay
    _same(rnd[1], rnd[0], "capture")
    _same(rnd[2], rnd[0], "replay")
    replays = eng.stats()["graph_replays"]
    assert replays >= 2 and not np.array_equal(rnd[0]["P"], want_plain["P"])
    eng.set_symmetry(None)  # off: the untouched engine's search, captured anew
    for i, r in enumerate(rounds(eng, 3)):
        _same(r, want_plain, ("off", i))
    assert eng.stats()["graph_replays"] >= replays + 2
    eng.set_symmetry("all")
    ens = rounds(eng, 3)
    _same(ens[2], ens[0], "ensemble")
    assert not np.array_equal(ens[0]["P"], rnd[0]["P"]) and not np.array_equal(ens[0]["P"], want_plain["P"])
    eng.set_symmetry("random")  # the ensemble is switched off on the way: the first random result again
    for i, r in enumerate(rounds(eng, 3)):
        _same(r, rnd[0], ("random again", i))
    eng.set_symmetry("all")
    _same(rounds(eng, 1)[0], ens[0], "ensemble again")
    eng.set_symmetry("random")

    # two searches on one root: the simulation counter goes on (no replay), s = 0 .. 23
    ev = HostDraw(hip, "othello6", members, GIDS, PLIES)
    ext = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, evaluator=E.EVAL_EXTERNAL, **FIXED)
    ext.set_evaluator(ev)
    for e in (eng, ext):
        e.set_roots(grids, players, game_ids=GIDS, plies=PLIES)
        e.search(12)
    ev.new_root(s0=12, root_pass=True)  # the second search runs its (empty) root-prior pass first
    for e in (eng, ext):
        e.search(12)
    _same(_readout(eng), _readout(ext), "12 + 12")
    _same(_readout(eng), rnd[0], "12 + 12 == 24")  # K = 1: how the simulations are split over calls changes nothing
    assert ev.calls == 26 and ev.rows[13] == 0
    eng.close()
    ext.close()


# ------------------------------------------------------------------------------------------------------------------ 10
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


def lb_roots(tag):
    """othello6: two mid-game roots; tictactoe: two roots at ply 4 (terminal leaves, duplicates, K above the child count)"""
    game, _, H, W, _, _, _ = GAMES[tag]
    rng, out = np.random.default_rng(2), []
    while len(out) < 2:
        b = make_board(game, H, W)
        for _ in range(4 if tag == "tictactoe" else 9 + len(out)):
            moves = sorted(b.get_moves(), key=lambda m: cf.move_to_action(game, m, H))
            b.play_move(moves[int(rng.integers(len(moves)))])
            if b.is_game_over():
                break
        if not b.is_game_over():
            out.append(b)
    return out


@pytest.mark.parametrize("tag", ["othello6", "tictactoe"])
def test_with_leaf_batch_the_engine_equals_the_model(tag):
    game, gid, H, W, A, _, _ = GAMES[tag]
    _, hip = setup(tag)
    members = S.members(game, H, W, "all")
    roots = lb_roots(tag)
    gids, plies = np.array([1000, 1003], np.uint32), np.array([4, 5], np.int32)
    grids, players = np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8)
    kw = dict(FIXED, temp_max_step=-1, temp_min_step=0)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=2, n_sim=1, net=hip, **kw)
    eng.set_symmetry("random")  # before set_leaf_batch
    other = E.SelfPlayEngine(gid, H, W, n_slots=2, n_sim=1, net=hip, **kw)
    dups = 0
    for K in (2, 5, 16):
        for n_sim in (7, 24):
            models = []
            for b, g, ply in zip(roots, gids, plies):
                m = RandomSymmetryModel(b, K=K, tie="lowest", seed=SEED, game_id=int(g), ply=int(ply))

                def net(grid, player, A_, m=m):
                    x = torch.tensor((player * np.asarray(grid)).astype(np.float32).reshape(1, -1), device="cuda")
                    code = S.random_code(SEED, m.gid, m.ply, m.s, members)
                    p, v = hip.forward_sym_codes(x, [code])
                    return p[0].cpu().numpy(), float(v[0].cpu())
                m.net = net
                models.append(m)
            eng.set_leaf_batch(K)
            other.set_symmetry(None)
            other.set_leaf_batch(K)  # the other order: leaf_batch first, then the symmetry mode
            other.set_symmetry("random")
            c0 = eng.collisions()
            for e in (eng, other):
                e.set_roots(grids, players, game_ids=gids, plies=plies)
                e.search(n_sim)
            for s, m in enumerate(models):
                m.search(n_sim)
                compare(eng, s, m, (tag, K, n_sim, s))
                compare(other, s, m, (tag, K, n_sim, s, "other order"))
            assert eng.collisions() - c0 == sum(m.dups for m in models), (tag, K, n_sim)
            eng.advance()  # folds the slots' evaluation counts into the statistics
            assert eng.stats()["net_evals"] == sum(m.rows for m in models), (tag, K, n_sim)  # since set_roots
            dups += sum(m.dups for m in models)
    assert dups > 0 and eng.stats()["error_flags"] == 0 and other.stats()["error_flags"] == 0
    # back to one walker: the engine of test 6 (the external route with the host's draws)
    ev = HostDraw(hip, tag, members, gids, plies)
    ext = E.SelfPlayEngine(gid, H, W, n_slots=2, n_sim=1, evaluator=E.EVAL_EXTERNAL, **kw)
    ext.set_evaluator(ev)
    eng.set_leaf_batch(1)
    for e in (eng, ext):
        e.set_roots(grids, players, game_ids=gids, plies=plies)
        e.search(24)
    _same(_readout(eng), _readout(ext), "K back to 1")
    for e in (eng, other, ext):
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 11
def sort_samples(d):
    d = {k: v.cpu().numpy() for k, v in d.items()}
    order = np.lexsort((d["meta"][:, 1], d["meta"][:, 0]))
    return {k: v[order] for k, v in d.items()}


def test_self_play_wave_does_not_depend_on_the_slot_count():
    _, hip = setup("othello6")

    def wave(n_slots, sym):
        eng = E.SelfPlayEngine(0, 6, 6, n_slots=n_slots, n_sim=8, net=hip, seed=7, node_capacity=8192, sample_capacity=37 * 72)  # random ties, Philox noise
        eng.set_symmetry(sym)
        got = sort_samples(eng.run(37, first_game_id=40))
        st = eng.stats()
        assert st["games_done"] == 37 and st["error_flags"] == 0
        eng.close()
        return got
    wide, narrow, plain = wave(37, "random"), wave(5, "random"), wave(37, None)
    for k in ("state", "pi", "z", "meta", "visits"):
        assert np.array_equal(wide[k], narrow[k]), k  # 5 slots refill 32 times
    assert not (len(plain["z"]) == len(wide["z"]) and np.array_equal(plain["visits"], wide["visits"]))


# ------------------------------------------------------------------------------------------------------------------ 12
def test_players_play_with_a_random_symmetry():
    game, gid, H, W, A, _, make = GAMES["othello6"]
    net, _ = setup("othello6")
    np.random.seed(4)
    single = AlphaZeroPlayer(n_sim=8, nn=net, symmetry="random")
    res = Arena(single, GreedyPlayer(), make()).play_game(return_results=True)
    assert res["winner"] in (0, 1, 2)
    assert single.mct._engine is not None and single.symmetry == "random" and single.mct._engine._sym_mode == "random"

    games = []
    rng = np.random.default_rng(8)
    while len(games) < 8:
        b = make()
        for _ in range(len(games)):
            moves = b.get_moves()
            b.play_move(moves[int(rng.integers(len(moves)))])
        games.append(b)
    moves = []
    for _ in range(2):
        np.random.seed(11)  # the players draw their game ids from numpy's global stream
        p = BatchedAlphaZeroPlayer(n_sim=16, nn=net, n_slots=8, symmetry="random", leaf_batch=4, seed=3)
        res = p.get_moves(games, temps=0)
        moves.append([r[0] for r in res])
        assert p._hipnet.max_batch == 4 * 8 and p._engine._sym_mode == "random" and p._engine.stats()["error_flags"] == 0
        p.close()
    for b, m in zip(games, moves[0]):
        assert _action_of(b, m) in [_action_of(b, x) for x in b.get_moves()]
    assert [_action_of(b, m) for b, m in zip(games, moves[0])] == [_action_of(b, m) for b, m in zip(games, moves[1])]


# ------------------------------------------------------------------------------------------------------------------ 13
def test_trainer_self_play_with_a_random_symmetry(tmp_path):
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"

    def wave(sym):
        tr = AlphaZeroTrainer(verbose=False, engine_slots=8, seed=4, materialize_memory=False, selfplay_symmetry=sym)
        tr.game = "othello"
        tr.config = OthelloConfig(board_size=6, simulations=8, episodes=8, epochs=1, batch_size=32, iterations=1, do_eval=False, device="cuda")
        torch.manual_seed(2)
        tr.setup()
        tr.self_play(0)
        assert tr.selfplay_symmetry == sym
        return tr, {k: v.cpu().numpy() for k, v in tr.device_samples.items()}
    tr, got = wave("random")
    _, plain = wave(None)
    c = tr.config
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=8, n_sim=8, net=tr._hipnet, dirichlet_alpha=c.dirichlet_alpha, dirichlet_epsilon=c.dirichlet_epsilon,
                           temp_max_step=c.temp_max_step, temp_min_step=c.temp_min_step, seed=4, max_plies=72, sample_capacity=8 * 72)
    eng.set_symmetry("random")
    ref = sort_samples(eng.run(8, first_game_id=0))
    for k in ("state", "pi", "z", "meta", "visits"):
        assert np.array_equal(got[k], ref[k]), k
    assert not (len(plain["z"]) == len(got["z"]) and np.array_equal(plain["visits"], got["visits"]))
    eng.close()
    tr.selfplay_symmetry = "all"  # set on the attribute: refused when the wave is prepared
    with pytest.raises(ValueError, match="selfplay_symmetry"):
        tr.self_play(1)


# ------------------------------------------------------------------------------------------------------------------ 14
def _plain_search_works(eng, board, n=4):
    grids = np.tile(board.grid.astype(np.int8)[None], (n, 1, 1))
    eng.set_roots(grids, np.full(n, board.player, np.int8))
    eng.search(6)
    assert (eng.root_readout(temps=0)["root_N"].cpu().numpy() == 6).all()


def test_refusals_leave_the_handles_usable():
    L = _lib.lib()
    net6, _ = setup("othello6")
    hip6 = net6.to_hip(max_batch=16)
    o6 = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=1, net=hip6, **FIXED)
    # the two modes exclude each other at the C level (SelfPlayEngine.set_symmetry switches the other off first)
    o6.set_symmetry((0, 1))
    with pytest.raises(ValueError, match="az_engine_set_symmetry"):
        _lib.check(L.az_engine_set_symmetry_random(o6.h, 0xFF))
    _plain_search_works(o6, OthelloBoard(n=6))
    o6.set_symmetry("random")
    with pytest.raises(ValueError, match="az_engine_set_symmetry_random"):
        _lib.check(L.az_engine_set_symmetry(o6.h, 0x3))
    _plain_search_works(o6, OthelloBoard(n=6))
    # rows: K * n_slots, not 8 * n_slots -- 4 walkers of 4 slots fit 16 rows, 8 do not; the ensemble keeps refusing leaf_batch
    o6.set_leaf_batch(4)
    with pytest.raises(ValueError, match=r"32 rows.*max_batch is 16"):
        o6.set_leaf_batch(8)
    _plain_search_works(o6, OthelloBoard(n=6))
    with pytest.raises(ValueError, match="leaf_batch"):
        o6.set_symmetry((0, 1))
    assert o6._sym_mode is None  # the random mode went off on the way, the ensemble was refused
    _plain_search_works(o6, OthelloBoard(n=6))
    o6.set_leaf_batch(1)
    small = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=1, net=net6.to_hip(max_batch=2), **FIXED)
    with pytest.raises(ValueError, match=r"4 rows.*max_batch is 2"):
        small.set_symmetry("random")
    # while a search is open
    o6.set_roots(np.tile(OthelloBoard(n=6).grid.astype(np.int8)[None], (4, 1, 1)), np.ones(4, np.int8))
    o6.search_begin(6)
    with pytest.raises(_lib.AzError, match=r"\[-3\]"):
        o6.set_symmetry("random")
    o6.search_end()
    _plain_search_works(o6, OthelloBoard(n=6))

    # rotation codes on Connect4
    net4, _ = setup("connect4")
    c4 = E.SelfPlayEngine(1, 6, 7, n_slots=4, n_sim=1, net=net4.to_hip(max_batch=16), **FIXED)
    for members in ((0, 2), (4,), 0xFF):
        with pytest.raises(ValueError, match="rotation"):
            c4.set_symmetry(("random", members))
    _plain_search_works(c4, Connect4Board(width=7, height=6))
    c4.set_symmetry("random")
    _plain_search_works(c4, Connect4Board(width=7, height=6))

    # engines that do not evaluate with the HIP network
    def uniform(batch):
        batch.probs.fill_(1.0 / batch.A)
        batch.value.zero_()
    others = []
    for ev in (E.EVAL_EXTERNAL, E.EVAL_FAKE):
        eng = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=1, evaluator=ev, **FIXED)
        if ev == E.EVAL_EXTERNAL:
            eng.set_evaluator(uniform)
        with pytest.raises(ValueError, match="az_engine_set_symmetry_random needs.*AZ_EVAL_NET"):
            eng.set_symmetry("random")
        _plain_search_works(eng, OthelloBoard(n=6))
        others.append(eng)
    for eng in (o6, small, c4, *others):
        eng.close()
