"""GPU: leaf evaluation averaged over the board's symmetries (csrc/az_symmetry.hip, az_net_forward_sym, az_engine_set_symmetry).

  4. forward_sym == twins -> HipNet.forward -> mapped back -> sequential float32 mean, bit for bit;
  5. forward_sym over the whole group is equivariant (1e-6: only the summation order differs; Connect4: bit-equal);
  6. the identity mask changes nothing in a self-play wave, graph replay included;
  7. the full mask through the engine == the same composition through the external-evaluator route, bit for bit;
  8. switching the ensemble off again gives a fresh engine's search: no stale graph is replayed;
  9. refusals leave the handles usable;
 10. the players play whole games with the ensemble on.
"""
import numpy as np
import pytest
import torch

from alphazero_amd import _lib
from alphazero_amd import engine as E
from alphazero_amd import symmetry as S
from alphazero_amd.arena import Arena
from alphazero_amd.games.connect4 import Connect4Board, Connect4Net
from alphazero_amd.games.othello import OthelloBoard, OthelloNet
from alphazero_amd.games.tictactoe import TicTacToeBoard, TicTacToeNet
from alphazero_amd.mcts import _action_of
from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer, GreedyPlayer

pytestmark = pytest.mark.gpu

# tag: (game, id, H, W, A, network, board)
GAMES = {
    "othello8": ("othello", 0, 8, 8, 65, lambda: OthelloNet(8, device="cuda"), lambda: OthelloBoard(n=8)),
    "othello6": ("othello", 0, 6, 6, 37, lambda: OthelloNet(6, device="cuda"), lambda: OthelloBoard(n=6)),
    "connect4": ("connect4", 1, 6, 7, 7, lambda: Connect4Net(7, 6, device="cuda"), lambda: Connect4Board(width=7, height=6)),
    "tictactoe": ("tictactoe", 2, 3, 3, 9, lambda: TicTacToeNet(device="cuda"), lambda: TicTacToeBoard()),
}
MAX_ROWS = 8 * 130
_CACHE = {}


def setup(tag):
    """one random-init network per game and its HIP twin (room for 8 twins of 130 boards), shared by the tests and left unchanged"""
    if tag not in _CACHE:
        torch.manual_seed(sorted(GAMES).index(tag) + 20)
        net = GAMES[tag][5]()
        net.eval()
        _CACHE[tag] = (net, net.to_hip(max_batch=MAX_ROWS))
    return _CACHE[tag]


def boards(tag, B, seed):
    _, _, H, W, _, _, _ = GAMES[tag]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (B, H, W), generator=g).to(torch.float32).cuda()


def compose(hip, x, codes, game, H, W):
    """the ensemble from its parts: the twins in torch, the plain forward, each member mapped back, a sequential float32 sum in
    member order, one division by float32(n)"""
    B, n = x.shape[0], len(codes)
    twins = torch.stack([S.twin_planes(x, c) for c in codes], dim=1).contiguous()  # [B, n, H, W]: row r * n + j
    p, v = hip.forward(twins.view(B * n, H * W))
    p, v = p.view(B, n, -1), v.view(B, n)
    sp, sv = S.untwin_probs(p[:, 0], codes[0], game, H, W).clone(), v[:, 0].clone()
    for j in range(1, n):
        sp = sp + S.untwin_probs(p[:, j], codes[j], game, H, W)
        sv = sv + v[:, j]
    div = torch.tensor(float(n), dtype=torch.float32, device=x.device)
    return sp / div, sv / div


# ------------------------------------------------------------------------------------------------------------------ 4
def _mask_cases():
    out = []
    for tag in GAMES:
        masks = ["all", (0,)] + ([] if tag == "connect4" else [(0, 4), (1, 6)])
        for B in (1, 5, 70, 130):  # 8 * 70 and 8 * 130 rows cross the small-batch kernels' row limits
            for m in masks:
                out.append(pytest.param(tag, B, m, id=f"{tag}-{B}-{m if m == 'all' else ''.join(map(str, m))}"))
    return out


@pytest.mark.parametrize("tag,B,mask", _mask_cases())
def test_forward_sym_equals_its_composition(tag, B, mask):
    game, gid, H, W, A, _, _ = GAMES[tag]
    _, hip = setup(tag)
    x = boards(tag, B, seed=B)
    codes = S.members(game, H, W, mask)
    p, v = hip.forward_sym(x, mask)
    rp, rv = compose(hip, x, codes, game, H, W)
    assert p.shape == (B, A) and v.shape == (B,)
    assert torch.equal(p, rp), (tag, B, mask, (p - rp).abs().max().item())
    assert torch.equal(v, rv), (tag, B, mask, (v - rv).abs().max().item())
    if len(codes) > 1:  # the network is not equivariant: the ensemble is not the plain forward
        assert not torch.equal(p, hip.forward(x)[0])


def test_forward_sym_mask_zero_is_the_plain_forward():
    _, hip = setup("othello6")
    x = boards("othello6", 9, seed=1)
    for off in (None, 0, ()):
        p, v = hip.forward_sym(x, off)
        rp, rv = hip.forward(x)
        assert torch.equal(p, rp) and torch.equal(v, rv)


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("tag", ["othello8", "tictactoe"])
def test_full_ensemble_is_equivariant(tag):
    """T_s x has the same eight twins as x, so both calls average the same eight member outputs, in another order: 7 float32
    additions with partial sums <= 8 round by <= 8 * 2^-24 each, 3.3e-6 on the sum, 4.2e-7 after the exact division by 8; two
    orders differ by at most twice that, 8.4e-7 < 1e-6"""
    game, gid, H, W, A, _, _ = GAMES[tag]
    _, hip = setup(tag)
    x = boards(tag, 33, seed=5)
    p, v = hip.forward_sym(x, "all")
    for s in range(8):
        ps, vs = hip.forward_sym(S.twin_planes(x, s).contiguous(), "all")
        dp = (ps - S.twin_pi(p, s, game, H, W)).abs().max().item()
        dv = (vs - v).abs().max().item()
        print(f"{tag} code {s}: max |dp| {dp:.3e}, max |dv| {dv:.3e}")
        assert dp <= 1e-6 and dv <= 1e-6, (tag, s, dp, dv)
    # and it is an ensemble of a network that is not equivariant by itself
    p1, _ = hip.forward(x)
    q1, _ = hip.forward(S.twin_planes(x, 2).contiguous())
    assert (q1 - S.twin_pi(p1, 2, game, H, W)).abs().max().item() > 1e-4


def test_connect4_ensemble_is_bit_equivariant():
    game, gid, H, W, A, _, _ = GAMES["connect4"]
    _, hip = setup("connect4")
    x = boards("connect4", 33, seed=6)
    p, v = hip.forward_sym(x, (0, 1))
    ps, vs = hip.forward_sym(S.twin_planes(x, 1).contiguous(), (0, 1))
    assert torch.equal(ps, S.twin_pi(p, 1, game, H, W)) and torch.equal(vs, v)  # a two-term sum commutes


# ------------------------------------------------------------------------------------------------------------------ 6
def sort_samples(d):
    d = {k: v.cpu().numpy() for k, v in d.items()}
    order = np.lexsort((d["meta"][:, 1], d["meta"][:, 0]))
    return {k: v[order] for k, v in d.items()}


def test_identity_mask_changes_nothing():
    _, hip = setup("othello6")
    kw = dict(n_slots=8, n_sim=16, net=hip, seed=7, node_capacity=8192)
    plain = E.SelfPlayEngine(0, 6, 6, **kw)
    ref = sort_samples(plain.run(8, first_game_id=40))
    eng = E.SelfPlayEngine(0, 6, 6, **kw)
    eng.set_symmetry((0,))
    got = sort_samples(eng.run(8, first_game_id=40))
    for k in ("state", "pi", "z", "meta", "visits"):
        assert np.array_equal(got[k], ref[k]), k
    st, rst = eng.stats(), plain.stats()
    assert st["games_done"] == 8 and st["net_evals"] == rst["net_evals"]
    assert st["graph_replays"] > 0 and rst["graph_replays"] > 0  # a wave is one search per ply: captured at the second, replayed after
    plain.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 7
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


def _readout(eng):
    r = eng.root_readout(temps=0)
    return {k: r[k].cpu().numpy() for k in ("visits", "Q", "P", "child", "root_N")}


FIXED = dict(tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, dirichlet_alpha=None, dirichlet_epsilon=None, node_capacity=8192)


@pytest.mark.parametrize("tag", ["othello6", "connect4"])
def test_engine_ensemble_equals_the_external_route(tag):
    game, gid, H, W, A, _, make_board = GAMES[tag]
    _, hip = setup(tag)
    codes = S.members(game, H, W, "all")
    grids, players, finals = _random_positions(make_board(), 8, np.random.default_rng(3))
    a = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **FIXED)
    a.set_symmetry("all")
    seen = {"calls": 0, "rows": [], "empty": 0}

    def evaluator(batch):  # the composition of test 4 on the engine's rows; only the pending ones are written
        n = int(batch.count[0].item())
        seen["calls"] += 1
        seen["rows"].append(n)
        if n == 0:
            seen["empty"] += 1
            return
        p, v = compose(hip, batch.x.reshape(batch.cap, H, W), codes, game, H, W)
        batch.probs[:n] = p[:n]
        batch.value[:n] = v[:n]
    b = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, evaluator=E.EVAL_EXTERNAL, **FIXED)
    b.set_evaluator(evaluator)
    for eng in (a, b):
        eng.set_roots(grids, players)
        eng.search(24)
    ra, rb = _readout(a), _readout(b)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), (tag, k)
    assert (ra["root_N"] == 24).all() and ra["child"].any(axis=1).all()
    assert a.stats()["net_evals"] == b.stats()["net_evals"]
    assert min(seen["rows"]) < 8  # the root one move from the end: some lock-steps had fewer pending rows than slots
    # a plain engine on the same roots searches differently: the ensemble is really in the loop
    plain = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **FIXED)
    plain.set_roots(grids, players)
    plain.search(24)
    rp = _readout(plain)
    assert not np.array_equal(rp["P"], ra["P"])

    # every slot's game over: no row is pending in any pass, nothing is evaluated and nothing written
    before = dict(seen)
    for eng in (a, b):
        eng.set_roots(np.array([f[0] for f in finals]), np.array([f[1] for f in finals], np.int8))
        evals = eng.stats()["net_evals"]
        eng.play([f[2] for f in finals])
        assert eng.root_status()[1].all()
        eng.search(24)
        st = eng.stats()
        assert st["net_evals"] == evals and st["error_flags"] == 0
    assert seen["empty"] - before["empty"] == seen["calls"] - before["calls"] > 0
    ra, rb = _readout(a), _readout(b)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]) and not ra[k].any(), (tag, k)
    for eng in (a, b, plain):
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ 8
def test_switching_the_ensemble_off_replays_no_stale_graph():
    game, gid, H, W, A, _, make_board = GAMES["othello6"]
    _, hip = setup("othello6")
    grids, players, _ = _random_positions(make_board(), 8, np.random.default_rng(9))
    fresh = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **FIXED)
    fresh.set_roots(grids, players)
    fresh.search(24)
    want = _readout(fresh)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=8, n_sim=1, net=hip, **FIXED)
    eng.set_symmetry("all")
    for _ in range(3):  # plain launches, capture, replay
        eng.set_roots(grids, players)
        eng.search(24)
    with_sym = _readout(eng)
    replays = eng.stats()["graph_replays"]
    assert replays >= 2 and not np.array_equal(with_sym["P"], want["P"])
    eng.set_symmetry(None)
    for i in range(3):
        eng.set_roots(grids, players)
        eng.search(24)
        got = _readout(eng)
        for k in want:
            assert np.array_equal(got[k], want[k]), (i, k)
    assert eng.stats()["graph_replays"] >= replays + 2  # the plain sequence was captured anew
    eng.set_symmetry("all")  # and back on: the first ensemble result again
    eng.set_roots(grids, players)
    eng.search(24)
    got = _readout(eng)
    for k in want:
        assert np.array_equal(got[k], with_sym[k]), k
    fresh.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 9
def _plain_search_works(eng, board, n=4):
    grids = np.tile(board.grid.astype(np.int8)[None], (n, 1, 1))
    eng.set_roots(grids, np.full(n, board.player, np.int8))
    eng.search(6)
    assert (eng.root_readout(temps=0)["root_N"].cpu().numpy() > 0).all()


def test_refusals_leave_the_handles_usable():
    # a rotation on Connect4
    net4, _ = setup("connect4")
    hip4 = net4.to_hip(max_batch=16)
    c4 = E.SelfPlayEngine(1, 6, 7, n_slots=4, n_sim=1, net=hip4, **FIXED)
    for mask in ((0, 2), (4,), 0xFF):
        with pytest.raises(ValueError, match="rotation"):
            c4.set_symmetry(mask)
    with pytest.raises(ValueError, match="rotation"):
        hip4.forward_sym(boards("connect4", 2, seed=1), (0, 6))
    _plain_search_works(c4, Connect4Board(width=7, height=6))
    c4.set_symmetry("all")  # 2 * 4 rows fit
    _plain_search_works(c4, Connect4Board(width=7, height=6))

    # a network too small for n twins of every slot
    net6, _ = setup("othello6")
    hip6 = net6.to_hip(max_batch=16)
    o6 = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=1, net=hip6, **FIXED)
    with pytest.raises(ValueError, match=r"32 rows.*max_batch is 16"):
        o6.set_symmetry("all")
    _plain_search_works(o6, OthelloBoard(n=6))
    o6.set_symmetry((0, 1, 4, 5))  # 4 * 4 rows fit

    # az_net_forward_sym beyond max_batch
    x = boards("othello6", 3, seed=2)
    with pytest.raises(ValueError, match=r"24 rows.*max_batch is 16"):
        hip6.forward_sym(x, "all")
    p, v = hip6.forward_sym(x, (0, 1))
    rp, rv = compose(hip6, x, [0, 1], "othello", 6, 6)
    assert torch.equal(p, rp) and torch.equal(v, rv)

    # while a search is open
    o6.set_roots(np.tile(OthelloBoard(n=6).grid.astype(np.int8)[None], (4, 1, 1)), np.ones(4, np.int8))
    o6.search_begin(6)
    with pytest.raises(_lib.AzError, match=r"\[-3\]"):
        o6.set_symmetry(None)
    o6.search_end()
    _plain_search_works(o6, OthelloBoard(n=6))

    # engines that do not evaluate with the HIP network
    def uniform(batch):
        batch.probs.fill_(1.0 / batch.A)
        batch.value.zero_()
    others = []
    for ev in (E.EVAL_EXTERNAL, E.EVAL_FAKE, E.EVAL_ROLLOUT):
        eng = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=1, evaluator=ev, **FIXED)
        if ev == E.EVAL_EXTERNAL:
            eng.set_evaluator(uniform)
        with pytest.raises(ValueError, match="AZ_EVAL_NET"):
            eng.set_symmetry((0, 1))
        _plain_search_works(eng, OthelloBoard(n=6))
        others.append(eng)
    for eng in (c4, o6, *others):
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("tag", ["tictactoe", "othello6"])
def test_players_play_with_the_ensemble(tag):
    game, gid, H, W, A, _, make_board = GAMES[tag]
    net, _ = setup(tag)
    np.random.seed(4)
    player = BatchedAlphaZeroPlayer(n_sim=16, nn=net, n_slots=4, symmetry="all")
    games = [make_board() for _ in range(3)]
    for _ in range(2 * H * W + 2):
        live = [None if b.is_game_over() else b for b in games]
        if not any(b is not None for b in live):
            break
        res = player.get_moves(live, temps=0)
        moves = [None if r is None else r[0] for r in res]
        for b, m in zip(games, moves):
            if m is not None:
                b.play_move(m)  # raises ValueError for an illegal move
        player.apply_moves(moves)
    assert all(b.is_game_over() for b in games)
    assert player._hipnet.max_batch == 8 * 4 and player._engine.stats()["error_flags"] == 0
    player.close()

    single = AlphaZeroPlayer(n_sim=16, nn=net, symmetry="all")
    res = Arena(single, GreedyPlayer(), make_board()).play_game(return_results=True)
    assert res["winner"] in (0, 1, 2)
    assert single.mct._engine is not None and single.symmetry == "all"
