"""GPU: the batched root readout (az_engine_root_readout / SelfPlayEngine.root_readout) and the many-games players on top of it.

The yardsticks are the engine's own one-slot paths, which the other suites pin against the oracle: root_children(slot) for the tree
statistics, what advance() records (samples: pi, visits, the move) for the policy and the draw, best_moves() for temperature 0.
Fake-network engines throughout (no weights needed) except the two player tests.  37 slots: two full blocks of 16 games and a
partial one, a partial wavefront in it.  set_roots(..., game_ids=arange(n)) and manual search / advance loops never refill a
slot, so slot g is game g."""
import numpy as np
import pytest
import torch

from conftest import TAGS
from alphazero_amd import engine as E
from alphazero_amd._lib import AzError

pytestmark = pytest.mark.gpu
G = 37


def start_grids(tag, n=G):
    game, gid, H, W, A, _ = TAGS[tag]
    g = np.zeros((H, W), np.int8)
    if game == "othello":
        h = H // 2
        g[h - 1, h - 1] = g[h, h] = 1
        g[h - 1, h] = g[h, h - 1] = -1
    return np.tile(g[None], (n, 1, 1)), np.ones(n, np.int8)


def engine(tag, n_sim, plies=None, **kw):
    game, gid, H, W, A, _ = TAGS[tag]
    kw.setdefault("seed", 11)
    eng = E.SelfPlayEngine(gid, H, W, n_slots=G, n_sim=n_sim, evaluator=E.EVAL_FAKE, node_capacity=8192, **kw)
    grids, players = start_grids(tag)
    eng.set_roots(grids, players, game_ids=np.arange(G), plies=plies)
    return eng


def host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def per_slot(eng, slot, A):
    """the dense rows of one slot, scattered from the one-slot path"""
    a, N, Q, P, root_n = eng.root_children(slot)
    out = {"visits": np.zeros(A, np.int32), "Q": np.zeros(A, np.float64), "P": np.zeros(A, np.float64), "child": np.zeros(A, np.uint8)}
    out["visits"][a], out["Q"][a], out["P"][a], out["child"][a] = N, Q, P, 1
    out["root_N"] = np.int32(root_n if len(a) else 0)
    return out


def assert_unserved(h, g, pv=False):
    assert h["action"][g] == -1 and h["root_N"][g] == 0, g
    for k in ("visits", "pi", "Q", "P", "child"):
        assert not h[k][g].any(), (k, g)
    if pv:
        assert (h["pv"][g] == -1).all(), g


def assert_equals_per_slot(eng, h, g, A):
    ref = per_slot(eng, g, A)
    for k in ("visits", "child", "root_N"):
        assert np.array_equal(h[k][g], ref[k]), (k, g)
    for k in ("Q", "P"):  # as bit patterns
        assert np.array_equal(h[k][g].view(np.uint64), ref[k].view(np.uint64)), (k, g)
    assert h["action"][g] >= 0 and h["child"][g, h["action"][g]] == 1 and h["pi"][g, h["action"][g]] > 0, g


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["othello8", "connect4", "tictactoe"])
def test_readout_equals_the_per_slot_path(tag):
    """production mode (random ties, Philox noise), after 0, 1 and 3 advances -- and after 6 and 8, when some TicTacToe games are
    over.  The slots start at ply counters 0..3, so they sit at different points of the temperature schedule."""
    A = TAGS[tag][4]
    eng = engine(tag, 24, plies=np.arange(G) % 4, max_plies=160)
    finished = 0
    for moved in range(9):
        eng.search(24)
        if moved in (0, 1, 3, 6, 8):
            h = host(eng.root_readout())
            assert h["visits"].shape == (G, A) and h["Q"].dtype == np.float64 and h["pi"].dtype == np.float32
            over = eng.root_status()[1]
            for g in range(G):
                if over[g]:
                    assert_unserved(h, g)
                    finished += 1
                else:
                    assert_equals_per_slot(eng, h, g, A)
        eng.advance()
    if tag == "tictactoe":
        assert finished > 0  # the finished-slot branch was reached
    eng.close()


# 2, 3 ---------------------------------------------------------------------------------------------------------------
def play_out(tag, tie_mode, reads, n_sim=20, pv_len=0):
    """every game to its end: search; `reads` readouts; advance.  Returns the samples sorted by (game, ply) and, per ply, the
    host copies of that ply's readouts."""
    eng = engine(tag, n_sim, temp_max_step=1, temp_min_step=6, tie_mode=tie_mode)
    log = []
    for _ in range(2 * TAGS[tag][2] * TAGS[tag][3] + 2):
        if eng.root_status()[1].all():
            break
        eng.search(n_sim)
        log.append([host(eng.root_readout(pv_len=pv_len)) for _ in range(reads)])
        eng.advance()
    else:
        raise AssertionError("games did not finish")
    s = host(eng.samples())
    order = np.lexsort((s["meta"][:, 1], s["meta"][:, 0]))
    eng.close()
    return {k: v[order] for k, v in s.items()}, log


@pytest.mark.parametrize("tie_mode", [E.TIE_RANDOM, E.TIE_LOWEST])
@pytest.mark.parametrize("tag", ["othello6", "connect4"])
def test_readout_equals_what_advance_records(tag, tie_mode):
    """temp_max_step 1 / temp_min_step 6: every game passes through tau = 1, 0.8 ... 0.2 and 0"""
    s, log = play_out(tag, tie_mode, reads=1)
    served = sum(int((ply[0]["action"] >= 0).sum()) for ply in log)
    assert served == len(s["z"]) and len(log) > 6
    for i in range(len(s["z"])):
        g, k = s["meta"][i, 0], s["meta"][i, 1]
        r = log[k][0]
        assert np.array_equal(r["pi"][g], s["pi"][i]), (g, k)
        assert np.array_equal(r["visits"][g], s["visits"][i]), (g, k)
        assert r["action"][g] == s["meta"][i, 3], (g, k)


def test_reading_changes_nothing():
    base, _ = play_out("connect4", E.TIE_RANDOM, reads=0)
    once, _ = play_out("connect4", E.TIE_RANDOM, reads=1)
    twice, log = play_out("connect4", E.TIE_RANDOM, reads=2, pv_len=4)
    for k in base:
        assert np.array_equal(base[k], once[k]) and np.array_equal(base[k], twice[k]), k
    for first, second in log:
        for k in first:
            assert np.array_equal(first[k], second[k]), k


# 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie_mode", [E.TIE_RANDOM, E.TIE_LOWEST])
def test_explicit_temperatures(tie_mode):
    eng = engine("othello6", 30, tie_mode=tie_mode)
    eng.search(30)
    eng.advance()
    eng.search(30)
    temps = np.array([0, 1, 0.5, 0.25, 2.0])[np.arange(G) % 5]
    h = host(eng.root_readout(temps=temps))
    best = eng.best_moves()
    for g in range(G):
        pi, a = h["pi"][g], h["action"][g]
        if temps[g] == 0:
            assert a == best[g] and pi[a] == 1 and pi.sum() == 1 and np.count_nonzero(pi) == 1, g
        else:
            w = h["visits"][g].astype(np.float64) ** (1.0 / temps[g])
            assert np.abs(pi - w / w.sum()).max() <= 1e-7, g  # the project's bound for float32 pi (test_gpu_engine.py)
            assert h["child"][g, a] == 1 and pi[a] > 0, g
    # one temperature for all slots is the same as a vector of it
    one = host(eng.root_readout(temps=0.5))
    vec = host(eng.root_readout(temps=np.full(G, 0.5)))
    assert all(np.array_equal(one[k], vec[k]) for k in one)
    eng.close()


# 5 ------------------------------------------------------------------------------------------------------------------
def test_principal_line():
    eng = engine("othello6", 100)
    eng.search(100)
    pv = host(eng.root_readout(pv_len=6))["pv"]
    assert pv.shape == (G, 6)
    live = np.ones(G, bool)
    for i in range(6):
        for g in np.flatnonzero(live):
            a, N, _, _, _ = eng.root_children(g)
            if len(a) == 0 or N.max() == 0:  # the line ends exactly here
                assert (pv[g, i:] == -1).all(), (g, i)
                live[g] = False
                continue
            order = np.argsort(a, kind="stable")
            top = order[np.argmax(N[order])]  # the first maximum of N over ascending actions
            assert N[top] > 0 and pv[g, i] == a[top], (g, i)
        assert (pv[~live, i] == -1).all()
        if live.any():
            eng.play(np.where(live, pv[:, i], -1))
    assert (pv[:, 0] >= 0).all() and (pv[:, 1] >= 0).any()
    eng.close()


# 6 ------------------------------------------------------------------------------------------------------------------
def test_arena_mode_serves_the_engines_colour_only():
    A = TAGS["othello6"][4]
    eng = engine("othello6", 20, dirichlet_alpha=None, dirichlet_epsilon=None, noise_mode=E.NOISE_OFF)
    sides = np.array([1, -1, 0])[np.arange(G) % 3].astype(np.int8)
    eng.set_sides(sides)
    for to_move in (1, -1):
        eng.search(20)
        h = host(eng.root_readout(pv_len=3))
        for g in range(G):
            if sides[g] in (0, to_move):
                assert_equals_per_slot(eng, h, g, A)
                assert h["pv"][g, 0] >= 0
            else:
                assert_unserved(h, g, pv=True)
        mine, other = eng.best_moves(), eng.baseline_moves("random", seed=3)
        assert np.array_equal(mine >= 0, h["action"] >= 0)
        eng.play(np.where(mine >= 0, mine, other))
    eng.close()


# 7 ------------------------------------------------------------------------------------------------------------------
def test_fewer_rows_than_slots_leave_the_rest_untouched():
    A, n = TAGS["connect4"][4], 21
    eng = engine("connect4", 20)
    eng.search(20)
    full = host(eng.root_readout(pv_len=4))
    out = {"visits": torch.full((G, A), 77, dtype=torch.int32), "pi": torch.full((G, A), 7.0), "Q": torch.full((G, A), 7.0, dtype=torch.float64),
           "P": torch.full((G, A), 7.0, dtype=torch.float64), "child": torch.full((G, A), 9, dtype=torch.uint8),
           "action": torch.full((G,), 55, dtype=torch.int32), "root_N": torch.full((G,), 55, dtype=torch.int32),
           "pv": torch.full((G, 4), 33, dtype=torch.int32)}
    out = {k: v.cuda() for k, v in out.items()}
    sentinel = host(out)
    r = eng.root_readout(pv_len=4, n=n, out=out)
    assert all(r[k] is out[k] for k in out)
    h = host(r)
    for k in h:
        assert np.array_equal(h[k][:n], full[k][:n]), k
        assert np.array_equal(h[k][n:], sentinel[k][n:]), k
    small = host(eng.root_readout(pv_len=4, n=n))  # allocated by the call: n rows
    assert all(small[k].shape[0] == n and np.array_equal(small[k], full[k][:n]) for k in small)
    eng.close()


# 8 ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    eng = engine("tictactoe", 10)
    eng.search(10)
    bad = np.zeros(G)
    bad[5], bad[9] = -0.5, -1
    with pytest.raises(ValueError, match="slot 5 "):
        eng.root_readout(temps=bad)
    bad[5], bad[9] = 1, np.nan
    with pytest.raises(ValueError, match="slot 9 "):
        eng.root_readout(temps=bad)
    with pytest.raises(ValueError, match="not finite"):
        eng.root_readout(temps=np.inf)
    with pytest.raises(ValueError, match="n must be"):
        eng.root_readout(n=0)
    with pytest.raises(ValueError, match="n must be"):
        eng.root_readout(n=G + 1)
    with pytest.raises(ValueError, match="pv_len"):
        eng.root_readout(pv_len=17)
    with pytest.raises(ValueError, match="pv_len"):
        eng.root_readout(pv_len=0, out={"pv": torch.zeros((G, 4), dtype=torch.int32, device="cuda")})
    before = host(eng.root_readout())
    eng.search_begin(10)
    try:
        with pytest.raises(AzError, match=r"\[-3\].*has not been ended"):
            eng.root_readout()
    finally:
        eng.search_end()  # the search still ends cleanly
    after = host(eng.root_readout())
    assert (after["root_N"] == before["root_N"] + 10).all()
    eng.close()


# 9 ------------------------------------------------------------------------------------------------------------------
def test_batched_players_equal_the_single_game_players(monkeypatch):
    from alphazero_amd import mcts
    from alphazero_amd.games.othello import OthelloBoard, OthelloNet
    from alphazero_amd.games.tictactoe import TicTacToeBoard
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer, BatchedMCTSPlayer
    torch.manual_seed(4)
    net = OthelloNet(n=6).eval()
    np.random.seed(5)
    b, boards = OthelloBoard(n=6), []
    for ply in range(19):
        if ply in (0, 3, 7, 12, 18):
            boards.append(b.clone())
        b.play_move(b.get_random_move())
    # ties pinned to the lowest action on both sides: on the device (TIE_LOWEST) and in the single player's host-side fair_max
    # over the visit counts (mcts.py:110-112), which would otherwise draw among equally visited moves
    monkeypatch.setattr(mcts, "fair_max", lambda elements, key=lambda x: x: max(list(elements), key=key))
    single = AlphaZeroPlayer(n_sim=20, nn=net)
    single.mct._tie_mode = E.TIE_LOWEST
    many = BatchedAlphaZeroPlayer(n_sim=20, nn=net, n_slots=8)
    many._tie_mode = E.TIE_LOWEST
    got = many.get_moves(boards, temps=0)
    assert len(got) == len(boards)
    for board, (move, probs, visits, priors) in zip(boards, got):
        m1, p1, v1, pr1 = single.get_move(board, 0)
        assert visits == v1 and move == m1 and probs == p1 == {move: 1}, (visits, v1, move, m1)
        assert list(visits) == list(v1) and priors.keys() == pr1.keys()
        assert max(abs(priors[k] - pr1[k]) for k in pr1) <= 1e-12
    many.close()
    # rollout trees: the playouts are keyed by game ids that each MCT draws for itself, so the streams differ from MCTSPlayer's;
    # checked instead: every simulation is in the visit counts, the moves are legal, priors are None as in MCT.get_prior_probs
    t = TicTacToeBoard()
    tb = [t.clone()]
    for mv in ((1, 1), (0, 0)):
        t.play_move(mv)
        tb.append(t.clone())
    roll = BatchedMCTSPlayer(n_sim=30, n_slots=4)
    for board, (move, probs, visits, priors) in zip(tb, roll.get_moves(tb, temps=[0, 1, 0.5])):
        assert sum(visits.values()) == 30 and board.is_legal_move(move) and set(visits) == set(board.get_moves())
        assert set(priors) == set(visits) and all(p is None for p in priors.values())
        assert abs(sum(probs.values()) - 1) < 1e-6 and probs[move] > 0
    roll.close()


# 10 -----------------------------------------------------------------------------------------------------------------
def test_whole_games_against_host_moves(monkeypatch):
    from alphazero_amd.games.othello import OthelloBoard, OthelloNet
    from alphazero_amd.players import BatchedAlphaZeroPlayer, RandomPlayer
    calls = []
    real = E.SelfPlayEngine.set_roots
    monkeypatch.setattr(E.SelfPlayEngine, "set_roots", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    torch.manual_seed(1)
    net = OthelloNet(n=6).eval()
    np.random.seed(8)
    n_sim, opponent = 12, RandomPlayer()
    player = BatchedAlphaZeroPlayer(n_sim=n_sim, nn=net, n_slots=8, dirichlet_alpha=0.3, dirichlet_epsilon=0.25)
    boards = [OthelloBoard(n=6) for _ in range(8)]
    for b in boards[1::2]:  # the opponent opens every second game
        b.play_move(opponent.get_move(b)[0])
    for turn in range(80):
        asked = [None if b.is_game_over() else b for b in boards]
        if all(b is None for b in asked):
            break
        got = player.get_moves(asked, temps=0 if turn > 2 else 1)
        moves = [None] * 8
        for i, b in enumerate(asked):
            if b is None:
                assert got[i] is None
                continue
            move, probs, visits, priors = got[i]
            assert b.is_legal_move(move) and set(visits) == set(b.get_moves()) and sum(visits.values()) >= n_sim
            b.play_move(move)
            moves[i] = move
        player.apply_moves(moves)
        replies = [None if b.is_game_over() else opponent.get_move(b)[0] for b in boards]
        for b, mv in zip(boards, replies):
            if mv is not None:
                b.play_move(mv)
        player.apply_moves(replies)
    else:
        raise AssertionError("games did not finish")
    assert all(b.is_game_over() for b in boards)
    assert len(calls) == 1  # the trees were carried from move to move
    with pytest.raises(ValueError, match="game over"):
        player.get_moves(boards)
    # a list in another order no longer matches the slots: every tree restarts, and the answers are as valid
    fresh = []
    for i in range(8):
        b = OthelloBoard(n=6)
        for _ in range(i):
            b.play_move(b.get_random_move())
        fresh.append(b)
    first = player.get_moves(fresh, temps=0)
    assert len(calls) == 2
    again = player.get_moves(fresh, temps=0)
    assert len(calls) == 2 and all(sum(a[2].values()) == sum(f[2].values()) + n_sim for a, f in zip(again, first))
    shuffled = player.get_moves(fresh[::-1], temps=0)
    assert len(calls) == 3
    for b, (move, probs, visits, priors) in zip(fresh[::-1], shuffled):
        assert b.is_legal_move(move) and sum(visits.values()) == n_sim and abs(sum(priors.values()) - 1) < 1e-5
    r, lines = player.analyze(fresh[::-1], pv_len=4)
    assert len(calls) == 3 and r["pv"].shape == (8, 4) and r["visits"].is_cuda
    for b, line in zip(fresh[::-1], lines):
        assert 1 <= len(line) <= 4
        c = b.clone()
        for mv in line:
            c.play_move(mv)  # a principal line is a sequence of legal moves
    player.close()
