"""GPU: searches whose leaves are evaluated outside the engine (AZ_EVAL_EXTERNAL, az_engine_set_evaluator).

  1. the golden G3 trees through the board path (the reference's fake net, whose evaluate() is overridden);
  2. external evaluation of the fake net == the built-in EVAL_FAKE bit for bit on production-mode self-play;
  3. the batched path (TorchEvaluator) == the board path bit for bit on a closed-form network with dyadic outputs;
  4. the batched path on the stock networks == the HIP network's root priors;
  5. errors: an exception in the evaluator, rejected outputs, re-entry;
  6. end to end: a user-defined architecture plays an Arena game and trains one AlphaZeroTrainer iteration.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import TAGS, golden
from alphazero_amd import _lib, base
from alphazero_amd import engine as E
from alphazero_amd.arena import Arena
from alphazero_amd.base import PolicyValueNetwork
from alphazero_amd.evaluators import BoardEvaluator, TorchEvaluator
from alphazero_amd.games.connect4 import Connect4Net
from alphazero_amd.games.othello import OthelloBoard, OthelloConfig, OthelloNet
from alphazero_amd.games.tictactoe import TicTacToeNet
from alphazero_amd.mcts import MCT, _move_of
from alphazero_amd.players import AlphaZeroPlayer, GreedyPlayer
from alphazero_amd.trainer import AlphaZeroTrainer
from tools import closed_form as cf

pytestmark = pytest.mark.gpu
MCT_TAGS = ["othello8", "othello6", "connect4", "tictactoe"]


def fake_net(tag):
    """tools/gen_golden.py fake_net_class: a subclass of the stock net whose evaluate() is the closed-form fake network"""
    game, gid, H, W, A, n = TAGS[tag]
    base_cls = {"othello": OthelloNet, "connect4": Connect4Net, "tictactoe": TicTacToeNet}[game]

    class FakeNet(base_cls):
        def evaluate(self, board):  # base.py:357-367 with the closed-form net in place of predict()
            probs, v_net = cf.fakenet(board.grid, board.player, A)
            return probs, board.player * v_net
    if game == "othello":
        return FakeNet(n=n)
    if game == "connect4":
        return FakeNet(board_width=W, board_height=H)
    return FakeNet()


def sort_samples(d):
    d = {k: v.cpu().numpy() for k, v in d.items()}
    order = np.lexsort((d["meta"][:, 1], d["meta"][:, 0]))
    return {k: v[order] for k, v in d.items()}


def external(gid, H, W, slots, n_sim, fn, **kw):
    eng = E.SelfPlayEngine(gid, H, W, n_slots=slots, n_sim=n_sim, evaluator=E.EVAL_EXTERNAL, **kw)
    eng.set_evaluator(fn)
    return eng


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("tag", MCT_TAGS)
def test_g3_through_the_board_path(tag):
    game, gid, H, W, A, n = TAGS[tag]
    fx = golden(f"mct_{tag}.npz")
    ro, stage = fx["row_off"], fx["stage"]
    starts = np.flatnonzero(stage == 0)
    net = fake_net(tag)

    def same(a, N, Q, P, rootn, rec):
        sl = slice(ro[rec], ro[rec + 1])
        assert np.array_equal(a, fx["action"][sl]), (tag, rec)
        assert np.array_equal(N, fx["N"][sl]), (tag, rec)
        assert rootn == fx["rootN"][rec]
        assert np.abs(Q - fx["Q"][sl]).max() <= 1e-12
        assert np.abs(P - fx["P"][sl]).max() <= 1e-12

    for noise in (0, 1):
        cases = [s for s in starts if fx["noise"][s] == noise]
        ev = BoardEvaluator(net, game, H, W)
        eng = external(gid, H, W, len(cases), 100, ev, dirichlet_alpha=0.03 if noise else None,
                       dirichlet_epsilon=0.25 if noise else None, temp_max_step=-1, temp_min_step=0, tie_mode=E.TIE_LOWEST,
                       noise_mode=E.NOISE_HASH if noise else E.NOISE_OFF, node_capacity=8192)
        eng.set_roots(np.array([fx["grids"][s] for s in cases]), np.array([fx["players"][s] for s in cases]))
        for k, sims in enumerate((1, 1, 8, 90)):
            eng.search(sims)
            for slot, s in enumerate(cases):
                same(*eng.root_children(slot), s + k)
        eng.advance()  # tau = 0 move (lowest-index tie-break), tree reuse
        eng.search(100)
        for slot, s in enumerate(cases):
            if s + 4 < len(stage) and stage[s + 4] == 4:
                same(*eng.root_children(slot), s + 4)
        st = eng.stats()
        assert st["graph_replays"] == 0
        eng.close()

        # the single-game MCT mirror itself, with its private deterministic modes
        for s in cases[:2]:
            b = _board(game, H, W, fx["grids"][s].astype(np.float64), int(fx["players"][s]))
            mct = MCT(eval_method="neural", nn=net, dirichlet_alpha=0.03 if noise else None, dirichlet_epsilon=0.25 if noise else None)
            mct._tie_mode, mct._noise_mode = E.TIE_LOWEST, E.NOISE_HASH
            for k, sims in enumerate((1, 1, 8, 90)):
                mct.search(b, n_sim=sims)
                same(*mct._engine.root_children(0), s + k)
            assert isinstance(mct._evaluator, BoardEvaluator)
            if s + 4 < len(stage) and stage[s + 4] == 4:
                move = _move_of(b, int(fx["moved"][s + 4]))
                mct.change_root(move)
                b.play_move(move)
                mct.search(b, n_sim=100)
                same(*mct._engine.root_children(0), s + 4)


def _board(game, H, W, grid, player):
    from alphazero_amd.games.connect4 import Connect4Board
    from alphazero_amd.games.tictactoe import TicTacToeBoard
    if game == "othello":
        return OthelloBoard(n=H, grid=grid, player=player)
    if game == "connect4":
        return Connect4Board(width=W, height=H, grid=grid, player=player)
    return TicTacToeBoard(grid=grid, player=player)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("tag,n_games,slots,n_sim", [("othello6", 12, 8, 12), ("othello8", 10, 6, 10), ("connect4", 16, 10, 12),
                                                     ("tictactoe", 24, 10, 12)])
def test_external_board_path_equals_builtin_fake(tag, n_games, slots, n_sim):
    game, gid, H, W, A, n = TAGS[tag]
    kw = dict(seed=5, node_capacity=8192, sample_capacity=n_games * 2 * H * W)
    ref_eng = E.SelfPlayEngine(gid, H, W, n_slots=slots, n_sim=n_sim, evaluator=E.EVAL_FAKE, **kw)
    ref = sort_samples(ref_eng.run(n_games, first_game_id=300))
    ev = BoardEvaluator(fake_net(tag), game, H, W)
    eng = external(gid, H, W, slots, n_sim, ev, **kw)
    got = sort_samples(eng.run(n_games, first_game_id=300))
    for k in ("state", "pi", "z", "meta", "visits"):
        assert np.array_equal(got[k], ref[k]), (tag, k)
    st, rst = eng.stats(), ref_eng.stats()
    assert st["games_done"] == n_games and st["net_evals"] == rst["net_evals"]
    assert ev.calls == st["net_evals"]  # root passes included
    assert st["graph_replays"] == 0


# ------------------------------------------------------------------------------------------------------------------ 3
class ClosedFormNet(PolicyValueNetwork):
    """predict() in integer torch ops on the device: dyadic probabilities and values, exact in float32"""

    def __init__(self, A):
        super().__init__()
        self.A, self.device = A, torch.device("cuda")

    def predict(self, input):
        c = (input.reshape(input.shape[0], -1).round().to(torch.int64) + 1)
        w = (torch.arange(c.shape[1], device=c.device) * 7 + 3) % 11 + 1
        h = (c * w).sum(1, keepdim=True)  # [B, 1]
        a = torch.arange(self.A, device=c.device)[None]
        num = 1 + (h * (a + 1) * 40503 + a * 97) % 64
        v = (h[:, 0] * 2654435761 % 1025) - 512
        return num.to(torch.float32) / 4096.0, (v.to(torch.float32) / 512.0)[:, None]


class ClosedFormTwin(ClosedFormNet):
    """the same function in numpy, one board at a time (the board path)"""

    def evaluate(self, board):
        c = (board.player * board.grid).reshape(-1).astype(np.int64) + 1
        w = (np.arange(c.size) * 7 + 3) % 11 + 1
        h = int((c * w).sum())
        a = np.arange(self.A)
        num = 1 + (h * (a + 1) * 40503 + a * 97) % 64
        v = (h * 2654435761 % 1025) - 512
        return (num.astype(np.float32) / np.float32(4096.0)), board.player * float(np.float32(v) / np.float32(512.0))


@pytest.mark.parametrize("slots", [16, 5])
def test_batched_path_equals_board_path(slots):
    gid, H, W, A, n_games = 0, 6, 6, 37, 16
    kw = dict(seed=8, node_capacity=8192, sample_capacity=n_games * 2 * H * W)
    out = []
    for ev in (TorchEvaluator(ClosedFormNet(A)), BoardEvaluator(ClosedFormTwin(A), "othello", H, W)):
        eng = external(gid, H, W, slots, 10, ev, **kw)
        out.append((sort_samples(eng.run(n_games, first_game_id=50)), eng.stats()))
        eng.close()
    (a, sa), (b, sb) = out
    for k in ("state", "pi", "z", "meta", "visits"):
        assert np.array_equal(a[k], b[k]), k
    assert sa["net_evals"] == sb["net_evals"] and sa["games_done"] == n_games


# ------------------------------------------------------------------------------------------------------------------ 4
def _random_positions(board, count, rng):
    grids, players = [], []
    while len(grids) < count:
        b = board.clone()
        b.reset()
        for _ in range(int(rng.integers(0, 12))):
            if b.is_game_over():
                break
            moves = b.get_moves()
            b.play_move(moves[int(rng.integers(len(moves)))])
        if not b.is_game_over():
            grids.append(b.grid.astype(np.int8))
            players.append(b.player)
    return np.array(grids), np.array(players, np.int8)


@pytest.mark.parametrize("which", ["othello8", "connect4"])
def test_batched_path_on_stock_networks_matches_hip_net(which):
    from alphazero_amd.games.connect4 import Connect4Board
    torch.manual_seed(2)
    if which == "othello8":
        net, board, gid, H, W = OthelloNet(8, device="cuda"), OthelloBoard(n=8), 0, 8, 8
    else:
        net, board, gid, H, W = Connect4Net(7, 6, device="cuda"), Connect4Board(width=7, height=6), 1, 6, 7
    net.eval()
    grids, players = _random_positions(board, 64, np.random.default_rng(4))
    kw = dict(tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, dirichlet_alpha=None, dirichlet_epsilon=None, node_capacity=4096)
    hip = E.SelfPlayEngine(gid, H, W, n_slots=64, n_sim=1, net=net.to_hip(max_batch=64), **kw)
    ext = external(gid, H, W, 64, 1, TorchEvaluator(net), **kw)
    for eng in (hip, ext):
        eng.set_roots(grids, players)
        eng.search(2)  # two leaves evaluated and backed up per slot: Q checks the value frame
    for slot in range(64):
        a1, n1, q1, p1, r1 = hip.root_children(slot)
        a2, n2, q2, p2, r2 = ext.root_children(slot)
        assert np.array_equal(a1, a2) and len(a1) > 0
        assert np.array_equal(n1, n2) and r1 == r2 == 2, slot
        assert np.abs(p1 - p2).max() <= 1e-5, (slot, np.abs(p1 - p2).max())
        assert np.abs(q1 - q2).max() <= 1e-5, (slot, q1, q2)
        assert np.abs(q1).max() > 0, slot


# ------------------------------------------------------------------------------------------------------------------ 5
def test_errors_from_the_evaluator():
    gid, H, W, A = 0, 6, 6, 37
    grids = np.tile(OthelloBoard(n=6).grid.astype(np.int8)[None], (4, 1, 1))
    players = np.ones(4, np.int8)
    good = TorchEvaluator(ClosedFormNet(A))
    kw = dict(tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, dirichlet_alpha=None, dirichlet_epsilon=None)

    # the mode exists only on external engines, and needs an evaluator
    plain = E.SelfPlayEngine(gid, H, W, n_slots=4, n_sim=1, evaluator=E.EVAL_FAKE, **kw)
    with pytest.raises(ValueError):
        plain.set_evaluator(good)
    bare = E.SelfPlayEngine(gid, H, W, n_slots=4, n_sim=1, evaluator=E.EVAL_EXTERNAL, **kw)
    bare.set_roots(grids, players)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*evaluator"):
        bare.search(2)

    # an exception raised in the callback comes out of search() unchanged
    state = {"calls": 0, "fail": True}
    boom = KeyError("boom")

    def flaky(b):
        state["calls"] += 1
        if state["fail"] and state["calls"] == 3:
            raise boom
        good(b)
    eng = external(gid, H, W, 4, 1, flaky, **kw)
    eng.set_roots(grids, players)
    with pytest.raises(KeyError) as ei:
        eng.search(6)
    assert ei.value is boom and isinstance(ei.value.__cause__, _lib.EvalError)
    assert "lock-step 1" in str(ei.value.__cause__)
    with pytest.raises(_lib.AzError, match=r"\[-3\]"):
        eng.search(6)
    state["fail"] = False
    eng.set_roots(grids, players)
    eng.search(6)
    fresh = external(gid, H, W, 4, 1, good, **kw)
    fresh.set_roots(grids, players)
    fresh.search(6)
    for slot in range(4):
        for x, y in zip(eng.root_children(slot), fresh.root_children(slot)):
            assert np.array_equal(x, y)

    # NaN in one row: ValueError naming that slot
    def nan_slot2(b):
        good(b)
        b.probs[b.slots == 2] = float("nan")
    bad = external(gid, H, W, 4, 1, nan_slot2, **kw)
    bad.set_roots(grids, players)
    with pytest.raises(ValueError, match="slot 2"):
        bad.search(2)
    with pytest.raises(_lib.AzError, match=r"\[-3\]"):
        bad.root_children(0)

    # a call back into its own engine is refused
    seen = []

    def reenter(b):
        try:
            inner.stats()
        except _lib.AzError as err:
            seen.append(str(err))
        good(b)
    inner = external(gid, H, W, 4, 1, reenter, **kw)
    inner.set_roots(grids, players)
    inner.search(2)
    assert seen and all("[-3]" in s and "inside" in s for s in seen)
    for e in (plain, bare, eng, fresh, bad, inner):
        e.close()


def test_mct_and_trainer_recover_after_a_failed_evaluation(tmp_path):
    """a failed evaluation leaves the engine refusing all but set_roots / run: the MCT restarts its tree at the next search,
    the trainer builds a fresh engine for the next wave"""
    fail = {"on": True}

    class Flaky(ClosedFormTwin):
        def evaluate(self, board):
            if fail["on"]:
                raise RuntimeError("evaluate failed")
            return super().evaluate(board)
    board = OthelloBoard(n=6)
    mct = MCT(eval_method="neural", nn=Flaky(37))
    with pytest.raises(RuntimeError, match="evaluate failed"):
        mct.search(board, n_sim=4)
    fail["on"] = False
    mct.search(board, n_sim=4)
    ref = MCT(eval_method="neural", nn=Flaky(37))
    ref.search(board, n_sim=4)
    assert mct.get_prior_probs() == ref.get_prior_probs()
    assert sum(mct.get_action_probs(board, 0)[1].values()) == 4

    class FlakyTiny(TinyOthello):
        def predict(self, input):
            if fail["on"]:
                raise RuntimeError("predict failed")
            return super().predict(input)
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    tr = AlphaZeroTrainer(verbose=False, engine_slots=4, seed=3, materialize_memory=False)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=4, episodes=4, epochs=1, batch_size=16, iterations=1, do_eval=False,
                              device="cuda", save=False, save_checkpoints=False)
    tr.setup()
    tr.nn = FlakyTiny(6)
    fail["on"] = True
    with pytest.raises(RuntimeError, match="predict failed"):
        tr.self_play(0)
    assert tr._engine is None
    fail["on"] = False
    tr.self_play(0)
    assert tr.device_samples["z"].shape[0] > 0 and tr._engine.cfg.evaluator == E.EVAL_EXTERNAL


# ------------------------------------------------------------------------------------------------------------------ 6
class TinyOthello(PolicyValueNetwork):
    """a user-defined architecture: two convolutions and two linear heads on Othello n x n"""

    def __init__(self, n=6, device="cuda"):
        super().__init__()
        self.n, self.device, self.action_size = n, torch.device(device), n * n + 1
        self.conv1 = nn.Conv2d(1, 8, 3, padding=1, device=self.device)
        self.conv2 = nn.Conv2d(8, 8, 3, padding=1, device=self.device)
        self.fc_probs = nn.Linear(8 * n * n, n * n + 1, device=self.device)
        self.fc_value = nn.Linear(8 * n * n, 1, device=self.device)

    def forward(self, input):
        x = input.view(-1, 1, self.n, self.n)
        x = F.relu(self.conv2(F.relu(self.conv1(x)))).flatten(1)
        return F.log_softmax(self.fc_probs(x), dim=1), torch.tanh(self.fc_value(x))

    # the board hooks of the shipped Othello network
    _index = OthelloNet._index
    _board_part = OthelloNet._board_part
    get_normalized_probs = OthelloNet.get_normalized_probs
    to_neural_output = OthelloNet.to_neural_output
    reflect_neural_output = OthelloNet.reflect_neural_output
    rotate_neural_output = OthelloNet.rotate_neural_output


def test_user_architecture_plays_and_trains(tmp_path):
    torch.manual_seed(1)
    np.random.seed(1)
    custom = TinyOthello(6)
    res = Arena(AlphaZeroPlayer(n_sim=8, nn=custom), GreedyPlayer(), OthelloBoard(n=6)).play_game(return_results=True)
    assert res["winner"] in (0, 1, 2)  # every move went through Board.play_move, which refuses an illegal one

    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    tr = AlphaZeroTrainer(verbose=False, engine_slots=8, seed=3)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=6, episodes=8, epochs=1, batch_size=16, iterations=1, eval_opponent="previous",
                              eval_episodes=2, device="cuda", save=False, save_checkpoints=False)
    tr.setup()
    tr.nn = custom
    tr.az_player = AlphaZeroPlayer(n_sim=6, nn=custom, dirichlet_alpha=0.03, dirichlet_epsilon=0.25)
    tr.self_play(0)
    assert tr._engine.cfg.evaluator == E.EVAL_EXTERNAL
    with pytest.warns(RuntimeWarning, match="stock PyTorch step"):
        tr.optimize_network(0)
    assert tr.sgd_backend_used == "torch"
    losses = tr.loss_values[0][0]
    assert len(losses["pi"]) > 0 and np.isfinite(losses["pi"]).all() and np.isfinite(losses["v"]).all()
    tr.update_network(0)
    tr.evaluate(0)
    assert sum(tr.eval_results["results"][0]["player1_starts"].values()) + sum(tr.eval_results["results"][0]["player2_starts"].values()) == 2
    m = tr.device_memory
    pi = m["pi"]
    legal = E.legal_batch(0, 6, 6, m["state"].contiguous(), torch.ones(pi.shape[0], dtype=torch.int8, device="cuda")).bool()
    assert torch.allclose(pi.sum(1), torch.ones_like(pi[:, 0]), atol=1e-5)
    assert (pi[~legal] == 0).all()
