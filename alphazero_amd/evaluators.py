"""What evaluates the leaves of a search, and what trains a module: one decision, made here.

The reference's MCT is duck-typed (mcts.py:158, 189, 232): it calls nn.evaluate(board) for every non-terminal leaf and for a
fresh root, so any PolicyValueNetwork -- or any object with evaluate() -- can search.  The device tree stays on the GPU in
every case; what changes is who fills the engine's probs / value rows:

  "hip"    the HIP network (az_net) and the HIP training step: the module IS a shipped architecture -- a shipped forward(),
           the stock net's state-dict keys and shapes for that board, and a plane az_net_create accepts (conv planes 5..8 on
           each side, TicTacToe 3x3).  For a search, evaluate() and predict() must not be overridden either.
  "torch"  TorchEvaluator: the module's own predict() on the engine's batch of rows (evaluate() is the base one).
  "board"  BoardEvaluator: the reference's semantics, one Board and one evaluate() call per row (evaluate() was customised,
           or the object is not a torch module).

Two things have no device counterpart and are refused: rules for a game other than the three compiled ones, and a
get_normalized_probs other than the shipped one (the device tree applies that rule, az_engine.hip create_children_grp).
"""
import functools
import warnings

import numpy as np
import torch

from .base import PolicyValueNetwork

GAMES = ("othello", "connect4", "tictactoe")


def check_game(board):
    """NotImplementedError for a board the device has no rules for (before any device work)"""
    game = getattr(board, "game", None)
    if game not in GAMES:
        raise NotImplementedError(f"no device rules for game {game!r}: the engine has compiled rule sets for {', '.join(GAMES)} only")


def _shipped():
    from .games._convnet import ConvPolicyValueNet
    from .games.connect4 import Connect4Net
    from .games.othello import OthelloNet
    from .games.tictactoe import TicTacToeNet
    return ConvPolicyValueNet, OthelloNet, Connect4Net, TicTacToeNet


def check_normalizer(nn):
    """NotImplementedError for an nn whose class brings its own get_normalized_probs: the device tree applies the shipped rule
    (legal gather, float32 sum in ascending action order, uniform below 1e-6) whatever the network"""
    fn = getattr(type(nn), "get_normalized_probs", None)
    if fn is None:
        return
    _, OthelloNet, Connect4Net, TicTacToeNet = _shipped()
    shipped = (PolicyValueNetwork.get_normalized_probs, OthelloNet.get_normalized_probs, Connect4Net.get_normalized_probs,
               TicTacToeNet.get_normalized_probs)
    if fn not in shipped:
        raise NotImplementedError(f"{type(nn).__name__} defines its own get_normalized_probs: the device tree applies the shipped "
                                  f"rule (renormalise over the legal moves, uniform below 1e-6) and cannot call it")


def _plane_accepted(gid, H, W):
    """(c): a shape az_net_create builds -- the game's board rules (az_make_game_desc) and a conv plane of 5..8 on each side
    (Connect4Net reads the H x W grid as a W x H plane, connect4.py:399), or TicTacToe 3x3"""
    if gid == 0:
        return H == W and H % 2 == 0 and 5 <= H <= 8
    if gid == 1:
        return 5 <= H <= 8 and 5 <= W <= 8
    return gid == 2 and (H, W) == (3, 3)


@functools.lru_cache(maxsize=None)
def _stock_shapes(gid, H, W):
    _, OthelloNet, Connect4Net, TicTacToeNet = _shipped()
    # shapes only: no storage, and the caller's torch generator state is left as it was (layer initialisation draws from it)
    with torch.random.fork_rng(devices=[]):
        dev = "meta"
        net = (OthelloNet(n=H, device=dev) if gid == 0 else
               (Connect4Net(board_width=W, board_height=H, device=dev) if gid == 1 else TicTacToeNet(device=dev)))
    return {k: tuple(v.shape) for k, v in net.state_dict().items()}


def hip_serves(module, search=True):
    """True when the HIP network (search) / the HIP training step (search=False) computes exactly this module's function:
    (a) a shipped forward, (b) the stock net's state-dict keys and shapes, (c) a plane az_net_create accepts; a search also
    needs evaluate() and predict() to be the base ones"""
    if not isinstance(module, PolicyValueNetwork) or not hasattr(module, "hip_shape"):
        return False
    ConvPolicyValueNet, _, _, TicTacToeNet = _shipped()
    try:
        gid, H, W = module.hip_shape()
    except NotImplementedError:
        return False
    cls = type(module)
    if cls.forward is not (TicTacToeNet.forward if gid == 2 else ConvPolicyValueNet.forward):  # (a)
        return False
    if search and not _plane_accepted(gid, H, W):  # (c)
        return False
    if {k: tuple(v.shape) for k, v in module.state_dict().items()} != _stock_shapes(gid, H, W):  # (b)
        return False
    if search and (cls.evaluate is not PolicyValueNetwork.evaluate or cls.predict is not PolicyValueNetwork.predict):
        return False
    return True


def route(nn):
    """"hip", "torch" or "board": what evaluates the leaves when `nn` searches (module docstring)"""
    if hip_serves(nn, search=True):
        return "hip"
    if isinstance(nn, PolicyValueNetwork) and type(nn).evaluate is PolicyValueNetwork.evaluate:
        return "torch"
    if callable(getattr(nn, "evaluate", None)):
        return "board"
    raise TypeError(f"{type(nn).__name__} has no evaluate(board): it cannot evaluate the positions of a search")


def make_evaluator(nn, game, H, W):
    """the external evaluator of an EVAL_EXTERNAL engine for nn (route "torch" or "board")"""
    check_normalizer(nn)
    r = route(nn)
    if r == "torch":
        return TorchEvaluator(nn)
    if r == "board":
        return BoardEvaluator(nn, game, H, W)
    raise ValueError(f"{type(nn).__name__} runs on the HIP network (route 'hip'), not through an external evaluator")


def _module_device(module):
    for p in module.parameters():
        return p.device
    for b in module.buffers():
        return b.device
    return torch.device(getattr(module, "device", "cpu"))


class TorchEvaluator:
    """the batched path: module.predict(x) on the engine's rows, as PolicyValueNetwork.evaluate (base.py:357-367) runs it on one
    board -- the input is player * grid, the value stays in the side-to-move frame.  On the GPU nothing is read back to the host,
    so the lock-step loop gains no host synchronisation; a module on the CPU is evaluated there (the batch goes through host
    memory, with one warning)."""

    def __init__(self, module):
        self.module = module
        self._warned = False

    def __call__(self, b):
        dev = _module_device(self.module)
        x = b.x
        if dev.type != x.device.type:
            if not self._warned:
                self._warned = True
                warnings.warn(f"{type(self.module).__name__} lives on {dev}: every batch of leaves goes through host memory",
                              RuntimeWarning, stacklevel=2)
            x = x.to(dev)
        p, v = self.module.predict(x)
        cap, A = b.cap, b.A
        if p.numel() != cap * A or v.numel() != cap:
            raise ValueError(f"{type(self.module).__name__}.predict on {cap} boards returned probabilities of shape {tuple(p.shape)} "
                             f"and values of shape {tuple(v.shape)}; expected ({cap}, {A}) and ({cap}, 1)")
        b.probs.copy_(p.reshape(cap, A))
        b.value.copy_(v.reshape(cap))


class BoardEvaluator:
    """the reference's semantics: per pending row a full Board (OthelloBoard(n, grid, player), Connect4Board(width, height, grid,
    player), TicTacToeBoard(grid, player)) and one nn.evaluate(board) call.  Synchronises the engine's stream per batch.
    probs are stored as float32 (float64 probabilities that float32 cannot represent are rounded); value = v * player is exact,
    so the engine's player * value gives back evaluate()'s v bit for bit when v is a float32 number."""

    def __init__(self, nn, game, H, W):
        self.nn, self.game, self.H, self.W = nn, game, H, W
        self.calls = 0  # evaluate() calls made
        if game == "othello":
            from .games.othello import OthelloBoard
            self._board = lambda g, p: OthelloBoard(n=H, grid=g, player=p)
        elif game == "connect4":
            from .games.connect4 import Connect4Board
            self._board = lambda g, p: Connect4Board(width=W, height=H, grid=g, player=p)
        elif game == "tictactoe":
            from .games.tictactoe import TicTacToeBoard
            self._board = lambda g, p: TicTacToeBoard(grid=g, player=p)
        else:
            raise NotImplementedError(f"no device rules for game {game!r}: the engine has compiled rule sets for {', '.join(GAMES)} only")

    def __call__(self, b):
        torch.cuda.current_stream().synchronize()
        n = int(b.count[0].item())
        if n == 0:
            return
        grids = b.grids[:n].cpu().numpy().astype(np.float64)
        players = b.players[:n].cpu().numpy()
        probs = np.empty((n, b.A), np.float32)
        value = np.empty(n, np.float32)
        for i in range(n):
            player = int(players[i])
            p, v = self.nn.evaluate(self._board(grids[i].copy(), player))
            p = np.asarray(p).reshape(-1)
            if p.size != b.A:
                raise ValueError(f"{type(self.nn).__name__}.evaluate returned {p.size} probabilities, the game has {b.A} actions")
            probs[i] = p
            value[i] = np.float32(v) * np.float32(player)
        self.calls += n
        b.probs[:n].copy_(torch.from_numpy(probs))
        b.value[:n].copy_(torch.from_numpy(value))
