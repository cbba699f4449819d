"""Host model of the search with leaf_batch = K walkers per lock-step: a plain restatement of the contract on the
mirror Board classes, for tests.  Not a conftest, not a test module.

A search of n_sim simulations is ceil(n_sim / K) lock-steps.  In lock-step t the walkers j = 0 .. k_t - 1 (simulation t K + j) run
one after the other: SELECT with the virtual counts of the earlier walkers' recorded paths (first 16 nodes), leaf status (terminal /
duplicate of an earlier pending leaf / one network row), then, once every walker has selected, BACKUP in ascending j.  K = 1 is
the sequential search of the reference (mcts.py:127-171, 197-223, 226-269) as the engine restates it: float32 ascending prior
renormalisation with the < 1e-6 uniform rule, children in ascending action order, outcome = player * v."""
import math

import numpy as np

from tools import closed_form as cf

LPG = 16  # recorded path positions


def make_board(game, H, W, grid=None, player=1):
    from alphazero_amd.games.connect4 import Connect4Board
    from alphazero_amd.games.othello import OthelloBoard
    from alphazero_amd.games.tictactoe import TicTacToeBoard
    g = None if grid is None else np.array(grid, dtype=np.float64)
    if game == "othello":
        return OthelloBoard(n=H, grid=g, player=int(player)) if g is not None else OthelloBoard(n=H)
    if game == "connect4":
        return Connect4Board(width=W, height=H, grid=g, player=int(player))
    return TicTacToeBoard(grid=g, player=int(player)) if g is not None else TicTacToeBoard()


def action_size(board):
    H, W = board.grid.shape
    return H * W + 1 if board.game == "othello" else (W if board.game == "connect4" else 9)


def _act(board, move):
    return cf.move_to_action(board.game, move, board.grid.shape[0])


def _move(board, action):
    return cf.action_to_move(board.game, action, board.grid.shape[0])


class Node:
    __slots__ = ("N", "Q", "P", "parent", "children", "act", "evaluated", "expanded", "terminal", "noised", "pf32", "win", "board")

    def __init__(self, act, parent, P, pf32):
        self.N, self.Q, self.P, self.parent, self.act = 0, 0.0, P, parent, act
        self.children, self.board, self.win = [], None, 0
        self.evaluated = self.expanded = self.terminal = self.noised = False
        self.pf32 = pf32


def _fakenet(grid, player, A):
    return cf.fakenet(grid, player, A)


class Model:
    """one slot of the engine.  net(grid, player, A) -> (probs float32 [A], v in the side-to-move frame); default: the closed-form
    fake network.  tie "lowest" / "random" (Philox, the kernel's counters); noise: None or (alpha, eps) with the hash noise."""

    def __init__(self, board, K=1, noise=None, tie="lowest", seed=0, game_id=0, ply=0, net=None):
        self.K, self.noise, self.tie, self.seed, self.gid, self.ply = int(K), noise, tie, int(seed), int(game_id), int(ply)
        self.net = net or _fakenet
        self.A = action_size(board)
        self.root = Node(0, None, 0.0, False)
        self.root.board = board.clone()
        self.sim_base = 0
        self.rows = 0        # network rows, the root-prior pass included
        self.dups = 0        # duplicates (collisions)
        self.max_path = 0

    # ---- tree
    def _board(self, node):
        if node.board is None:
            b = self._board(node.parent).clone()
            b.play_move(_move(b, node.act))
            node.board = b
        return node.board

    def _evaluate(self, node):
        """the network on the node's board + create_children (get_normalized_probs in float32, ascending action order)"""
        b = self._board(node)
        probs, v = self.net(b.grid, b.player, self.A)
        self.rows += 1
        acts = sorted(_act(b, m) for m in b.get_moves())
        s = np.float32(0.0)
        for a in acts:
            s = np.float32(s + np.float32(probs[a]))
        uniform = bool(s < np.float32(1e-6))
        for a in acts:
            P = 1.0 / float(len(acts)) if uniform else float(np.float32(np.float32(probs[a]) / s))
            node.children.append(Node(a, node, P, not uniform))
        node.evaluated = True
        return float(b.player) * float(np.float32(v))

    def _apply_noise(self):
        alpha, eps = self.noise
        r, b = self.root, self._board(self.root)
        eta = cf.hash_noise(b.grid, b.player, [c.act for c in r.children])
        for c in r.children:
            keep = float(np.float32(np.float32(1.0 - eps) * np.float32(c.P))) if c.pf32 else (1.0 - eps) * c.P
            c.P = keep + eps * eta[c.act]
            c.pf32 = False
        r.noised = True

    def _pick(self, parent, earlier, sim, depth):
        vp = sum(1 for s in earlier if id(parent) in s)
        sq = math.sqrt(float(parent.N + vp))
        keys = []
        for c in parent.children:
            vc = sum(1 for s in earlier if id(c) in s)
            q = c.Q if vc == 0 else (float(c.N) * c.Q - float(vc)) / float(c.N + vc)
            keys.append(q + (c.P * sq) / float(1 + c.N + vc))
        best = max(keys)
        ties = [i for i, k in enumerate(keys) if k == best]
        k = 0
        if self.tie == "random" and len(ties) > 1:
            r = cf.philox4x32(self.seed, self.gid, self.ply, (sim + self.sim_base) & 0xFFFFFFFF, cf.P_TIE_SELECT, depth)
            k = (r[0] * len(ties)) >> 32
        return parent.children[ties[k]]

    @staticmethod
    def _backup(path, player_to_play, outcome):
        if abs(outcome) < 1e-4:
            reward = 0.0
        else:
            reward = -abs(outcome) if float(player_to_play) * outcome > 0.0 else abs(outcome)
        for up, n in enumerate(reversed(path)):
            r = 0.0 if reward == 0.0 else (-reward if up & 1 else reward)
            n.Q = (float(n.N) * n.Q + r) / float(n.N + 1)
            n.N += 1

    # ---- search
    def search(self, n_sim):
        root = self.root
        if not (root.evaluated or root.terminal):  # mcts.py:231-233 : the value is discarded
            self._evaluate(root)
        K = self.K
        for t in range((n_sim + K - 1) // K):
            kt = min(K, n_sim - t * K)
            earlier, pend = [], []  # recorded paths (sets of node ids) / (status, path, player, outcome or index)
            for j in range(kt):
                sim = t * K + j
                if self.noise is not None and root.expanded and not root.noised:
                    self._apply_noise()
                node, path, depth = root, [root], 0
                while True:
                    fresh = False
                    if not node.expanded:
                        if node.terminal:
                            break
                        assert node.evaluated
                        node.expanded = fresh = True
                    node = self._pick(node, earlier, sim, depth)
                    depth += 1
                    path.append(node)
                    if fresh or node.N == 0:
                        break
                self.max_path = max(self.max_path, len(path))
                earlier.append({id(n) for n in path[:LPG]})
                b = self._board(node)
                if node.terminal:
                    pend.append(("term", path, b.player, float(node.win)))
                elif b.is_game_over():
                    node.terminal, node.win = True, int(b.get_winner())
                    pend.append(("term", path, b.player, float(node.win)))
                else:
                    dup = [i for i, p in enumerate(pend) if p[0] == "eval" and p[1][-1] is node]
                    if dup:
                        self.dups += 1
                        pend.append(("dup", path, b.player, dup[0]))
                    else:
                        pend.append(("eval", path, b.player, None))
            out = [None] * kt
            for j, (st, path, player, x) in enumerate(pend):
                if st == "eval":
                    out[j] = self._evaluate(path[-1])
                elif st == "dup":
                    out[j] = out[x]
                else:
                    out[j] = x
                self._backup(path, player, out[j])
        self.sim_base += n_sim

    def advance(self):
        """the temperature-0 move of k_move (most visited child, ties by tie mode) + change_root; returns the action"""
        ch = self.root.children
        best = max(c.N for c in ch)
        ties = [c for c in ch if c.N == best]
        k = 0
        if self.tie == "random" and len(ties) > 1:
            k = (cf.philox4x32(self.seed, self.gid, self.ply, 0xFFFF, cf.P_TIE_MOVE, 0)[0] * len(ties)) >> 32
        new = ties[k]
        self._board(new)
        new.parent = None
        self.root, self.ply, self.sim_base = new, self.ply + 1, 0
        return new.act

    # ---- what the tests compare
    def root_children(self):
        """[(action, N, Q, P)] of the root's children, [] while they are not materialised (root not expanded)"""
        r = self.root
        return [(c.act, c.N, c.Q, c.P) for c in r.children] if r.expanded else []

    def node_count(self):
        n, stack = 0, [self.root]
        while stack:
            x = stack.pop()
            n += 1
            stack.extend(x.children)
        return n
