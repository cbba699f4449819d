"""Host model of the Gumbel root search (az_engine_set_gumbel): the sequential search of leaf_batch_model.Model at
K = 1 with the root's child taken from the Sequential Halving schedule, plus the move and the policy target of the completed
Q-values.  A plain restatement of the contract for tests.  Not a conftest, not a test module."""
import numpy as np

from alphazero_amd import gumbel as G
from leaf_batch_model import Model, make_board
from tools import closed_form as cf


def playout(game, H, W, rng, plies):
    """the position after `plies` seeded random legal moves from the start (None when the game ended before)"""
    b = make_board(game, H, W)
    for _ in range(plies):
        if b.is_game_over():
            return None
        moves = sorted(b.get_moves(), key=lambda m: cf.move_to_action(game, m, H))
        b.play_move(moves[int(rng.integers(len(moves)))])
    return None if b.is_game_over() else b


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


class GumbelModel(Model):
    """one slot of an engine with az_engine_set_gumbel(m, c_visit, c_scale, gumbel_scale) in force"""

    def __init__(self, board, m=16, c_visit=50.0, c_scale=0.5, gumbel_scale=1.0, tie="lowest", seed=0, game_id=0, ply=0, net=None):
        super().__init__(board, K=1, noise=None, tie=tie, seed=seed, game_id=game_id, ply=ply, net=net)
        self.m, self.cv, self.cs, self.gs = int(m), float(c_visit), float(c_scale), float(gumbel_scale)
        self.mask = []  # considered children, ascending child indices ([]: all)
        self._n = 0

    # ---- the quantities of the root
    def _sigma_terms(self):
        ch = self.root.children
        num = den = 0.0
        for c in ch:
            if c.N > 0:
                num += c.P * c.Q
                den += c.P
        vmix = num / den if den > 0.0 else 0.0
        k = (self.cv + float(max(c.N for c in ch))) * self.cs
        return [G.det_log(c.P) for c in ch], [k * (c.Q if c.N > 0 else vmix) for c in ch]

    def scores(self):
        logit, sigma = self._sigma_terms()
        g = [G.gumbel_g(self.seed, self.gid, self.ply, c.act, self.gs) for c in self.root.children]
        return [(gi + li) + si for gi, li, si in zip(g, logit, sigma)]

    # ---- the walk
    def _pick(self, parent, earlier, sim, depth):
        if depth != 0:
            return super()._pick(parent, earlier, sim, depth)
        nch = len(parent.children)
        m0 = min(self.m, nch)
        p, mp, i = G.locate(sim, self._n, m0)
        if i == 0:
            if m0 == 1:
                self.mask = [0]
            else:
                sc = self.scores()
                assert not any(s != s for s in sc)
                prev = range(nch) if p == 0 else self.mask
                self.mask = sorted(sorted(prev, key=lambda a: (-sc[a], a))[:mp])
        return parent.children[self.mask[i % mp]]

    def search(self, n_sim):
        self._n = int(n_sim)
        super().search(n_sim)

    # ---- move and policy target
    def considered(self):
        return list(self.mask)

    def move_index(self):
        sc = self.scores()
        cand = self.mask or range(len(sc))
        return min(cand, key=lambda a: (-sc[a], a))

    def move(self):
        return self.root.children[self.move_index()].act

    def policy(self):
        """pi' as float32 [A]"""
        logit, sigma = self._sigma_terms()
        x = [li + si for li, si in zip(logit, sigma)]
        xmax = max(x)
        e = [G.det_exp(xi - xmax) for xi in x]
        s = 0.0
        for ei in e:
            s += ei
        out = np.zeros(self.A, np.float32)
        for c, ei in zip(self.root.children, e):
            out[c.act] = np.float32(ei / s)
        return out

    def visits(self):
        out = np.zeros(self.A, np.int32)
        for c in self.root.children:
            out[c.act] = c.N
        return out

    def advance(self):
        new = self.root.children[self.move_index()]
        self._board(new)
        new.parent = None
        self.root, self.ply, self.sim_base, self.mask = new, self.ply + 1, 0, []
        return new.act

    def play_game(self, n_sim, max_plies=200):
        """a whole self-play game as az_engine_run plays it: [(canonical state, pi' float32, visits, action, player)], winner"""
        rec = []
        while not self.root.board.is_game_over():
            assert len(rec) < max_plies
            self.search(n_sim)
            b = self.root.board
            state = (b.player * b.grid).astype(np.int8)
            pi, vis, player = self.policy(), self.visits(), int(b.player)
            rec.append((state, pi, vis, self.advance(), player))
        return rec, int(self.root.board.get_winner())
