"""Host model of the Gumbel root search with gumbel_batch = K walkers per lock-step (az_engine_set_gumbel_batch):
GumbelModel with the lock-steps cut by the slot's own cursor instead of at multiples of K.  A plain restatement of the contract for
tests.  Not a conftest, not a test module.

A search call of n simulations keeps a cursor s (0 at its start).  A lock-step runs kt = min(K, end of the current phase - s, n - s)
walkers j = 0 .. kt - 1, walker j being simulation s + j, then s += kt: no lock-step crosses a phase boundary of
gumbel.schedule(n, m0), m0 = min(m, nch) (1 for a root that has no children to walk to).  The walkers run one after the other: the
root step is GumbelModel._pick's (forced by the schedule, no virtual count; a re-ranking can only fall on walker 0), below the root
Model._pick scores with the virtual counts of the earlier walkers' recorded paths; leaf status, duplicates and the backup in
ascending j are leaf_batch_model.Model's."""
import numpy as np

from alphazero_amd import gumbel as G
from gumbel_model import GumbelModel, playout
from leaf_batch_model import LPG


def wide_root(least=16, most=64, seed=17):
    """an Othello 8x8 midgame position with `least` .. `most` legal moves, found by seeded random playouts: with 16 or more, m = 16
    and K = 16 a search of 16 is one lock-step there"""
    rng = np.random.default_rng(seed)
    while True:
        b = playout("othello", 8, 8, rng, int(rng.integers(10, 30)))
        if b is not None and least <= len(b.get_moves()) <= most:
            return b


class GumbelBatchModel(GumbelModel):
    """one slot of an engine with az_engine_set_gumbel(...) and az_engine_set_gumbel_batch(K) in force"""

    def __init__(self, board, K=1, **kw):
        super().__init__(board, **kw)
        self.K = int(K)
        self.plan = []      # [(s, kt)] of the last search call
        self.leaves = []    # per lock-step of the last search call: [(status, id of the leaf node)]

    def search(self, n_sim):
        n = self._n = int(n_sim)
        root = self.root
        if not (root.evaluated or root.terminal):  # the root-prior pass: the value is discarded
            self._evaluate(root)
        walks = (root.expanded or (root.evaluated and not root.terminal)) and len(root.children) > 0
        m0 = min(self.m, len(root.children)) if walks else 1
        ends, e = [], 0
        for mp, v in G.schedule(n, m0):
            e = min(n, e + mp * v)
            ends.append(e)
        self.plan, self.leaves = [], []
        s = 0
        while s < n:
            end = next(x for x in ends if x > s)
            kt = min(self.K, end - s, n - s)
            self.plan.append((s, kt))
            earlier, pend = [], []
            for j in range(kt):
                sim = s + j
                node, path, depth = root, [root], 0
                while True:
                    fresh = False
                    if not node.expanded:
                        if node.terminal:
                            break
                        assert node.evaluated
                        node.expanded = fresh = True
                    node = self._pick(node, earlier, sim, depth)  # depth 0: the scheduled child, whatever `earlier` holds
                    depth += 1
                    path.append(node)
                    if fresh or node.N == 0:
                        break
                self.max_path = max(self.max_path, len(path))
                earlier.append({id(x) for x in path[:LPG]})
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
            self.leaves.append([(p[0], id(p[1][-1])) for p in pend])
            out = [None] * kt
            for j, (st, path, player, x) in enumerate(pend):
                if st == "eval":
                    out[j] = self._evaluate(path[-1])
                elif st == "dup":
                    out[j] = out[x]
                else:
                    out[j] = x
                self._backup(path, player, out[j])
            s += kt
        self.sim_base += n
