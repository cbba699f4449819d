"""Host model of the full Gumbel search (az_engine_set_gumbel_full): GumbelBatchModel in which every evaluated node
keeps its network value, v_mix is the paper's -- the node's own value mixed with its visited children -- at the root and below, and
the child below the root is gumbel.nonroot_choice's instead of PUCT's.  A plain restatement of the contract for tests.  Not a
conftest, not a test module.

For a node p with children b, float64, one operation at a time, sums in child-index order:
  vhat = the float32 value the network gave p, in the frame of the player to move at p
  sumN = sum N(b);  num, den = the sums over N(b) > 0 of P(b) Q(b) and of P(b)
  vmix(p) = vhat when sumN == 0 or not den > 0, else (vhat + sumN * (num / den)) / (1 + sumN)
  pi'(b)  = det_exp(x(b) - max x) / sum,  x(b) = det_log(P(b)) + ((c_visit + maxN) * c_scale) * (N(b) > 0 ? Q(b) : vmix(p))
Walker j at parent p (depth >= 1) takes nonroot_choice(pi', N, v) with v(b) = the earlier walkers of the lock-step whose recorded
path holds b.  full=False is GumbelBatchModel, statement for statement."""
from alphazero_amd import gumbel as G
from gumbel_batch_model import GumbelBatchModel


class GumbelFullModel(GumbelBatchModel):
    """one slot of an engine with az_engine_set_gumbel(...), az_engine_set_gumbel_batch(K) and az_engine_set_gumbel_full(full) in force"""

    def __init__(self, board, K=1, full=True, **kw):
        super().__init__(board, K=K, **kw)
        self.full = bool(full)
        self.nval = {}  # id(node) -> (node, vhat): the node is kept so that its id stays its own

    def _evaluate(self, node):
        out = super()._evaluate(node)  # player * v
        if self.full:
            self.nval[id(node)] = (node, float(self._board(node).player) * out)  # player is +-1: v again, exactly
        return out

    def value_of(self, node):
        """vhat of an evaluated node; a value that was never stored is never read"""
        kept, v = self.nval[id(node)]
        assert kept is node and node.evaluated
        return v

    def root_value(self):
        return self.value_of(self.root)

    def _vmix(self, node):
        ch = node.children
        num = den = 0.0
        for c in ch:
            if c.N > 0:
                num += c.P * c.Q
                den += c.P
        sumN = sum(c.N for c in ch)
        vhat = self.value_of(node)
        if sumN == 0 or not den > 0.0:
            return vhat
        wq = num / den
        return (vhat + float(sumN) * wq) / float(1 + sumN)

    def _terms(self, node):
        """logit and sigma of the node's children with the paper's vmix"""
        ch = node.children
        vmix = self._vmix(node)
        k = (self.cv + float(max(c.N for c in ch))) * self.cs
        return [G.det_log(c.P) for c in ch], [k * (c.Q if c.N > 0 else vmix) for c in ch]

    def _sigma_terms(self):
        return self._terms(self.root) if self.full else super()._sigma_terms()

    def improved_policy(self, node):
        """pi' over the node's children in float64 (the policy target's formula, before the float32 store)"""
        logit, sigma = self._terms(node)
        x = [li + si for li, si in zip(logit, sigma)]
        xmax = max(x)
        e = [G.det_exp(xi - xmax) for xi in x]
        s = 0.0
        for ei in e:
            s += ei
        return [ei / s for ei in e]

    def _pick(self, parent, earlier, sim, depth):
        if depth == 0 or not self.full:
            return super()._pick(parent, earlier, sim, depth)
        ch = parent.children
        virtual = [sum(1 for s in earlier if id(c) in s) for c in ch]
        return ch[G.nonroot_choice(self.improved_policy(parent), [c.N for c in ch], virtual)]
