"""Host model of the search with one board symmetry drawn per evaluation, on top of the leaf_batch model
(tests/leaf_batch_model.py).  Not a conftest, not a test module.

Every network row is evaluated in the member  random_code(seed, game id, root ply, s, members)  of the candidate codes: s is
ROOT_PASS for the root-prior pass and `sim + sim_base` for the leaf of simulation sim (walker j of lock-step t: sim = t K + j).  The
model's net is called as net(grid, player, A) like the base model's; the subclass publishes the `s` of the row being evaluated in
`self.s` just before."""
from alphazero_amd.symmetry import ROOT_PASS

from leaf_batch_model import Model


class RandomSymmetryModel(Model):
    """a leaf is evaluated by the first walker that ever picks it (a node is picked for the first time with N == 0, which ends the
    walk; later walkers of the same lock-step that land on it are duplicates and bring no row): _pick records that walker's
    simulation index, _evaluate hands it to the net as self.s"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.s = None
        self._first = {}  # id(node) -> (node, s); the node is kept so that its id is not reused

    def _pick(self, parent, earlier, sim, depth):
        child = super()._pick(parent, earlier, sim, depth)
        self._first.setdefault(id(child), (child, (sim + self.sim_base) & 0xFFFFFFFF))
        return child

    def _evaluate(self, node):
        # the root is only ever evaluated by the root-prior pass: every walk from an evaluated root picks at least one child
        self.s = ROOT_PASS if node is self.root else self._first[id(node)][1]
        return super()._evaluate(node)
