"""Host model of proof backup (az_engine_set_proof_backup; include/az_amd.h): a plain restatement of the contract
on leaf_batch_model.Model at K = 1, with exact_endgame_model's solved leaf or without, for tests.  Not a conftest, not a test module.

Outcomes are absolute player ids; the mover at path position i is root_player * (-1)^i.
  proven      a node with N > 0 that is terminal (finished, or solved) has its winner; an expanded node of mover m is marked with
              outcome m when some child is proven with m, and when every child is proven with 0 if some child's outcome is 0, else -m
  propagation after the backup of a simulation whose leaf was terminal or proven: the rule from the leaf's parent upward, until the
              first node it does not prove
  walk        below the root a walk stops on a marked node: its outcome, no network row, no solve
  selection   a child proven as the parent's mover's loss is no candidate unless every child is one; at the root a child proven
              as the mover's win has the key +inf; the tie draw runs among the candidates
  policy      counts(): a proven win among the root's children keeps the wins' counts alone; else proven losses count 0 unless all
              children are losses, or no other child has been visited; then the usual temperature arithmetic, at 0 too
  counters    proven_nodes (marks, each once), proof_stops (walks ended on a marked node), pruned_plies (plies played whose counts
              the rule changed)
The marks are kept incrementally, as the engine keeps them; brute_marks() recomputes them from scratch for the host test."""
import numpy as np

import playout_cap_model as PC
from exact_endgame_model import ExactModel, UNSOLVED, empties, value
from leaf_batch_model import action_size, make_board
from tools import closed_form as cf


class ProofModel(ExactModel):
    def __init__(self, board, E=0, proof=True, **kw):
        super().__init__(board, E, **kw)
        self.proof = bool(proof)
        self.mark = {}  # id(node) -> outcome of the interior nodes marked proven
        self._pin = []  # the marked nodes themselves: a node the re-rooting drops must not hand its id to a later one
        self.proven_nodes = self.proof_stops = self.pruned_plies = 0

    def outcome(self, node):
        """the proven outcome of a node as its parent sees it, or None"""
        if node.N > 0:
            if node.terminal:
                return int(node.win)
            if id(node) in self.mark:
                return self.mark[id(node)]
        return None

    def root_proof(self):
        """az_engine_root_proofs for this slot"""
        r = self.root
        return int(r.win) if r.terminal else self.mark.get(id(r), UNSOLVED)

    def _mover(self, pos):
        p = int(self._board(self.root).player)
        return -p if pos & 1 else p

    def _pick(self, parent, earlier, sim, depth):
        if not self.proof:
            return super()._pick(parent, earlier, sim, depth)
        m, ch = self._mover(depth), parent.children
        sq = float(np.sqrt(np.float64(parent.N)))
        keys = [c.Q + (c.P * sq) / float(1 + c.N) for c in ch]
        outs = [self.outcome(c) for c in ch]
        loss = [o == -m for o in outs]
        if all(loss):
            loss = [False] * len(ch)
        if depth == 0:
            keys = [float("inf") if o == m else k for k, o in zip(keys, outs)]
        cand = [i for i in range(len(ch)) if not loss[i]]
        best = max(keys[i] for i in cand)
        ties = [i for i in cand if keys[i] == best]
        k = 0
        if self.tie == "random" and len(ties) > 1:
            r = cf.philox4x32(self.seed, self.gid, self.ply, (sim + self.sim_base) & 0xFFFFFFFF, cf.P_TIE_SELECT, depth)
            k = (r[0] * len(ties)) >> 32
        return ch[ties[k]]

    def rule(self, node, pos):
        """the outcome the rule gives an expanded node at path position pos, or None"""
        m = self._mover(pos)
        outs = [self.outcome(c) for c in node.children]
        if any(o == m for o in outs):
            return m
        if outs and all(o is not None for o in outs):
            return 0 if any(o == 0 for o in outs) else -m
        return None

    def _propagate(self, path):
        for pos in range(len(path) - 2, -1, -1):
            out = self.rule(path[pos], pos)
            if out is None:
                break
            if id(path[pos]) not in self.mark:
                self.mark[id(path[pos])] = out
                self._pin.append(path[pos])
                self.proven_nodes += 1

    def search(self, n_sim):
        root = self.root
        if not (root.evaluated or root.terminal):  # the root-prior pass: the value is discarded
            self._evaluate(root)
        for sim in range(n_sim):
            if self.noise is not None and root.expanded and not root.noised:
                self._apply_noise()
            node, path, depth = root, [root], 0
            while True:
                fresh = False
                if self.proof and node is not root and id(node) in self.mark:
                    break
                if not node.expanded:
                    if node.terminal:
                        break
                    assert node.evaluated
                    node.expanded = fresh = True
                node = self._pick(node, [], sim, depth)
                depth += 1
                path.append(node)
                if fresh or node.N == 0:
                    break
            self.max_path = max(self.max_path, len(path))
            b = self._board(node)
            term = True
            if node.terminal:
                out = float(node.win)
            elif self.proof and node is not root and id(node) in self.mark:
                out = float(self.mark[id(node)])
                self.proof_stops += 1
            elif b.is_game_over():
                node.terminal, node.win = True, int(b.get_winner())
                out = float(node.win)
            elif self.E > 0 and len(path) > 1 and empties(b) <= self.E:
                node.terminal, node.win = True, value(b, self.memo)
                self.solved_ids.add(id(node))
                self.solved += 1
                out = float(node.win)
            else:
                out, term = self._evaluate(node), False
            self._backup(path, b.player, out)
            if self.proof and term:
                self._propagate(path)
        self.sim_base += n_sim

    # ---- move and policy target
    def counts(self):
        """(the counts move and policy are made of, whether the rule changed one)"""
        ch = self.root.children
        raw = [c.N for c in ch]
        if not self.proof:
            return raw, False
        return prune_counts(raw, [self.outcome(c) for c in ch], self._mover(0))


def prune_counts(raw, outs, mover):
    """the pruning rule on a root's children: raw visit counts, proven outcomes (None: not proven) and the root's mover"""
    if any(o == mover for o in outs):
        new = [n if o == mover else 0 for n, o in zip(raw, outs)]
    else:
        loss = [o == -mover for o in outs]
        if all(loss) or not any(n > 0 and not lo for n, lo in zip(raw, loss)):
            new = list(raw)
        else:
            new = [0 if lo else n for n, lo in zip(raw, loss)]
    return new, new != list(raw)


def move_policy(m, temp):
    """PC.move_policy on the pruned counts: (index of the chosen child, pi float32 [A], whether the rule changed a count)"""
    ch = m.root.children
    N, changed = m.counts()
    pi = np.zeros(m.A, np.float32)
    if temp == 0.0:
        best = max(N)
        ties = [i for i, n in enumerate(N) if n == best]
        k = 0
        if m.tie == "random" and len(ties) > 1:
            k = (cf.philox4x32(m.seed, m.gid, m.ply, 0xFFFF, cf.P_TIE_MOVE, 0)[0] * len(ties)) >> 32
        pi[ch[ties[k]].act] = 1.0
        return ties[k], pi, changed
    inv = 1.0 / temp
    total = 0.0
    for n in N:
        total += PC._pow(n, temp, inv)
    u = cf.move_sample_u(m.seed, m.gid, m.ply) if len(ch) > 1 else 2.0
    cum, chosen, last, found = 0.0, 0, 0, False
    for i, c in enumerate(ch):
        p = PC._pow(N[i], temp, inv) / total
        pi[c.act] = np.float32(p)
        if p > 0.0:
            last = i
        cum += p
        if not found and u < cum:
            chosen, found = i, True
    if not found:
        chosen = 0 if len(ch) == 1 else last
    return chosen, pi, changed


def advance(m, tmax, tmin, temp=None):
    """k_move on the model: the sample (raw visits, pruned pi), the move, the re-rooting"""
    b = m._board(m.root)
    idx, pi, changed = move_policy(m, PC.linear_temp(m.ply, tmax, tmin) if temp is None else temp)
    m.pruned_plies += 1 if changed else 0
    vis = np.zeros(m.A, np.int32)
    for c in m.root.children:
        vis[c.act] = c.N
    smp = {"state": (b.player * b.grid).astype(np.int8), "pi": pi, "visits": vis,
           "meta": np.array([m.gid, m.ply, b.player, m.root.children[idx].act], np.int64).astype(np.uint32).view(np.int32)}
    PC.reroot(m, idx)
    m.became_root()
    return smp


CTRS = ("plies", "rows", "solved", "proven_nodes", "proof_stops", "pruned_plies", "proven_roots")


def play_game(game, H, W, seed, game_id, n_sim, E, proof, noise, tie, tmax, tmin, net=None):
    m = ProofModel(make_board(game, H, W), E, proof, noise=None, tie=tie, seed=seed, game_id=game_id, net=net)
    samples, roots = [], 0
    while True:
        PC.search_call(m, n_sim, None, noise)
        roots += 1 if m.root_proof() != UNSOLVED else 0
        samples.append(advance(m, tmax, tmin))
        b = m.root.board
        if b.is_game_over():
            w = int(b.get_winner())
            for s in samples:
                s["z"] = np.int8(w * int(s["meta"][2]))
            break
    return samples, {"plies": len(samples), "rows": m.rows, "solved": m.solved, "proven_nodes": m.proven_nodes,
                     "proof_stops": m.proof_stops, "pruned_plies": m.pruned_plies, "proven_roots": roots}


def play_wave(game, H, W, seed, first_game_id, n_games, n_sim, E, proof, noise, tie, tmax, tmin, net=None):
    """az_engine_run on the model: the samples as arrays sorted by (game id, move idx), and the counters (rows = net_evals;
    proven_roots = the plies whose root was proven when its move was played)"""
    A = action_size(make_board(game, H, W))
    out = {"state": [], "pi": [], "visits": [], "meta": [], "z": []}
    ctr = dict.fromkeys(CTRS, 0)
    for g in range(first_game_id, first_game_id + n_games):
        smp, c = play_game(game, H, W, seed, g, n_sim, E, proof, noise, tie, tmax, tmin, net)
        for k in ctr:
            ctr[k] += c[k]
        for s in smp:
            for k in out:
                out[k].append(s[k])
    S = len(out["z"])
    arr = {"state": np.array(out["state"], np.int8).reshape(S, H, W), "pi": np.array(out["pi"], np.float32).reshape(S, A),
           "visits": np.array(out["visits"], np.int32).reshape(S, A), "meta": np.array(out["meta"], np.int32).reshape(S, 4),
           "z": np.array(out["z"], np.int8).reshape(S)}
    ctr["samples"] = S
    return arr, ctr


NOISE, TMAX, TMIN = (0.5, 0.25), 2, 7
_WAVES = {}


def wave(game, H, W, seed, first, n_games, n_sim, E, tie, proof=True, noise=NOISE):
    """the model's wave with the fake network, computed once per process"""
    key = (game, H, W, seed, first, n_games, n_sim, E, tie, proof, noise)
    if key not in _WAVES:
        _WAVES[key] = play_wave(game, H, W, seed, first, n_games, n_sim, E, proof, noise, tie, TMAX, TMIN)
    return _WAVES[key]


# ---- the brute-force restatement: every node's status from scratch, bottom up, knowing nothing of the marks ------------------------
def brute_marks(m):
    """{id(node): outcome} of every expanded node the rule proves, recomputed over the whole tree"""
    out = {}

    def status(node, pos):  # the node's proven outcome as its parent sees it, or None
        kids = [status(c, pos + 1) for c in node.children] if node.expanded else []
        if node.N == 0:
            return None
        if node.terminal:
            return int(node.win)
        if not node.expanded:
            return None
        mover = m._mover(pos)
        res = None
        if any(o == mover for o in kids):
            res = mover
        elif kids and all(o is not None for o in kids):
            res = 0 if any(o == 0 for o in kids) else -mover
        if res is not None:
            out[id(node)] = res
        return res

    status(m.root, 0)
    return out
