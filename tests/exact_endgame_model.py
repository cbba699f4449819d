"""Host model of exact endgames (az_solve_batch; include/az_amd.h): a plain restatement of the contract on the mirror Board classes,
for tests.  Not a conftest, not a test module.

solve(board) is a negamax over the mirror's Board objects, memoised by position: the outcome under optimal play by both sides as an
absolute player id, and the LOWEST action index whose successor has that outcome.  Every root move is searched for its exact value,
so no cut-off decides the action; below the root a node stops at its mover's first win, which cannot change a value in {-1, 0, +1}.
An Othello pass is the one legal action of its position (action n * n), as the rules have it.

positions(...) draws the seeded random playouts the GPU test and its fixture (tests/golden/exact_endgame.npz, written by
tools/gen_exact_endgame_golden.py) share."""
import numpy as np

from leaf_batch_model import _act, _move, make_board

UNSOLVED = 2  # AZ_UNSOLVED


def empties(board):
    return int(np.sum(board.grid == 0))


def _key(board):
    return (board.grid.astype(np.int8).tobytes(), int(board.player))


def value(board, memo=None, prune=True):
    """the winner under optimal play (absolute player id).  prune=False: every move of every node is searched (plain minimax)"""
    memo = {} if memo is None else memo
    if board.is_game_over():
        return int(board.get_winner())
    k = _key(board)
    if k in memo:
        return memo[k]
    p, best = int(board.player), -2
    for a in sorted(_act(board, m) for m in board.get_moves()):
        c = board.clone()
        c.play_move(_move(c, a))
        best = max(best, p * value(c, memo, prune))
        if prune and best == 1:
            break
    memo[k] = p * best
    return memo[k]


def solve(board, memo=None, prune=True):
    """(winner, action) of a position whose game is not over; a finished game: (its winner, -1)"""
    memo = {} if memo is None else memo
    if board.is_game_over():
        return int(board.get_winner()), -1
    p, vals = int(board.player), []
    for a in sorted(_act(board, m) for m in board.get_moves()):
        c = board.clone()
        c.play_move(_move(c, a))
        vals.append((a, p * value(c, memo, prune)))
    best = max(v for _, v in vals)
    return p * best, min(a for a, v in vals if v == best)


def solve_contract(board, max_empties, memo=None):
    """az_solve_batch's answer: finished games and candidates are solved, anything else is (AZ_UNSOLVED, -1)"""
    if board.is_game_over() or empties(board) <= max_empties:
        return solve(board, memo)
    return UNSOLVED, -1


def must_pass(board):
    return board.game == "othello" and not board.is_game_over() and _act(board, board.get_moves()[0]) == board.grid.size


def playout(game, H, W, rng, stop_empties=None):
    """a uniformly random playout from the start (lowest-index draw over the sorted actions, so it depends on rng alone); stops at
    the first position with at most stop_empties empty cells, or at the end of the game"""
    b = make_board(game, H, W)
    while not b.is_game_over():
        if stop_empties is not None and empties(b) <= stop_empties:
            break
        acts = sorted(_act(b, m) for m in b.get_moves())
        b.play_move(_move(b, acts[int(rng.integers(len(acts)))]))
    return b


def positions(game, H, W, seed, n, lo, hi, n_over=0, n_above=0, above=None):
    """n boards from seeded random playouts stopped at lo..hi empty cells (cycling; a game that ends above its stop is kept as the
    finished game it is), then n_over finished games and n_above positions stopped at `above` empty cells"""
    rng = np.random.default_rng(seed)
    out = [playout(game, H, W, rng, lo + i % (hi - lo + 1)) for i in range(n)]
    out += [playout(game, H, W, rng) for _ in range(n_over)]
    out += [playout(game, H, W, rng, above) for _ in range(n_above)]
    return out


def arrays(boards):
    """(grids int8 [n, H, W], players int8 [n]) of a list of boards"""
    return (np.stack([b.grid.astype(np.int8) for b in boards]), np.array([int(b.player) for b in boards], np.int8))


# ---- the search with exact endgames (az_engine_set_exact_endgame; include/az_amd.h) ----------------------------------------------------
# solved leaf  the leaf a simulation's walk ends on (depth >= 1), not game over, with at most E empty cells: a terminal node whose
#              winner is value(board); no network row, never children, backed up with that winner now and on every later visit
# solved root  a solved node that becomes the root loses the terminal mark and keeps N and Q: an unevaluated, unexpanded root, which
#              the root-prior pass evaluates
# Everything else is leaf_batch_model.Model at K = 1 and playout_cap_model's move_policy / wave loop with the cap off.
import playout_cap_model as PC  # noqa: E402
from leaf_batch_model import Model, action_size  # noqa: E402


class ExactModel(Model):
    def __init__(self, board, E, **kw):
        super().__init__(board, K=1, **kw)
        self.E = int(E or 0)
        self.solved_ids = set()  # id() of the nodes that are terminal because they were solved
        self.solved = 0          # first-time solves
        self.memo = {}

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
            if node.terminal:
                out = float(node.win)
            elif b.is_game_over():
                node.terminal, node.win = True, int(b.get_winner())
                out = float(node.win)
            elif self.E > 0 and len(path) > 1 and empties(b) <= self.E:
                node.terminal, node.win = True, value(b, self.memo)
                self.solved_ids.add(id(node))
                self.solved += 1
                out = float(node.win)
            else:
                out = self._evaluate(node)
            self._backup(path, b.player, out)
        self.sim_base += n_sim

    def became_root(self):
        """after a re-rooting: a solved node that is the root now is an unevaluated, unexpanded root again"""
        r = self.root
        if id(r) in self.solved_ids:
            self.solved_ids.discard(id(r))
            r.terminal, r.win = False, 0


def play_game(game, H, W, seed, game_id, n_sim, E, noise, tie, tmax, tmin):
    m = ExactModel(make_board(game, H, W), E, noise=None, tie=tie, seed=seed, game_id=game_id)
    samples, plies = [], 0
    while True:
        PC.search_call(m, n_sim, None, noise)
        samples.append(PC.advance(m, tmax, tmin, True))
        m.became_root()
        plies += 1
        b = m.root.board
        if b.is_game_over():
            w = int(b.get_winner())
            for s in samples:
                s["z"] = np.int8(w * int(s["meta"][2]))
            break
    return samples, {"plies": plies, "rows": m.rows, "solved": m.solved}


def play_wave(game, H, W, seed, first_game_id, n_games, n_sim, E, noise, tie, tmax, tmin):
    """az_engine_run on the model: the samples as arrays sorted by (game id, move idx), and the counters (rows = net_evals)"""
    A = action_size(make_board(game, H, W))
    out = {"state": [], "pi": [], "visits": [], "meta": [], "z": []}
    ctr = {"plies": 0, "rows": 0, "solved": 0}
    for g in range(first_game_id, first_game_id + n_games):
        smp, c = play_game(game, H, W, seed, g, n_sim, E, noise, tie, tmax, tmin)
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


def wave(game, H, W, seed, first, n_games, n_sim, E, tie):
    """the model's wave, computed once per process"""
    key = (game, H, W, seed, first, n_games, n_sim, E, tie)
    if key not in _WAVES:
        _WAVES[key] = play_wave(game, H, W, seed, first, n_games, n_sim, E, NOISE, tie, TMAX, TMIN)
    return _WAVES[key]
