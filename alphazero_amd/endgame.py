"""Exact endgames (az_solve_batch, az_engine_set_exact_endgame): the option's form, checked where it is given, and
the batched solver on the mirror's Board objects.  A spec is None (off) or E: an int in [1, 10] -- a leaf of the search with at most E
empty cells is solved by alpha-beta on the device and backed up with its outcome instead of the network's value.  Which search modes
serve it is the engine's to check."""
import numbers

MAX_EMPTIES = 10        # AZ_EXACT_MAX_EMPTIES: the search's limit
SOLVE_MAX_EMPTIES = 12  # AZ_SOLVE_MAX_EMPTIES: solve()'s limit
UNSOLVED = 2            # AZ_UNSOLVED


def parse(spec, name="exact_endgame"):
    """None, or int E of a checked spec; ValueError naming `name` otherwise"""
    if spec is None:
        return None
    if isinstance(spec, bool) or not isinstance(spec, numbers.Integral) or not 1 <= spec <= MAX_EMPTIES:
        raise ValueError(f"{name}={spec!r}: expected None or an int E in [1, {MAX_EMPTIES}] (the empty cells of a leaf that is solved)")
    return int(spec)


def check_combination(spec, name, others):
    """`others`: {option name: value} of the modes exact endgames do not combine with (None / 1 / False = off); ValueError naming both"""
    e = parse(spec, name)
    if e is None:
        return None
    for oname, val in others.items():
        if val is not None and val is not False and val != 1:
            raise ValueError(f"{name}={spec!r} does not combine with {oname}={val!r}: exact endgames are served in the plain PUCT search "
                             f"only (one leaf per lock-step, no playout cap, no forced playouts)")
    return e


def check_exact_endgame(spec, nn=None, symmetry=None, leaf_batch=None, gumbel=None, neural=True, name="exact_endgame"):
    """the E of `spec` (None: off); ValueError -- before any device work -- for a malformed one, for a rollout-mode tree, for a network
    that evaluates its leaves through an external evaluator (evaluators.route), and next to symmetry, leaf_batch > 1 or gumbel"""
    e = check_combination(spec, name, {"symmetry": symmetry, "leaf_batch": leaf_batch, "gumbel": gumbel})
    if e is None:
        return None
    if not neural:
        raise ValueError(f"{name}={spec!r} needs eval_method 'neural': a rollout tree (random playouts) is not served by exact endgames")
    if nn is not None:
        from .evaluators import route
        if route(nn) != "hip":
            raise ValueError(f"{name}={spec!r} needs a network the HIP network serves; {type(nn).__name__} evaluates its leaves through "
                             f"an external evaluator, which exact endgames are not served for")
    return e


def solve(boards, max_empties=SOLVE_MAX_EMPTIES, node_budget=0):
    """[(winner, move)] of the mirror's Board objects (one game and board shape), solved on the device (az_solve_batch).  winner = the
    outcome under optimal play by both sides as an absolute player id; move = the lowest-indexed move that keeps it, in the board's
    own move type (Othello's pass move where the side to move must pass).  A finished game: (its winner, None).  A board with more than
    max_empties empty cells, or one that spent node_budget: (None, None)."""
    import numpy as np
    import torch
    from . import engine as E
    from .mcts import _move_of
    boards = list(boards)
    if not isinstance(max_empties, numbers.Integral) or isinstance(max_empties, bool) or not 1 <= max_empties <= SOLVE_MAX_EMPTIES:
        raise ValueError(f"max_empties={max_empties!r}: expected an int in [1, {SOLVE_MAX_EMPTIES}]")
    if not boards:
        return []
    b0 = boards[0]
    H, W = b0.grid.shape
    if any(b.game != b0.game or b.grid.shape != (H, W) for b in boards):
        raise ValueError("solve: the boards must be of one game and one shape")
    gid = E.GAME_IDS[b0.game]
    grids = torch.from_numpy(np.stack([np.asarray(b.grid).astype(np.int8) for b in boards])).cuda()
    players = torch.tensor([int(b.player) for b in boards], dtype=torch.int8).cuda()
    win, act = E.solve_batch(gid, H, W, grids, players, max_empties, node_budget)
    win, act = win.cpu().tolist(), act.cpu().tolist()
    out = []
    for b, w, a in zip(boards, win, act):
        if w == UNSOLVED:
            out.append((None, None))
        else:
            out.append((w, None if a < 0 else _move_of(b, a)))
    return out
