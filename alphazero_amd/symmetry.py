"""The board symmetries a leaf evaluation can be averaged over (ensemble inference), and their one convention.

Transform codes are those of the device augmentation (csrc/az_device.h aug_source, engine.TRANSFORM_NAMES) plus 0 for the
identity: `code & 1` is a horizontal reflection (np.flip(axis=1)) applied first, `code >> 1` the quarter turns (np.rot90) applied
to the reflected board.  A symmetry *mask* is a set of codes, bit t = code t; its members are visited in ascending code order.
Square Othello and TicTacToe boards have all eight codes; Connect4 has the identity and the reflection only (gravity rules the
rotations out, on a square board too).

A *random* spec -- "random" (every code the board has) or ("random", members), members anything resolve() takes -- evaluates
every leaf in ONE member drawn per evaluation instead of averaging over all of them (az_engine_set_symmetry_random): parse() tells
the two kinds apart, random_code() restates the draw on the host.

The helpers work on numpy arrays and torch tensors alike and never touch the library: the device kernels (csrc/az_symmetry.hip)
are tested against them.
"""
import numpy as np

from ._lib import GAME_IDS, SYM_ALL

INVERSE = (0, 1, 6, 3, 4, 5, 2, 7)  # reflections (rotated or not) are involutions; rot90 <-> rot270


def resolve(symmetry):
    """the mask az_engine_set_symmetry / az_net_forward_sym take: "all" -> SYM_ALL (every code the board has), None -> 0 (off),
    an int mask as it is, an iterable of codes -> their bits.  The board is not known here: members() checks a mask against it."""
    if symmetry is None:
        return 0
    if isinstance(symmetry, str):
        if symmetry != "all":
            raise ValueError(f"symmetry {symmetry!r}: expected 'all', None, a mask or an iterable of transform codes 0..7")
        return SYM_ALL
    if isinstance(symmetry, (bool, np.bool_)):
        raise ValueError("symmetry: expected 'all', None, a mask or an iterable of transform codes 0..7, got a bool")
    if isinstance(symmetry, (int, np.integer)):
        mask = int(symmetry)
        if mask != SYM_ALL and not 0 <= mask <= 0xFF:
            raise ValueError(f"symmetry mask {mask}: a mask is a set of the transform codes 0..7 (bits 0..7) or SYM_ALL")
        return mask
    mask = 0
    for code in symmetry:
        if isinstance(code, (bool, np.bool_)) or not isinstance(code, (int, np.integer)) or not 0 <= int(code) <= 7:
            raise ValueError(f"symmetry code {code!r}: transform codes are the integers 0..7")
        mask |= 1 << int(code)
    return mask


def parse(symmetry):
    """(mask, is_random) of a symmetry spec: everything resolve() takes is an ensemble (or off) -> (resolve(symmetry), False);
    "random" -> (SYM_ALL, True); ("random", members) -> (resolve(members), True).  ValueError for anything else."""
    if isinstance(symmetry, str) and symmetry == "random":
        return SYM_ALL, True
    if isinstance(symmetry, (tuple, list)) and len(symmetry) >= 1 and isinstance(symmetry[0], str):
        if symmetry[0] != "random" or len(symmetry) != 2:
            raise ValueError(f"symmetry {symmetry!r}: a random spec is 'random' or ('random', members)")
        if isinstance(symmetry[1], str) and symmetry[1] == "random":
            raise ValueError(f"symmetry {symmetry!r}: the members of a random spec are 'all', a mask or transform codes 0..7")
        return resolve(symmetry[1]), True
    if isinstance(symmetry, str) and symmetry != "all":
        raise ValueError(f"symmetry {symmetry!r}: expected 'all', 'random', ('random', members), None, a mask or an iterable of "
                         f"transform codes 0..7")
    return resolve(symmetry), False


ROOT_PASS = 0xFFFFFFFF  # the `s` of the root-prior pass in random_code (a leaf's is its simulation index)


def _closed_form():
    try:
        from tools import closed_form
        return closed_form
    except ImportError:  # the package used from outside its tree: tools/ lies beside it
        import importlib.util
        import os
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "closed_form.py")
        spec = importlib.util.spec_from_file_location("_az_closed_form", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod


def random_code(seed, game_id, ply, s, members):
    """the transform code a random-mode engine evaluates a pending row in (k_sym_pick, csrc/az_engine.hip): `members` the
    candidate codes in ascending order, n of them;  r = philox4x32(seed, game_id, ply, s, P_SYMMETRY, 0),
    m = (r[0] * n) >> 32, code = members[m].  s: the simulation index of the leaf (counted from the first search on this root;
    leaf_batch K: t * K + j for walker j of lock-step t), ROOT_PASS for the root-prior pass; ply: the root's."""
    cf = _closed_form()
    members = [int(t) for t in members]
    if not members or sorted(set(members)) != members:
        raise ValueError(f"members {members!r}: the candidate codes in ascending order, at least one")
    m32 = 0xFFFFFFFF
    r = cf.philox4x32(int(seed) & m32, int(game_id) & m32, int(ply) & m32, int(s) & m32, cf.P_SYMMETRY, 0)
    return members[(r[0] * len(members)) >> 32]


def _game_id(game):
    if isinstance(game, str):
        if game not in GAME_IDS:
            raise ValueError(f"unknown game {game!r}")
        return GAME_IDS[game]
    if int(game) not in GAME_IDS.values():
        raise ValueError(f"unknown game id {game!r}")
    return int(game)


def members(game, H, W, mask):
    """the transform codes of `mask` (anything resolve() takes) in the order they are visited; ValueError for a code the board
    does not have (rotations on Connect4 or on a board that is not square)"""
    gid, mask = _game_id(game), resolve(mask)
    valid = 0xFF if gid != GAME_IDS["connect4"] and H == W else 0x3
    if mask == SYM_ALL:
        mask = valid
    if mask & ~valid:
        what = "Connect4" if gid == GAME_IDS["connect4"] else f"a {H}x{W} board"
        raise ValueError(f"symmetry mask {mask:#x} holds rotation codes: {what} has the identity and the horizontal reflection only")
    return [t for t in range(8) if mask >> t & 1]


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def twin_planes(x, code):
    """the twin of boards x[..., H, W] under `code`: what Sample.create_reflection_twin / create_rotation_twin make of a state"""
    if not 0 <= code <= 7:
        raise ValueError(f"transform code {code}: codes are 0..7")
    if _is_torch(x):
        import torch
        y = torch.flip(x, dims=(-1,)) if code & 1 else x
        return torch.rot90(y, code >> 1, dims=(-2, -1)) if code >> 1 else y
    y = np.flip(x, axis=-1) if code & 1 else x
    return np.rot90(y, code >> 1, axes=(-2, -1)) if code >> 1 else y


def twin_pi(p, code, game, H, W):
    """the twin of policies p[..., A] under `code`: reflect_neural_output / rotate_neural_output of the shipped networks
    (Othello's pass entry stays in place, Connect4 flips its columns)"""
    gid = _game_id(game)
    if gid == GAME_IDS["connect4"]:
        if code >> 1:
            raise ValueError("Connect4 has no rotations")
        if not code & 1:
            return p
        return p.flip(-1) if _is_torch(p) else np.flip(p, axis=-1)
    cells = H * W
    lead = tuple(p.shape[:-1])
    board = twin_planes(p[..., :cells].reshape(lead + (H, W)), code).reshape(lead + (cells,))
    if p.shape[-1] == cells:
        return board
    if _is_torch(p):
        import torch
        return torch.cat([board, p[..., cells:]], dim=-1)
    return np.concatenate([board, p[..., cells:]], axis=-1)


def untwin_probs(p, code, game, H, W):
    """maps policies the network produced on the twin under `code` back to the original orientation: entry a of the result is
    the twin's entry for the cell that holds original cell a (the pi mapping of the inverse code)"""
    return twin_pi(p, INVERSE[code], game, H, W)
