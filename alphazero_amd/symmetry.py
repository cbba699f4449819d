"""The board symmetries a leaf evaluation can be averaged over (ensemble inference), and their one convention.

Transform codes are those of the device augmentation (csrc/az_device.h aug_source, engine.TRANSFORM_NAMES) plus 0 for the
identity: `code & 1` is a horizontal reflection (np.flip(axis=1)) applied first, `code >> 1` the quarter turns (np.rot90) applied
to the reflected board.  A symmetry *mask* is a set of codes, bit t = code t; its members are visited in ascending code order.
Square Othello and TicTacToe boards have all eight codes; Connect4 has the identity and the reflection only (gravity rules the
rotations out, on a square board too).

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
