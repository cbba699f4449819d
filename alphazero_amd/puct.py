"""PUCT exploration settings (az_engine_set_puct): the option's form, checked where it is given.  The option is None
(off: the reference's PUCT, exploration constant 1 and an unvisited child's Q at 0), a number (taken as c_init) or a dict with any of
c_init, c_base and fpu: the exploration constant c(s) = c_init + log((1 + N(s) + c_base) / c_base) of the AlphaZero pseudocode
(c_base 0: no growth) and first-play urgency, an unvisited child's Q = the parent's value - fpu * sqrt(visited prior mass) (fpu None
or negative: off).  Which search modes serve it is the engine's to check, and is checked here before any device work."""
import math

import numpy as np

OFF = (1.0, 0.0, -1.0)  # the neutral triple: the mode off (fpu off is canonically -1)
KEYS = ("c_init", "c_base", "fpu")


def _number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_))


def parse(spec, name="puct"):
    """(c_init, c_base, fpu) as floats of a checked spec, fpu -1.0 for off (None: OFF); ValueError naming `name` otherwise"""
    if spec is None:
        return OFF
    if _number(spec):
        spec = {"c_init": spec}
    if not isinstance(spec, dict):
        raise ValueError(f"{name}={spec!r}: expected None, a number (c_init) or a dict with the keys {', '.join(KEYS)}")
    unknown = sorted(set(spec) - set(KEYS), key=str)
    if unknown:
        raise ValueError(f"{name}={spec!r}: unknown key(s) {unknown}; the keys are {', '.join(KEYS)}")
    c_init, c_base, fpu = spec.get("c_init", 1.0), spec.get("c_base", 0.0), spec.get("fpu", None)
    fpu = -1.0 if fpu is None else fpu
    for key, v in (("c_init", c_init), ("c_base", c_base), ("fpu", fpu)):
        if not _number(v):
            raise ValueError(f"{name}={spec!r}: {key} must be a number, got {v!r}")
    c_init, c_base, fpu = float(c_init), float(c_base), float(fpu)
    if not (math.isfinite(c_init) and 0.0 < c_init <= 64.0):
        raise ValueError(f"{name}={spec!r}: c_init must be finite and in (0, 64], got {c_init!r}")
    if not (c_base == 0.0 or (math.isfinite(c_base) and 1.0 <= c_base <= 1e9)):
        raise ValueError(f"{name}={spec!r}: c_base must be 0 (no growth) or finite and in [1, 1e9], got {c_base!r}")
    if not (fpu < 0.0 or (math.isfinite(fpu) and 0.0 <= fpu <= 4.0)):
        raise ValueError(f"{name}={spec!r}: fpu must be None or negative (off) or finite and in [0, 4], got {fpu!r}")
    return (c_init, c_base, -1.0 if fpu < 0.0 else fpu)


def is_on(triple):
    return tuple(triple) != OFF


def check_combination(spec, name, others):
    """`others`: {option name: value} of the modes the settings do not combine with (None / 1 / False = off); the checked triple, or
    ValueError naming both"""
    triple = parse(spec, name)
    if not is_on(triple):
        return triple
    for oname, val in others.items():
        on = bool(val) if isinstance(val, (bool, np.bool_)) else (val is not None and val != 1)  # a bool is a switch (True == 1)
        if on:
            raise ValueError(f"{name}={spec!r} does not combine with {oname}={val!r}: PUCT exploration settings are served in the plain "
                             f"PUCT search only (one leaf per lock-step, no symmetry mode, no Gumbel search, no playout cap, no forced "
                             f"playouts, no exact endgames, no proof backup)")
    return triple


def check_puct(spec, nn=None, symmetry=None, leaf_batch=None, gumbel=None, exact_endgame=None, proof_backup=False, neural=True, name="puct"):
    """the checked triple of `spec` (OFF when it switches nothing on); ValueError -- before any device work -- for a malformed one, for a
    rollout-mode tree, for a network that evaluates its leaves through an external evaluator (evaluators.route), and next to symmetry,
    leaf_batch > 1, gumbel, exact_endgame or proof_backup"""
    triple = check_combination(spec, name, {"symmetry": symmetry, "leaf_batch": leaf_batch, "gumbel": gumbel,
                                            "exact_endgame": exact_endgame, "proof_backup": proof_backup})
    if not is_on(triple):
        return triple
    if not neural:
        raise ValueError(f"{name}={spec!r} needs eval_method 'neural': a rollout tree (random playouts) is not served by the PUCT "
                         f"exploration settings")
    if nn is not None:
        from .evaluators import route
        if route(nn) != "hip":
            raise ValueError(f"{name}={spec!r} needs a network the HIP network serves; {type(nn).__name__} evaluates its leaves through "
                             f"an external evaluator, which the PUCT exploration settings are not served for")
    return triple
