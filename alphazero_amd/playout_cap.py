"""Playout cap randomization of the self-play wave (az_engine_set_playout_cap): the option's form, checked where it
is given.  A spec is None (off) or (n_fast, p_full): n_fast >= 1 simulations on a fast ply, p_full in (0, 1] the share of full plies.
That n_fast is below the search's simulations is the engine's to check: only it knows them."""
import math
import numbers


def parse(spec, name="playout_cap"):
    """None, or (int n_fast, float p_full) of a checked spec; ValueError naming `name` otherwise"""
    if spec is None:
        return None
    form = f"{name}={spec!r}: expected None or (n_fast, p_full) with an integer n_fast >= 1 and p_full in (0, 1]"
    if isinstance(spec, (str, bytes)) or not hasattr(spec, "__len__") or len(spec) != 2:
        raise ValueError(form)
    n_fast, p_full = spec
    if isinstance(n_fast, bool) or not isinstance(n_fast, numbers.Integral) or n_fast < 1 or n_fast >= 1 << 31:
        raise ValueError(form)
    if isinstance(p_full, bool) or not isinstance(p_full, numbers.Real) or math.isnan(p_full) or not 0.0 < p_full <= 1.0:
        raise ValueError(form)
    return int(n_fast), float(p_full)
