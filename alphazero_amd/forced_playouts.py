"""Forced playouts and policy target pruning of the self-play wave (az_engine_set_forced_playouts): the option's
form, checked where it is given.  A spec is None (off) or KataGo's k: a real number in (0, 64] (KataGo uses 2).  Which search modes
serve it is the engine's to check."""
import math
import numbers

K_MAX = 64.0


def parse(spec, name="forced_playouts"):
    """None, or float k of a checked spec; ValueError naming `name` otherwise"""
    if spec is None:
        return None
    if isinstance(spec, bool) or not isinstance(spec, numbers.Real) or math.isnan(spec) or not 0.0 < spec <= K_MAX:
        raise ValueError(f"{name}={spec!r}: expected None or a number k in (0, 64] (KataGo: 2)")
    return float(spec)
