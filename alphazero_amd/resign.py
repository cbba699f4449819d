"""Resignation in self-play (az_engine_set_resign): the option's form, checked where it is given, and the
calibration of the threshold from a wave's game log.

A spec is None (off) or a dict of
  threshold    v_resign in [-1, 0): a side whose last `consecutive` tested values are all below it triggers
  consecutive  k in [1, 4] (default 1)
  min_ply      >= 0 (default 0): earlier plies are untested
  holdout      in [0, 1] (default 0.1): the share of games played out whatever the rule says; 1.0 records and never resigns
and, where the caller allows it (the trainer), calibrate = None or target_fp in [0, 1): the next wave's threshold is calibrate() of this
wave's log."""
import math
import numbers

import numpy as np

MAX_CONSECUTIVE = 4
KEYS = ("threshold", "consecutive", "min_ply", "holdout")
BELOW_ZERO = float(np.nextafter(0.0, -1.0))  # the greatest threshold: v_resign < 0


def _real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and not math.isnan(v)


def _int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def parse(spec, name="resign", calibrate=False):
    """None, or the checked spec as a dict of float threshold, int consecutive, int min_ply, float holdout (and, with calibrate=True,
    calibrate = None or a float target); ValueError naming `name` otherwise"""
    if spec is None:
        return None
    keys = KEYS + (("calibrate",) if calibrate else ())
    form = (f"{name}={spec!r}: expected None or a dict of threshold in [-1, 0), consecutive in [1, {MAX_CONSECUTIVE}], min_ply >= 0, "
            f"holdout in [0, 1]" + (", calibrate None or a target false-positive rate in [0, 1)" if calibrate else ""))
    if not isinstance(spec, dict) or "threshold" not in spec or any(k not in keys for k in spec):
        raise ValueError(form)
    t, k, mp, ho = spec["threshold"], spec.get("consecutive", 1), spec.get("min_ply", 0), spec.get("holdout", 0.1)
    if not _real(t) or not -1.0 <= t < 0.0:
        raise ValueError(form)
    if not _int(k) or not 1 <= k <= MAX_CONSECUTIVE:
        raise ValueError(form)
    if not _int(mp) or mp < 0 or mp >= 1 << 31:
        raise ValueError(form)
    if not _real(ho) or not 0.0 <= ho <= 1.0:
        raise ValueError(form)
    out = {"threshold": float(t), "consecutive": int(k), "min_ply": int(mp), "holdout": float(ho)}
    if calibrate:
        c = spec.get("calibrate")
        if c is not None and (not _real(c) or not 0.0 <= c < 1.0):
            raise ValueError(form)
        out["calibrate"] = None if c is None else float(c)
    return out


def calibrate(low, winner, target_fp, current, holdout=None):
    """The threshold for the next wave from this wave's game log.  low: [n, 2] float64, the games' low values (column 0 player +1,
    column 1 player -1; 2.0: the side's window was never full); winner: [n] in {-1, 0, +1}; holdout: None (every row is a holdout
    game) or [n] truth values selecting them.  Over the non-losing sides of the holdout games -- player +1 where winner >= 0, player
    -1 where winner <= 0, both in a draw -- the low values are sorted ascending, c = floor(target_fp * n_sides), and the result is
    low[c] clipped into [-1, 0): at most c of those sides have low < the result, that is, would have resigned a game they did not
    lose.  Without such a side the current threshold is returned."""
    if not _real(target_fp) or not 0.0 <= target_fp < 1.0:
        raise ValueError(f"calibrate: target_fp={target_fp!r} must be in [0, 1)")
    low = np.asarray(low, np.float64).reshape(-1, 2)
    winner = np.asarray(winner).reshape(-1).astype(np.int64)
    if len(low) != len(winner):
        raise ValueError(f"calibrate: {len(low)} rows of low for {len(winner)} winners")
    keep = np.ones(len(winner), bool) if holdout is None else np.asarray(holdout).reshape(-1).astype(bool)
    if len(keep) != len(winner):
        raise ValueError(f"calibrate: {len(keep)} holdout flags for {len(winner)} winners")
    sides = np.sort(np.concatenate([low[keep & (winner >= 0), 0], low[keep & (winner <= 0), 1]]))
    if len(sides) == 0:
        return float(current)
    c = int(math.floor(float(target_fp) * len(sides)))
    return float(min(max(float(sides[c]), -1.0), BELOW_ZERO))
