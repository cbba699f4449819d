"""The Gumbel root search ("Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022) as the engine runs it
(az_engine_set_gumbel, include/az_amd.h): the spec the players take, the Sequential Halving schedule, and plain
Python restatements of the engine's deterministic log / exp and of its Gumbel draw.  No device work here.

Every operation of det_log / det_exp is one IEEE float64 operation (no fma), so Python floats follow az_det_log / az_det_exp bit
for bit."""
import math
import struct

import numpy as np

_INF = float("inf")
MAX_GUMBEL = 16  # AZ_MAX_GUMBEL (include/az_amd.h)
P_GUMBEL = 9     # AZ_P_GUMBEL: Philox counter word 2 of the root's Gumbel draws
DEFAULTS = {"m": 16, "c_visit": 50.0, "c_scale": 0.5, "gumbel_scale": 1.0}


def parse(spec):
    """None (off) -> None; an int m, or a dict with any of m / c_visit / c_scale / gumbel_scale -> (m, c_visit, c_scale,
    gumbel_scale) with the defaults filled in.  c_scale 0.5 on this engine's Q in [-1, 1] is the paper's c_scale 1 on values in
    [0, 1].  ValueError for a bool or non-integer m, m outside 1..16, a constant that is negative or not finite, an unknown key."""
    if spec is None:
        return None
    d = dict(DEFAULTS)
    if isinstance(spec, dict):
        unknown = set(spec) - set(DEFAULTS)
        if unknown:
            raise ValueError(f"gumbel: unknown keys {sorted(unknown)}; expected {sorted(DEFAULTS)}")
        d.update(spec)
    else:
        d["m"] = spec
    m = d["m"]
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)):
        raise ValueError(f"gumbel: m must be an integer in 1..{MAX_GUMBEL}, got {m!r}")
    if not 1 <= int(m) <= MAX_GUMBEL:
        raise ValueError(f"gumbel: m must be in 1..{MAX_GUMBEL}, got {int(m)}")
    out = [int(m)]
    for k in ("c_visit", "c_scale", "gumbel_scale"):
        v = d[k]
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"gumbel: {k} must be a number, got {v!r}")
        v = float(v)
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"gumbel: {k} must be finite and >= 0, got {v!r}")
        out.append(v)
    return tuple(out)


def check_gumbel(gumbel, nn=None, leaf_batch=None, neural=True, compute_time=None):
    """parse(gumbel); ValueError -- before any device work -- when the mode is asked for together with compute_time, leaf_batch > 1,
    rollout evaluation (`neural` False) or a network the external evaluator serves (evaluators.route)."""
    g = parse(gumbel)
    if g is None:
        return None
    if compute_time is not None:
        raise ValueError("gumbel: the schedule is a function of n_sim; a compute_time search has none")
    if not neural:
        raise ValueError("gumbel needs eval_method 'neural': random playouts give the root no priors to sample from")
    if leaf_batch is not None and not isinstance(leaf_batch, (bool, np.bool_)) and isinstance(leaf_batch, (int, np.integer)) and int(leaf_batch) > 1:
        raise ValueError(f"gumbel does not combine with leaf_batch={int(leaf_batch)}: the Gumbel root search takes one leaf per lock-step")
    if nn is not None:
        from .evaluators import route
        if route(nn) != "hip":
            raise ValueError(f"gumbel needs a network the HIP network serves; {type(nn).__name__} evaluates its leaves through an "
                             f"external evaluator, which searches with the PUCT root only")
    return g


def schedule(n, m0):
    """the phases [(m_p, v_p)] of a search call of n simulations over m0 = min(m, n_children) sampled actions: phase p visits each
    of its m_p candidates v_p times, one round after the other; the last phase is cut where the n simulations end."""
    n, m0 = int(n), int(m0)
    if n <= 0 or m0 <= 0:
        return []
    if m0 == 1:
        return [(1, n)]
    L = (m0 - 1).bit_length()  # ceil(log2 m0)
    out, dealt, mp = [], 0, m0
    while dealt < n:
        v = max(1, n // (L * mp))
        out.append((mp, v))
        dealt += mp * v
        mp = max(2, mp // 2)
    return out


def locate(s, n, m0):
    """(phase, m_p, index inside the phase) of simulation s of a search call of n"""
    start = 0
    for p, (mp, v) in enumerate(schedule(n, m0) if 0 <= s < n else []):
        if s < start + mp * v:
            return p, mp, s - start
        start += mp * v
    raise ValueError(f"simulation {s} is beyond the {n} of the search")


MAX_GUMBEL_BATCH = 16  # AZ_MAX_LEAF_BATCH: walkers per slot and lock-step


def check_gumbel_batch(gumbel_batch, gumbel=None, symmetry=None):
    """int(gumbel_batch) (az_engine_set_gumbel_batch); ValueError -- before any device work -- for a bool or a
    non-integer, a value outside 1..16, and for a value > 1 without the Gumbel mode or together with the symmetry ensemble "all"."""
    k = gumbel_batch
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"gumbel_batch must be an integer in 1..{MAX_GUMBEL_BATCH}, got {k!r}")
    k = int(k)
    if not 1 <= k <= MAX_GUMBEL_BATCH:
        raise ValueError(f"gumbel_batch must be in 1..{MAX_GUMBEL_BATCH}, got {k}")
    if k > 1 and gumbel is None:
        raise ValueError(f"gumbel_batch={k} needs the Gumbel root search (gumbel=...): it batches the simulations of Sequential Halving")
    if k > 1 and isinstance(symmetry, str) and symmetry == "all":
        raise ValueError(f"gumbel_batch={k} does not combine with symmetry='all' (the ensemble evaluates one leaf per slot and lock-step)")
    return k


def check_gumbel_full(full, gumbel=None):
    """bool(full) (az_engine_set_gumbel_full; DESIGN section 18: the paper's v_mix and its deterministic selection below the root);
    ValueError -- before any device work -- for anything but a bool, and for True without the Gumbel mode (gumbel=...)."""
    if not isinstance(full, (bool, np.bool_)):
        raise ValueError(f"gumbel_full must be True or False, got {full!r}")
    if full and gumbel is None:
        raise ValueError("gumbel_full=True needs the Gumbel root search (gumbel=...): it completes that search below the root")
    return bool(full)


def nonroot_choice(pi, counts, virtual=None):
    """the child the full Gumbel search takes below the root: the index of the greatest
    key(b) = pi[b] - (counts[b] + virtual[b]) / (1 + sum(counts) + sum(virtual)) in float64, the lowest index among equals.
    pi: the improved policy pi' at the parent (real counts only); counts: the children's real visit counts; virtual: their virtual
    counts (None: all 0).  ValueError when no key compares (NaN)."""
    n = len(pi)
    virtual = [0] * n if virtual is None else virtual
    tot = float(1 + sum(int(c) for c in counts) + sum(int(v) for v in virtual))
    best, pick = -_INF, -1
    for b in range(n):
        key = float(pi[b]) - float(int(counts[b]) + int(virtual[b])) / tot
        if pick < 0 and key == key or key > best:
            best, pick = key, b
    if pick < 0:
        raise ValueError("nonroot_choice: every key is NaN")
    return pick


def lockstep_plan(n, m0, K):
    """the lock-steps [(s, kt)] of a search call of n simulations over m0 sampled actions with gumbel_batch = K: s is the slot's
    cursor at the start of the lock-step, kt = min(K, end of the current phase - s, n - s) its walkers.  No lock-step crosses a
    phase boundary of schedule(n, m0); m0 <= 1 (also a root without children) is the one phase of n."""
    n, m0, K = int(n), max(1, int(m0)), int(K)
    if K < 1:
        raise ValueError(f"K must be >= 1, got {K}")
    ends, e = [], 0
    for mp, v in schedule(n, m0):
        e = min(n, e + mp * v)
        ends.append(e)
    out, s, p = [], 0, 0
    while s < n:
        while ends[p] <= s:
            p += 1
        kt = min(K, ends[p] - s)
        out.append((s, kt))
        s += kt
    return out


def locksteps(n, m, K):
    """Lmax(n, m, K): the lock-steps the host enqueues per search call (plus the final backup-only launch) -- the longest plan of
    any m0 in 1..m, a pure function, so the launch sequence is the same for every slot count and captures as a graph"""
    return max((len(lockstep_plan(n, m0, K)) for m0 in range(1, int(m) + 1)), default=0)


def det_log(x):
    """az_det_log (csrc/az_device.h)"""
    x = float(x)
    if not x > 0.0:
        return -_INF
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    e = ((u >> 52) & 0x7FF) - 1023
    m = struct.unpack("<d", struct.pack("<Q", (u & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000))[0]
    if m > 1.4142135623730951:
        m = m * 0.5
        e += 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = 1.0 / 25.0
    for d in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * z + 1.0 / d
    lm = 2.0 * s * (1.0 + z * p)
    de = float(e)
    return de * 0.693147180369123816490 + (lm + de * 1.90821492927058770002e-10)


def det_exp(x):
    """az_det_exp (csrc/az_device.h)"""
    x = float(x)
    if not x > -700.0:
        return 0.0
    if x > 700.0:
        x = 700.0
    k = float(math.floor(x * 1.4426950408889634 + 0.5))
    r = (x - k * 0.693147180369123816490) - k * 1.90821492927058770002e-10
    p = 1.0 / 87178291200.0
    for d in (6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / d
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    return p * struct.unpack("<d", struct.pack("<Q", (int(k) + 1023) << 52))[0]


def gumbel_g(seed, gid, ply, action, scale=1.0):
    """g(action) of the root of game `gid` at `ply`: 0.0 (no draw) for scale 0, else scale * -log(-log(u)) on the Philox stream"""
    from tools.closed_form import philox4x32, u53
    scale = float(scale)
    if scale == 0.0:
        return 0.0
    r = philox4x32(int(seed) & 0xFFFFFFFF, int(gid) & 0xFFFFFFFF, int(ply) & 0xFFFFFFFF, 0xFFFF, P_GUMBEL, int(action))
    u = u53(r[0], r[1])
    if u == 0.0:
        u = 1.0 / 9007199254740992.0
    return scale * (-det_log(-det_log(u)))
