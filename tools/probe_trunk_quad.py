#!/usr/bin/env python3
"""Diagnostic (needs `make -C alphazero_amd/csrc -B PROBE=1`): k_trunk_quad's own clocks beside another chain, for both forms
(AZ_TRUNK_QUAD_PREFETCH=0 as it was, 1 prefetching; one child process each, the library reads the switch once).  OthelloNet 8x8,
2048-row launches with a device count of 1885 under the beside flag: lane 0 alone, then lanes 0 and 1 side by side on two streams.
Every wave stamps 23 places (az_net.hip: TSTAMP).  Printed, as means over the waves that hold a board, in shader cycles: per phase the
cycles inside the MFMA chain (from behind the issue of the phase's first k-step to behind its last) and outside it (everything from
the phase before up to that first k-step: the waits for weights, input and patches, the transforms' start, stores); per barrier the
wait of the wave that arrives first and of the one that arrives last in its workgroup.  The stamps drain the LDS counter, so a probed
kernel is a little slower than an unprobed one: compare the forms, not the absolute figures.  fc1 / fc2 stamp the first 3840 words of
the same buffer behind the trunk, so workgroups 0 .. 39 are left out.  AZ_TRUNK_QUAD_STORES in the environment reaches both children
(0 / 1: the prefetching form's scalar / vector stores); one leg alone: AZ_TRUNK_QUAD_PREFETCH=1 ... child.
  python tools/probe_trunk_quad.py [child]"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNT, ROWS, FIRST_WG = 1885, 2048, 40
# (name, stamp the phase starts behind, first k-step, last k-step); ideal chain cycles of the 8x8 plane in the comment column
PHASES = [("conv2 pass 0", 3, 4, 5), ("conv2 pass 1", 5, 6, 7), ("conv2 pass 2", 7, 8, 9), ("conv2 pass 3", 9, 10, 11), ("conv3", 13, 14, 15), ("conv4", 19, 20, 21)]
OTHER = [("entry -> count known", 0, 1), ("count -> input in LDS", 1, 2), ("conv1 (chain and store)", 2, 3), ("conv2 carries, store", 11, 12),
         ("conv3 tail", 15, 16), ("conv3 store", 17, 18), ("conv4 store", 21, 22)]
BARRIERS = [("barrier 1 (conv2 in LDS)", 12, 13), ("barrier 2 (conv2 planes read)", 16, 17), ("barrier 3 (conv3 in LDS)", 18, 19)]


def child():
    import numpy as np
    import torch

    from alphazero_amd import engine as E
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(0)
    hnet = OthelloNet(n=8).eval().to_hip(max_batch=ROWS)
    L = E.lib()
    L.az_debug_read_probe.argtypes = [C.c_void_p, C.c_int]
    E.check(L.az_net_set_lanes(hnet.h, 2, ROWS))
    x = [torch.randint(-1, 2, (ROWS, 64), device="cuda").float() for _ in range(2)]
    cnt = torch.tensor([COUNT], dtype=torch.int32, device="cuda")
    pr = [torch.zeros((ROWS, hnet.A), device="cuda") for _ in range(2)]
    va = [torch.zeros(ROWS, device="cuda") for _ in range(2)]
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]

    def run(lanes, n):
        for _ in range(n):
            for l in lanes:
                E.check(L.az_net_forward_lane(hnet.h, l, 1, x[l].data_ptr(), cnt.data_ptr(), ROWS, pr[l].data_ptr(), va[l].data_ptr(), C.c_void_p(ss[l].cuda_stream)))
        torch.cuda.synchronize()

    form = ("prefetching, vector stores" if hnet.trunk_stores(ROWS, 1) else "prefetching") if hnet.trunk_prefetch(ROWS, 1) else "as it was"
    for lanes, what in (((0,), "alone"), ((0, 1), "two chains")):
        run(lanes, 20)
        n_wg = (COUNT + 3) // 4
        buf = np.zeros(n_wg * 4 * 24, dtype=np.uint64)
        assert L.az_debug_read_probe(buf.ctypes.data, buf.size) == 0
        t = buf.reshape(n_wg, 4, 24)[FIRST_WG:].astype(np.float64)
        assert (t[:, :, 23] > 0).all(), "a wave left no stamps: is this a PROBE=1 build, and did k_trunk_quad run?"
        has = t[:, :, 23] == 2
        w = t[has]  # [waves with a board][24]
        print("k_trunk_quad %s (AZ_TRUNK_QUAD_PREFETCH=%s), %s: %d workgroups, %d waves with a board; whole kernel %.0f cycles per wave"
              % (form, os.environ["AZ_TRUNK_QUAD_PREFETCH"], what, len(t), len(w), (w[:, 22] - w[:, 0]).mean()))
        inside = outside = 0.0
        for name, a, b, c in PHASES:
            inside += (w[:, c] - w[:, b]).mean(); outside += (w[:, b] - w[:, a]).mean()
            print("  %-34s in the chain %6.0f   ahead of its first k-step %6.0f" % (name, (w[:, c] - w[:, b]).mean(), (w[:, b] - w[:, a]).mean()))
        for name, a, b in OTHER:
            outside += (w[:, b] - w[:, a]).mean()
            print("  %-34s %6.0f" % (name, (w[:, b] - w[:, a]).mean()))
        full = t[has.all(axis=1)]  # workgroups of four boards: [wg][wave][24]
        for name, a, b in BARRIERS:
            wait = full[:, :, b] - full[:, :, a]
            outside += (w[:, b] - w[:, a]).mean()
            print("  %-34s mean wait %6.0f   first-arriving wave %6.0f   last-arriving wave %6.0f" % (name, wait.mean(), wait.max(axis=1).mean(), wait.min(axis=1).mean()))
        print("  sum: in the MFMA chains %.0f, outside %.0f" % (inside, outside), flush=True)
    os._exit(0)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
    for form in ("0", "1"):
        env = {k: v for k, v in os.environ.items() if k != "AZ_TRUNK_QUAD_PREFETCH"}
        env["AZ_TRUNK_QUAD_PREFETCH"] = form
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "child"], env=env)
        if rc != 0:  # nothing more on the GPU behind a failed leg
            sys.exit(rc)
