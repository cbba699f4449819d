#!/usr/bin/env python3
"""Diagnostic (needs `make -C alphazero_amd/csrc -B PROBE=1`): k_gemm's own clocks on the 64 x 64 tile beside another chain, for both
forms (AZ_GEMM_FORM=0 double buffer, 1 ring; one child process each, the library reads the switch once).  OthelloNet 8x8, 2048-row
launches with a device count of 1885 under the beside flag: lane 0 alone, then lanes 0 and 1 side by side on two streams.  Per layer
(told apart by the K tiles a block stamps: fc1 16, fc2 32): shader cycles per K tile of wave 0 of every block over the tile loop
(ideal: 16 MFMAs x 64 = 1024), the part of it between the stamps around the k-steps, and the share of the loop outside the MFMA
chain = 1 - 1024 T / loop.  That share is against ONE chain: fc1 has two waves on most SIMDs (480 blocks), whose ideal is 2048 per K
tile for the two, so its printed share counts the partner's MFMAs as a stop (2590 cycles: 59 % printed, 21 % of the pair's time).
The stamps drain the LDS counter, so a probed tile is a little slower than an unprobed one: compare the forms, not the absolute
figures.
  python tools/probe_gemm.py"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import numpy as np
    import torch

    from alphazero_amd import engine as E
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(0)
    hnet = OthelloNet(n=8).eval().to_hip(max_batch=2048)
    L = E.lib()
    L.az_debug_read_probe.argtypes = [C.c_void_p, C.c_int]
    E.check(L.az_net_set_lanes(hnet.h, 2, 2048))
    x = [torch.randint(-1, 2, (2048, 64), device="cuda").float() for _ in range(2)]
    cnt = torch.tensor([1885], dtype=torch.int32, device="cuda")
    pr = [torch.zeros((2048, hnet.A), device="cuda") for _ in range(2)]
    va = [torch.zeros(2048, device="cuda") for _ in range(2)]
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]

    def run(lanes, n):
        for _ in range(n):
            for l in lanes:
                E.check(L.az_net_forward_lane(hnet.h, l, 1, x[l].data_ptr(), cnt.data_ptr(), 2048, pr[l].data_ptr(), va[l].data_ptr(), C.c_void_p(ss[l].cuda_stream)))
        torch.cuda.synchronize()

    for lanes, what in (((0,), "alone"), ((0, 1), "two chains")):
        run(lanes, 20)
        buf = np.zeros(480 * 8, dtype=np.uint64)  # 30 row bands x 16 column tiles of fc1; fc2's 240 blocks stamp the first 240 slots
        assert L.az_debug_read_probe(buf.ctypes.data, buf.size) == 0
        b = buf.reshape(-1, 8).astype(np.float64)
        for name, T in (("fc1", 16), ("fc2", 32)):
            s = b[b[:, 4] == T]
            loop = s[:, 6] - s[:, 5]
            print("form %s, %s, %s: %d blocks; loop %.0f cycles = %.0f per K tile (ideal 1024), %.0f of them in the k-steps, %.0f at the barrier, "
                  "%.0f in the staging phases; outside the MFMA chain %.1f %%; %.2f GHz"
                  % (os.environ["AZ_GEMM_FORM"], what, name, len(s), loop.mean(), (loop / T).mean(), (s[:, 1] / T).mean(), (s[:, 3] / T).mean(),
                     ((s[:, 0] + s[:, 2]) / T).mean(), 100.0 * (1.0 - 1024.0 * T / loop).mean(), (loop / (s[:, 7] * 10.0)).mean()), flush=True)
    os._exit(0)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
    for form in ("0", "1"):
        env = {k: v for k, v in os.environ.items() if k != "AZ_GEMM_FORM"}
        env["AZ_GEMM_FORM"] = form
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "child"], env=env)
        if rc != 0:  # nothing more on the GPU behind a failed leg
            sys.exit(rc)
