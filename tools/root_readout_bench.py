"""Wall time of reading back every root of a wave of games: one SelfPlayEngine.root_readout (one kernel launch, all outputs, principal
line of 8) against one root_children call per slot (a stream synchronisation and four blocking copies each), on the same engine.
Othello 8x8, fake network (the readout does not depend on what evaluated the leaves), one search.  Medians of repeats after a warm-up;
both calls block until the data is there, so the host clock brackets finished work.
usage: python tools/root_readout_bench.py [slots=4096] [sims=100]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_amd import engine as E  # noqa: E402


def main():
    G = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    sims = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    assert torch.cuda.is_available(), "needs the GPU"
    grid = np.zeros((8, 8), np.int8)
    grid[3, 3] = grid[4, 4] = 1
    grid[3, 4] = grid[4, 3] = -1
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=G, n_sim=sims, evaluator=E.EVAL_FAKE, seed=1)
    eng.set_roots(np.tile(grid[None], (G, 1, 1)), np.ones(G, np.int8), game_ids=np.arange(G))
    eng.search(sims)

    def readout():
        t = time.perf_counter()
        r = eng.root_readout(pv_len=8)
        return time.perf_counter() - t, r

    def readout_to_host():
        t = time.perf_counter()
        h = {k: v.cpu() for k, v in eng.root_readout(pv_len=8).items()}
        return time.perf_counter() - t, h

    def per_slot():
        t = time.perf_counter()
        rows = [eng.root_children(g) for g in range(G)]
        return time.perf_counter() - t, rows

    for _ in range(3):
        readout(), readout_to_host()
    per_slot()
    dev = [readout()[0] for _ in range(15)]
    hst = [readout_to_host()[0] for _ in range(15)]
    one = [per_slot()[0] for _ in range(5)]
    _, h = readout_to_host()
    _, rows = per_slot()
    a, N, Q, P, rn = rows[G - 1]
    assert np.array_equal(h["visits"][G - 1].numpy()[a], N) and int(h["root_N"][G - 1]) == rn == sims  # the two paths read the same tree
    med = statistics.median
    print(f"Othello 8x8, {G} slots, {sims} simulations searched once (fake network), {torch.cuda.get_device_name(0)}")
    print(f"root_readout (visits, pi, Q, P, child, action, root_N, pv_len 8), device tensors : median {med(dev) * 1e3:9.3f} ms"
          f"  (min {min(dev) * 1e3:.3f}, max {max(dev) * 1e3:.3f}, 15 repeats)")
    print(f"root_readout + every tensor copied to the host                                  : median {med(hst) * 1e3:9.3f} ms"
          f"  (min {min(hst) * 1e3:.3f}, max {max(hst) * 1e3:.3f}, 15 repeats)")
    print(f"{G} root_children calls (host arrays)                                          : median {med(one) * 1e3:9.3f} ms"
          f"  (min {min(one) * 1e3:.3f}, max {max(one) * 1e3:.3f}, 5 repeats) = {med(one) / G * 1e6:.1f} us per slot")
    print(f"ratio per-slot / readout-to-host: {med(one) / med(hst):.0f}x")
    print(f"slot {G - 1}: action {int(h['action'][G - 1])}, line {h['pv'][G - 1].tolist()}, visits of its children {N.tolist()}")


if __name__ == "__main__":
    main()
