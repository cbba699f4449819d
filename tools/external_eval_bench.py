"""External evaluator cost on Othello 8x8, 25 simulations: ms per lock-step and games/s (writes profiles/r06_external_eval.txt).

  net    AZ_EVAL_NET: the HIP network, searches replayed as HIP graphs
  torch  AZ_EVAL_EXTERNAL + TorchEvaluator on the stock OthelloNet module (random weights, eval mode), next to that module's own
         predict() time on the same number of rows: the engine's overhead is the difference
  board  AZ_EVAL_EXTERNAL + BoardEvaluator on the golden G3 fake net (one Board and one evaluate() per row), 64 games only

usage: python tools/external_eval_bench.py [OUT]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphazero_amd import engine as E  # noqa: E402
from alphazero_amd.evaluators import BoardEvaluator, TorchEvaluator  # noqa: E402
from alphazero_amd.games.othello import OthelloNet  # noqa: E402
from tools import closed_form as cf  # noqa: E402

SIMS = 25


class FakeNet(OthelloNet):
    def evaluate(self, board):
        probs, v_net = cf.fakenet(board.grid, board.player, 65)
        return probs, board.player * v_net


def run(games, evaluator=None, hipnet=None):
    kw = dict(seed=1, node_capacity=max(4096, 96 * SIMS))
    if evaluator is None:
        eng = E.SelfPlayEngine(0, 8, 8, n_slots=games, n_sim=SIMS, net=hipnet, **kw)
    else:
        eng = E.SelfPlayEngine(0, 8, 8, n_slots=games, n_sim=SIMS, evaluator=E.EVAL_EXTERNAL, **kw)
        eng.set_evaluator(evaluator)
    eng.run(games, first_game_id=0)  # warm-up: kernels loaded, graphs captured
    torch.cuda.synchronize()
    t = time.perf_counter()
    eng.run(games, first_game_id=games)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    st = eng.stats()
    eng.close()
    return 1e3 * dt / st["lockstep_iters"], games / dt, st["lockstep_iters"]


def predict_ms(net, rows, iters=20):
    x = torch.randint(-1, 2, (rows, 8, 8), device="cuda").float()
    net.predict(x)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        net.predict(x)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_external_eval.txt")
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda").eval()
    lines = [f"# tools/external_eval_bench.py: Othello 8x8, {SIMS} simulations, {torch.cuda.get_device_name(0)}",
             "# mode   games  ms/lock-step  games/s  lock-steps  | module predict() ms at `games` rows"]
    for games in (64, 512, 4096):
        hip = net.to_hip(max_batch=games)
        ms, gps, it = run(games, hipnet=hip)
        lines.append(f"net    {games:6d} {ms:12.3f} {gps:9.1f} {it:10d}")
        hip.close()
        ms, gps, it = run(games, evaluator=TorchEvaluator(net))
        lines.append(f"torch  {games:6d} {ms:12.3f} {gps:9.1f} {it:10d}  | {predict_ms(net, games):.3f}")
    ms, gps, it = run(64, evaluator=BoardEvaluator(FakeNet(8), "othello", 8, 8))
    lines.append(f"board  {64:6d} {ms:12.3f} {gps:9.1f} {it:10d}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
