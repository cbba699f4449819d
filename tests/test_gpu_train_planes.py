"""The hand-written training step (csrc/az_train.hip) on EVERY Connect4 plane the trainer accepts: width and height 5..8, sixteen
planes.  CH = W, CW = H, P4 = (W - 4)(H - 4), FIN = 32 P4: every kernel that depends on the plane -- fc1's K split over the waves
(FIN 32 .. 512), the fc1 weight-gradient tiles, bn4's backward sums over P4 positions, the conv indexing (a 1x1 conv4 output at 5x5,
64 positions with Connect4's narrow dense layers at 8x8), six- to eight-wide heads, the fc1 weight relayout -- takes other values than
on the three planes the other files run (7x6, 5x8, 8x5 at 32 rows).
  a. every tensor's gradient, the workspace, the losses and the BatchNorm statistics of one step against float64 autograd, exactly as
     part 1 of tests/test_gpu_train_update.py (gradients per element in torch's layout: a transposed relayout or plane shows) --
     check_train_step.PLANE_CASES: the extreme planes 5x5, 7x7, 8x8 at every dense dispatch with seeds 0-2, every other plane once;
  b. three steps at the reference's hyper-parameters with dropout on the extreme planes (part 3 of that file);
  c. train_step.supports() and az_trainer_create accept the same planes.
Allowances: the project's own (check_train_step.update_rows), none new -- profiles/r32_train_planes.txt holds what the stock float32
torch step and the MI355X measured against them.  tests/test_gpu_train_state.py runs 5x5 and 7x7 for bit-reproducibility and under a
poisoned workspace (check_train_step.STATE_CASES)."""
import ctypes
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_train_step as C  # noqa: E402

pytestmark = pytest.mark.gpu

# Data seeds of part a: PLANE_CASES' own (a seed whose float32 step resolves a ReLU tie of the float64 run the other way is replaced there
# by the next unused one, under the rule beside check_train_step.PLANE_FLIPS; the flip's signature: GRAD_SEEDS in
# tests/test_gpu_train_update.py).  Part b, by (tag, batch, dropout), default 0, under the same rule:
STEPS_SEED = {("connect4_8x8", 64, 0.3): 1}  # seed 0 flips in step 1 (ties in b2, b3, a1 there; step 0 clean, then error / allowance 102)


@pytest.mark.parametrize("tag,B", [c[:2] for c in C.PLANE_CASES])
def test_every_gradient_equals_float64_autograd_on_every_plane(tag, B):
    """max|g_hip - g_ref| <= 2e-4 max|g_ref| per tensor (+ the measured zero-gradient floor on the biases a BatchNorm follows, + the
    rounding of the stored parameters elsewhere: check_train_step.update_rows), and the workspace, losses and running statistics of the
    same step under report()'s rule"""
    for seed in {c[:2]: c[2] for c in C.PLANE_CASES}[tag, B]:
        g = C.gradient_check(tag, B, seed)
        print(f"{tag} {B} seed {seed}: worst error / allowance {g['ratio']:.3g}; err / max|g_ref| {g['rel']:.3g}; zero-gradient biases {g['zero']:.3g}; ties {g['ties']}")
        assert not g["bad"] and not g["workspace_bad"] and g["ratio"] <= 1.0, (seed, g)


def test_every_connect4_plane_is_held_to_float64():
    """the sixteen planes az_trainer_create accepts, each in at least one gradient comparison of this file or of test_gpu_train_update.py"""
    tags = {t for t, *_ in C.PLANE_CASES} | {t for t, _ in C.UPDATE_CASES}
    planes = {(7, 6) if t == "connect4" else tuple(int(n) for n in t.split("_")[1].split("x")) for t in tags if t.startswith("connect4")}
    assert planes == {(w, h) for w in range(5, 9) for h in range(5, 9)}


@pytest.mark.parametrize("tag,B,dropout", [("connect4_5x5", 144, 0.3), ("connect4_7x7", 400, 0.0), ("connect4_8x8", 64, 0.3)])
def test_three_steps_on_the_extreme_planes(tag, B, dropout):
    """lr 0.1, momentum 0.9, weight decay 1e-4, the Philox mask read back into the float64 model: every step's change of every tensor
    within 2e-4 of the float64 run's largest change of that tensor (+ lr x floor) -- momentum buffers and the dropout mask where fc1's K
    is shortest (32), most ragged (288) and longest (512)"""
    seed = STEPS_SEED.get((tag, B, dropout), 0)
    rows = C.report(tag, B, 3, dropout, verbose=False, seed=seed, lr=0.1, mom=0.9, wd=1e-4)
    ratios = C.update_rows(rows, 0.1, tag, B, C.report.pmax)
    assert len(ratios) == 3 * len(C.report.pmax) and {"step0.delta.fc1.weight", "step2.delta.fc2.bias", "step1.delta.fc_value.bias"} <= {n for n, _ in ratios}
    worst = max(ratios, key=lambda r: r[1])
    print(f"{tag} {B} dropout {dropout} seed {seed}: worst change error / allowance {worst[1]:.3g} ({worst[0]}); ties {C.report.ties[:4]}")
    bad = [(n, e, s) for n, e, s in rows if ".delta." not in n and e > 2e-4 * max(s, 1e-3) + 1e-6]
    assert worst[1] <= 1.0 and not bad, ([r for r in ratios if r[1] > 1.0][:8], bad[:4], C.report.ties[:4])


def test_supports_and_create_agree():
    """width and height 4..9: train_step.supports(Connect4Net(W, H), 64) is true exactly where az_trainer_create(1, H, W, 64) succeeds;
    everywhere else the call is AZ_EINVAL and its message names the board.  Planes with a side of 4 have no conv4 output: the module
    cannot run, there is nothing to ask supports() about, and az_trainer_create refuses them too."""
    from alphazero_amd import _lib, train_step
    from alphazero_amd.games.connect4 import Connect4Net
    L = _lib.lib()
    served = set()
    for W in range(4, 10):
        for H in range(4, 10):
            h = ctypes.c_void_p()
            rc = L.az_trainer_create(1, H, W, 64, ctypes.byref(h))
            if rc == _lib.AZ_OK:
                assert h.value
                L.az_trainer_destroy(h)
                served.add((W, H))
            else:
                assert rc == _lib.AZ_EINVAL and not h.value and f"{W}x{H}".encode() in L.az_last_error(), (W, H, rc, L.az_last_error())
            if W < 5 or H < 5:
                assert rc == _lib.AZ_EINVAL
                continue
            assert train_step.supports(Connect4Net(W, H), 64) == (rc == _lib.AZ_OK), (W, H, rc)
    assert served == {(w, h) for w in range(5, 9) for h in range(5, 9)}
