"""The hand-written training step's PARAMETER UPDATE at its own scale (csrc/az_train.hip; helpers in tools/check_train_step.py).

tests/test_gpu_train_step.py compares the parameters after 1-3 steps with a tolerance of 2e-4 of the parameter: one step of weight decay
is 0.025 of that, and no weight gradient of the step is readable (fc1 / fc2 update inside the gradient tile's epilogue, everything else
through sgd() from several kernels, TicTacToeNet in k_ttt_step).  Here the hyper-parameters of begin() isolate each quantity:
  1. every tensor's gradient, (p0 - p1) / L of one step at momentum 0, weight decay 0, learning rate L = 16, against float64 autograd
     at 2e-4 of the GRADIENT's largest magnitude -- every dispatch of enqueue_step and every heads width, seeds 0-2;
  2. weight decay, momentum and set_lr() as identities of the step with itself, to rounding bounds derived from the three fmaf of the
     update (no reference, no measured tolerance, no exceptions);
  3. three steps at the reference's hyper-parameters against float64 by per-step change, row-split batch sizes included;
  4. one steps() call of 11 steps (plain launch, the eight-step graph, one-step replays) bit-equal to 11 calls of one step;
  5. every value of every AZ_TRAIN_* switch in child processes: 1 and 2 again where the switch changes the launch sequence, with float64
     as the judge, and 4's result bit-equal without graphs and with three-step graphs.
Allowances: check_train_step.update_rows / identity_check say where each figure comes from; profiles/r07_update_parity.txt holds what
the MI355X and the stock float32 torch step measured against them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_train_step as C  # noqa: E402

pytestmark = pytest.mark.gpu

# (tag, batch, steps, dropout, seed) of parts 1, 3 and 5 whose float64 run has a ReLU input on the kink AND whose float32 step resolves
# it the other way (tools/check_train_step.py::relu_ties; parts 1 and 5 run (tag, batch, 1, 0.0, seed)).  Parts 2 and 4 have no exceptions.
KNOWN_RELU_TIES = set()
assert len(KNOWN_RELU_TIES) <= 3


# Data seeds.  Seeds 0, 1, 2 as in tests/test_gpu_train_step.py, except where the float32 step resolves a ReLU tie of the float64 run
# the other way: with up to 512 x 64 x 32 ReLU inputs per layer and three steps at lr 0.1 that is one run in three at the large batch
# sizes, far more than the three excuses KNOWN_RELU_TIES may hold, so those (case, seed) pairs take the next seed that has no such flip
# (tools/list_relu_ties.py finds them; the replaced seed is named beside its replacement).
# Measured on an MI355X over seeds 0-7 (profiles/r07_update_parity.txt): a run is either clean (error / allowance <= 0.03 in part 1,
# <= 0.27 in part 3) or has flipped a unit (>= 4, typically 20 .. 1000; a flip in the last step shows as 0.8 with one workspace row off).
GRAD_SEEDS = {("othello8", 144): (3, 1, 2), ("othello8", 320): (3, 1, 2), ("connect4", 144): (3, 1, 2),  # part 1 (part 5: first entry); seed 0 flips
              ("othello6", 48): (0, 3, 2)}                                                              # seed 1 flips; default (0, 1, 2)
STEPS_SEED = {("othello8", 272, 0.0): 1, ("othello8", 272, 0.3): 3, ("othello8", 512, 0.0): 1, ("connect4", 512, 0.3): 1,  # part 3: seed 0 flips (default 0)
              ("othello6", 400, 0.0): 3, ("othello6", 48, 0.0): 1}


def _excused(key, ties):
    if key in KNOWN_RELU_TIES:
        assert ties, ("listed as a ReLU tie, but the float64 run has no unit on a kink", key)
        return True
    return False


@pytest.mark.parametrize("tag,B", C.UPDATE_CASES)
def test_every_gradient_equals_float64_autograd(tag, B):
    """part 1.  max|g_hip - g_ref| <= 2e-4 max|g_ref| per tensor (+ the measured zero-gradient floor on the biases a BatchNorm follows,
    + the rounding of the stored parameters elsewhere: check_train_step.update_rows), and the workspace of the same step under the
    existing rule: at L = 16 a kernel that read an already-updated weight would be 16 steps off."""
    for seed in GRAD_SEEDS.get((tag, B), (0, 1, 2)):
        g = C.gradient_check(tag, B, seed)
        print(f"{tag} {B} seed {seed}: worst error / allowance {g['ratio']:.3g}; err / max|g_ref| {g['rel']:.3g}; zero-gradient biases {g['zero']:.3g}; ties {g['ties']}")
        if _excused((tag, B, 1, 0.0, seed), g["ties"]):
            continue
        assert not g["bad"] and not g["workspace_bad"] and g["ratio"] <= 1.0, (seed, g)


@pytest.mark.parametrize("tag,B", C.UPDATE_CASES)
def test_weight_decay_momentum_and_learning_rate_identities(tag, B):
    """part 2, every tensor:  p1(wd = 1/2) - p1(0) = -L p0 / 2;  step 1 bit-equal at momentum 0 and 1/2 (begin() cleared the buffers of
    the run before), then p2(mu) - p2(0) = mu (p1 - p0);  after set_lr(2 lr) the replayed one-step graph changes every tensor by twice
    what it does otherwise.  Each to IDENTITY_SLACK = 2 times the bound its roundings give (check_train_step.identity_check derives
    them); a site that skips the decay, applies it to the buffer, stores gg for mm or keeps the old lr is 1e3 .. 1e5 bounds off."""
    i = C.identity_check(tag, B, 0)
    print(f"{tag} {B}: observed / (slack x bound): weight decay {i['wd']:.3f}, momentum {i['mom']:.3f}, learning rate {i['lr']:.3f}")
    assert i["exact"] and i["moved"], i
    assert i["wd"] <= 1.0 and i["mom"] <= 1.0 and i["lr"] <= 1.0, i


@pytest.mark.parametrize("tag,B,dropout", [("othello8", 272, 0.0), ("othello8", 272, 0.3), ("othello8", 512, 0.0), ("othello8", 512, 0.3), ("connect4", 512, 0.0),
                                           ("connect4", 512, 0.3), ("othello6", 400, 0.0), ("othello6", 400, 0.3), ("othello8", 64, 0.3), ("othello6", 48, 0.0),
                                           ("connect4", 32, 0.3), ("connect4_5x8", 64, 0.0), ("tictactoe", 64, 0.0)])
def test_three_steps_equal_float64_by_per_step_change(tag, B, dropout):
    """part 3: lr 0.1, momentum 0.9, weight decay 1e-4 (the reference's), the Philox mask read back into the float64 model.  Every
    step's change of every tensor, p_s - p_(s-1), within 2e-4 of the float64 run's largest change of that tensor (+ lr x floor): the
    second step compares momentum on the row-split path, the third a buffer that was read correctly but stored wrongly."""
    seed = STEPS_SEED.get((tag, B, dropout), 0)
    rows = C.report(tag, B, 3, dropout, verbose=False, seed=seed, lr=0.1, mom=0.9, wd=1e-4)
    ratios = C.update_rows(rows, 0.1, tag, B, C.report.pmax)
    assert len(ratios) == 3 * len(C.report.pmax) and {"step0.delta.fc1.weight", "step2.delta.fc2.bias", "step1.delta.fc_value.bias"} <= {n for n, _ in ratios}
    worst = max(ratios, key=lambda r: r[1])
    print(f"{tag} {B} dropout {dropout} seed {seed}: worst change error / allowance {worst[1]:.3g} ({worst[0]}); ties {C.report.ties[:4]}")
    if _excused((tag, B, 3, dropout, seed), C.report.ties):
        return
    bad = [(n, e, s) for n, e, s in rows if ".delta." not in n and e > 2e-4 * max(s, 1e-3) + 1e-6]
    assert worst[1] <= 1.0 and not bad, ([r for r in ratios if r[1] > 1.0][:8], bad[:4], C.report.ties[:4])


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())


def test_one_call_of_many_steps_equals_many_calls_of_one_step():
    """part 4: 11 steps = 1 plain + 8 in the eight-step graph + 2 replays of the one-step graph, against 11 calls (each a plain launch or
    a one-step graph): losses, parameters, BatchNorm statistics and counters bit for bit"""
    for tag, B, p in C.MANY_STEPS_CASES:
        one, many = C.many_steps(tag, B, 11, p, True), C.many_steps(tag, B, 11, p, False)
        assert np.isfinite(one["loss_pi"]).all() and np.isfinite(one["loss_v"]).all() and (one["loss_pi"] > 0).all() and int(one["bn1.num_batches_tracked"]) == 11
        _same(one, many, (tag, B))


def _child(env, spec, timeout=300):
    e = {k: v for k, v in os.environ.items() if not k.startswith("AZ_TRAIN_")}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_train_step.py"), "--update-child", json.dumps(spec)], env=e, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, (env, p.returncode, p.stdout[-3000:], p.stderr[-2000:])  # the children after it are not started
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_every_switch_of_the_training_step(tmp_path):
    """part 5.  The AZ_TRAIN_* variables are read once per process: five children, one after another, each with the switches that do not
    interact at the batch sizes where they change the launch sequence.  Parts 1 (seed 0) and 2 run in the child against float64 and the
    identities' bounds -- not against the default path -- and the parent asserts on the child's JSON line with the same allowances.  The
    three-step-graph child and the no-graph child also run part 4's 11 steps in one call; the parent compares the bits with its own."""
    o8 = lambda *bs: [["othello8", b, GRAD_SEEDS.get(("othello8", b), (0,))[0]] for b in bs]  # noqa: E731
    children = [({"AZ_TRAIN_RB": "0", "AZ_TRAIN_SPLIT": "2"}, o8(16, 64, 256, 512), False),  # the unsplit templates <16,4,1> / <32,4,0>; two workgroups per board
                ({"AZ_TRAIN_RB": "64", "AZ_TRAIN_SPLIT": "4"}, o8(16, 64, 512), False),      # eight row blocks of 64; four workgroups per board
                # row blocks of 128 where the default takes 64; part 4's sizes (64, 512 -> blocks of 128 by default, TicTacToe) do not see RB
                ({"AZ_TRAIN_RB": "128", "AZ_TRAIN_GRAPH_STEPS": "3"}, o8(256), True),
                ({"AZ_TRAIN_FOLD1": "0", "AZ_TRAIN_WG_LATE": "0", "AZ_TRAIN_FC2_RB64": "0"}, o8(64, 320, 512), False),
                ({"AZ_TRAIN_GRAPH": "0"}, [], True)]
    default = None
    for n, (env, cases, graphs) in enumerate(children):
        npz = str(tmp_path / f"steps{n}.npz")
        out = _child(env, {"cases": cases, "npz": npz if graphs else None})
        assert sorted(out["cases"]) == sorted(f"{t}/{b}/{sd}" for t, b, sd in cases)
        for name, r in out["cases"].items():
            g, i = r["grad"], r["identity"]
            print(env, name, f"gradient error / allowance {g['ratio']:.3g}; identities {i['wd']:.3f} {i['mom']:.3f} {i['lr']:.3f}")
            assert i["exact"] and i["moved"] and i["wd"] <= 1.0 and i["mom"] <= 1.0 and i["lr"] <= 1.0, (env, name, i)
            if _excused((name.split("/")[0], int(name.split("/")[1]), 1, 0.0, int(name.split("/")[2])), g["ties"]):
                continue
            assert not g["bad"] and not g["workspace_bad"] and g["ratio"] <= 1.0, (env, name, g)
        if graphs:
            if default is None:
                default = {f"{tag}/{B}/{k}": v for tag, B, p in C.MANY_STEPS_CASES for k, v in C.many_steps(tag, B, 11, p, True).items()}
            with np.load(npz) as f:
                _same(default, {k: f[k] for k in f.files}, env)
