#!/usr/bin/env python3
"""The hand-written training step (csrc/az_train.hip) against torch autograd in float64 on the CPU: every activation, every
gradient the step keeps in its workspace, the losses, and the parameters / BatchNorm statistics after k steps.
    python tools/check_train_step.py [tag] [batch] [steps] [dropout]      tag: othello8 | othello6 | connect4 | connect4_<W>x<H> | tictactoe
Prints one line per buffer (max abs error, scale); tests/test_gpu_train_step.py asserts on the same report.
    python tools/check_train_step.py --update-profile
The parameter update at its own scale (gradients from one step at momentum 0 / weight decay 0, the hyper-parameters as identities of
the step with itself): the helpers of tests/test_gpu_train_update.py, and the figures of profiles/r07_update_parity.txt.
The step as a function of nothing but its inputs (StateProblem, state_run, poison_workspace, copy_state, Banded): the helpers of
tests/test_gpu_train_state.py."""
import copy
import os
import re
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_net(tag, seed=0):
    from alphazero_amd.games.connect4 import Connect4Net
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(seed)
    from alphazero_amd.games.tictactoe import TicTacToeNet
    plane = re.fullmatch(r"connect4_(\d+)x(\d+)", tag)  # connect4_<W>x<H>: Connect4Net(W, H) on any plane; "connect4" is the standard 7x6
    if plane:
        net = Connect4Net(int(plane.group(1)), int(plane.group(2)))
    else:
        net = {"othello8": lambda: OthelloNet(n=8), "othello6": lambda: OthelloNet(n=6), "connect4": lambda: Connect4Net(7, 6), "tictactoe": lambda: TicTacToeNet()}[tag]()
    with torch.no_grad():  # BatchNorm affine / running statistics away from their defaults, so that a mix-up shows
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3); m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 2.0)
    return net


def make_samples(net, S, seed=1):
    g = torch.Generator().manual_seed(seed)
    gid, H, W = net.hip_shape()
    state = torch.randint(-1, 2, (S, H, W), generator=g, dtype=torch.int8)
    pi = torch.rand(S, net.action_size, generator=g) ** 3
    pi = (pi / pi.sum(1, keepdim=True)).float()
    z = torch.randint(-1, 2, (S,), generator=g, dtype=torch.int8)
    return state, pi, z


def _relu(x, name, flip):
    """F.relu, or with flip = (layer, flat index) and that layer's name: the same with that ONE unit on the other branch"""
    if flip is None or flip[0] != name:
        return F.relu(x)
    m = (x > 0).to(x.dtype)
    m.view(-1)[flip[1]] = 1.0 - m.view(-1)[flip[1]]
    return x * m


def torch_step(net, x, pi, z, bs, masks=None, p=0.0, flip=None):
    """forward + backward of the reference's loss with every intermediate kept (float64 module); flip: see relu_flip_effect"""
    keep = {}
    if not hasattr(net, "conv1"):  # TicTacToeNet: the module's own forward (no workspace to compare: the step is one launch)
        logp, v = net(x)
        loss_pi = -torch.sum(pi * logp) / bs
        loss_v = torch.sum((v - z) ** 2) / bs
        (loss_pi + loss_v).backward()
        return float(loss_pi.detach()), float(loss_v.detach()), keep

    def k(name, t):
        t.retain_grad()
        keep[name] = t
        return t
    h = x.view(-1, 1, *net.plane)
    for i, (conv, bn) in enumerate(((net.conv1, net.bn1), (net.conv2, net.bn2), (net.conv3, net.bn3), (net.conv4, net.bn4))):
        c = k(f"c{i + 1}", conv(h))
        b = k(f"b{i + 1}", bn(c))
        h = _relu(b, f"b{i + 1}", flip)
    h = h.reshape(-1, net.fc1_input_size)
    y1 = k("y1", net.fc1(h))
    a1 = net.fc_bn1(y1)
    keep["a1"] = a1
    h1 = _relu(a1, "a1", flip)
    if masks is not None:
        h1 = h1 * masks[0] / (1.0 - p)
    h1 = k("h1", h1)
    y2 = k("y2", net.fc2(h1))
    a2 = net.fc_bn2(y2)
    keep["a2"] = a2
    h2 = _relu(a2, "a2", flip)
    if masks is not None:
        h2 = h2 * masks[1] / (1.0 - p)
    h2 = k("h2", h2)
    lp = k("lp", net.fc_probs(h2))
    u = k("u", net.fc_value(h2))
    logp, v = F.log_softmax(lp, dim=1), torch.tanh(u)
    loss_pi = -torch.sum(pi * logp) / bs
    loss_v = torch.sum((v - z) ** 2) / bs
    (loss_pi + loss_v).backward()
    return float(loss_pi.detach()), float(loss_v.detach()), keep


def nhwc(t):  # torch [B, C, H, W] -> the step's [B, H*W, C]
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


def relu_ties(keep, rel=2e-6):
    """ReLU inputs of the float64 run that are zero to float32 rounding (|x| < rel * max|x| of their layer): such a unit may take the
    other branch in the float32 step, and the one-unit difference then spreads downstream -- a property of the data, not of the
    kernels.  -> [(layer, count, smallest |x| / max|x|)] of the layers that have any"""
    out = []
    for name in ("b1", "b2", "b3", "b4", "a1", "a2"):
        if name in keep:
            x = keep[name].detach().abs()
            m = float(x.max())
            n = int((x < rel * m).sum())
            if n:
                out.append((name, n, float(x.min()) / m))
    return out


def relu_flip_effect(tag, B, seed=0, rel=2e-6, closest_only=False):
    """What ONE ReLU unit on the other branch does to the gradients of problem(tag, B, 1, seed), in float64 on the CPU: for every unit
    relu_ties() counts (closest_only: the one with the smallest |x| / max|x| of its layer, over all layers), the float64 step again
    with that unit's branch forced the other way -> [(layer, flat index, |x| / max|x|, err / max|g_ref|)], the last figure being
    gradient_check's "rel" of the forced run against the plain one.  A float32 step that resolved that tie the other way shows exactly
    this error and nothing else: it tells a flipped unit (the data's property; the seed is replaced) from a wrong kernel."""
    net, state, pi, z, perm = problem(tag, B, 1, seed)
    m = copy.deepcopy(net).double().train()
    args = (state[perm].double(), pi[perm].double(), z[perm].double().unsqueeze(1), B)

    def grads(flip):
        m.zero_grad()
        _, _, keep = torch_step(m, *args, flip=flip)  # (train mode moves the running statistics; the batch statistics do not read them)
        return {k: p.grad.clone() for k, p in m.named_parameters() if not zero_gradient(k)}, keep
    g0, keep = grads(None)
    units = []
    for name in ("b1", "b2", "b3", "b4", "a1", "a2"):
        x = keep[name].detach().abs().reshape(-1)
        units += [(float(x[i]) / float(x.max()), name, i) for i in (x < rel * float(x.max())).nonzero().flatten().tolist()]
    out = []
    for r, name, i in (sorted(units)[:1] if closest_only else units):
        g1, _ = grads((name, i))
        out.append((name, i, r, max(float((g1[k] - g0[k]).abs().max()) / float(g0[k].abs().max()) for k in g0)))
    return out


def problem(tag, B, steps, seed=0):
    """-> (net, state, pi, z, perm): the network, samples and batch order of report(tag, B, steps, seed=seed)"""
    net = make_net(tag, seed)
    S = B * steps + 7
    state, pi, z = make_samples(net, S, seed=1 + 17 * seed)
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(5 + seed))[: B * steps].contiguous()
    return net, state, pi, z, perm


def report(tag="othello8", B=64, steps=3, dropout=0.0, verbose=True, seed=0, lr=0.05, mom=0.9, wd=1e-4):
    """-> rows (buffer, max abs error, scale); report.ties = relu_ties() of every step (empty: no unit of the run sits on a ReLU kink).
    step<s>.delta.<name> is the change step s made to a tensor of the state dict, p_s - p_(s-1), with the float64 run's largest change
    as its scale: the update at its own scale (update_bad() judges those rows; with mom = wd = 0 a delta is -lr times the gradient)"""
    from alphazero_amd.train_step import HipTrainStep
    report.ties = []
    net, state, pi, z, perm = problem(tag, B, steps, seed)
    ref = copy.deepcopy(net).double().train()
    opt = torch.optim.SGD(ref.parameters(), lr=lr, momentum=mom, weight_decay=wd)
    hip = HipTrainStep(net, max_batch=B)
    hip.load(net.cuda())
    hip.begin(lr, mom, wd, dropout, seed=3)
    d = {"state": state.cuda(), "pi": pi.cuda(), "z": z.cuda(), "perm": perm.cuda()}
    lpi, lv = torch.zeros(steps, device="cuda"), torch.zeros(steps, device="cuda")
    rows = []

    def cmp(name, got, want):
        shape = tuple(want.shape)
        got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
        diff = (got - want).abs()
        err = float(diff.max())
        scale = float(want.abs().max()) + 1e-30
        rows.append((name, err, scale))
        if verbose:
            where = ""
            if err > 1e-4 * scale + 1e-7:  # where the error sits: index of the maximum, how many elements are off, which rows / last-dim columns
                bad = (diff > 1e-4 * scale + 1e-7).reshape(shape)
                idx = np.unravel_index(int(diff.argmax()), shape)
                r = bad.reshape(shape[0], -1).any(1).nonzero().flatten().tolist()
                c = bad.reshape(-1, shape[-1]).any(0).nonzero().flatten().tolist()
                where = f"  at {idx}, {int(bad.sum())}/{bad.numel()} off; rows {r[:6]}..{r[-3:]} ({len(r)}); cols {c[:6]}..{c[-3:]} ({len(c)})"
            print(f"{name:28s} max|err| {err:10.3e}   max|ref| {scale:10.3e}   rel {err / scale:9.2e}{where}")

    gid, H, W = net.hip_shape()
    A = net.action_size
    NHP = (A + 1 + 15) // 16 * 16
    floats = [kname for kname, v in net.state_dict().items() if v.dtype == torch.float32]
    before = {kname: net.state_dict()[kname].detach().double().cpu().clone() for kname in floats}
    report.pmax = {kname: float(before[kname].abs().max()) for kname in floats}  # largest magnitude a tensor had at any step: the rounding of a stored value
    rbefore = {kname: ref.state_dict()[kname].detach().clone() for kname in floats}
    for s in range(steps):
        rws = perm[s * B:(s + 1) * B]
        # one step at a time so that the workspace of step s can be inspected: a separate perm / loss slice per call
        pcall = d["perm"][s * B:(s + 1) * B].contiguous()
        hip.steps(d["state"], d["pi"], d["z"], pcall, 1, B, lpi[s:s + 1], lv[s:s + 1])
        torch.cuda.synchronize()
        x = state[rws].double()
        masks = None
        if dropout > 0:
            F1, F2 = net.fc1.out_features, net.fc2.out_features
            masks = ((hip.debug("h1", (hip.max_batch, F1))[:B] != 0).double().cpu(), (hip.debug("h2", (hip.max_batch, F2))[:B] != 0).double().cpu())
        opt.zero_grad()
        t_pi, t_v, keep = torch_step(ref, x, pi[rws].double(), z[rws].double().unsqueeze(1), B, masks, dropout)
        report.ties += [(s,) + t for t in relu_ties(keep)]
        if s in (0, steps - 1) and hasattr(net, "conv1"):
            pre = f"step{s}."
            for i in range(4):
                c = keep[f"c{i + 1}"]
                cmp(pre + f"c{i + 1}", hip.debug(f"c{i + 1}")[: c.numel()].view(B, -1, 32), nhwc(c))
                cmp(pre + f"dy{i + 1}", hip.debug(f"dy{i + 1}")[: c.numel()].view(B, -1, 32), nhwc(keep[f"b{i + 1}"].grad))
            F1, F2 = keep["y1"].shape[1], keep["y2"].shape[1]
            cmp(pre + "y1", hip.debug("y1")[: B * F1].view(B, F1), keep["y1"]); cmp(pre + "h1", hip.debug("h1")[: B * F1].view(B, F1), keep["h1"])
            cmp(pre + "y2", hip.debug("y2")[: B * F2].view(B, F2), keep["y2"]); cmp(pre + "h2", hip.debug("h2")[: B * F2].view(B, F2), keep["h2"])
            dl = hip.debug("dlog")[: B * NHP].view(B, NHP)
            cmp(pre + "dlog.policy", dl[:, :A], keep["lp"].grad); cmp(pre + "dlog.value", dl[:, A:A + 1], keep["u"].grad)
            if NHP > A + 1:
                cmp(pre + "dlog.padding", dl[:, A + 1:], torch.zeros(B, NHP - A - 1))
            cmp(pre + "dz2", hip.debug("dz2")[: B * F2].view(B, F2), keep["y2"].grad); cmp(pre + "dz1", hip.debug("dz1")[: B * F1].view(B, F1), keep["y1"].grad)
        cmp(f"step{s}.loss_pi", lpi[s:s + 1], torch.tensor([t_pi])); cmp(f"step{s}.loss_v", lv[s:s + 1], torch.tensor([t_v]))
        opt.step()
        out = copy.deepcopy(net)  # a fresh copy every time: store() adds the steps done so far to num_batches_tracked
        hip.store(out)
        rsd = ref.state_dict()
        for kname in floats:
            now, rnow = out.state_dict()[kname].detach().double().cpu(), rsd[kname].detach().clone()
            cmp(f"step{s}.delta.{kname}", now - before[kname], rnow - rbefore[kname])
            report.pmax[kname] = max(report.pmax[kname], float(now.abs().max()))
            before[kname], rbefore[kname] = now, rnow
    for kname, v in out.state_dict().items():
        if v.dtype == torch.float32:
            cmp("final." + kname, v, rsd[kname])
        else:
            rows.append(("final." + kname, float(abs(int(v) - int(rsd[kname]))), 1.0))
    hip.close()
    return rows


# ---------------------------------------------------------------------------------------------------------------- the update at its own scale
# (tests/test_gpu_train_update.py).  No weight gradient of the step is readable: the update happens in the epilogue of the gradient tiles
# (fc1 / fc2), in sgd() from several kernels, and in k_ttt_step.  What IS readable is the parameter before and after a step, and
# begin()'s hyper-parameters are free: momentum 0, weight decay 0 and a power-of-two learning rate L turn one step into
# p1 = p0 - L g, so (p0 - p1) / L is the gradient; the other hyper-parameters are checked as identities of the step with itself.
UPDATE_CASES = ([("othello8", b) for b in (16, 64, 128, 144, 320, 512)] + [("othello6", b) for b in (48, 80, 400)] + [("connect4", b) for b in (32, 144, 512)]
                + [("connect4_5x8", 64)] + [("tictactoe", b) for b in (2, 64, 250)])
# Every Connect4 plane the trainer accepts (width and height 5..8: CH = W, CW = H, P4 = (W - 4)(H - 4), FIN = 32 P4, A = W outputs), for
# tests/test_gpu_train_planes.py: (tag, batch, seeds) of gradient_check; seeds 0-2 or 0, except where the float32 step resolves a ReLU tie of
# the float64 run the other way (the rule: PLANE_FLIPS below; the replaced seed is named beside its replacement).  UPDATE_CASES above holds 7x6 and 5x8; these rows hold the
# other fourteen.  Dense dispatches of plan_train_step: <= 64 rows <4,16,1,0> | 65..128 <8,8,1,0> | 144..368 row-split, 64-row blocks |
# >= 384 row-split, 128-row blocks (fc2 on 64-row blocks, the late fc1 weight gradient in k_conv1_bwd); 144 and 400 end in a 16-row block.
PLANE_CASES = [
    # the extreme planes at every dense dispatch, seeds 0-2
    ("connect4_5x5", 16, (0, 1, 2)),    # FIN 32, P4 1 (conv4 output 1x1, conv3 3x3): 2 K steps, 2 of 16 waves work one step each; <4,16,1,0> with one row tile
    ("connect4_5x5", 128, (0, 1, 2)),   # FIN 32, P4 1: 2 of 8 waves work; <8,8,1,0>; 2 live fc1 weight-gradient tiles in a 4-wave block
    ("connect4_5x5", 144, (0, 1, 2)),   # FIN 32, P4 1: row-split, 64-row blocks, last block 16 rows
    ("connect4_5x5", 400, (0, 1, 2)),   # FIN 32, P4 1: row-split, 128-row blocks, last block 16 rows; late fc1 weight gradient: 2 tiles
    ("connect4_7x7", 16, (0, 1, 2)),    # FIN 288, P4 9 (3x3): 18 K steps over 16 waves, 9 waves of 2 steps work; <4,16,1,0>; bn4 sums 9 = 8 + 1 positions
    ("connect4_7x7", 128, (0, 1, 2)),   # FIN 288, P4 9: 18 K steps over 8 waves, 6 waves of 3 steps work (an odd count in the two-deep prefetch loop); <8,8,1,0>
    ("connect4_7x7", 144, (0, 1, 2)),   # FIN 288, P4 9: row-split, 64-row blocks, last block 16 rows; 18 fc1 weight-gradient tiles, no multiple of 4
    ("connect4_7x7", 400, (0, 1, 2)),   # FIN 288, P4 9: row-split, 128-row blocks, last block 16 rows; late fc1 weight gradient: 18 tiles
    ("connect4_8x8", 16, (0, 1, 2)),    # FIN 512, P4 16, P1 64 with F1 64 / F2 32 (Othello8's plane, Connect4's dense widths); <4,16,1,0>
    ("connect4_8x8", 128, (3, 1, 2)),   # (seed 0 flips b4[9907]) FIN 512, P4 16, P1 64; <8,8,1,0>
    ("connect4_8x8", 144, (0, 1, 2)),   # FIN 512, P4 16, P1 64; row-split, 64-row blocks, last block 16 rows
    ("connect4_8x8", 400, (0, 1, 3)),   # (seed 2 flips b4[84663]) FIN 512, P4 16, P1 64; row-split, 128-row blocks, last block 16 rows
    # every other plane never held to float64 at the update's scale, once, with the dispatch rotated
    ("connect4_5x6", 32, (0,)),         # FIN 64, P4 2 (1x2); <4,16,1,0>: 4 K steps for 16 waves
    ("connect4_6x5", 128, (0,)),        # FIN 64, P4 2 (2x1), 6 outputs; <8,8,1,0>
    ("connect4_5x7", 144, (0,)),        # FIN 96, P4 3 (1x3): 6 K steps, 6 fc1 weight-gradient tiles; row-split 64, last block 16 rows
    ("connect4_7x5", 400, (0,)),        # FIN 96, P4 3 (3x1); row-split 128, last block 16 rows; late fc1 weight gradient: 6 tiles
    ("connect4_6x6", 64, (0,)),         # FIN 128, P4 4 (2x2), 6 outputs; <4,16,1,0> at its largest batch
    ("connect4_6x7", 48, (0,)),         # FIN 192, P4 6 (2x3: the relayout's H4 / W4 order shows), 6 outputs; <4,16,1,0>, three row tiles
    ("connect4_6x8", 272, (1,)),        # (seed 0 flips b2[227885], in the stock float32 torch step too) FIN 256, P4 8 (2x4), 6 outputs; row-split 64: four full blocks and one of 16 rows
    ("connect4_8x6", 16, (0,)),         # FIN 256, P4 8 (4x2); <4,16,1,0>, one row tile
    ("connect4_7x8", 384, (0,)),        # FIN 384, P4 12 (3x4); row-split 128: three full blocks
    ("connect4_8x7", 96, (0,)),         # FIN 384, P4 12 (4x3); <8,8,1,0>, six row tiles
    ("connect4_8x5", 144, (0,)),        # FIN 128, P4 4 (4x1); row-split 64, last block 16 rows
]
# The (case, seed) pairs PLANE_CASES replaced, with the HIP step's err / max|g_ref| on an MI355X (profiles/r32_train_planes.txt): each is
# relu_flip_effect's figure for the float64 run's closest tie, to the four digits recorded -- one unit on the other branch and nothing else
# (tests/test_train_plane_seeds.py asserts that on the CPU).  A replacement needs a non-empty relu_ties AND the flip's signature (error /
# allowance >= 4 where a clean run is <= 0.03); at most one seed per case; a case that fails on two of its first four seeds is a finding.
PLANE_FLIPS = {("connect4_8x8", 128, 0): ("b4", 0.03017), ("connect4_8x8", 400, 2): ("b4", 0.01265), ("connect4_6x8", 272, 0): ("b2", 0.004108)}
EPS = 2.0 ** -24  # half an ulp of a float32 relative to its magnitude: one rounding
# One step at L = 16: the stored p1 is rounded to EPS |p1|, EPS |p| / L = 6e-9 in gradient units for the largest parameters (BatchNorm
# weights, 1.5) -- under the float32 noise of their gradients (1e-6 of 1e-2) -- and one step at L = 16 is still a finite network.
GRAD_L = 16.0
# Biases that feed a BatchNorm have a true gradient of zero (the batch mean removes them); a float32 step leaves rounding there.
# Measured on the stock float32 torch step on the CPU over UPDATE_CASES x seeds 0-2 (profiles/r07_update_parity.txt), largest value:
# conv nets 4.17e-7, TicTacToeNet at 64 / 250 rows 4.1e-8, TicTacToeNet at 2 rows 1.05e-5 (two rows: 1 / sqrt(var + eps) of a variance
# that may be tiny multiplies the rounding).  The allowance is 8x that: the kernels sum the same terms in another order.
GRAD_FLOOR = {"conv": 8 * 4.17e-7, "tictactoe": 8 * 4.1e-8, "tictactoe2": 8 * 1.05e-5}
IDENTITY_SLACK = 2.0  # over the derived rounding bounds of the identities (emulated fmaf chains reach 0.98 of them)


def grad_floor(tag, B):
    return GRAD_FLOOR["conv" if tag != "tictactoe" else ("tictactoe2" if B == 2 else "tictactoe")]


def zero_gradient(name):
    return name in ("conv1.bias", "conv2.bias", "conv3.bias", "conv4.bias", "fc1.bias", "fc2.bias")


def update_rows(rows, lr, tag, B, pmax):
    """the step<s>.delta.<name> rows of report() against their allowance -> [(row name, error / allowance)].  Allowance: 2e-4 of the
    float64 run's largest change of that tensor (the project's float32-against-float64 figure, at the change's own scale) plus, for the
    zero-gradient biases, lr x grad_floor; for every other tensor only the rounding of the two stored values the change is the
    difference of (2 EPS max|p|, never more than lr x grad_floor)"""
    out = []
    for n, e, s in rows:
        if ".delta." in n:
            k = n.split(".delta.")[1]
            fl = lr * grad_floor(tag, B)
            out.append((n, e / (2e-4 * s + (fl if zero_gradient(k) else min(fl, 2 * EPS * pmax[k])))))
    return out


def gradient_check(tag, B, seed=0, L=GRAD_L):
    """one step at momentum 0, weight decay 0, dropout 0, learning rate L against float64 autograd: every tensor's gradient
    (p0 - p1) / L through update_rows(), and the step's workspace, losses and counters under report()'s own rule (a kernel that reads a
    weight another kernel of the same step has already updated shows there, magnified by L; the final.* rows of the float tensors are
    the delta rows again at the parameter's scale, where L x the zero-gradient floor does not belong)"""
    rows = report(tag, B, 1, 0.0, verbose=False, seed=seed, lr=L, mom=0.0, wd=0.0)
    ratios = update_rows(rows, L, tag, B, report.pmax)
    assert len(ratios) == len(report.pmax)
    g = {n.split(".delta.")[1]: (e / L, s / L) for n, e, s in rows if ".delta." in n and "running_" not in n}
    return {"ratio": max(r for _, r in ratios), "bad": [(n, r) for n, r in ratios if not r <= 1.0][:6],
            "workspace_bad": [(n, e, s) for n, e, s in rows if ".delta." not in n and not (n.startswith("final.") and not n.endswith("num_batches_tracked")) and not e <= 2e-4 * max(s, 1e-3) + 1e-6][:6], "ties": report.ties[:4],
            "rel": max(e / s for k, (e, s) in g.items() if not zero_gradient(k)), "zero": max([e for k, (e, s) in g.items() if zero_gradient(k)] or [0.0])}


def stock_float32_noise(tag, B, seed=0):
    """the same gradient figures ("rel", "zero") for the stock float32 torch step on the CPU against float64: the reference's own error"""
    net, state, pi, z, perm = problem(tag, B, 1, seed)
    g = {}
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(net).to(dt).train()
        torch_step(m, state[perm].to(dt), pi[perm].to(dt), z[perm].to(dt).unsqueeze(1), B)
        g[dt] = {k: p.grad.double() for k, p in m.named_parameters()}
    err = {k: (float((g[torch.float32][k] - v).abs().max()), float(v.abs().max())) for k, v in g[torch.float64].items()}
    return {"rel": max(e / s for k, (e, s) in err.items() if not zero_gradient(k)), "zero": max(e for k, (e, s) in err.items() if zero_gradient(k))}


class UpdateRun:
    """one trainer on problem(tag, B, steps, seed): begin() reloads the initial weights, step(s, n) runs steps s .. s+n-1 in ONE call
    (its permutation / loss pointers are those of step s: the same s gives the same pointers, so a captured graph is replayed),
    snap() reads the state dict back (float64 copies on the CPU; exact, every float32 is a float64)"""

    def __init__(self, tag, B, steps, seed=0):
        from alphazero_amd.train_step import HipTrainStep
        self.net, state, pi, z, perm = problem(tag, B, steps, seed)
        self.B = B
        self.hip = HipTrainStep(self.net, max_batch=B)
        self.net.cuda()
        self.state, self.pi, self.z, self.perm = state.cuda(), pi.cuda(), z.cuda(), perm.cuda()
        self.lp, self.lv = torch.zeros(steps, device="cuda"), torch.zeros(steps, device="cuda")
        self.p0 = {k: v.detach().double().cpu() for k, v in self.net.state_dict().items() if v.dtype == torch.float32}

    def begin(self, lr, mom, wd, dropout=0.0):
        self.hip.load(self.net)
        self.hip.begin(lr, mom, wd, dropout, seed=3)

    def step(self, s, n=1):
        self.hip.steps(self.state, self.pi, self.z, self.perm[s * self.B:], n, self.B, self.lp[s:], self.lv[s:])

    def stored(self):
        out = copy.deepcopy(self.net)  # fresh every time: store() adds the steps done to num_batches_tracked
        self.hip.store(out)
        return out.state_dict()

    def snap(self):
        return {k: v.detach().double().cpu() for k, v in self.stored().items() if v.dtype == torch.float32}

    def close(self):
        self.hip.close()


def identity_check(tag, B, seed=0, L=1.0, w=0.5, mu=0.5):
    """weight decay, momentum and learning rate as identities of the step with itself, on every tensor; no reference and no measured
    tolerance.  The step is bit-reproducible, and the hyper-parameters enter only through
        gg = fmaf(wd, p, g);  mm = fmaf(momentum, m, gg);  m = mm;  p = fmaf(-lr, mm, p)
    (sgd(), the epilogues of fc_wgrad_tile / fc_wgrad_tile_ks, k_ttt_step), each rounding once, by at most EPS of its result.
    -> worst observed / (IDENTITY_SLACK x bound) per identity ("wd", "mom", "lr": must be <= 1), "exact": every bit-equality held"""
    r = UpdateRun(tag, B, 2, seed)
    par = [k for k, _ in r.net.named_parameters()]
    stats = [k for k in r.p0 if k not in par]
    p0, res, exact = r.p0, {}, True

    def worst(diff, bound):
        return float((diff.abs() / (IDENTITY_SLACK * bound).clamp_min(1e-300)).max())
    # weight decay: gg(0) = g exactly and mm = gg at momentum 0, so p1(0) = rnd(p0 - L g), p1(w) = rnd(p0 - L rnd(g + w p0)):
    # p1(w) - p1(0) = -L w p0 within EPS (L |gg| + |p1(0)| + |p1(w)|), L |gg| read off the run as |p1(w) - p0|
    r.begin(L, 0.0, 0.0); r.step(0); a = r.snap()
    r.begin(L, 0.0, w); r.step(0); b = r.snap()
    res["wd"] = max(worst((b[k] - a[k]) + L * w * p0[k], EPS * ((b[k] - p0[k]).abs() + a[k].abs() + b[k].abs())) for k in par)
    exact &= all(torch.equal(a[k], b[k]) for k in stats)
    # momentum: the buffers start at zero (begin() clears what the runs above left), so step 1 is the same bits at any momentum;
    # step 2 then sees the same weights and batch, hence the same g2, and mm2 = rnd(mu gg1 + gg2) against gg2:
    # p2(mu) - p2(0) = -L mu gg1 = mu (p1 - p0) within EPS (L |mm2| + |p2(0)| + |p2(mu)| + |p1|), L |mm2| read off as |p2(mu) - p1|
    r.begin(L, 0.0, 0.0); r.step(0); a1 = r.snap(); r.step(1); a2 = r.snap()
    r.begin(L, mu, 0.0); r.step(0); b1 = r.snap(); r.step(1); b2 = r.snap()
    exact &= all(torch.equal(a1[k], b1[k]) for k in a1) and all(torch.equal(a2[k], b2[k]) for k in stats)
    res["mom"] = max(worst((b2[k] - a2[k]) - mu * (a1[k] - p0[k]), EPS * ((b2[k] - a1[k]).abs() + a2[k].abs() + b2[k].abs() + a1[k].abs())) for k in par)
    # learning rate: two steps in one call (a plain step, then the captured one-step graph), then a third call on the same pointers,
    # which replays that graph -- once as it is, once after set_lr(2 lr).  mm3 does not depend on lr, so the third step's change
    # doubles: (p3' - p2) = 2 (p3 - p2) within the rounding of the two stored values, EPS (|p3'| + 2 |p3|)
    lr = L / 8
    r.begin(lr, mu, 1e-4); r.step(0, 2); c2 = r.snap(); r.step(0); c3 = r.snap()
    r.begin(lr, mu, 1e-4); r.step(0, 2); d2 = r.snap(); r.hip.set_lr(2 * lr); r.step(0); d3 = r.snap()
    exact &= all(torch.equal(c2[k], d2[k]) for k in c2) and all(torch.equal(c3[k], d3[k]) for k in stats)
    res["lr"] = max(worst((d3[k] - c2[k]) - 2 * (c3[k] - c2[k]), EPS * (d3[k].abs() + 2 * c3[k].abs())) for k in par)
    res["moved"] = min(float((c3[k] - c2[k]).abs().max()) for k in par) > 0.0  # every tensor took part
    res["exact"] = bool(exact)
    r.close()
    return res


def many_steps(tag, B, n=11, dropout=0.3, one_call=True, seed=0):
    """n steps at the reference's hyper-parameters in one steps() call (a plain step, graphs of AZ_TRAIN_GRAPH_STEPS steps, one-step
    replays) or as n calls of one step -> {name: numpy array} of the losses and the whole state dict"""
    r = UpdateRun(tag, B, n, seed)
    r.begin(0.1, 0.9, 1e-4, dropout)
    if one_call:
        r.step(0, n)
    else:
        for s in range(n):
            r.step(s)
    out = {k: v.detach().cpu().numpy() for k, v in r.stored().items()}
    out["loss_pi"], out["loss_v"] = r.lp.cpu().numpy(), r.lv.cpu().numpy()
    r.close()
    return out


MANY_STEPS_CASES = [("othello8", 64, 0.3), ("othello8", 512, 0.3), ("tictactoe", 64, 0.0)]  # (TicTacToeNet has no dropout)


def update_child(spec):
    """a child process of tests/test_gpu_train_update.py (the AZ_TRAIN_* switches are read once per process): gradient_check and
    identity_check on spec["cases"] ([tag, batch, seed]), many_steps on MANY_STEPS_CASES into spec["npz"] if given -> one JSON-able dict"""
    out = {"cases": {}}
    for tag, B, seed in spec.get("cases", []):
        out["cases"][f"{tag}/{B}/{seed}"] = {"grad": gradient_check(tag, B, seed), "identity": identity_check(tag, B, seed)}
    if spec.get("npz"):
        res = {}
        for tag, B, p in MANY_STEPS_CASES:
            res.update({f"{tag}/{B}/{k}": v for k, v in many_steps(tag, B, 11, p, True).items()})
        np.savez(spec["npz"], **res)
    return out


def update_profile():
    """the figures of profiles/r07_update_parity.txt, one line per (case, seed)"""
    print(f"L = {GRAD_L}; floors {GRAD_FLOOR}; identity slack {IDENTITY_SLACK}")
    print("case seed | HIP step: worst err / max|g_ref| over real-gradient tensors, largest zero-gradient bias | stock float32 torch (CPU): the same two | allowance used | ReLU ties")
    for tag, B in UPDATE_CASES:
        for seed in (0, 1, 2):
            g, f = gradient_check(tag, B, seed), stock_float32_noise(tag, B, seed)
            print(f"{tag:13s}{B:4d} {seed} | {g['rel']:9.2e} {g['zero']:9.2e} | {f['rel']:9.2e} {f['zero']:9.2e} | {g['ratio']:8.2e} | {g['ties']}", flush=True)
    print("case | identities, worst observed / derived bound: weight decay, momentum, learning rate | bit-equalities")
    for tag, B in UPDATE_CASES:
        i = identity_check(tag, B, 0)
        print(f"{tag:13s}{B:4d} | {i['wd'] * IDENTITY_SLACK:6.3f} {i['mom'] * IDENTITY_SLACK:6.3f} {i['lr'] * IDENTITY_SLACK:6.3f} | {i['exact']}", flush=True)


# ---------------------------------------------------------------------------------------------------------------- the step as a function of its inputs
# (tests/test_gpu_train_state.py).  Every comparison below is bit equality: the step has no float atomics and fixed combination orders,
# so parameters, momenta, running statistics, Hyper and the batch decide every bit of a step -- whatever the workspace held before,
# whatever ran earlier in the process, wherever the caller's arrays lie.  No tolerance, no float64 model, hence no ReLU ties.
STATE_CASES = [("connect4", 32), ("connect4", 144), ("connect4", 512), ("connect4_5x8", 64), ("othello6", 48), ("othello6", 80), ("othello8", 144),
               ("tictactoe", 2), ("tictactoe", 64),  # the smallest batch that reaches each dispatch of enqueue_step
               ("connect4_5x5", 16), ("connect4_7x7", 144)]  # fc1's K = 32: most waves have an empty range; K = 288: the last working wave a short one
STATE_HYPER = (0.1, 0.9, 1e-4)  # lr, momentum, weight decay: the reference's


def state_dropout(tag):
    return 0.0 if tag == "tictactoe" else 0.3  # (TicTacToeNet has no dropout)


class StateProblem:
    """problem(tag, B, steps) on the GPU with a batch order that includes row 0 and the LAST row of the sample arrays (a read before or
    past a row shows at the arrays' ends); `net` is the CUDA module every run loads"""

    def __init__(self, tag, B, steps=2, seed=0):
        self.tag, self.B, self.n = tag, B, steps
        net, state, pi, z, _ = problem(tag, B, steps, seed)
        S = state.shape[0]
        perm = torch.randperm(S, generator=torch.Generator().manual_seed(5 + seed))[: B * steps].clone()
        for row, slot in ((0, 1), (S - 1, B * steps - 2)):  # into a slot that does not hold the other one
            if not (perm == row).any():
                perm[slot if perm[slot] not in (0, S - 1) else slot + 1] = row
        assert len(set(perm.tolist())) == B * steps and 0 in perm and S - 1 in perm
        self.net = net.cuda()
        self.arrays = {"state": state.cuda(), "pi": pi.cuda(), "z": z.cuda(), "perm": perm.cuda(),
                       "loss_pi": torch.zeros(steps, device="cuda"), "loss_v": torch.zeros(steps, device="cuda")}

    def trainer(self, max_batch=None):
        from alphazero_amd.train_step import HipTrainStep
        return HipTrainStep(self.net, max_batch=max_batch or self.B)


TWO_CALLS = ((0, 1), (1, 1))  # step 0 as a plain launch, step 1 from other pointers as a freshly captured graph


def state_begin(hip, prob, load=None, begin=True):
    """load: the module to load (None: prob.net; False: keep the trainer's parameters); begin: a fresh optimizer at STATE_HYPER, the
    case's dropout and Philox seed 3 -> the (still empty) result of the run"""
    if load is not False:
        hip.load(prob.net if load is None else load)
    if begin:
        hip.begin(*STATE_HYPER, state_dropout(prob.tag), seed=3)
    return {}


def state_call(hip, prob, res, k, call, B=None, arrays=None):
    """call k = (s, n) of a run: n steps in one az_trainer_steps from the pointers of step s (perm[s * B:], loss[s:]); the losses it wrote
    go into res"""
    (s, n), B, a = call, B or prob.B, arrays or prob.arrays
    hip.steps(a["state"], a["pi"], a["z"], a["perm"][s * B:], n, B, a["loss_pi"][s:], a["loss_v"][s:])
    hip.check()
    torch.cuda.synchronize()
    res[f"call{k}.loss_pi"], res[f"call{k}.loss_v"] = a["loss_pi"][s:s + n].cpu().numpy(), a["loss_v"][s:s + n].cpu().numpy()


def state_end(hip, prob, res, out=None, workspace=False):
    """reads the trainer back into res: every tensor of the state dict store() writes (into `out`; None: a copy of prob.net), and with
    `workspace` every workspace buffer's bytes"""
    out = copy.deepcopy(prob.net) if out is None else out
    hip.store(out)
    res.update({"sd." + k: v.detach().cpu().numpy() for k, v in out.state_dict().items()})
    if workspace:
        res.update({"ws." + k: v.cpu().numpy() for k, v in hip.views("workspace")})
    return res


def state_run(hip, prob, calls=TWO_CALLS, B=None, arrays=None, load=None, begin=True, out=None, before_call=None, workspace=False):
    """state_begin, every call of `calls` (before_call(k) runs before call k; k = 0: after begin()), state_end -> {name: numpy array}"""
    res = state_begin(hip, prob, load, begin)
    for k, call in enumerate(calls):
        if before_call is not None:
            before_call(k)
        state_call(hip, prob, res, k, call, B, arrays)
    return state_end(hip, prob, res, out, workspace)


def same_bits(a, b, what):
    """asserts two results of state_run() equal bit for bit (as bytes: a NaN equals itself, -0.0 differs from 0.0)"""
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        if a[k].tobytes() != b[k].tobytes():
            x, y = np.ascontiguousarray(a[k]).reshape(-1), np.ascontiguousarray(b[k]).reshape(-1)
            off = np.flatnonzero(x.view(np.uint8) != y.view(np.uint8)) // x.itemsize
            raise AssertionError((what, k, f"{len(set(off.tolist()))} of {x.size} elements differ, first at {int(off[0])}: {x[off[0]]!r} != {y[off[0]]!r}"))


def all_finite(res):
    return all(np.isfinite(v).all() for k, v in res.items() if not k.startswith("ws.") and v.dtype.kind == "f")


def poison_workspace(hip, kind):
    """every byte of every workspace-class buffer: 0xFF (a NaN as float and as double: a multiplication by zero does not hide it) or
    the float 1e30 repeated (finite, but nothing of the step's scale survives it)"""
    n = 0
    for _, v in hip.views("workspace"):
        if kind == "nan":
            v.fill_(0xFF)
        else:
            v.view(torch.float32).fill_(1e30)
        n += 1
    torch.cuda.synchronize()
    return n


def copy_state(src, dst):
    """everything a step depends on besides its batch -- parameters, momenta, running statistics, Hyper (learning rate, step counter of
    the dropout stream) -- from one trainer into another of the same network (their sizes do not depend on max_batch)"""
    theirs = {name: (cls, p, n) for name, cls, p, n in dst.buffers()}
    mine = [(name, cls, n) for name, cls, p, n in src.buffers() if cls != "workspace"]
    assert sorted((name, cls, n) for name, (cls, p, n) in theirs.items() if cls != "workspace") == sorted(mine)
    for cls in ("parameter", "momentum", "running_stat", "hyper"):
        for (name, s), (name2, d) in zip(src.views(cls), dst.views(cls)):
            assert name == name2
            d.copy_(s)
    dst.steps_done = src.steps_done
    torch.cuda.synchronize()


class Banded:
    """Tensors carved as contiguous views out of larger buffers: on either side of a view lie at least `rows` rows of its array, every
    byte of them `fill`; with `odd` the view starts at an odd element offset (the ABI promises no alignment beyond the element's own).
    A stray read finds the band's bytes instead of whatever the allocator put there, a stray write is found by check()."""

    def __init__(self, rows, fill, odd):
        self.rows, self.fill, self.odd, self.items = rows, fill, odd, []

    def empty(self, shape, dtype):
        shape = tuple(shape)
        n = int(np.prod(shape))
        row = max(1, n // shape[0]) if shape and shape[0] else 1
        band = (self.rows * row + 63) // 64 * 64
        start = band + (1 if self.odd else 0)
        buf = torch.empty(start + n + band, dtype=dtype, device="cuda")
        buf.view(torch.uint8).fill_(self.fill)
        self.items.append((buf, start, n))
        return buf[start:start + n].view(shape)

    def carve(self, t):
        v = self.empty(t.shape, t.dtype)
        v.copy_(t)
        return v

    def module(self, net):
        """a copy of `net` whose float tensors -- what load() reads from and store() writes into -- are such views"""
        m = copy.deepcopy(net)
        for t in list(m.parameters()) + [b for b in m.buffers() if b.dtype == torch.float32]:
            t.data = self.carve(t.data)
        assert all(v.is_cuda and v.is_contiguous() for v in m.state_dict().values())
        return m

    def check(self):
        """every band byte is what was written into it -> the number of band bytes checked"""
        torch.cuda.synchronize()
        total = 0
        for buf, start, n in self.items:
            b, e = buf.view(torch.uint8), buf.element_size()
            lo, hi = b[: start * e], b[(start + n) * e:]
            assert lo.numel() >= self.rows and hi.numel() >= self.rows
            assert bool((lo == self.fill).all()) and bool((hi == self.fill).all()), ("a guard band was written", tuple(buf.shape), start, n)
            total += lo.numel() + hi.numel()
        return total

if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--update-child":
        import json
        print(json.dumps(update_child(json.loads(a[1]))))
        sys.exit(0)
    if a and a[0] == "--update-profile":
        update_profile()
        sys.exit(0)
    rows = report(a[0] if a else "othello8", int(a[1]) if len(a) > 1 else 64, int(a[2]) if len(a) > 2 else 3, float(a[3]) if len(a) > 3 else 0.0)
    bad = [(n, e, s) for n, e, s in rows if e > 2e-4 * max(s, 1e-3) + 1e-6]
    print("WORST", sorted(rows, key=lambda r: -r[1] / max(r[2], 1e-3))[:5])
    print("BAD", bad[:20], len(bad))
    print("RELU TIES (step, layer, units, smallest |x| / max|x|)", report.ties)
