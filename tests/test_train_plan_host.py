"""CPU: the launch sequence the training step plans for a batch size (alphazero_amd/csrc/az_train_plan.h: plan_train_step, TrainTuning),
pinned without a GPU.  tests/train_plan_table.cpp is compiled with the host C++ compiler and run as a child process; an AZ_TRAIN_*
switch goes through the child's environment, so every case reads its switches afresh (the library reads them once per process).  What is
pinned: the number of launches (14 / 15 / 19 / 1), every launch's kernel with its template configuration, grid, threads, LDS request,
integer argument and the row block its TDims carries."""
import collections
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

OTH8, OTH6, C4, TTT = (0, 8, 8), (0, 6, 6), (1, 6, 7), (2, 3, 3)  # game id, H, W
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
NRBMAX, MAX_LAUNCHES, TPB = 8, 19, 256
CONV_FWD_LDS = (288 * 36 + 100 * 36 + 64 * 36 + 64 * 36 + 4 * 32 + 64) * 4 + 8 * 32 * 3 * 8
CONV_BWD_LDS = (288 * 36 + 100 * 36 + 100 * 36 + 64 * 36 + 64 * 36 + 10 * 32 + 192 + 64 * 36 + 128 + 64) * 4 + 2048 * 8
CONV1_WG_LDS = 4 * 1024 * 4 + 4 * 32 * 4 + 768 * 8

Plan = collections.namedtuple("Plan", "S NB RB NRB F1B n launches")
Launch = collections.namedtuple("Launch", "kernel gx gy threads lds arg RB NRB")


def fc_lds(NW, rows):
    return (NW * rows * 16 + 4 * 32) * 4 + 768 * 8


def ttt_lds(B):
    return (320 + 8 * B * 12 + 320 + 64) * 4 + (512 + 16 * 5) * 8


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("train_plan") / "train_plan_table")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "train_plan_table.cpp"), "-o", out])
    return out


def plans(exe, net, rows, **switches):
    """((graphs_ok, graph_steps), {B: Plan}) of one child process; no AZ_* variable but `switches` reaches it.  Every plan is checked
    against the bounds that hold for all of them."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AZ_")}
    env.update({k: str(v) for k, v in switches.items()})
    out = subprocess.run([exe, *map(str, net), *map(str, rows)], env=env, capture_output=True, text=True, check=True).stdout
    tuning, got = None, {}
    for line in out.splitlines():
        f = line.split("\t")
        if f[0] == "tuning":
            tuning = (int(f[1]), int(f[2]))
        elif f[0] == "plan":
            got[int(f[1])] = Plan(*map(int, f[2:]), [])
        else:
            assert int(f[1]) == len(got[int(f[0])].launches)  # the index counts up
            got[int(f[0])].launches.append(Launch(f[2], *map(int, f[3:])))
    assert sorted(got) == sorted(rows)
    for B, p in got.items():
        assert 1 <= p.n == len(p.launches) <= MAX_LAUNCHES, (B, p.n)
        assert 1 <= p.NRB <= NRBMAX and all(1 <= l.NRB <= NRBMAX for l in p.launches), B
        assert all(l.gx >= 1 and l.gy >= 1 and l.threads >= 64 and l.lds >= 0 for l in p.launches), B
    return tuning, got


def plan(exe, net, B, **switches):
    return plans(exe, net, (B,), **switches)[1][B]


def names(p):
    return [l.kernel for l in p.launches]


def only(p, kernel):
    (l,) = [l for l in p.launches if l.kernel == kernel]
    return l


def unsplit_names(cfg, nt=5, conv1_bwd=False):
    return (["k_conv1_fwd"] + ["k_conv_fwd"] * 3 + [f"k_fc_fwd<{cfg},false>"] * 2 + [f"k_heads_fwd<{nt},8>", f"k_heads_bwd<{cfg.split(',')[0]},{nt},false>",
            f"k_fc_dgrad<{cfg},false>", f"k_mix1<{cfg},false>", "k_mix2", "k_conv_bwd", "k_conv_bwd"] + ["k_conv1_bwd"] * conv1_bwd + ["k_update"])


def split_names(cfg, fc2=None, nt=5, wg_late=True):
    rtm = cfg.split(",")[0]
    return (["k_conv1_fwd"] + ["k_conv_fwd"] * 3 + [f"k_fc_fwd<{cfg},true>", "k_fc_fin", f"k_fc_fwd<{fc2 or cfg},true>", "k_fc_fin", f"k_heads_fwd<{nt},8>",
            f"k_heads_bwd<{rtm},{nt},true>", "k_bn1d_bwd_fin", f"k_fc_dgrad<{cfg},true>", "k_bn1d_bwd_fin", f"k_mix1<{cfg},true>",
            "k_conv_bwd" if wg_late else "k_mix2", "k_conv_bwd", "k_conv_bwd", "k_conv1_bwd", "k_update"])


# ---- OthelloNet 8x8 (F1 1024, F2 512, FIN 512, NHP 80, NT 5), defaults

def test_othello8_up_to_128_rows_is_fourteen_launches(exe):
    _, got = plans(exe, OTH8, (16, 64, 80, 128))
    for B, cfg, NW in ((16, "4,16,1", 16), (64, "4,16,1", 16), (80, "8,8,1", 8), (128, "8,8,1", 8)):
        p = got[B]
        assert (p.S, p.NB, p.RB, p.NRB, p.F1B, p.n) == (1, B, B, 1, 1, 14)
        assert names(p) == unsplit_names(cfg)
        assert all((l.RB, l.NRB, l.gy) == (B, 1, 1) for l in p.launches)
        assert [(l.gx, l.threads, l.lds, l.arg) for l in p.launches[:6]] == [(B, TPB, 0, 0)] + [(B, TPB, CONV_FWD_LDS, i) for i in (1, 2, 3)] + \
            [(64, NW * 64, fc_lds(NW, B), 1), (32, NW * 64, fc_lds(NW, B), 2)]
        assert p.launches[6][1:6] == (B // 16, 1, 512, 0, 0)
        assert p.launches[7][1:6] == (32, 1, TPB, B * 16 * 4 + 768 * 8, 0)
        assert p.launches[8][1:6] == (64, 1, NW * 64, fc_lds(NW, B), 0)
        assert [(l.gx, l.lds, l.arg) for l in p.launches[10:13]] == [(128 + B, CONV_BWD_LDS, 128), (B, CONV_BWD_LDS, 2), (B, CONV_BWD_LDS, 1)]
    p = got[64]
    assert only(p, "k_mix1<4,16,1,false>")[1:6] == (32 + 32, 1, 1024, 72192, 32)  # 32 weight-gradient workgroups, 32 column groups
    assert only(p, "k_mix2").gx == 128 + 64 and only(p, "k_update").gx == 443 + 4 + 6 == 453
    assert p.launches[4].lds == 72192 and "k_conv1_bwd" not in names(p)
    assert only(got[128], "k_mix1<8,8,1,false>")[1:6] == (64 + 32, 1, 512, fc_lds(8, 128), 64)


@pytest.mark.parametrize("B,NRB", [(144, 3), (368, 6)])
def test_othello8_row_blocks_of_64(exe, B, NRB):
    p = plan(exe, OTH8, B)
    assert (p.S, p.NB, p.RB, p.NRB, p.F1B, p.n) == (1, min(B, 256), 64, NRB, 0, 19)
    assert names(p) == split_names("4,16,1")
    assert all((l.RB, l.NRB) == (64, NRB) for l in p.launches)
    by = p.launches
    assert [(l.gx, l.gy, l.threads, l.lds, l.arg) for l in by[4:8]] == [(64, NRB, 1024, fc_lds(16, 64), 1), (64, NRB, TPB, 0, 1),
                                                                       (32, NRB, 1024, fc_lds(16, 64), 2), (32, NRB, TPB, 0, 2)]
    assert by[9][1:6] == (32, NRB, TPB, 64 * 16 * 4 + 768 * 8, 0) and by[10][1:6] == (32, NRB, TPB, 0, 2)  # k_bn1d_bwd_fin behind k_heads_bwd
    assert by[11][1:6] == (64, NRB, 1024, fc_lds(16, 64), 0) and by[12][1:6] == (64, NRB, TPB, 0, 1)  # ... and behind k_fc_dgrad
    assert by[13][1:6] == (128 + 32 * NRB, 1, 1024, fc_lds(16, 64), 128)  # four waves of the sixteen per tile: 512 / 4
    assert [(l.gx, l.lds, l.arg) for l in by[14:17]] == [(p.NB, CONV_BWD_LDS, i) for i in (3, 2, 1)]  # k_conv_bwd with l = 3 where k_mix2 stood
    assert by[17][1:6] == (p.NB + 512, 1, TPB, CONV1_WG_LDS, 0)
    assert by[18].gx == 447


@pytest.mark.parametrize("B,NRB", [(384, 3), (512, 4)])
def test_othello8_row_blocks_of_128_and_fc2_in_blocks_of_64(exe, B, NRB):
    p = plan(exe, OTH8, B)
    assert (p.S, p.NB, p.RB, p.NRB, p.F1B, p.n) == (1, 256, 128, NRB, 0, 19)
    assert names(p) == split_names("8,8,1", fc2="4,16,1")
    assert [(l.RB, l.NRB) for l in p.launches] == [(128, NRB)] * 6 + [(64, 2 * NRB)] * 2 + [(128, NRB)] * 11
    by = p.launches
    assert by[4][1:6] == (64, NRB, 512, fc_lds(8, 128), 1) and by[5][1:6] == (64, NRB, TPB, 0, 1)
    assert by[6][1:6] == (32, 2 * NRB, 1024, fc_lds(16, 64), 2) and by[7][1:6] == (32, 2 * NRB, TPB, 0, 2)
    assert by[9][1:6] == (32, NRB, TPB, 128 * 16 * 4 + 768 * 8, 0)
    assert by[13][1:6] == (256 + 32 * NRB, 1, 512, fc_lds(8, 128), 256)  # 512: 256 plus 128
    assert by[17][1:6] == (256 + 512, 1, TPB, CONV1_WG_LDS, 0) and by[18].gx == 447


# ---- OthelloNet 8x8, switches

def test_rb_0_never_splits(exe):
    _, got = plans(exe, OTH8, (144, 256, 272, 512), AZ_TRAIN_RB=0)
    for B, cfg, NW in ((144, "16,4,1", 4), (256, "16,4,1", 4), (272, "32,4,0", 4), (512, "32,4,0", 4)):
        p = got[B]
        assert (p.S, p.NB, p.RB, p.NRB, p.F1B, p.n) == (1, min(B, 256), B, 1, 1, 14)
        assert names(p) == unsplit_names(cfg)
        assert p.launches[4][1:6] == (64, 1, 256, fc_lds(4, B), 1) and only(p, f"k_mix1<{cfg},false>").arg == 128


def test_rb_64_and_128_need_a_larger_batch(exe):
    _, got = plans(exe, OTH8, (64, 80, 512), AZ_TRAIN_RB=64)
    assert got[64] == plan(exe, OTH8, 64)
    for B, NRB in ((80, 2), (512, 8)):
        assert (got[B].RB, got[B].NRB, got[B].n) == (64, NRB, 19) and names(got[B]) == split_names("4,16,1")
    _, got = plans(exe, OTH8, (128, 256), AZ_TRAIN_RB=128)
    assert got[128] == plan(exe, OTH8, 128)
    assert (got[256].RB, got[256].NRB, got[256].n) == (128, 2, 19) and names(got[256]) == split_names("8,8,1", fc2="4,16,1")
    assert names(plan(exe, OTH8, 256, AZ_TRAIN_RB=128, AZ_TRAIN_FC2_RB64=0)) == split_names("8,8,1")


def test_split_4_shares_a_board_while_the_grid_stays_within_256(exe):
    _, got = plans(exe, OTH8, (16, 64, 128, 512), AZ_TRAIN_SPLIT=4)
    for B, S, NB, cfg in ((16, 4, 64, "4,16,1"), (64, 4, 256, "4,16,1"), (128, 2, 256, "8,8,1")):
        p = got[B]
        assert (p.S, p.NB, p.RB, p.NRB, p.F1B, p.n) == (S, NB, B, 1, 0, 15)
        assert names(p) == unsplit_names(cfg, conv1_bwd=True)
        assert only(p, "k_conv1_bwd")[1:6] == (NB, 1, TPB, 0, 0) and only(p, "k_update").gx == 447 and only(p, "k_mix2").gx == 128 + NB
    assert got[512].S == 1 and got[512] == plan(exe, OTH8, 512)
    assert plan(exe, OTH8, 64, AZ_TRAIN_SPLIT=2).S == 2 and plan(exe, OTH8, 64, AZ_TRAIN_SPLIT=3) == plan(exe, OTH8, 64)


def test_fold1_0_launches_conv1_bwd(exe):
    p = plan(exe, OTH8, 64, AZ_TRAIN_FOLD1=0)
    assert (p.S, p.F1B, p.n) == (1, 0, 15) and names(p) == unsplit_names("4,16,1", conv1_bwd=True)
    assert only(p, "k_conv1_bwd")[1:6] == (64, 1, TPB, 0, 0)


def test_wg_late_0_keeps_fc1s_weight_gradient_in_mix2(exe):
    p = plan(exe, OTH8, 320, AZ_TRAIN_WG_LATE=0)
    assert (p.NB, p.RB, p.NRB, p.n) == (256, 64, 5, 19) and names(p) == split_names("4,16,1", wg_late=False)
    assert only(p, "k_mix2")[1:6] == (128 + 256, 1, TPB, CONV_BWD_LDS, 128) and only(p, "k_conv1_bwd")[1:6] == (256, 1, TPB, 0, 0)


def test_fc2_rb64_0_keeps_the_steps_row_block(exe):
    p = plan(exe, OTH8, 512, AZ_TRAIN_FC2_RB64=0)
    assert names(p) == split_names("8,8,1") and all((l.RB, l.NRB) == (128, 4) for l in p.launches)
    assert p.launches[6][1:6] == (32, 4, 512, fc_lds(8, 128), 2)


@pytest.mark.parametrize("switches,want", [({"AZ_TRAIN_GRAPH": 0}, (0, 8)), ({"AZ_TRAIN_GRAPH_STEPS": 3}, (1, 3)), ({"AZ_TRAIN_GRAPH_STEPS": 0}, (1, 8)),
                                           ({"AZ_TRAIN_GRAPH_STEPS": 65}, (1, 8)), ({}, (1, 8))])
def test_graph_switches(exe, switches, want):
    tuning, got = plans(exe, OTH8, (64,), **switches)
    assert tuning == want and got[64] == plan(exe, OTH8, 64)


# ---- the other nets

def test_othello6_heads(exe):
    p = plan(exe, OTH6, 32)  # NHP 48
    assert names(p) == unsplit_names("4,16,1", nt=3) and p.launches[4][1:6] == (64, 1, 1024, fc_lds(16, 32), 1)


def test_connect4(exe):
    p = plan(exe, C4, 32)  # F1 64, F2 32, FIN 192, NHP 16
    assert names(p) == unsplit_names("4,16,1", nt=1) and p.n == 14
    assert [l.gx for l in p.launches[4:6]] == [4, 2] and p.launches[7].gx == 2 and p.launches[8].gx == 4
    assert only(p, "k_mix1<4,16,1,false>")[1:6] == (1 + 12, 1, 1024, fc_lds(16, 32), 1) and only(p, "k_mix2")[1:6] == (3 + 32, 1, TPB, CONV_BWD_LDS, 3)
    p = plan(exe, C4, 512)
    assert p.n == 19 and names(p) == split_names("8,8,1", fc2="4,16,1", nt=1)
    assert only(p, "k_conv1_bwd").gx == 256 + 2 * 6 and only(p, "k_mix1<8,8,1,true>")[1:6] == (1 + 12 * 4, 1, 512, fc_lds(8, 128), 1)


def test_tictactoe_is_one_launch(exe):
    _, got = plans(exe, TTT, (2, 250))
    for B in (2, 250):
        assert got[B].n == 1 and got[B].launches == [Launch("k_ttt_step", 1, 1, TPB, ttt_lds(B), 0, B, 1)]
