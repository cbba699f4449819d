"""GPU: az_engine_run as slot groups with a real network at the sizes the defaults run.  groups_auto plays Othello 8x8
as 2 groups from 4096 to 8191 slots and Connect4 6x7 as 4 groups from 8192 slots; every group forwards on its own lane of the az_net
with beside = 1.  A run replays captured graphs, whose launch sizes must not change: below 4096 rows a chain's network launch keeps
the chain's full width for the whole run and only the device row count falls as games end; from 4096 rows the cap follows the live
slots in steps of 512 (do_search: cap_q).  The kernels per shape (az_net_plan.h: plan_trunk, plan_dense):

  othello8, 2112 slots   2 x 1056: k_trunk_quad, k_gemm<64,64> (fc1) and k_gemm<64,128> (fc2), just above k_dense_frag's beside limit;
                         4 x 528 (lanes 2 and 3 in use): k_trunk_quad + k_dense_frag;  1 x 2112: k_trunk, k_gemm<64,64> twice
  othello8, 4096 slots   auto = 2 x 2048: k_trunk_quad + k_gemm<64,64> twice;  1 x 4096: k_trunk2, then k_trunk / k_trunk_q as the cap
                         comes down through 3584 .. 512, the dense layers from k_gemm to k_dense_frag
  connect4, 2112 / 8192  k_trunk_quad on the 7x6 plane and the fused tail (k_tail_mfma) on four lanes; 1 x 8192: k_trunk2 first
  othello6, 1040 slots   k_trunk (no quad form) with games refilled across the groups;  Connect4Net 7x7: k_trunk, generic dense kernels
  tictactoe, 48 slots    k_mlp: a lane is a name only

(a kernel trace of the 4 x 528 run listed k_trunk_quad<8, 8>, k_dense_frag twice and k_heads2 per forward on four queues, and no other
network kernel from the first ply to the last.)

A game depends on (seed, game id) only and a network row on its board only.  Every case therefore holds the grouped runs to the
one-group run of the same shape bit for bit (samples in (game id, move index) order, and the counters), and pins that result to the
CPU oracle: single games replayed alone by O.selfplay must equal their rows of the GPU run -- always the first and the last game id
and the ids on both sides of every group boundary (make_chain: blocks of 16 slots, ceil(blocks / n) blocks per group).  One Othello
8x8 game costs the oracle about 0.5 s at 4 simulations (0.8 s at 8; Othello 6x6 0.2 s, Connect4 0.06 s), hence n_sim = 4 there."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from alphazero_amd import engine as E
from test_gpu_engine_groups import KEYS, same, sort_samples

pytestmark = pytest.mark.gpu
_CACHE = {}


def _np_sd(module):
    return {k: v.detach().cpu().numpy() for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")}


def get_net(kind):
    """per kind, once: (game id, H, W, HipNet, oracle evaluator) of a torch.manual_seed network"""
    if kind not in _CACHE:
        from alphazero_amd.games.connect4 import Connect4Net
        from alphazero_amd.games.othello import OthelloNet
        from alphazero_amd.games.tictactoe import TicTacToeNet
        torch.manual_seed(5)
        gid, H, W, net, max_batch = {"othello8": lambda: (0, 8, 8, OthelloNet(n=8), 8192), "othello6": lambda: (0, 6, 6, OthelloNet(n=6), 4096),
                                     "connect4": lambda: (1, 6, 7, Connect4Net(7, 6), 8192), "connect4_7x7": lambda: (1, 7, 7, Connect4Net(7, 7), 1040),
                                     "tictactoe": lambda: (2, 3, 3, TicTacToeNet(), 64)}[kind]()
        net = net.eval()
        sd = _np_sd(net)
        ev = ("mlp", O.MlpNet(sd)) if kind == "tictactoe" else ("conv", O.ConvNet(gid, H, W, sd))
        _CACHE[kind] = (gid, H, W, net.to_hip(max_batch=max_batch), ev)
    return _CACHE[kind]


def net_run(kind, slots, games, n_sim, seed, groups, expect_groups=None):
    """(sorted samples, stats) of one run; groups None: the measured default, which must be expect_groups"""
    gid, H, W, net, ev = get_net(kind)
    max_plies = 2 * H * W if gid == 0 else H * W + 1
    eng = E.SelfPlayEngine(gid, H, W, n_slots=slots, n_sim=n_sim, net=net, seed=seed, groups=groups, sample_capacity=max(slots, games) * max_plies)
    assert eng.groups() == (groups if groups is not None else expect_groups), (kind, slots, eng.groups())
    out = (sort_samples(eng.run(games)), eng.stats())
    eng.close()
    return out


def boundary_ids(slots, games, group_counts):
    """the first and the last game id, and the ids seated on both sides of every group boundary (k_reset_all seats game i in slot i)"""
    ids = {0, games - 1}
    blocks = (slots + 15) // 16
    for n in group_counts:
        per = (blocks + n - 1) // n
        for i in range(1, n):
            if i * per * 16 < slots:
                ids |= {i * per * 16 - 1, i * per * 16}
    return sorted(ids)


def pin_to_oracle(kind, run, ids, n_sim, seed):
    gid, H, W, net, ev = get_net(kind)
    got = run[0]
    for g in ids:
        ref = O.selfplay(gid, H, W, 1, n_sim, ev, seed=seed, first_game_id=g)
        rows = got["meta"][:, 0] == g
        assert rows.sum() == len(ref["meta"]) > 0, (kind, g)
        for k in KEYS:
            assert np.array_equal(got[k][rows], ref[k]), (kind, g, k)


def test_boundary_ids_follow_make_chain():
    assert boundary_ids(2112, 2112, (2, 4)) == [0, 527, 528, 1055, 1056, 1583, 1584, 2111]
    assert boundary_ids(1040, 2081, (2, 4)) == [0, 271, 272, 527, 528, 543, 544, 815, 816, 2080]
    assert boundary_ids(40, 40, (4,)) == [0, 15, 16, 31, 32, 39]  # 16, 16, 8, 0 slots: the empty last group has no boundary


@pytest.mark.parametrize("kind,n_sim", [("othello8", 4), ("connect4", 8)])
def test_2112_slots_in_two_and_four_groups(kind, n_sim):
    """groups of 1056 launch just above k_dense_frag's beside limit while their row counts fall through 1024 and 512 as games end; groups
    of 528 put lanes 2 and 3 of the az_net in use (connect4: k_trunk_quad on the 7x6 plane and the fused tail on four lanes)"""
    ref = net_run(kind, 2112, 2112, n_sim, 11, 1)
    for groups in (2, 4):
        same(net_run(kind, 2112, 2112, n_sim, 11, groups), ref)
    pin_to_oracle(kind, ref, boundary_ids(2112, 2112, (2, 4)), n_sim, 11)


def test_othello8_headline_slots_default_to_two_groups():
    """4096 slots, nothing asked for: the rule plays 2 x 2048 (k_trunk_quad, both dense layers on k_gemm<64,64>); the one-group run of
    the same shape starts on k_trunk2 and ends on k_trunk_q, so this holds the trunks to each other as well"""
    auto = net_run("othello8", 4096, 4096, 4, 12, None, expect_groups=2)
    ref = net_run("othello8", 4096, 4096, 4, 12, 1)
    same(auto, ref)
    pin_to_oracle("othello8", ref, boundary_ids(4096, 4096, (2,)), 4, 12)


def test_connect4_config4_slots_default_to_four_groups():
    """8192 slots, nothing asked for: 4 x 2048 against 1 x 8192"""
    auto = net_run("connect4", 8192, 8192, 8, 13, None, expect_groups=4)
    ref = net_run("connect4", 8192, 8192, 8, 13, 1)
    same(auto, ref)
    pin_to_oracle("connect4", ref, boundary_ids(8192, 8192, (4,)), 8, 13)


def test_refill_across_groups_with_a_real_network():
    """1040 slots, two waves and one game: every finished slot draws its next game id from the dispenser all groups share, the last
    wave leaves most groups empty.  The ids checked on the oracle include the first refilled ones and the last"""
    games = 1040 * 2 + 1
    ref = net_run("othello6", 1040, games, 6, 14, 1)
    for groups in (2, 4):
        same(net_run("othello6", 1040, games, 6, 14, groups), ref)
    pin_to_oracle("othello6", ref, boundary_ids(1040, games, (2, 4)) + [1039, 1040, 1041], 6, 14)


def test_auto_rule_table():
    """groups_auto where it answers 1 (its 2 and 4 are asserted by the two default cases above, before their runs): Othello 8x8 below
    4096 and from 8192 slots, Connect4 6x7 below 8192, every other shape, and the fake evaluator"""
    for kind, slots in (("othello8", 4095), ("othello8", 8192), ("connect4", 8191), ("othello6", 4096)):
        gid, H, W, net, ev = get_net(kind)
        eng = E.SelfPlayEngine(gid, H, W, n_slots=slots, n_sim=4, net=net)
        assert eng.groups() == 1, (kind, slots, eng.groups())
        eng.close()
    fake = E.SelfPlayEngine(0, 8, 8, n_slots=4096, n_sim=4, evaluator=E.EVAL_FAKE)
    assert fake.groups() == 1
    fake.close()


def test_untuned_plane_in_two_groups():
    """Connect4Net on a 7x7 board: the plane has neither a quad trunk nor the fused tail, so two lanes run k_trunk and the generic dense
    kernels side by side (2 x 528 slots and the ragged last block of 1040)"""
    ref = net_run("connect4_7x7", 1040, 1040, 8, 15, 1)
    same(net_run("connect4_7x7", 1040, 1040, 8, 15, 2), ref)
    pin_to_oracle("connect4_7x7", ref, boundary_ids(1040, 1040, (2,)), 8, 15)


def test_tictactoe_in_groups_with_its_network():
    """the MLP keeps no activation rows, so its lanes are names: 48 slots, two waves and one game, in 2 and 4 groups -- the one-group
    run, which is the oracle's whole run game for game"""
    games = 48 * 2 + 1
    gid, H, W, net, ev = get_net("tictactoe")
    ref = net_run("tictactoe", 48, games, 8, 16, 1)
    for groups in (2, 4):
        same(net_run("tictactoe", 48, games, 8, 16, groups), ref)
    whole = O.selfplay(gid, H, W, games, 8, ev, seed=16)
    assert ref[1]["net_evals"] == whole["n_evals"]
    for k in KEYS:
        assert np.array_equal(ref[0][k], whole[k]), k
