"""CPU: the host side of the random symmetry mode (one board symmetry drawn per evaluation).

  1. symmetry.parse tells ensemble and random specs apart and refuses malformed ones;
  2. symmetry.random_code -- the host restatement of the device draw -- is uniform over the members and always a member;
  3. refusals happen before any device work; leaf_batch combines with a random spec;
  4. the two new entry points are declared, exported and listed (test_abi.py checks the whole header).
"""
import numpy as np
import pytest

from alphazero_amd import _lib
from alphazero_amd import symmetry as S
from alphazero_amd.games.othello import OthelloBoard, OthelloNet
from alphazero_amd.mcts import MCT, check_leaf_batch
from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
from alphazero_amd.trainer import AlphaZeroTrainer
from tools import closed_form as cf


class OwnForward(OthelloNet):
    def forward(self, input):  # the stock layers, another function: the torch route (external evaluator)
        log_p, v = super().forward(input)
        return log_p, -v


# ------------------------------------------------------------------------------------------------------------------ 1
def test_parse():
    assert S.parse("random") == (S.SYM_ALL, True)
    assert S.parse(("random", [0, 1])) == (0b11, True)
    assert S.parse(("random", "all")) == (S.SYM_ALL, True)
    assert S.parse(("random", 0x55)) == (0x55, True)
    assert S.parse(("random", None)) == (0, True)
    # everything resolve() accepts today is an ensemble spec (or off) with the mask resolve() gives
    for spec in (None, "all", 0, 5, 0xFF, S.SYM_ALL, (), (0,), [0, 4], (1, 6), np.array([2, 3]), range(8)):
        assert S.parse(spec) == (S.resolve(spec), False), spec
    for bad in ("Random", ("random",), ("random", [8]), ("random", "random"), ("random", [0], [1]), ("all", [0]), "some", True,
                ("random", True), ("random", 256)):
        with pytest.raises(ValueError):
            S.parse(bad)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("members,bound,measured", [(list(range(8)), 24.32, 2.22), ([0, 1], 10.83, 1.25)])
def test_random_code_is_uniform(members, bound, measured):
    """8000 draws of one fixed stream: chi-square against uniform below the p = 0.001 point of n - 1 degrees of freedom"""
    assert cf.P_SYMMETRY == 8
    n, counts = len(members), dict.fromkeys(members, 0)
    for gid in range(64):
        for ply in range(5):
            for s in range(25):
                code = S.random_code(11, gid, ply, s, members)
                assert code == members[(cf.philox4x32(11, gid, ply, s, 8, 0)[0] * n) >> 32]
                counts[code] += 1  # KeyError: not a member
    expect = 8000 / n
    chi2 = sum((c - expect) ** 2 / expect for c in counts.values())
    print(f"{n} members: chi2 {chi2:.3f}")
    assert chi2 < bound
    assert abs(chi2 - measured) < 0.01  # the stream is fixed, so is the figure


def test_random_code_members():
    assert S.ROOT_PASS == 0xFFFFFFFF
    for m in range(8):
        assert S.random_code(3, 9, 2, S.ROOT_PASS, [m]) == m
    picks = {S.random_code(3, g, 0, S.ROOT_PASS, [1, 4, 6]) for g in range(64)}
    assert picks == {1, 4, 6}
    # a function of (seed, game, ply, s) alone
    assert S.random_code(3, 9, 2, 5, list(range(8))) == S.random_code(3, 9, 2, 5, list(range(8)))
    draws = [[S.random_code(sd, g, p, s, list(range(8))) for s in range(32)] for sd, g, p in ((3, 9, 2), (4, 9, 2), (3, 10, 2), (3, 9, 3))]
    assert all(draws[0] != d for d in draws[1:])
    for bad in ([], [1, 0], [2, 2]):
        with pytest.raises(ValueError):
            S.random_code(0, 0, 0, 0, bad)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_refusals_before_any_device_work(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    ext, hip_routed = OwnForward(6, device="cpu"), OthelloNet(6, device="cpu")
    for spec in ("random", ("random", [0, 1])):
        with pytest.raises(ValueError, match="external evaluator"):
            MCT(eval_method="neural", nn=ext, symmetry=spec)
        with pytest.raises(ValueError, match="external evaluator"):
            AlphaZeroPlayer(n_sim=4, nn=ext, symmetry=spec)
        with pytest.raises(ValueError, match="external evaluator"):
            BatchedAlphaZeroPlayer(n_sim=4, nn=ext, n_slots=2, symmetry=spec)
    # a rollout-mode tree evaluates no leaf
    with pytest.raises(ValueError, match="neural"):
        MCT(eval_method="rollout", symmetry="random").search(OthelloBoard(n=6), n_sim=2)
    # the self-play wave takes a random spec or nothing
    for bad in ("all", 7, [0, 1], "Random", ("random", [9])):
        with pytest.raises(ValueError, match="selfplay_symmetry"):
            AlphaZeroTrainer(selfplay_symmetry=bad)
    assert AlphaZeroTrainer().selfplay_symmetry is None
    assert AlphaZeroTrainer(selfplay_symmetry="random").selfplay_symmetry == "random"
    assert AlphaZeroTrainer(selfplay_symmetry=("random", [0, 1])).selfplay_symmetry == ("random", [0, 1])
    # leaf_batch combines with a random spec and keeps refusing the ensemble
    mct = MCT(eval_method="neural", nn=hip_routed, symmetry="random", leaf_batch=4)
    assert mct.symmetry == "random" and mct.leaf_batch == 4 and mct._engine is None
    assert check_leaf_batch(16, hip_routed, ("random", [0, 1])) == 16
    p = AlphaZeroPlayer(n_sim=4, nn=hip_routed, symmetry=("random", "all"), leaf_batch=2)
    assert p.clone().symmetry == ("random", "all") and p.clone().leaf_batch == 2
    b = BatchedAlphaZeroPlayer(n_sim=4, nn=hip_routed, n_slots=3, symmetry="random", leaf_batch=8)
    assert b.symmetry == "random" and b._engine is None
    for ens in ("all", [0, 1], 3):
        with pytest.raises(ValueError, match="does not combine"):
            MCT(eval_method="neural", nn=hip_routed, symmetry=ens, leaf_batch=4)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_the_new_entry_points_are_listed():
    assert {"az_net_forward_sym_codes", "az_engine_set_symmetry_random"} <= set(_lib.SYMBOLS)
    L = _lib.lib()
    assert hasattr(L, "az_net_forward_sym_codes") and hasattr(L, "az_engine_set_symmetry_random")
    # argument checks that need no device
    assert L.az_engine_set_symmetry_random(None, 1) == -1  # AZ_EINVAL: null engine
    assert L.az_net_forward_sym_codes(None, None, 1, None, None, None, None) == -1
