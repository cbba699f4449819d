"""CPU checks of the symmetry ensemble's convention (alphazero_amd/symmetry.py): the twins are the trainer's, the inverse table
maps a twin's policy back, masks resolve per game, and the players carry the option and refuse it before any device work where
it cannot run."""
import numpy as np
import pytest
import torch

from alphazero_amd import symmetry as S
from alphazero_amd.base import DataTransf
from alphazero_amd.games.connect4 import Connect4Net
from alphazero_amd.games.othello import OthelloNet
from alphazero_amd.games.tictactoe import TicTacToeNet
from alphazero_amd.mcts import MCT
from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
from alphazero_amd.trainer import Sample

ROTATIONS = {1: DataTransf.ROTATE_90, 2: DataTransf.ROTATE_180, 3: DataTransf.ROTATE_270}
CASES = {  # tag: (game, H, W, A, network factory, codes)
    "othello6": ("othello", 6, 6, 37, lambda: OthelloNet(6, device="cpu"), range(1, 8)),
    "othello8": ("othello", 8, 8, 65, lambda: OthelloNet(8, device="cpu"), range(1, 8)),
    "tictactoe": ("tictactoe", 3, 3, 9, lambda: TicTacToeNet(device="cpu"), range(1, 8)),
    "connect4": ("connect4", 6, 7, 7, lambda: Connect4Net(7, 6, device="cpu"), (1,)),
}


def trainer_twin(net, state, pi, code):
    """the twin of one sample as the trainer's augmentation builds it: the reflection first, then the rotation"""
    s = Sample(state=state, pi=pi, player=1, outcome=0, episode_idx=0, move_idx=2)
    if code & 1:
        s = s.create_reflection_twin(net.reflect_neural_output, mode=DataTransf.REFLECT_H)
    if code >> 1:
        s = s.create_rotation_twin(net.rotate_neural_output, mode=ROTATIONS[code >> 1])
    return s.state, s.pi


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("tag", list(CASES))
def test_twins_match_the_trainers(tag):
    game, H, W, A, make, codes = CASES[tag]
    net = make()
    rng = np.random.default_rng(11)
    for code in codes:
        for _ in range(4):
            state = rng.integers(-1, 2, (H, W)).astype(np.float64)
            pi = rng.random(A)
            ref_state, ref_pi = trainer_twin(net, state, pi, code)
            assert np.array_equal(S.twin_planes(state, code), ref_state), (tag, code)
            assert np.array_equal(S.twin_pi(pi, code, game, H, W), ref_pi), (tag, code)
            # torch tensors and leading batch axes take the same path
            t_state = S.twin_planes(torch.from_numpy(state)[None, None], code)[0, 0]
            t_pi = S.twin_pi(torch.from_numpy(pi)[None], code, game, H, W)[0]
            assert np.array_equal(t_state.numpy(), ref_state) and np.array_equal(t_pi.numpy(), ref_pi), (tag, code)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("tag", list(CASES))
def test_untwin_round_trip_pins_the_inverse_table(tag):
    game, H, W, A, _, codes = CASES[tag]
    rng = np.random.default_rng(12)
    p = rng.random((3, A)).astype(np.float32)
    for code in [0, *codes]:
        assert np.array_equal(S.untwin_probs(S.twin_pi(p, code, game, H, W), code, game, H, W), p), (tag, code)
        assert np.array_equal(S.twin_pi(S.untwin_probs(p, code, game, H, W), code, game, H, W), p), (tag, code)
        tp = torch.from_numpy(p)
        assert torch.equal(S.untwin_probs(S.twin_pi(tp, code, game, H, W), code, game, H, W), tp), (tag, code)
        if game != "connect4":  # the board twin is undone by the inverse code's twin
            x = rng.integers(-1, 2, (2, H, W)).astype(np.float32)
            assert np.array_equal(S.twin_planes(S.twin_planes(x, code), S.INVERSE[code]), x), (tag, code)
    # a distinct value per entry: any other table would move some entry
    assert sorted(S.INVERSE) == list(range(8))


# ------------------------------------------------------------------------------------------------------------------ 3
def test_resolve():
    assert S.resolve(None) == 0
    assert S.resolve("all") == S.SYM_ALL == -1
    assert S.resolve(0x41) == 0x41 and S.resolve(np.int32(3)) == 3 and S.resolve(-1) == -1
    assert S.resolve([0, 4]) == 0x11 and S.resolve({1, 6}) == 0x42 and S.resolve(range(8)) == 0xFF and S.resolve(()) == 0
    for bad in ("ALL", "none", 256, -2, [8], [-1], [0.5], ["1"], True, [True]):
        with pytest.raises(ValueError):
            S.resolve(bad)


def test_members():
    assert S.members("othello", 8, 8, "all") == list(range(8))
    assert S.members("othello", 6, 6, "all") == list(range(8))
    assert S.members("tictactoe", 3, 3, "all") == list(range(8))
    assert S.members(2, 3, 3, -1) == list(range(8))
    assert S.members("connect4", 6, 7, "all") == [0, 1]
    assert S.members("connect4", 8, 8, "all") == [0, 1]  # gravity: no rotations on a square Connect4 board either
    assert S.members(1, 8, 8, [1]) == [1]
    assert S.members("othello", 8, 8, {6, 1}) == [1, 6]  # ascending code order
    assert S.members("othello", 8, 8, None) == [] and S.members("connect4", 6, 7, 0) == []
    for game, H, W, mask in (("connect4", 6, 7, [0, 2]), ("connect4", 8, 8, [4]), ("connect4", 6, 7, 0xFF), (1, 8, 8, [3]),
                             ("othello", 6, 8, [2]), ("othello", 6, 8, [0, 1, 5])):
        with pytest.raises(ValueError, match="rotation"):
            S.members(game, H, W, mask)
    assert S.members("othello", 6, 8, "all") == [0, 1]  # a board that is not square keeps the reflection
    with pytest.raises(ValueError):
        S.members("chess", 8, 8, "all")


class OwnForward(OthelloNet):
    def forward(self, input):  # the stock layers, another function: the torch route
        log_p, v = super().forward(input)
        return log_p, -v


class Duck:
    def evaluate(self, board):
        A = board.get_action_size()
        return np.full(A, 1.0 / A, np.float32), 0.0


def test_players_accept_and_carry_symmetry():
    net = OthelloNet(6, device="cpu")
    assert MCT(eval_method="neural", nn=net).symmetry is None
    assert MCT(eval_method="neural", nn=net, symmetry="all").symmetry == "all"
    p = AlphaZeroPlayer(n_sim=4, nn=net, symmetry=[0, 1])
    assert p.symmetry == [0, 1] and p.mct.symmetry == [0, 1]
    assert p.clone().symmetry == [0, 1]
    p.reset()
    assert p.symmetry == [0, 1] and p.mct.nn is net
    assert AlphaZeroPlayer(n_sim=4, nn=net).clone().symmetry is None
    b = BatchedAlphaZeroPlayer(n_sim=4, nn=net, n_slots=3, symmetry="all")
    assert b.symmetry == "all"
    assert BatchedAlphaZeroPlayer(n_sim=4, nn=net, n_slots=3).symmetry is None
    # nothing above loaded the library's engine or a device: the trees are built at the first search
    assert p.mct._engine is None and b._engine is None
    for bad in ("some", [9]):
        with pytest.raises(ValueError):
            MCT(eval_method="neural", nn=net, symmetry=bad)
        with pytest.raises(ValueError):
            BatchedAlphaZeroPlayer(n_sim=4, nn=net, symmetry=bad)


@pytest.mark.parametrize("make", [lambda: OwnForward(6, device="cpu"), Duck])
def test_symmetry_with_an_externally_evaluated_network_is_refused_before_any_device_work(make, monkeypatch):
    from alphazero_amd import _lib

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    nn = make()
    with pytest.raises(ValueError, match="external evaluator"):
        MCT(eval_method="neural", nn=nn, symmetry="all")
    with pytest.raises(ValueError, match="external evaluator"):
        AlphaZeroPlayer(n_sim=4, nn=nn, symmetry="all")
    with pytest.raises(ValueError, match="external evaluator"):
        BatchedAlphaZeroPlayer(n_sim=4, nn=nn, n_slots=2, symmetry=[0, 1])
    mct = MCT(eval_method="neural", nn=OthelloNet(6, device="cpu"), symmetry="all")
    with pytest.raises(ValueError, match="external evaluator"):
        mct.nn = nn  # the setter checks too
    # off is off: the same networks are accepted without a symmetry
    assert MCT(eval_method="neural", nn=nn, symmetry=None).symmetry is None
    assert BatchedAlphaZeroPlayer(n_sim=4, nn=nn, n_slots=2).symmetry is None
    # set on the attribute after construction: refused when the trees are built, still before the engine exists
    late = BatchedAlphaZeroPlayer(n_sim=4, nn=nn, n_slots=2)
    late.symmetry = "all"
    from alphazero_amd.games.othello import OthelloBoard
    with pytest.raises(ValueError, match="external evaluator"):
        late.get_moves([OthelloBoard(n=6)])
