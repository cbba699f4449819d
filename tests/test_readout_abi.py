"""CPU-only checks of the batched root readout's C entry point and of the many-games players' argument checks (no GPU call)."""
import ctypes as C

import pytest

import alphazero_amd
from alphazero_amd import _lib, players
from alphazero_amd.games.tictactoe import TicTacToeBoard


def test_root_readout_refuses_null_arguments():
    L = _lib.lib()
    ro = _lib.RootReadout()
    assert L.az_engine_root_readout(None, None, 1, C.byref(ro)) == _lib.AZ_EINVAL
    assert "null argument" in L.az_last_error().decode()
    with pytest.raises(ValueError, match="null argument"):
        _lib.check(L.az_engine_root_readout(None, None, 1, None))
    assert L.az_version() >= 106


@pytest.mark.parametrize("cls", [players.BatchedMCTSPlayer, players.BatchedAlphaZeroPlayer])
def test_batched_player_constructor_and_board_count(cls):
    with pytest.raises(ValueError, match="n_sim"):
        cls(n_sim=None, n_slots=4)
    with pytest.raises(ValueError, match="n_slots"):
        cls(n_sim=5, n_slots=0)
    p = cls(n_sim=5, n_slots=2)
    with pytest.raises(ValueError, match="3 boards for 2 slots"):
        p.get_moves([TicTacToeBoard() for _ in range(3)])
    with pytest.raises(ValueError, match="3 boards for 2 slots"):
        p.analyze([TicTacToeBoard() for _ in range(3)])
    assert p._engine is None  # refused before any device work
    p.apply_moves([(0, 0)])  # no trees yet: nothing to do, as MCT.change_root
    p.reset()


def test_batched_players_are_exported_but_not_registered():
    assert alphazero_amd.BatchedMCTSPlayer is players.BatchedMCTSPlayer
    assert alphazero_amd.BatchedAlphaZeroPlayer is players.BatchedAlphaZeroPlayer
    assert set(players.PLAYERS_REGISTER) == {"random", "greedy", "mcts", "alphazero"}  # pinned against the live reference
