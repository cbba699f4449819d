"""CPU checks of the external evaluator (AZ_EVAL_EXTERNAL): which networks the HIP net / the HIP training step may stand in for,
the loud refusals that come before any device work, and the new C ABI symbols."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from alphazero_amd import _lib, train_step
from alphazero_amd.evaluators import hip_serves, route
from alphazero_amd.games.connect4 import Connect4Net
from alphazero_amd.games.othello import OthelloBoard, OthelloNet
from alphazero_amd.games.tictactoe import TicTacToeBoard, TicTacToeNet
from alphazero_amd.mcts import MCT
from tools import closed_form as cf


class FakeOthello8(OthelloNet):
    """the fake network the golden G3 trees were built with (tools/gen_golden.py fake_net_class): evaluate() overridden"""

    def evaluate(self, board):
        probs, v_net = cf.fakenet(board.grid, board.player, 65)
        return probs, board.player * v_net


class OwnForward(OthelloNet):
    def forward(self, input):  # the stock layers, another function
        log_p, v = super().forward(input)
        return log_p, -v


class ExtraLayer(OthelloNet):
    def __init__(self, n):
        super().__init__(n=n)
        self.extra = torch.nn.Linear(4, 4)


class OwnNormalizer(OthelloNet):
    def get_normalized_probs(self, probs, legal_moves):
        return {m: 1.0 / len(legal_moves) for m in legal_moves}


class Duck:
    def evaluate(self, board):
        A = board.get_action_size()
        return np.full(A, 1.0 / A, np.float32), 0.0


def test_route_shipped_networks_run_on_the_hip_net():
    assert route(OthelloNet(8)) == "hip"
    assert route(OthelloNet(6)) == "hip"
    assert route(Connect4Net(7, 6)) == "hip"
    assert route(TicTacToeNet()) == "hip"


def test_route_custom_evaluate_and_duck_types_take_the_board_path():
    assert route(FakeOthello8(8)) == "board"
    assert route(Duck()) == "board"
    with pytest.raises(TypeError):
        route(object())


def test_route_other_functions_and_shapes_take_the_torch_path():
    assert route(OwnForward(8)) == "torch"
    assert route(ExtraLayer(8)) == "torch"
    # planes az_net_create has no conv-trunk kernel for (4 x 4 Othello, a 4-wide Connect4 board)
    assert route(OthelloNet(4)) == "torch"
    assert route(Connect4Net(4, 6)) == "torch"


def test_training_step_serves_only_the_shipped_function():
    assert train_step.supports(OthelloNet(8), 64)
    assert not train_step.supports(OwnForward(8), 64)
    assert not train_step.supports(ExtraLayer(8), 64)
    assert hip_serves(FakeOthello8(8), search=False)  # evaluate() is not part of training
    assert not hip_serves(FakeOthello8(8), search=True)


def test_unknown_game_is_refused_before_device_work():
    board = TicTacToeBoard()
    board.game = "gomoku"
    mct = MCT(eval_method="neural", nn=TicTacToeNet())
    with pytest.raises(NotImplementedError, match="othello, connect4, tictactoe"):
        mct.search(board, n_sim=2)
    assert mct._engine is None


def test_custom_normalizer_is_refused_at_the_first_search():
    mct = MCT(eval_method="neural", nn=OwnNormalizer(6))
    with pytest.raises(NotImplementedError, match="get_normalized_probs"):
        mct.search(OthelloBoard(n=6), n_sim=2)
    assert mct._engine is None


def test_abi_declares_and_exports_the_external_evaluator():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    declared = set(re.findall(r"\b(az_[a-z_0-9]+)\s*\(", hdr))
    assert "az_engine_set_evaluator" in declared and "az_engine_set_evaluator" in _lib.SYMBOLS
    assert "az_eval_fn" not in declared  # the callback typedef is no export
    assert re.search(r"#define AZ_EVAL_EXTERNAL 3\b", hdr) and _lib.EVAL_EXTERNAL == 3
    assert re.search(r"#define AZ_EEVAL \(-6\)", hdr) and _lib.AZ_EEVAL == -6
    L = _lib.lib()
    assert hasattr(L, "az_engine_set_evaluator")
    assert L.az_version() >= 105
    with pytest.raises(_lib.EvalError):
        _lib.check(_lib.AZ_EEVAL)


def test_set_evaluator_argument_checks_without_a_device():
    L = _lib.lib()
    with pytest.raises(ValueError, match="null"):
        _lib.check(L.az_engine_set_evaluator(None, _lib.EVAL_FN(lambda u, b, s: 0), None))
