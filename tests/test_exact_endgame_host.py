"""CPU: exact endgames without a GPU.
  1. the host model's solver (tests/exact_endgame_model.py: win cut-offs below the root, memoised) against a plain minimax that searches
     every move of every node: TicTacToe from the empty board (a draw, action 0) and Othello 4x4 from the start (12 empty cells: the
     side that moves second wins and every first move loses, so the action is the lowest legal one);
  2. the model's search: with E = 0 it is leaf_batch_model.Model at K = 1; a solved node takes no network row and becomes an
     unevaluated root when the move leads to it;
  3. endgame.parse and every Python combination check, before any device work;
  4. the header declares the three exports and _lib.py binds them."""
import os
import re

import numpy as np
import pytest

import exact_endgame_model as M
from conftest import ROOT
from leaf_batch_model import Model, make_board


# ------------------------------------------------------------------------------------------------------------------ 1
def test_tictactoe_from_the_empty_board_is_a_draw():
    b = make_board("tictactoe", 3, 3)
    assert M.solve(b) == (0, 0) == M.solve(b, prune=False)


def test_othello4_from_the_start_is_a_win_for_the_second_player():
    b = make_board("othello", 4, 4)
    assert M.empties(b) == 12
    assert M.solve(b) == (-1, 2) == M.solve(b, prune=False)
    legal = sorted(4 * r + c for r, c in b.get_moves())
    assert legal[0] == 2
    for a in legal:  # every first move loses
        c = b.clone()
        c.play_move((a // 4, a % 4))
        assert M.value(c) == -1


def test_pruned_and_plain_agree_along_playouts():
    for game, H, W in (("othello", 6, 6), ("connect4", 4, 4)):
        for b in M.positions(game, H, W, 3, 12, 1, 6):
            assert M.solve(b) == M.solve(b, prune=False), (game, b.grid, b.player)


def test_the_contract_above_the_limit_and_at_the_end():
    over = M.playout("othello", 6, 6, np.random.default_rng(0))
    assert over.is_game_over() and M.solve_contract(over, 1) == (int(over.get_winner()), -1)
    assert M.solve_contract(make_board("othello", 6, 6), 12) == (M.UNSOLVED, -1)
    passes = [b for b in M.positions("othello", 6, 6, 1, 256, 1, 8) if M.must_pass(b)]
    assert passes and all(M.solve(b)[1] == 36 for b in passes)


# ------------------------------------------------------------------------------------------------------------------ 2
def test_the_search_model_with_the_mode_off_is_the_plain_model():
    a = M.ExactModel(make_board("othello", 6, 6), 0, noise=(0.5, 0.25), tie="random", seed=5, game_id=9)
    b = Model(make_board("othello", 6, 6), K=1, noise=(0.5, 0.25), tie="random", seed=5, game_id=9)
    for _ in range(3):
        a.search(20)
        b.search(20)
        assert a.root_children() == b.root_children() and a.rows == b.rows
        assert a.advance() == b.advance()
        a.became_root()
    assert a.solved == 0


def test_a_solved_leaf_takes_no_row_and_a_solved_root_is_evaluated_again():
    root = next(b for b in M.positions("othello", 6, 6, 7, 24, 4, 4) if not b.is_game_over() and not M.must_pass(b))
    m = M.ExactModel(root, 6, tie="lowest", seed=1)
    m.search(32)
    assert m.rows == 1 and m.solved > 0  # the root prior alone
    for c in m.root.children:
        if c.N > 0:
            assert c.terminal and c.Q in (-1.0, 0.0, 1.0) and not c.children
            assert c.Q == -float(c.board.player * (c.win if c.board.is_game_over() else M.value(c.board)))
    n_before = max(m.root.children, key=lambda c: c.N).N
    m.advance()
    was_solved = id(m.root) in m.solved_ids
    m.became_root()
    if was_solved:
        assert not m.root.terminal and not m.root.evaluated and not m.root.expanded and m.root.N == n_before
        m.search(8)
        assert m.rows == 2 and m.root.evaluated  # the root-prior pass evaluated it


# ------------------------------------------------------------------------------------------------------------------ 3
def test_parse():
    from alphazero_amd import endgame
    assert endgame.parse(None) is None and endgame.parse(1) == 1 and endgame.parse(10) == 10 and endgame.parse(np.int64(6)) == 6
    for bad in (0, 11, -1, True, False, 6.0, "6", (6,)):
        with pytest.raises(ValueError, match="exact_endgame="):
            endgame.parse(bad)
    with pytest.raises(ValueError, match="selfplay_exact_endgame=12"):
        endgame.parse(12, "selfplay_exact_endgame")


def test_combination_checks_name_both_options():
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    for cls, kw in ((MCT, dict(eval_method="neural")), (AlphaZeroPlayer, dict(n_sim=8)), (BatchedAlphaZeroPlayer, dict(n_sim=8))):
        assert cls(exact_endgame=6, **kw).exact_endgame == 6 and cls(**kw).exact_endgame is None
        for other, val in (("symmetry", "all"), ("symmetry", "random"), ("leaf_batch", 4), ("gumbel", 8)):
            with pytest.raises(ValueError, match=f"exact_endgame=6 does not combine with {other}="):
                cls(exact_endgame=6, **{other: val}, **kw)
        cls(exact_endgame=6, leaf_batch=1, **kw)
        with pytest.raises(ValueError, match="exact_endgame=11"):
            cls(exact_endgame=11, **kw)
    with pytest.raises(ValueError, match="exact_endgame=6 needs eval_method 'neural'"):
        MCT(eval_method="rollout", exact_endgame=6)

    class Other:  # a network the HIP network does not serve: routed to the external evaluator
        def evaluate(self, board):
            return {}, 0.0
    with pytest.raises(ValueError, match="exact_endgame=6 needs a network the HIP network serves"):
        MCT(eval_method="neural", nn=Other(), exact_endgame=6)
    assert AlphaZeroTrainer(selfplay_exact_endgame=6).selfplay_exact_endgame == 6
    for other, val in (("selfplay_gumbel", 8), ("selfplay_symmetry", "random"), ("selfplay_playout_cap", (4, 0.5)), ("selfplay_forced_playouts", 2.0)):
        with pytest.raises(ValueError, match=f"selfplay_exact_endgame=6 does not combine with {other}="):
            AlphaZeroTrainer(selfplay_exact_endgame=6, **{other: val})
    with pytest.raises(ValueError, match="selfplay_exact_endgame=0"):
        AlphaZeroTrainer(selfplay_exact_endgame=0)


def test_solve_checks_its_arguments_before_any_device_work():
    from alphazero_amd import endgame
    assert endgame.solve([]) == []
    with pytest.raises(ValueError, match="max_empties=13"):
        endgame.solve([make_board("othello", 6, 6)], max_empties=13)
    with pytest.raises(ValueError, match="one game and one shape"):
        endgame.solve([make_board("othello", 6, 6), make_board("othello", 8, 8)])


# ------------------------------------------------------------------------------------------------------------------ 4
def test_header_and_binding_name_the_exports():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_solve_batch\(int game, int H, int W, const int8_t \*d_grids, const int8_t \*d_players, int64_t n,\s*"
                     r"int32_t max_empties, int64_t node_budget,\s*int8_t \*d_winner, int32_t \*d_action, int64_t \*d_nodes, void \*stream\);", hdr)
    assert re.search(r"int az_engine_set_exact_endgame\(az_engine \*e, int32_t max_empties\);", hdr)
    assert re.search(r"int az_engine_exact_endgame_stats\(az_engine \*e, int64_t \*solved_leaves, int64_t \*solver_nodes\);", hdr)
    assert "#define AZ_SOLVE_MAX_EMPTIES 12" in hdr and "#define AZ_UNSOLVED 2" in hdr and "#define AZ_EXACT_MAX_EMPTIES 10" in hdr
    from alphazero_amd import _lib, endgame
    assert {"az_solve_batch", "az_engine_set_exact_endgame", "az_engine_exact_endgame_stats"} <= set(_lib.SYMBOLS)
    assert (_lib.SOLVE_MAX_EMPTIES, _lib.UNSOLVED, _lib.EXACT_MAX_EMPTIES) == (12, 2, 10)
    assert (endgame.SOLVE_MAX_EMPTIES, endgame.UNSOLVED, endgame.MAX_EMPTIES) == (12, 2, 10)
    L = _lib.lib()
    assert all(hasattr(L, s) for s in ("az_solve_batch", "az_engine_set_exact_endgame", "az_engine_exact_endgame_stats"))
    assert L.az_engine_set_exact_endgame(None, 6) == _lib.AZ_EINVAL and L.az_engine_exact_endgame_stats(None, None, None) == _lib.AZ_EINVAL
    assert L.az_solve_batch(0, 6, 6, None, None, 0, 0, 0, None, None, None, None) == _lib.AZ_EINVAL  # max_empties 0, before any launch
