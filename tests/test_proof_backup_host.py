"""CPU: proof backup (az_engine_set_proof_backup) without a GPU.

  1. the host model's incremental marks (tests/proof_backup_model.py, what the engine keeps) against a brute-force restatement that
     recomputes every node's proven status from scratch after every simulation, over TicTacToe games with re-rooting, with and without
     solved leaves; and that the proofs are sound: a proven root has the game-theoretic outcome;
  2. the pruning rule on hand-written count vectors;
  3. the share of plies with a proven root in the waves the GPU soundness test plays, against its floor;
  4. the Python options: forms and combination checks, before any device work; 5. the header and the binding name the exports.
"""
import os
import re

import numpy as np
import pytest

import exact_endgame_model as X
import proof_backup_model as M
from conftest import ROOT
from leaf_batch_model import make_board

W, D, L = 1, 0, -1  # outcomes as seen by a mover +1


# ------------------------------------------------------------------------------------------------------------------ 1
def live_marks(m):
    live, stack = {}, [m.root]
    while stack:
        x = stack.pop()
        if id(x) in m.mark:
            live[id(x)] = m.mark[id(x)]
        stack.extend(x.children)
    return live


@pytest.mark.parametrize("tie,e,noise", [("lowest", 0, None), ("random", 0, M.NOISE), ("random", 3, None), ("lowest", 5, M.NOISE)])
def test_incremental_marks_are_the_brute_force_ones_after_every_simulation(tie, e, noise):
    memo, proven_roots, marked = {}, 0, 0
    for game_id in range(6):
        m = M.ProofModel(make_board("tictactoe", 3, 3), e, True, noise=noise, tie=tie, seed=5, game_id=game_id)
        while not m.root.board.is_game_over():
            for _ in range(20):
                m.search(1)
                assert live_marks(m) == M.brute_marks(m)
            if m.root_proof() != X.UNSOLVED:
                proven_roots += 1
                assert m.root_proof() == X.value(m.root.board, memo)  # sound: the game-theoretic outcome
            marked = max(marked, len(live_marks(m)))
            M.advance(m, 2, 5)
            assert live_marks(m) == M.brute_marks(m)  # the re-rooting keeps the marks; a solved root is cleared
    assert proven_roots > 0 and marked > 1


def test_mode_off_is_the_exact_model_and_marks_nothing():
    for e in (0, 4):
        a = M.ProofModel(make_board("tictactoe", 3, 3), e, False, tie="random", seed=3, game_id=1)
        b = X.ExactModel(make_board("tictactoe", 3, 3), e, tie="random", seed=3, game_id=1)
        while not a.root.board.is_game_over():
            a.search(16)
            b.search(16)
            assert a.root_children() == b.root_children() and a.counts() == ([c.N for c in a.root.children], False)
            M.advance(a, -1, 0)
            b.advance()
            b.became_root()
        assert not a.mark and (a.proven_nodes, a.proof_stops, a.pruned_plies) == (0, 0, 0) and a.rows == b.rows


def test_a_proven_child_has_been_visited():
    """a terminal child counts once its first visit is backed up (N = 1); an interior node is marked in a propagation that starts
    below it, on a path that holds it: it was evaluated at one visit, expanded at a later one (N >= 2)"""
    m = M.ProofModel(make_board("tictactoe", 3, 3, [[1, 0, 1], [0, -1, 0], [1, 0, -1]], -1), 0, True, tie="lowest")
    m.search(40)
    stack = [m.root]
    while stack:
        x = stack.pop()
        stack.extend(x.children)
        if id(x) in m.mark:
            assert x.N >= 2 and x.expanded
        if x.terminal and x is not m.root:
            assert (m.outcome(x) is not None) == (x.N >= 1)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("raw,outs,want", [
    ([5, 3, 2], [None, None, None], None),            # nothing proven
    ([5, 3, 2], [W, None, L], [5, 0, 0]),             # a proven win: the wins alone
    ([5, 3, 2, 4], [W, D, W, None], [5, 0, 2, 0]),    # two wins keep theirs
    ([5, 3, 2], [None, L, D], [5, 0, 2]),             # no win: the losses count 0, a draw stays
    ([5, 3, 2], [L, L, L], None),                     # every child loses: nothing is pruned
    ([4, 0, 0], [L, None, None], None),               # no other child visited: the counts stay
    ([4, 1, 0], [L, None, None], [0, 1, 0]),
    ([5, 3], [D, D], None),                           # draws are not pruned
    ([7, 0, 0], [W, None, None], None),               # the win holds every visit already: unchanged
])
def test_the_pruning_rule(raw, outs, want):
    for mover in (1, -1):
        new, changed = M.prune_counts(raw, [None if o is None else o * mover for o in outs], mover)
        assert new == (raw if want is None else want) and changed == (want is not None)


def test_the_policy_runs_on_the_pruned_counts_at_every_temperature():
    m = M.ProofModel(make_board("tictactoe", 3, 3, [[0, 1, 1], [0, 0, -1], [-1, 0, 1]], -1), 0, True, tie="lowest")
    m.search(40)  # three moves lose, one draws
    counts, changed = m.counts()
    assert changed and [c > 0 for c in counts] == [True, False, False, False] and all(c.N > 0 for c in m.root.children)
    for temp in (0.0, 0.5, 1.0):
        idx, pi, ch = M.move_policy(m, temp)
        assert idx == 0 and ch and pi[m.root.children[0].act] == 1.0 and pi.sum() == 1.0


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("game,H,Wd,share", [("tictactoe", 3, 3, 47 / 118), ("othello", 4, 4, 106 / 202), ("connect4", 4, 4, 102 / 256)])
def test_the_soundness_waves_clear_their_floor(game, H, Wd, share):
    """tests/test_gpu_proof_backup.py, test 2: 16 games, 24 simulations, temperature 0, hash noise, random ties"""
    _, ctr = M.play_wave(game, H, Wd, 11, 1000, 16, 24, 0, True, M.NOISE, "random", -1, 0)
    got = ctr["proven_roots"] / ctr["plies"]
    assert got >= 0.10 and got == share, (game, ctr["proven_roots"], ctr["plies"])


# ------------------------------------------------------------------------------------------------------------------ 4
def test_parse():
    from alphazero_amd import proof
    assert proof.parse(None) is False and proof.parse(False) is False and proof.parse(True) is True and proof.parse(np.bool_(True)) is True
    for bad in (0, 1, "on", 1.0, (True,)):
        with pytest.raises(ValueError, match="proof_backup="):
            proof.parse(bad)
    with pytest.raises(ValueError, match="selfplay_proof_backup=1"):
        proof.parse(1, "selfplay_proof_backup")


def test_combination_checks_name_both_options():
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    for cls, kw in ((MCT, dict(eval_method="neural")), (AlphaZeroPlayer, dict(n_sim=8)), (BatchedAlphaZeroPlayer, dict(n_sim=8))):
        assert cls(proof_backup=True, **kw).proof_backup is True and cls(**kw).proof_backup is False
        for other, val in (("symmetry", "all"), ("symmetry", "random"), ("leaf_batch", 4), ("gumbel", 8)):
            with pytest.raises(ValueError, match=f"proof_backup=True does not combine with {other}="):
                cls(proof_backup=True, **{other: val}, **kw)
        cls(proof_backup=True, leaf_batch=1, exact_endgame=6, **kw)  # exact endgames combine with it
        with pytest.raises(ValueError, match="proof_backup=1"):
            cls(proof_backup=1, **kw)
    with pytest.raises(ValueError, match="proof_backup=True needs eval_method 'neural'"):
        MCT(eval_method="rollout", proof_backup=True)

    class Other:  # a network the HIP network does not serve: routed to the external evaluator
        def evaluate(self, board):
            return {}, 0.0
    with pytest.raises(ValueError, match="proof_backup=True needs a network the HIP network serves"):
        MCT(eval_method="neural", nn=Other(), proof_backup=True)
    assert MCT(eval_method="neural", proof_backup=True).root_proof() is None  # nothing searched yet
    assert AlphaZeroTrainer(selfplay_proof_backup=True).selfplay_proof_backup is True
    assert AlphaZeroTrainer(selfplay_proof_backup=True, selfplay_exact_endgame=6).selfplay_exact_endgame == 6
    for other, val in (("selfplay_gumbel", 8), ("selfplay_symmetry", "random"), ("selfplay_playout_cap", (4, 0.5)), ("selfplay_forced_playouts", 2.0)):
        with pytest.raises(ValueError, match=f"selfplay_proof_backup=True does not combine with {other}="):
            AlphaZeroTrainer(selfplay_proof_backup=True, **{other: val})
    with pytest.raises(ValueError, match="selfplay_proof_backup=2"):
        AlphaZeroTrainer(selfplay_proof_backup=2)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_header_and_binding_name_the_exports():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_proof_backup\(az_engine \*e, int32_t on\);", hdr)
    assert re.search(r"int az_engine_proof_backup_stats\(az_engine \*e, int64_t \*proven_nodes, int64_t \*proof_stops, int64_t \*pruned_plies\);", hdr)
    assert re.search(r"int az_engine_root_proofs\(az_engine \*e, int8_t \*d_out\);", hdr)
    assert "F_PROVEN = 64" in hdr
    from alphazero_amd import _lib
    names = ("az_engine_set_proof_backup", "az_engine_proof_backup_stats", "az_engine_root_proofs")
    assert set(names) <= set(_lib.SYMBOLS)
    Lb = _lib.lib()
    assert all(hasattr(Lb, s) for s in names) and Lb.az_version() >= 114
    assert Lb.az_engine_set_proof_backup(None, 1) == _lib.AZ_EINVAL and Lb.az_engine_proof_backup_stats(None, None, None, None) == _lib.AZ_EINVAL
    assert Lb.az_engine_root_proofs(None, None) == _lib.AZ_EINVAL
