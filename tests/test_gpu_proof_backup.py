"""GPU: proof backup, MCTS-Solver (az_engine_set_proof_backup; include/az_amd.h).

  1. whole az_engine_run waves are the host model's (tests/proof_backup_model.py) bit for bit -- samples, visits, pi, z, moves, plies,
     net_evals, solved_leaves and the three counters: TicTacToe, Connect4 4x4 and 6x7, Othello 4x4 and 6x6, with slot refill on fewer
     slots than a block, hash noise, both tie modes, exact endgames off, at E = 3 and at E = 6; the same games under 1, 2 and 4 slot
     groups; a real network against the model on that network's outputs, and with the evaluation cache on and off;
  2. soundness against the solver: at every ply of waves of TicTacToe, Othello 4x4 and Connect4 4x4 a root that root_proofs reports
     proven has solve_batch's outcome, and the temperature-0 move played from it leads to a position of the same outcome;
  3. hand-built positions through set_roots: a win in one, a forced loss in two, a forced draw, and on Othello 6x6 a proven node below
     a pass;
  4. a terminal leaf at the end of a path of more than 16 nodes (the parent-chasing branch of the propagation);
  5. off is off; 6. every refusal, both ways, by name, and the AZ_ESTATE cases; 7. the Python surface.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_endgame_model as X
import proof_backup_model as M
from alphazero_amd import _lib
from alphazero_amd import engine as E
from leaf_batch_model import _move, make_board

pytestmark = pytest.mark.gpu

KEYS = ("state", "pi", "visits", "z", "meta")
TIES = {"lowest": E.TIE_LOWEST, "random": E.TIE_RANDOM}
SEED, FIRST, N_SIM = 11, 1000, 24
GAMES = {"tictactoe": ("tictactoe", 2, 3, 3), "connect4": ("connect4", 1, 4, 4), "connect4_67": ("connect4", 1, 6, 7),
         "othello4": ("othello", 0, 4, 4), "othello6": ("othello", 0, 6, 6)}


def fake_engine(tag, tie, n_slots, n_sim=N_SIM, noise=True, temp0=False, **kw):
    _, gid, H, W = GAMES[tag]
    return E.SelfPlayEngine(gid, H, W, n_slots=n_slots, n_sim=n_sim, evaluator=E.EVAL_FAKE, tie_mode=TIES[tie],
                            noise_mode=E.NOISE_HASH if noise else E.NOISE_OFF, dirichlet_alpha=M.NOISE[0] if noise else None,
                            dirichlet_epsilon=M.NOISE[1] if noise else None, temp_max_step=-1 if temp0 else M.TMAX,
                            temp_min_step=0 if temp0 else M.TMIN, seed=SEED, node_capacity=8192, sample_capacity=4096, **kw)


def ordered(smp):
    a = {k: v.cpu().numpy() for k, v in smp.items()}
    order = np.lexsort((a["meta"][:, 1], a["meta"][:, 0]))
    return {k: v[order] for k, v in a.items()}


def same_rows(got, want, what):
    for k in KEYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


def counters(eng):
    st, xs, ps = eng.stats(), eng.exact_endgame_stats(), eng.proof_backup_stats()
    assert st["error_flags"] == 0
    return {"samples": st["samples"], "plies": st["plies"], "rows": st["net_evals"], "solved": xs["solved_leaves"], **ps}


def model_counters(ctr):
    return {k: ctr[k] for k in ("samples", "plies", "rows", "solved", "proven_nodes", "proof_stops", "pruned_plies")}


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("tag,tie,e,games", [
    ("tictactoe", "lowest", 0, 16), ("tictactoe", "random", 0, 16), ("tictactoe", "random", 6, 16),
    ("connect4", "lowest", 0, 16), ("connect4", "random", 3, 16), ("connect4_67", "random", 0, 8),
    ("othello4", "lowest", 0, 16), ("othello4", "random", 3, 16), ("othello4", "lowest", 6, 16),
    ("othello6", "random", 0, 8), ("othello6", "lowest", 3, 8), ("othello6", "random", 6, 8)])
def test_a_wave_is_the_host_models(tag, tie, e, games):
    game, _, H, W = GAMES[tag]
    want, ctr = M.wave(game, H, W, SEED, FIRST, games, N_SIM, e, tie)
    # (TicTacToe at E = 6: everything below a late root is a solved leaf, no walk meets a proven interior node)
    assert ctr["proven_nodes"] > 0 and (ctr["proof_stops"] > 0 or (tag, e) == ("tictactoe", 6)) and (e == 0 or ctr["solved"] > 0)
    eng = fake_engine(tag, tie, games // 2)  # every slot is refilled; 4 or 8 slots: less than a block
    eng.set_proof_backup(True)
    eng.set_exact_endgame(e or None)
    got = ordered(eng.run(games, first_game_id=FIRST))
    same_rows(got, want, (tag, tie, e))
    assert counters(eng) == model_counters(ctr)
    assert eng.stats()["games_done"] == games
    eng.close()


def test_slot_groups_and_slot_counts_do_not_change_a_game():
    outs = []
    for slots, groups in ((32, 1), (32, 2), (32, 4), (8, 1)):
        eng = fake_engine("othello6", "random", slots)
        eng.set_proof_backup(True)
        eng.set_exact_endgame(3)
        eng.set_groups(groups)
        assert eng.groups() == groups
        got = ordered(eng.run(32, first_game_id=FIRST))
        assert eng.stats()["games_done"] == 32
        outs.append((got, counters(eng)))
        eng.close()
    for got, counts in outs[1:]:
        same_rows(got, outs[0][0], "shape")
        assert counts == outs[0][1]
    want, _ = M.wave("othello", 6, 6, SEED, FIRST, 8, N_SIM, 3, "random")  # the first 8 games are test 1's wave
    first = outs[0][0]["meta"][:, 0] < FIRST + 8
    same_rows({k: v[first] for k, v in outs[0][0].items()}, want, "shape against the model")


def othello6_net(max_batch):
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(0)
    net = OthelloNet(n=6).eval()
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    return E.HipNet(0, 6, 6, sd, max_batch=max_batch)


def test_a_real_networks_game_is_the_models_on_its_outputs():
    hip = othello6_net(32)

    def net(grid, player, A):
        x = torch.tensor((player * np.asarray(grid)).astype(np.float32).reshape(1, -1), device="cuda")
        p, v = hip.forward(x)
        return p[0].cpu().numpy(), float(v[0].cpu())
    want, ctr = M.play_wave("othello", 6, 6, SEED, FIRST, 1, 16, 3, True, M.NOISE, "random", M.TMAX, M.TMIN, net=net)
    assert ctr["proven_nodes"] > 0 and ctr["solved"] > 0
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=1, n_sim=16, net=hip, tie_mode=E.TIE_RANDOM, noise_mode=E.NOISE_HASH,
                           dirichlet_alpha=M.NOISE[0], dirichlet_epsilon=M.NOISE[1], temp_max_step=M.TMAX, temp_min_step=M.TMIN, seed=SEED)
    eng.set_proof_backup(True)
    eng.set_exact_endgame(3)
    got = ordered(eng.run(1, first_game_id=FIRST))
    same_rows(got, want, "real network")
    assert counters(eng) == model_counters(ctr)
    eng.close()
    hip.close()


def test_with_the_evaluation_cache_the_samples_stay():
    net = othello6_net(32)
    outs = []
    for cache in (True, False):
        eng = E.SelfPlayEngine(0, 6, 6, n_slots=32, n_sim=16, net=net, seed=SEED)
        eng.set_proof_backup(True)
        eng.set_exact_endgame(3)
        eng.set_eval_cache(cache)
        got = ordered(eng.run(32, first_game_id=FIRST))
        cs, ctr = eng.eval_cache_stats(), counters(eng)
        assert cs["in_force"] == cache and (cs["cache_hits"] > 0) == cache and ctr["proven_nodes"] > 0 and ctr["proof_stops"] > 0
        outs.append((got, ctr))
        eng.close()
    same_rows(outs[0][0], outs[1][0], "cache on / off")
    assert outs[0][1] == outs[1][1]
    net.close()


# ------------------------------------------------------------------------------------------------------------------ 2
# The share of plies with a proven root that the host model finds for these very waves (16 games, 24 simulations, temperature 0, hash
# noise, random ties, SEED): tictactoe 47 / 118 = 0.40, othello4 106 / 202 = 0.52, connect4 102 / 256 = 0.40 -- asserted with the floor in
# tests/test_proof_backup_host.py.  Connect4 4x4 opens with 16 empty cells, four more than solve_batch takes: no root is proven there
# (asserted), every later position is within the limit.
PROVEN_ROOT_FLOOR = 0.10
SOUND = (("tictactoe", 16, 24), ("othello4", 16, 24), ("connect4", 16, 24))


@pytest.mark.parametrize("tag,n,n_sim", SOUND)
def test_a_proven_root_has_the_solvers_outcome_and_the_move_keeps_it(tag, n, n_sim):
    game, gid, H, W = GAMES[tag]
    eng = fake_engine(tag, "random", n, n_sim=n_sim, temp0=True)
    eng.set_proof_backup(True)
    boards = [make_board(game, H, W) for _ in range(n)]
    g, p = X.arrays(boards)
    eng.set_roots(g, p, game_ids=np.arange(FIRST, FIRST + n, dtype=np.uint32))
    live = list(range(n))
    plies = proven = 0
    while live:
        eng.search(n_sim)
        proofs = eng.root_proofs().cpu().numpy()
        moves = eng.player_moves(0.0)
        now = [boards[s] for s in live]
        gg, pp = X.arrays(now)
        sol = E.solve_batch(gid, H, W, torch.from_numpy(gg).cuda(), torch.from_numpy(pp).cuda(), 12)[0].cpu().numpy()
        eng.advance()
        after = []
        for s in live:
            assert moves[s] >= 0
            boards[s].play_move(_move(boards[s], int(moves[s])))
            after.append(boards[s])
        ga, pa = X.arrays(after)
        sol_after = E.solve_batch(gid, H, W, torch.from_numpy(ga).cuda(), torch.from_numpy(pa).cuda(), 12)[0].cpu().numpy()
        for i, s in enumerate(live):
            plies += 1
            if proofs[s] != X.UNSOLVED:
                proven += 1
                assert sol[i] != X.UNSOLVED, (tag, s, "a proven root above solve_batch's limit")
                assert proofs[s] == sol[i], (tag, s, int(proofs[s]), int(sol[i]))
                assert sol_after[i] == sol[i], (tag, s, "the move gave the outcome away", int(sol[i]), int(sol_after[i]))
        assert all(proofs[s] == X.UNSOLVED for s in range(n) if s not in live)  # a slot without a game
        live = [s for s in live if not boards[s].is_game_over()]
    assert eng.stats()["error_flags"] == 0
    assert proven >= PROVEN_ROOT_FLOOR * plies, (tag, proven, plies)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3
# (grid, player, simulations, the root's proven outcome).  A win in one is decided by a terminal child: no walk can end on an F_PROVEN
# node there (proof_stops counts those alone), so that case pins proof_stops == 0; the other three must stop walks on proven nodes.
HAND = {
    "win_in_one": ("tictactoe", [[1, 1, 0], [-1, -1, 0], [0, 0, 0]], 1, 40, 1),
    "loss_in_two": ("tictactoe", [[1, 0, 1], [0, -1, 0], [1, 0, -1]], -1, 40, 1),
    "forced_draw": ("tictactoe", [[0, 1, 1], [0, 0, -1], [-1, 0, 1]], -1, 40, 0),
    "below_a_pass": ("othello6", [[-1, 1, -1, -1, -1, 1], [-1, -1, -1, -1, -1, 0], [0, 1, -1, 1, -1, -1], [1, 1, 1, 1, -1, 0],
                                  [1, 1, 1, 1, 0, -1], [1, 1, 1, 1, 0, 0]], 1, 60, 1),
}


def marks_below_a_pass(m, pass_action):
    n, stack = 0, [(m.root, False)]
    while stack:
        x, below = stack.pop()
        n += 1 if below and id(x) in m.mark else 0
        stack.extend((c, below or c.act == pass_action) for c in x.children)
    return n


@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_built_positions(case):
    tag, grid, player, n_sim, outcome = HAND[case]
    game, gid, H, W = GAMES[tag]
    board = make_board(game, H, W, grid, player)
    m = M.ProofModel(board, 0, True, noise=None, tie="lowest", seed=SEED, game_id=7)
    m.search(n_sim)
    assert m.root_proof() == outcome
    eng = fake_engine(tag, "lowest", 1, n_sim=n_sim, noise=False, temp0=True)
    eng.set_proof_backup(True)
    eng.set_roots(np.array(grid, np.int8)[None], np.array([player], np.int8), game_ids=np.array([7], np.uint32))
    eng.search(n_sim)
    assert eng.root_proofs().cpu().tolist() == [outcome]
    acts, N, Q, P, root_n = eng.root_children(0)
    want = m.root_children()
    assert root_n == n_sim and [(int(a), int(n)) for a, n in zip(acts, N)] == [(a, n) for a, n, _, _ in want]
    assert np.array_equal(Q, np.array([q for _, _, q, _ in want])) and np.array_equal(P, np.array([p for _, _, _, p in want]))
    ro = eng.root_readout(temps=1.0)
    counts, changed = m.counts()
    pi = np.zeros(m.A, np.float32)
    for c, k in zip(m.root.children, counts):
        pi[c.act] = np.float32(float(k) / float(sum(counts)))
    assert np.array_equal(ro["pi"].cpu().numpy()[0], pi)
    vis = np.zeros(m.A, np.int32)
    vis[acts] = N
    assert np.array_equal(ro["visits"].cpu().numpy()[0], vis)  # the visits stay raw
    outs = [m.outcome(c) for c in m.root.children]
    if case == "win_in_one":
        # one visit proves the winning child and the root; every simulation from then on goes there
        assert outs == [1, None, None, None, None] and list(N) == [n_sim, 0, 0, 0, 0] and pi[2] == 1.0 and not changed
    elif case == "loss_in_two":
        assert outs == [1] * 4 and not changed and all(n > 0 for n in N)  # every child loses: none is pruned
    elif case == "forced_draw":
        # three moves lose, one draws: the losers keep the few visits it took to prove them, the target holds the draw alone
        assert outs == [0, 1, 1, 1] and changed and pi[0] == 1.0 and sum(N[1:]) <= 15 and N[0] >= n_sim - 15
    else:
        assert marks_below_a_pass(m, H * W) > 0
    move = eng.player_moves(0.0)[0]
    idx, _, _ = M.move_policy(m, 0.0)
    assert move == m.root.children[idx].act
    ps = eng.proof_backup_stats()
    assert (ps["proven_nodes"], ps["proof_stops"]) == (m.proven_nodes, m.proof_stops)
    assert (ps["proof_stops"] > 0) == (case != "win_in_one")
    eng.advance()
    st = eng.stats()
    # a simulation that ended on a terminal or a proven node took no network row: the rows are the root's prior and the other leaves'
    assert st["net_evals"] == m.rows and st["error_flags"] == 0 and m.rows <= 1 + n_sim - ps["proof_stops"]
    assert eng.proof_backup_stats()["pruned_plies"] == (1 if changed else 0)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4
class _Counting(M.ProofModel):
    """the model, counting the propagations that start below path position 16"""
    long_props = 0

    def _propagate(self, path):
        self.long_props += 1 if len(path) > 16 else 0
        super()._propagate(path)


def test_a_terminal_leaf_beyond_16_path_nodes_is_propagated_by_parent_chasing():
    """an Othello 6x6 root with 17 empty cells, its tree deepened by 60 search calls of 60 simulations: terminal leaves end paths of
    18 nodes, whose backup and proof propagation chase parent pointers (chosen on the CPU: the model's first such leaf is in call 50)"""
    root = [b for b in X.positions("othello", 6, 6, 2, 4, 15, 18) if not b.is_game_over()][2]
    assert X.empties(root) == 17
    m = _Counting(root, 0, True, noise=None, tie="lowest", seed=SEED, game_id=7)
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=1, n_sim=60, evaluator=E.EVAL_FAKE, tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF,
                           dirichlet_alpha=None, dirichlet_epsilon=None, temp_max_step=-1, temp_min_step=0, seed=SEED, node_capacity=1 << 15)
    eng.set_proof_backup(True)
    eng.set_roots(root.grid.astype(np.int8)[None], np.array([root.player], np.int8), game_ids=np.array([7], np.uint32))
    for _ in range(60):
        m.search(60)
        eng.search(60)
    assert m.long_props > 0 and m.max_path > 16, "no terminal leaf on a long path: the test would prove nothing"
    assert eng.stats()["max_path_len"] == m.max_path and eng.stats()["error_flags"] == 0
    acts, N, Q, P, root_n = eng.root_children(0)
    want = m.root_children()
    assert root_n == 3600 and [(int(a), int(n)) for a, n in zip(acts, N)] == [(a, n) for a, n, _, _ in want]
    assert np.array_equal(Q, np.array([q for _, _, q, _ in want])) and np.array_equal(P, np.array([p for _, _, _, p in want]))
    ps = eng.proof_backup_stats()
    assert (ps["proven_nodes"], ps["proof_stops"]) == (m.proven_nodes, m.proof_stops) and m.proven_nodes > 0
    assert eng.root_proofs().cpu().tolist() == [m.root_proof()]
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5
def test_off_is_off():
    outs = []
    for touched in (True, False):
        eng = fake_engine("othello6", "random", 8)
        if touched:
            eng.set_proof_backup(True)
            eng.set_proof_backup(False)
        g, p = X.arrays([make_board("othello", 6, 6)] * 8)
        eng.set_roots(g, p)
        eng.search(N_SIM)
        kids = [eng.root_children(s) for s in range(8)]
        assert eng.root_proofs().cpu().tolist() == [X.UNSOLVED] * 8
        got = ordered(eng.run(16, first_game_id=FIRST))
        st = eng.stats()
        assert eng.proof_backup_stats() == {"proven_nodes": 0, "proof_stops": 0, "pruned_plies": 0}
        outs.append((got, kids, {k: st[k] for k in ("samples", "plies", "net_evals", "games_done", "graph_replays", "lockstep_iters")}))
        eng.close()
    same_rows(outs[0][0], outs[1][0], "on, off, run")
    assert outs[0][2] == outs[1][2]
    for a, b in zip(outs[0][1], outs[1][1]):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    want, _ = M.wave("othello", 6, 6, SEED, FIRST, 16, N_SIM, 0, "random", proof=False)
    same_rows(outs[0][0], want, "mode off against the model")


# ------------------------------------------------------------------------------------------------------------------ 6
def test_refusals_name_the_mode_both_ways():
    L = _lib.lib()
    net = othello6_net(64)

    def net_engine():
        return E.SelfPlayEngine(0, 6, 6, n_slots=8, n_sim=16, net=net, seed=SEED)

    modes = [("leaf_batch", lambda e: e.set_leaf_batch(2), lambda e: e.set_leaf_batch(1)),
             ("Gumbel", lambda e: e.set_gumbel(4), lambda e: e.set_gumbel(None)),
             ("symmetry ensemble", lambda e: e.set_symmetry("all"), lambda e: e.set_symmetry(None)),
             ("random symmetry", lambda e: e.set_symmetry("random"), lambda e: e.set_symmetry(None)),
             ("playout cap", lambda e: e.set_playout_cap((4, 0.5)), lambda e: e.set_playout_cap(None)),
             ("forced playouts", lambda e: e.set_forced_playouts(2.0), lambda e: e.set_forced_playouts(None))]
    for name, on, off in modes:
        eng = net_engine()
        on(eng)
        with pytest.raises(ValueError, match=f"proof backup is not served for .*{name}"):
            eng.set_proof_backup(True)
        off(eng)
        eng.set_proof_backup(True)
        with pytest.raises(ValueError, match="proof backup is on"):
            on(eng)
        eng.set_proof_backup(False)
        on(eng)  # and with the mode off again the other one is accepted
        eng.close()
    for evaluator, name in ((E.EVAL_ROLLOUT, "AZ_EVAL_ROLLOUT"), (E.EVAL_EXTERNAL, "AZ_EVAL_EXTERNAL")):
        eng = E.SelfPlayEngine(0, 6, 6, n_slots=8, n_sim=16, evaluator=evaluator, seed=SEED)
        with pytest.raises(ValueError, match=f"proof backup is not served for .*{name}"):
            eng.set_proof_backup(True)
        eng.set_proof_backup(False)  # off stays accepted
        eng.close()
    eng = fake_engine("othello6", "lowest", 8)
    eng.set_proof_backup(True)   # the modes it composes with are accepted beside it, in either order
    eng.set_exact_endgame(6)
    eng.set_groups(1)
    eng.set_exact_endgame(None)
    eng.set_proof_backup(False)
    for bad in (-1, 2):
        assert L.az_engine_set_proof_backup(eng.h, bad) == _lib.AZ_EINVAL and b"on must be 0 or 1" in L.az_last_error()
    assert L.az_engine_set_proof_backup(None, 1) == _lib.AZ_EINVAL
    assert L.az_engine_proof_backup_stats(eng.h, None, None, None) == _lib.AZ_EINVAL
    assert L.az_engine_root_proofs(eng.h, None) == _lib.AZ_EINVAL
    # state: a search is open; the trees have been searched
    gr, pl = X.arrays([make_board("othello", 6, 6)] * 8)
    eng.set_roots(gr, pl)
    eng.search_begin(4)
    i64 = C.c_int64
    out = torch.empty(8, dtype=torch.int8, device="cuda")
    assert L.az_engine_set_proof_backup(eng.h, 1) == _lib.AZ_ESTATE
    assert L.az_engine_proof_backup_stats(eng.h, C.byref(i64()), C.byref(i64()), C.byref(i64())) == _lib.AZ_ESTATE
    assert L.az_engine_root_proofs(eng.h, out.data_ptr()) == _lib.AZ_ESTATE
    eng.search_end()
    assert L.az_engine_set_proof_backup(eng.h, 1) == _lib.AZ_ESTATE and b"searched trees" in L.az_last_error()
    assert L.az_engine_set_proof_backup(eng.h, 0) == _lib.AZ_OK  # no change: nothing to refuse
    eng.set_roots(gr, pl)
    eng.set_proof_backup(True)
    eng.search(4)
    assert L.az_engine_set_proof_backup(eng.h, 0) == _lib.AZ_ESTATE and b"searched trees" in L.az_last_error()
    assert L.az_engine_set_proof_backup(eng.h, 1) == _lib.AZ_OK
    eng.set_roots(gr, pl)
    eng.set_proof_backup(False)
    eng.close()
    net.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_the_python_surface_plays_the_models_moves():
    """MCT, AlphaZeroPlayer and BatchedAlphaZeroPlayer with proof_backup=True on late Othello 6x6 positions, a real network: the move
    at temperature 0, the visit counts and the root's proof are the host model's on that network's outputs (ties to the lowest action)"""
    from alphazero_amd.games.othello import OthelloNet
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from leaf_batch_model import _act
    torch.manual_seed(4)
    nn = OthelloNet(n=6).eval()
    hip = nn.to_hip(max_batch=16)

    def net(grid, player, A):
        x = torch.tensor((player * np.asarray(grid)).astype(np.float32).reshape(1, -1), device="cuda")
        p, v = hip.forward(x)
        return p[0].cpu().numpy(), float(v[0].cpu())
    boards = [b for b in X.positions("othello", 6, 6, 7, 12, 2, 5) if not b.is_game_over()][:8]  # 2 .. 5 empty cells
    n_sim, models = 60, []
    for b in boards:
        m = M.ProofModel(b, 0, True, noise=None, tie="lowest", net=net)
        m.search(n_sim)
        models.append(m)
    want = [(m.root.children[M.move_policy(m, 0.0)[0]].act, {c.act: c.N for c in m.root.children},
             None if m.root_proof() == X.UNSOLVED else m.root_proof()) for m in models]
    assert sum(w[2] is not None for w in want) >= 2 and any(m.counts()[1] for m in models)  # proofs, and targets they change
    single = AlphaZeroPlayer(n_sim=n_sim, nn=nn, proof_backup=True)
    single.mct._tie_mode = E.TIE_LOWEST
    for b, (act, visits, proof) in zip(boards, want):
        mct = MCT(eval_method="neural", nn=nn, proof_backup=True)
        mct._tie_mode = E.TIE_LOWEST
        mct.search(b, n_sim=n_sim)
        probs, counts = mct.get_action_probs(b, 0)
        assert [_act(b, mv) for mv in probs] == [act] and {_act(b, mv): n for mv, n in counts.items()} == visits
        assert mct.root_proof() == proof
        soft, _ = mct.get_action_probs(b, 1)
        assert abs(sum(soft.values()) - 1.0) < 1e-6
        move, p1, v1, _ = single.get_move(b, 0)
        assert _act(b, move) == act and p1 == {move: 1} and {_act(b, mv): n for mv, n in v1.items()} == visits
        single.reset()
    many = BatchedAlphaZeroPlayer(n_sim=n_sim, nn=nn, n_slots=8, proof_backup=True)
    many._tie_mode = E.TIE_LOWEST
    for b, (move, probs, visits, _), (act, vis, _) in zip(boards, many.get_moves(boards, temps=0), want):
        assert _act(b, move) == act and probs == {move: 1} and {_act(b, mv): n for mv, n in visits.items()} == vis
    assert many._engine.proof_backup_stats()["proven_nodes"] == sum(m.proven_nodes for m in models)
    many.close()
    hip.close()


def test_one_trainer_iteration(tmp_path):
    from alphazero_amd import base
    from alphazero_amd.games.othello import OthelloConfig
    from alphazero_amd.trainer import AlphaZeroTrainer
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    tr = AlphaZeroTrainer(verbose=False, engine_slots=16, seed=6, materialize_memory=True, selfplay_proof_backup=True, selfplay_exact_endgame=3)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=8, episodes=16, epochs=1, batch_size=16, iterations=1, do_eval=False, device="cuda")
    torch.manual_seed(3)
    tr.setup()
    tr.self_play(0)
    ps = tr._engine.proof_backup_stats()
    got = ordered(tr.device_samples)
    assert ps["proven_nodes"] > 0 and ps["pruned_plies"] > 0 and len(got["z"]) == tr._engine.stats()["samples"]
    c = tr.config
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=16, n_sim=8, net=tr._hipnet, dirichlet_alpha=c.dirichlet_alpha, dirichlet_epsilon=c.dirichlet_epsilon,
                           temp_max_step=c.temp_max_step, temp_min_step=c.temp_min_step, seed=6, max_plies=72, sample_capacity=16 * 72)
    eng.set_proof_backup(True)
    eng.set_exact_endgame(3)
    want = ordered(eng.run(16, first_game_id=0))
    assert eng.proof_backup_stats() == ps
    eng.set_proof_backup(False)  # and the wave without the mode records other targets
    plain = ordered(eng.run(16, first_game_id=0))
    eng.close()
    same_rows(got, want, "trainer")
    assert plain["pi"].shape != want["pi"].shape or not np.array_equal(plain["pi"], want["pi"])
    tr.optimize_network(0)
    tr.update_network(0)
    assert tr.loss_values[0] and tr.sgd_backend_used is not None
