"""Host model of BatchedArena with its players in the search modes: the existing slot models -- leaf_batch_model.Model,
RandomSymmetryModel, GumbelModel / GumbelBatchModel / GumbelFullModel -- driven as Arena.play_game and BatchedArena._play drive their
players.  A plain restatement of the contract for tests.  Not a conftest, not a test module.

What is added to the slot models:
  apply(model, action)   k_apply_moves' rule for a move chosen outside the tree's own search: the root's child that holds the action
                         becomes the root if the root is expanded, else a fresh root is made on the new board; ply + 1, sim_base 0, an
                         empty candidate set
  sampled_index(N, u)    the visit-based move at temperature 1 (move_policy): p = N / sum N in float64 in child-index order, running
                         sum, the first child with u < cum; u = cf.move_sample_u(seed, game id, ply); no draw for a single child
  arena_games(...)       the driver: game id (round + seed * 100003) mod 2^32, engine seeds `seed` and `seed + 1`, colour +1 moves first,
                         both trees receive every move, the side to move searches its n_sim and plays the move of its mode
Opening rule (opening_plies = k; the ply is the root's, passes count): a visit-based tree player plays sampled_index while ply < k and
the most visited child from ply k on; a Gumbel player has gumbel_scale s (the spec's, 1.0 where that is 0) while ply < k and 0 from
ply k on; k = None switches nothing."""
from collections import defaultdict

from alphazero_amd import gumbel as G
from alphazero_amd.symmetry import parse as parse_symmetry
from gumbel_full_model import GumbelFullModel
from leaf_batch_model import Model, Node, _move, make_board
from symmetry_random_model import RandomSymmetryModel
from tools import closed_form as cf

SPEC_DEFAULTS = {"symmetry": None, "leaf_batch": None, "gumbel": None, "gumbel_batch": 1, "gumbel_full": False}


class RandomSymmetryGumbelModel(RandomSymmetryModel, GumbelFullModel):
    """the Gumbel models with one symmetry drawn per evaluation: RandomSymmetryModel's bookkeeping of the simulation that first picks
    a node, on top of GumbelFullModel's walk (walker j of a lock-step at cursor s is simulation s + j)"""


def fill(spec):
    out = dict(SPEC_DEFAULTS)
    out.update(spec or {})
    return out


def opening_scale(gumbel, opening_plies, ply):
    """gumbel_scale of a Gumbel player at the root's `ply`"""
    gs = G.parse(gumbel)[3]
    if opening_plies is None:
        return gs
    return (gs if gs != 0.0 else 1.0) if ply < opening_plies else 0.0


def make_model(board, spec, opening_plies, tie, seed, game_id, net=None):
    """the slot model of a network player in the modes of `spec` (None: the plain PUCT search), at ply 0"""
    spec = fill(spec)
    rnd = parse_symmetry(spec["symmetry"])[1]
    if spec["symmetry"] is not None and not rnd:
        raise ValueError("the model restates the random symmetry mode only")
    kw = dict(tie=tie, seed=seed, game_id=game_id, net=net)
    if spec["gumbel"] is None:
        return (RandomSymmetryModel if rnd else Model)(board, K=spec["leaf_batch"] or 1, **kw)
    m, cv, cs, _ = G.parse(spec["gumbel"])
    cls = RandomSymmetryGumbelModel if rnd else GumbelFullModel
    return cls(board, K=spec["gumbel_batch"], full=spec["gumbel_full"], m=m, c_visit=cv, c_scale=cs,
               gumbel_scale=opening_scale(spec["gumbel"], opening_plies, 0), **kw)


def apply(model, action):
    """k_apply_moves on one slot: Board.play_move + MCT.change_root for a move chosen outside this tree's search"""
    root, new = model.root, None
    if root.expanded:
        for c in root.children:
            if c.act == action:
                new = c
    if new is not None:
        model._board(new)
        new.parent = None
    else:
        b = model._board(root).clone()
        b.play_move(_move(b, action))
        new = Node(0, None, 0.0, False)
        new.board = b
    model.root, model.ply, model.sim_base = new, model.ply + 1, 0
    if hasattr(model, "mask"):
        model.mask = []


def sampled_index(counts, u):
    """move_policy at temperature 1 over the children's visit counts; u: the move-sample draw (not read for a single child)"""
    nc = len(counts)
    if nc == 1:
        u = 2.0
    total = 0.0
    for n in counts:
        total += float(n)
    cum, chosen, last = 0.0, None, 0
    for i, n in enumerate(counts):
        p = float(n) / total
        if p > 0.0:
            last = i
        cum += p
        if chosen is None and u < cum:
            chosen = i
    if chosen is None:
        chosen = 0 if nc == 1 else last
    return chosen


def most_visited_index(model):
    """move_policy at temperature 0: fair_max by N under the model's tie mode (the AZ_P_TIE_MOVE draw)"""
    ch = model.root.children
    best = max(c.N for c in ch)
    ties = [i for i, c in enumerate(ch) if c.N == best]
    k = 0
    if model.tie == "random" and len(ties) > 1:
        k = (cf.philox4x32(model.seed, model.gid, model.ply, 0xFFFF, cf.P_TIE_MOVE, 0)[0] * len(ties)) >> 32
    return ties[k]


def player_move(model, temp):
    """SelfPlayEngine.player_moves(temp) for one searched slot: the Gumbel move in the Gumbel mode, else the visit-based move"""
    ch = model.root.children
    if isinstance(model, GumbelFullModel):
        return ch[model.move_index()].act
    if temp == 0.0:
        return ch[most_visited_index(model)].act
    assert temp == 1.0
    return ch[sampled_index([c.N for c in ch], cf.move_sample_u(model.seed, model.gid, model.ply))].act


def _baseline(board, kind, seed, game_id, ply, tie):
    """RandomPlayer / GreedyPlayer on the oracle (oracle.baseline_move), from the mirror board's grid"""
    import ctypes as C
    from oracle import oracle as O
    H, W = board.grid.shape
    b = O.new_board(O.GAME_IDS[board.game], H, W)
    for r in range(H):
        for c in range(W):
            b.grid[r * W + c] = int(board.grid[r, c])
    b.player = int(board.player)
    return O.baseline_move(b, kind, seed, game_id, ply, O.TIE_RANDOM if tie == "random" else O.TIE_LOWEST)


def play_round(game, H, W, rnd, seed, p2_starts, n_sim, opp_sim, search=None, opponent="fake", opponent_search=None, opening_plies=None,
               tie="lowest", net1=None, net2=None, bind1=None, bind2=None, trace=None):
    """one round: (moves, winner colour, |score|).  opponent: "fake" / "net" (a tree player on net2, the closed-form network when None),
    "random" or "greedy".  bind1 / bind2(model) -> the net of that model (a network that needs to read the model, as the random
    symmetry mode does).  trace: a list that receives (ply, player 1 or 2, the model's gumbel_scale or None, its candidate set)."""
    side1 = -1 if p2_starts else 1
    gid = (rnd + seed * 100003) & 0xFFFFFFFF
    board = make_board(game, H, W)
    t1 = make_model(board, search, opening_plies, tie, seed, gid, net1)
    if bind1 is not None:
        t1.net = bind1(t1)
    t2 = None
    if opponent not in ("random", "greedy"):
        t2 = make_model(board, opponent_search, opening_plies, tie, seed + 1, gid, net2)
        if bind2 is not None:
            t2.net = bind2(t2)
    k = opening_plies
    ply, moves = 0, []
    while not board.is_game_over():
        if k is not None and k > 0 and ply == k:  # one set_gumbel between the plies k - 1 and k
            for t in (t1, t2):
                if isinstance(t, GumbelFullModel):
                    t.gs, t.mask = 0.0, []
        temp = 1.0 if k is not None and ply < k else 0.0
        mine = board.player == side1
        if mine or t2 is not None:
            t, ns = (t1, n_sim) if mine else (t2, opp_sim)
            assert t.ply == ply
            t.search(ns)
            a = player_move(t, temp)
            if trace is not None:
                trace.append((ply, 1 if mine else 2, getattr(t, "gs", None), list(getattr(t, "mask", []))))
        else:
            a = _baseline(board, opponent, seed + 7, gid, ply, tie)
        board.play_move(cf.action_to_move(game, a, H))
        apply(t1, a)
        if t2 is not None:
            apply(t2, a)
        moves.append(a)
        ply += 1
    return moves, int(board.get_winner()), abs(board.get_score())


def arena_games(game, H, W, n_sim, opp_sim, seed, n_rounds, start_player=None, rounds=None, **kw):
    """BatchedArena.play_games on the models: (moves per game, winners, scores, the stats dict of arena.py:141-147).  `rounds`: play
    only these round indices (a round is a function of (seed, round, the specs, opening_plies) alone)."""
    p2_starts = [{1: False, 2: True}.get(start_player, bool(r % 2)) for r in range(n_rounds)]
    played = list(range(n_rounds)) if rounds is None else [int(r) for r in rounds]
    all_moves, winners, scores = [], [], []
    for r in played:
        mv, w, sc = play_round(game, H, W, r, seed, p2_starts[r], n_sim, opp_sim, **kw)
        all_moves.append(mv); winners.append(w); scores.append(sc)
    stats = {"player1": [], "player2": [], "draw": 0, "player1_starts": defaultdict(int), "player2_starts": defaultdict(int)}
    for i, r in enumerate(played):
        starter = f"player{2 if p2_starts[r] else 1}_starts"
        if winners[i] == 0:
            stats["draw"] += 1
            stats[starter]["draw"] += 1
        else:
            who = 1 if winners[i] == (-1 if p2_starts[r] else 1) else 2
            stats[f"player{who}"].append(scores[i])
            stats[starter]["win" if who == (2 if p2_starts[r] else 1) else "loss"] += 1
    return all_moves, winners, scores, stats
