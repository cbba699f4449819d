"""MCT with the reference's interface (mcts.py:49-269).

The tree lives on the GPU -- one slot of the HIP self-play engine (csrc/az_engine.hip): `search` runs the
simulations there, `change_root` re-roots / compacts the device tree.

* eval_method "neural": PUCT with the policy/value network (lock-step k_step + network forward).  A shipped network runs as the
  HIP network; any other PolicyValueNetwork, or any object with evaluate(board), evaluates the engine's leaves through an external
  evaluator (alphazero_amd.evaluators decides which).
* eval_method "rollout": plain UCT with random playouts (BASELINE config 1), k_rollout_step -- one launch per
  simulation, no network.

For many games at once use alphazero_amd.engine.SelfPlayEngine / alphazero_amd.arena.BatchedArena directly;
this class is the single-game plugin surface (Arena, interactive play).
"""
from time import time

import numpy as np

from .base import TreeEval
from .utils import fair_max

_GAME_IDS = {"othello": 0, "connect4": 1, "tictactoe": 2}


def _action_of(board, move):
    if board.game == "connect4":
        return int(move)
    w = board.grid.shape[1]
    if board.game == "othello" and tuple(move) == tuple(board.pass_move):
        return w * w
    return int(move[0]) * w + int(move[1])


def _move_of(board, action):
    if board.game == "connect4":
        return np.int64(action)
    w = board.grid.shape[1]
    if board.game == "othello" and action == w * w:
        return board.pass_move
    return (action // w, action % w)


def check_symmetry(symmetry, nn):
    """the mask of `symmetry` (symmetry.parse: an ensemble or a random spec); ValueError -- before any device work -- for a malformed
    one, or when `nn` would evaluate the leaves through an external evaluator (evaluators.route): both modes run on the HIP network only"""
    from .symmetry import parse
    mask, _ = parse(symmetry)
    if mask != 0 and nn is not None:
        from .evaluators import route
        if route(nn) != "hip":
            raise ValueError(f"symmetry={symmetry!r} needs a network the HIP network serves; {type(nn).__name__} evaluates its leaves "
                             f"through an external evaluator, which has no symmetry ensemble")
    return mask


MAX_LEAF_BATCH = 16  # AZ_MAX_LEAF_BATCH (include/az_amd.h)

from .gumbel import check_gumbel, check_gumbel_batch, check_gumbel_full  # noqa: E402  (the Gumbel root search's spec and refusals)
from .endgame import check_exact_endgame  # noqa: E402  (exact endgames' spec and refusals)
from .proof import check_proof_backup  # noqa: E402  (proof backup's spec and refusals)
from .puct import OFF as PUCT_OFF, check_puct, is_on as puct_is_on  # noqa: E402  (the PUCT exploration settings' spec and refusals)


def check_leaf_batch(leaf_batch, nn, symmetry=None, neural=True):
    """the walkers per lock-step of `leaf_batch` (None: 1); ValueError -- before any device work -- for a bool, a non-integer or a
    value outside 1..16, and for a value above 1 with a network evaluated through an external evaluator (evaluators.route), a
    rollout-mode tree (`neural` False) or a symmetry ensemble: virtual-loss batching runs on the HIP network's plain evaluation, or
    with one random symmetry per evaluation (a "random" spec), only"""
    if leaf_batch is None:
        return 1
    if isinstance(leaf_batch, (bool, np.bool_)) or not isinstance(leaf_batch, (int, np.integer)):
        raise ValueError(f"leaf_batch must be an integer in 1..{MAX_LEAF_BATCH}, got {leaf_batch!r}")
    k = int(leaf_batch)
    if not 1 <= k <= MAX_LEAF_BATCH:
        raise ValueError(f"leaf_batch must be in 1..{MAX_LEAF_BATCH}, got {k}")
    if k > 1:
        if not neural:
            raise ValueError(f"leaf_batch={k} needs eval_method 'neural': random playouts evaluate no leaf with a network")
        if nn is not None:
            from .evaluators import route
            if route(nn) != "hip":
                raise ValueError(f"leaf_batch={k} needs a network the HIP network serves; {type(nn).__name__} evaluates its leaves "
                                 f"through an external evaluator, which takes one leaf per lock-step")
        from .symmetry import parse
        mask, rnd = parse(symmetry)
        if mask != 0 and not rnd:
            raise ValueError(f"leaf_batch={k} does not combine with symmetry={symmetry!r}")
    return k


class MCT:
    def __init__(self, eval_method=None, nn=None, dirichlet_alpha=None, dirichlet_epsilon=None, seed=None, symmetry=None,
                 leaf_batch=None, gumbel=None, gumbel_batch=1, gumbel_full=False, exact_endgame=None, proof_backup=False, puct=None):
        self.n_rollouts = 0
        self.simulation_time = 0
        self.eval_method = TreeEval.to_dict()["rollout" if eval_method is None else eval_method]
        self._nn = nn
        self.dirichlet_alpha = dirichlet_alpha
        self.dirichlet_epsilon = dirichlet_epsilon
        if self._nn is not None and self.eval_method != TreeEval.NEURAL:
            raise ValueError(f"A neural network has been set for the MCT but the evaluation method is {self.eval_method}")
        self._seed = int(np.random.randint(0, 2**31 - 1)) if seed is None else int(seed)
        self._engine = None           # device tree (one engine slot)
        self._engine_board = None     # (game, H, W) the engine was built for
        self._engine_lb = 1           # the leaf_batch the engine is set to
        self._hipnet = None
        self._evaluator = None        # external evaluator of a network the HIP net does not serve (evaluators.route)
        self._root_key = None         # (grid bytes, player) of the position the device root stands for
        self._last_board = None
        self._tie_mode = None         # tests: engine.TIE_LOWEST (None: fair_max draws among equals, utils.py:28-34)
        self._noise_mode = None       # tests: engine.NOISE_HASH (None: Dirichlet noise from the Philox stream)
        # leaf evaluations averaged over the board's symmetries, or ("random") each in one drawn at random (alphazero_amd.symmetry;
        # None: off); HIP-routed networks only
        self.symmetry = symmetry
        check_symmetry(symmetry, self._nn)
        # simulations per lock-step, kept apart by virtual loss (None / 1: the reference's sequential search); HIP-routed networks only
        self.leaf_batch = leaf_batch
        check_leaf_batch(leaf_batch, self._nn, symmetry, self.eval_method == TreeEval.NEURAL)
        # the Gumbel root search (alphazero_amd.gumbel: None = off, an int m or a dict): Sequential Halving at the root, move and
        # action probabilities from the completed Q-values; n_sim searches on HIP-routed networks at leaf_batch 1 only
        self.gumbel = gumbel
        self._engine_gumbel = None    # the spec the engine is set to
        check_gumbel(gumbel, self._nn, leaf_batch, self.eval_method == TreeEval.NEURAL)
        # Sequential Halving leaves per lock-step of the Gumbel root search (1: one); needs `gumbel`, not symmetry "all"
        self.gumbel_batch = gumbel_batch
        self._engine_gb = 1           # the gumbel_batch the engine is set to
        check_gumbel_batch(gumbel_batch, gumbel, symmetry)
        # the full Gumbel search: the paper's v_mix with every node's own network value and its deterministic
        # selection below the root; needs `gumbel`
        self.gumbel_full = gumbel_full
        self._engine_gf = False       # the gumbel_full the engine is set to
        check_gumbel_full(gumbel_full, gumbel)
        # exact endgames (alphazero_amd.endgame: None = off, or E in 1..10): a leaf with at most E empty cells is solved, not evaluated;
        # the plain PUCT search on HIP-routed networks only
        self.exact_endgame = exact_endgame
        self._engine_exact = None     # the E the engine is set to
        check_exact_endgame(exact_endgame, self._nn, symmetry, leaf_batch, gumbel, self.eval_method == TreeEval.NEURAL)
        # proof backup (alphazero_amd.proof: a bool): a node is proven as soon as its children decide it, proven nodes are not searched
        # again, move and action probabilities respect the proofs; the plain PUCT search on HIP-routed networks only
        self.proof_backup = proof_backup
        self._engine_proof = False    # whether the engine has the mode on
        check_proof_backup(proof_backup, self._nn, symmetry, leaf_batch, gumbel, self.eval_method == TreeEval.NEURAL)
        # the PUCT exploration settings (alphazero_amd.puct: None, c_init or a dict of c_init, c_base, fpu): the exploration constant, its
        # growth with the parent's visits and first-play urgency; the plain PUCT search on HIP-routed networks only
        self.puct = puct
        self._engine_puct = PUCT_OFF  # the triple the engine is set to
        check_puct(puct, self._nn, symmetry, leaf_batch, gumbel, exact_endgame, proof_backup, self.eval_method == TreeEval.NEURAL)

    # ------------------------------------------------------------------ reference surface
    @property
    def nn(self):
        return self._nn

    @nn.setter
    def nn(self, nn):
        if self.eval_method != TreeEval.NEURAL:
            raise ValueError(f"Trying to set a neural network for the MCT but the evaluation method is {self.eval_method}")
        check_symmetry(self.symmetry, nn)
        check_leaf_batch(self.leaf_batch, nn, self.symmetry)
        check_gumbel(self.gumbel, nn, self.leaf_batch)
        check_exact_endgame(self.exact_endgame, nn, self.symmetry, self.leaf_batch, self.gumbel)
        check_proof_backup(self.proof_backup, nn, self.symmetry, self.leaf_batch, self.gumbel)
        check_puct(self.puct, nn, self.symmetry, self.leaf_batch, self.gumbel, self.exact_endgame, self.proof_backup)
        self._nn = nn
        self._hipnet = None
        self._evaluator = None
        self._engine = None
        self._root_key = None

    def get_stats(self):
        return self.n_rollouts, self.simulation_time

    def search(self, board, n_sim=None, compute_time=None):
        self.n_rollouts = 0
        start = time()
        if n_sim is None and compute_time is None:
            raise ValueError("MCT.search needs to have either n_sim or compute_time specified.")
        check_gumbel(self.gumbel, self._nn, self.leaf_batch, self.eval_method == TreeEval.NEURAL, compute_time)
        check_gumbel_batch(self.gumbel_batch, self.gumbel, self.symmetry)
        check_gumbel_full(self.gumbel_full, self.gumbel)
        self._sync_device_root(board, n_sim)
        if n_sim is not None:
            self._ensure_room(n_sim)
            self._device_search(n_sim)
            self.n_rollouts = n_sim
        else:
            # one lock-step per chunk: a simulation, or leaf_batch of them
            chunk = check_leaf_batch(self.leaf_batch, None) if self.eval_method == TreeEval.NEURAL else 8
            # at least one chunk: the clock started before _sync_device_root, which may have built the engine (longer than a short budget),
            # and a root without a visit has no move to return
            while self.n_rollouts == 0 or time() - start < compute_time:
                self._ensure_room(chunk)
                self._device_search(chunk)
                self.n_rollouts += chunk
        self.simulation_time = time() - start

    def get_prior_probs(self):
        a, _, _, p, _ = self._children()
        if self.eval_method != TreeEval.NEURAL:
            return {_move_of(self._last_board, int(ai)): None for ai in a}
        return {_move_of(self._last_board, int(ai)): float(pi) for ai, pi in zip(a, p)}

    def get_action_probs(self, board, temp=0):
        a, n, _, _, _ = self._children()
        counts = {_move_of(board, int(ai)): int(ni) for ai, ni in zip(a, n)}
        if len(counts) == 0:
            return {board.pass_move: 1.}
        if self.gumbel is not None:
            # the move and the improved policy of the Gumbel root search, as the engine would record and play them (a one-row
            # readout); a temperature other than 0 returns the policy, renormalised in float64 for the caller's draw
            r = self._engine.root_readout(temps=0, n=1)
            if temp == 0:
                return {_move_of(board, int(r["action"][0])): 1}, counts
            pi = r["pi"][0].cpu().numpy().astype(np.float64)
            total = float(sum(pi[int(ai)] for ai in a))
            return {_move_of(board, int(ai)): float(pi[int(ai)]) / total for ai in a}, counts
        if self._engine_proof:
            # the move and the policy on the counts the proofs leave (a proven win's alone, or without the proven losses), as the
            # engine would record and play them (a one-row readout); renormalised in float64 for the caller's draw
            r = self._engine.root_readout(temps=float(temp), n=1)
            if temp == 0:
                return {_move_of(board, int(r["action"][0])): 1}, counts
            pi = r["pi"][0].cpu().numpy().astype(np.float64)
            total = float(sum(pi[int(ai)] for ai in a))
            return {_move_of(board, int(ai)): float(pi[int(ai)]) / total for ai in a}, counts
        if temp == 0:
            best, _ = fair_max(counts.items(), key=lambda kv: kv[1])
            return {best: 1}, counts
        powered = {m: c ** (1. / temp) for m, c in counts.items()}
        total = sum(powered.values())
        return {m: v / total for m, v in powered.items()}, counts

    def root_proof(self):
        """the proven outcome of the searched root -- the winner's player id, 0 for a draw -- or None while it is not decided
        (proof_backup; engine.root_proofs)"""
        from .endgame import UNSOLVED
        if self._engine is None or self._root_key is None:
            return None
        w = int(self._engine.root_proofs()[0])
        return None if w == UNSOLVED else w

    def change_root(self, move):
        if self._engine is None or self._root_key is None:
            return  # no device tree yet: the next search starts from the board it is given
        b = self._last_board.clone()
        b.play_move(move)  # raises ValueError for an illegal move, like the engine would
        self._engine.play([_action_of(self._last_board, move)])
        self._last_board = b
        self._root_key = (b.grid.astype(np.int8).tobytes(), int(b.player))

    # ------------------------------------------------------------------ device tree
    def _device_search(self, n_sim):
        try:
            self._engine.search(n_sim)
        except BaseException:
            if self._evaluator is not None:
                # a failed external evaluation leaves leaves in the device tree that were never evaluated (the engine then
                # accepts set_roots / run only): the next search starts the tree afresh from the board it is given
                self._root_key = None
            raise

    def _children(self):
        if self._engine is None:
            return [], [], [], [], 0
        return self._engine.root_children(0)

    def _sync_device_root(self, board, n_sim=None):
        from .engine import EVAL_EXTERNAL, EVAL_NET, EVAL_ROLLOUT, NOISE_OFF, NOISE_PHILOX, TIE_RANDOM, SelfPlayEngine
        from .evaluators import check_game, check_normalizer, make_evaluator, route
        from .symmetry import members, parse
        check_game(board)
        neural = self.eval_method == TreeEval.NEURAL
        if neural and self._nn is None:
            raise ValueError("The MCT has no neural network to evaluate positions with.")
        if neural:
            check_normalizer(self._nn)
        H, W = board.grid.shape
        if self._engine is not None and self._engine_board != (board.game, H, W):
            # the device storage was carried over a reset() from a game on another board (players.py keeps the engine); the
            # reference's reset() yields a tree usable on any board: rebuild rather than search with the wrong rules
            self._engine.close()
            self._engine, self._root_key = None, None
            if self._hipnet is not None and (self._hipnet.H, self._hipnet.W) != (H, W):
                self._hipnet = None
        if self._engine is None:
            external = neural and route(self._nn) != "hip"
            sym = members(board.game, H, W, check_symmetry(self.symmetry, self._nn if neural else None))
            if sym and not neural:
                raise ValueError("symmetry needs eval_method 'neural': random playouts evaluate no leaf")
            check_leaf_batch(self.leaf_batch, self._nn if neural else None, self.symmetry, neural)
            if neural and not external and self._hipnet is None:
                self._hipnet = self._nn.to_hip(max_batch=16)  # >= the 8 twins / the 16 walkers of the one slot
            noisy = self.dirichlet_alpha is not None and self.dirichlet_epsilon is not None
            self._engine = SelfPlayEngine(_GAME_IDS[board.game], H, W, n_slots=1, n_sim=1, net=None if external else self._hipnet,
                                          dirichlet_alpha=self.dirichlet_alpha, dirichlet_epsilon=self.dirichlet_epsilon,
                                          temp_max_step=-1, temp_min_step=0, tie_mode=TIE_RANDOM if self._tie_mode is None else self._tie_mode,
                                          noise_mode=(NOISE_PHILOX if noisy else NOISE_OFF) if self._noise_mode is None else self._noise_mode,
                                          evaluator=EVAL_EXTERNAL if external else (EVAL_NET if neural else EVAL_ROLLOUT),
                                          seed=self._seed, sample_capacity=4 * H * W + 16, max_plies=4 * H * W + 16,
                                          # one slot: the pools start small and grow on demand (_ensure_room)
                                          node_capacity=1 << 14)
            if external:
                self._evaluator = make_evaluator(self._nn, board.game, H, W)
                self._engine.set_evaluator(self._evaluator)
            if sym:
                self._engine.set_symmetry(("random", sym) if parse(self.symmetry)[1] else sym)
            self._engine_board = (board.game, H, W)
            self._plies = 0
            self._engine_lb = 1
            self._engine_gumbel = None
            self._engine_gb = 1
            self._engine_gf = False
            self._engine_exact = None
            self._engine_proof = False
            self._engine_puct = PUCT_OFF
        pu = check_puct(self.puct, self._nn if neural else None, self.symmetry, self.leaf_batch, self.gumbel, self.exact_endgame,
                        self.proof_backup, neural)
        if self._engine_puct != pu and not puct_is_on(pu):  # off before a mode it excludes may come on (no node depends on the settings)
            self._engine.set_puct(None)
            self._engine_puct = pu
        ex = check_exact_endgame(self.exact_endgame, self._nn if neural else None, self.symmetry, self.leaf_batch, self.gumbel, neural)
        if self._engine_exact is not None and ex is None:  # off before a mode it excludes may come on
            self._root_key = None  # over a fresh tree only: the kept one was searched under the old value
            self._engine.set_roots(board.grid.astype(np.int8)[None], np.array([board.player], np.int8))
            self._engine.set_exact_endgame(None)
            self._engine_exact = None
        pb = check_proof_backup(self.proof_backup, self._nn if neural else None, self.symmetry, self.leaf_batch, self.gumbel, neural)
        if self._engine_proof and not pb:  # likewise: off over a fresh tree, before a mode it excludes may come on
            self._root_key = None
            self._engine.set_roots(board.grid.astype(np.int8)[None], np.array([board.player], np.int8))
            self._engine.set_proof_backup(False)
            self._engine_proof = False
        lb = check_leaf_batch(self.leaf_batch, self._nn if neural else None, self.symmetry, neural)
        if self._engine_lb != lb:
            self._engine.set_leaf_batch(lb)
            self._engine_lb = lb
        gum = check_gumbel(self.gumbel, self._nn if neural else None, self.leaf_batch, neural)
        gf = check_gumbel_full(self.gumbel_full, self.gumbel)
        if self._engine_gf and not gf:  # off before the mode may change: the switch never comes into force with set_gumbel
            self._engine.set_gumbel_full(False)
            self._engine_gf = False
        if self._engine_gumbel != gum:
            self._engine.set_gumbel(self.gumbel)
            self._engine_gumbel = gum
        gb = check_gumbel_batch(self.gumbel_batch, self.gumbel, self.symmetry)
        if self._engine_gb != gb:
            self._engine.set_gumbel_batch(gb)
            self._engine_gb = gb
        key = (board.grid.astype(np.int8).tobytes(), int(board.player))
        if self._engine_exact != ex or self._engine_proof != pb:
            self._root_key = None  # the engine refuses a change over a searched tree: start it afresh
        if key != self._root_key:  # tree restarted from an unexplored state (mcts.py:124-125, 231-233)
            self._engine.set_roots(board.grid.astype(np.int8)[None], np.array([board.player], np.int8),
                                   game_ids=np.array([np.random.randint(0, 2**31 - 1)], np.uint32))
            self._root_key = key
            self._used_bound = 1  # a fresh tree: the root
        if self._engine_exact != ex:
            self._engine.set_exact_endgame(ex)
            self._engine_exact = ex
        if self._engine_proof != pb:
            self._engine.set_proof_backup(pb)
            self._engine_proof = pb
        if self._engine_puct != pu:  # on, or other values: after every mode it excludes has gone off; the kept tree stays
            self._engine.set_puct({"c_init": pu[0], "c_base": pu[1], "fpu": pu[2]})
            self._engine_puct = pu
        if self._engine_gf != gf:  # on after set_roots: a fresh tree holds no node evaluated without its value; a kept one is refused
            self._engine.set_gumbel_full(gf)
            self._engine_gf = gf
        self._last_board = board.clone()

    _MAX_POOL = 1 << 24  # nodes per pool (512 MiB): beyond it the engine reports AZ_ECAPACITY

    def _ensure_room(self, n_sim):
        """the reference's tree grows without bound while search() is called again and again on one root (mcts.py:226-269);
        the device pools have a size: before a search of n_sim simulations (each allocates at most one node's children, <= A <= 65
        nodes) the pools are re-allocated when what is left could run out.  The tree is kept (az_engine_grow_pools).

        The device is only asked for the node count (a stream synchronisation + a blocking copy) when a HOST-side upper bound --
        the last count read plus 66 nodes per simulation since -- nears the capacity: a compute_time search of one simulation per
        chunk would otherwise pay that round trip per simulation.  A tree that cannot fit the largest pool is refused up front."""
        eng = self._engine
        cap = eng.cfg.node_capacity
        self._used_bound = getattr(self, "_used_bound", cap) + 66 * n_sim
        if self._used_bound + 66 <= cap:
            return
        need = eng.nodes_used(0) + 66 * n_sim + 66
        self._used_bound = need - 66
        if need > cap:
            if need > self._MAX_POOL:
                raise MemoryError(f"MCT.search: the tree would need {need} nodes, beyond the device pool limit of {self._MAX_POOL} "
                                  f"(the search has run {need // 66} simulations' worth of expansions on one root without a move)")
            eng.grow_pools(min(self._MAX_POOL, max(2 * cap, need + 66 * 1024)))  # one growth covers many chunks
