"""Players (players.py:76-247).  HumanPlayer (interactive stdin) is out of scope.

BatchedMCTSPlayer / BatchedAlphaZeroPlayer answer get_move for many boards at once: one search over all of them and one root
readout (SelfPlayEngine.root_readout) instead of one device round trip per game."""
from time import sleep

import numpy as np

from .base import Player
from .gumbel import check_gumbel, check_gumbel_batch, check_gumbel_full
from .endgame import check_exact_endgame
from .proof import check_proof_backup
from .puct import check_puct, is_on as puct_is_on
from .mcts import MCT, _action_of, _move_of, check_leaf_batch, check_symmetry
from .utils import fair_max


class RandomPlayer(Player):
    def __init__(self, lock_time=None, verbose=False):
        super().__init__(verbose=verbose)
        self.lock_time = lock_time

    def clone(self):
        return RandomPlayer(lock_time=self.lock_time, verbose=self.verbose)

    def get_move(self, board, temp=None):
        if self.lock_time is not None:
            sleep(self.lock_time)
        return board.get_random_move(), None, None, None


class GreedyPlayer(Player):
    """picks the move with the best immediate score (players.py:97-123)"""

    def clone(self):
        return GreedyPlayer(verbose=self.verbose)

    def get_move(self, board, temp=None):
        scored = {}
        for move in board.get_moves():
            after = board.clone()
            after.play_move(move)
            scored[move] = -after.get_score()
        return fair_max(scored.items(), key=lambda kv: kv[1])[0], None, None, None


class MCTSPlayer(Player):
    def __init__(self, n_sim=None, compute_time=None, verbose=False):
        super().__init__(verbose=verbose)
        self.n_sim, self.compute_time = n_sim, compute_time
        if self.n_sim is None and self.compute_time is None:
            raise ValueError("MCTSPlayer needs to have either n_sim or compute_time specified.")
        if self.n_sim is not None and self.compute_time is not None:
            raise ValueError("MCTSPlayer can't have both n_sim and compute_time specified.")
        self.mct = MCT()

    def clone(self):
        return MCTSPlayer(n_sim=self.n_sim, compute_time=self.compute_time, verbose=self.verbose)

    def reset(self):
        old = self.mct
        self.mct = MCT()
        # a reset drops the tree, not the device storage behind it (one engine slot: node pools, sample buffers)
        self.mct._engine, self.mct._engine_board, self.mct._engine_lb = old._engine, old._engine_board, old._engine_lb

    def apply_move(self, move, player=None):
        self.mct.change_root(move)

    def get_move(self, board, temp=0):
        if board.is_game_over():
            raise ValueError(f"{self}.get_move was called with a board in game over state...")
        self.mct.search(board=board, n_sim=self.n_sim, compute_time=self.compute_time)
        action_probs, visit_counts = self.mct.get_action_probs(board, temp)
        items = list(action_probs.items())
        if len(items) == 1:
            best = items[0][0]
        else:
            best = items[np.random.choice(len(items), p=[p for _, p in items])][0]
        return best, action_probs, visit_counts, self.mct.get_prior_probs()

    def get_stats_after_move(self):
        n_rollouts, simulation_time = self.mct.get_stats()
        return {"n_rollouts": n_rollouts, "time": simulation_time}


class AlphaZeroPlayer(MCTSPlayer):
    def __init__(self, n_sim=None, compute_time=None, nn=None, dirichlet_alpha=None, dirichlet_epsilon=None, verbose=False,
                 symmetry=None, leaf_batch=None, gumbel=None, gumbel_batch=1, gumbel_full=False, exact_endgame=None, proof_backup=False,
                 puct=None):
        super().__init__(n_sim=n_sim, compute_time=compute_time, verbose=verbose)
        check_gumbel(gumbel, nn, leaf_batch, True, compute_time)
        check_gumbel_batch(gumbel_batch, gumbel, symmetry)
        check_gumbel_full(gumbel_full, gumbel)
        check_exact_endgame(exact_endgame, nn, symmetry, leaf_batch, gumbel)
        check_proof_backup(proof_backup, nn, symmetry, leaf_batch, gumbel)
        check_puct(puct, nn, symmetry, leaf_batch, gumbel, exact_endgame, proof_backup)
        self.mct = MCT(eval_method="neural", nn=nn, dirichlet_alpha=dirichlet_alpha, dirichlet_epsilon=dirichlet_epsilon,
                       symmetry=symmetry, leaf_batch=leaf_batch, gumbel=gumbel, gumbel_batch=gumbel_batch, gumbel_full=gumbel_full,
                       exact_endgame=exact_endgame, proof_backup=proof_backup, puct=puct)

    @property
    def puct(self):
        """the PUCT exploration settings (alphazero_amd.puct; None: off)"""
        return self.mct.puct

    @property
    def proof_backup(self):
        """proof backup (alphazero_amd.proof; False: off)"""
        return self.mct.proof_backup

    @property
    def exact_endgame(self):
        """exact endgames' E (alphazero_amd.endgame; None: off)"""
        return self.mct.exact_endgame

    @property
    def gumbel(self):
        """the Gumbel root search's spec (alphazero_amd.gumbel; None: the PUCT root)"""
        return self.mct.gumbel

    @property
    def gumbel_batch(self):
        """Sequential Halving leaves per lock-step of the Gumbel root search (1: one)"""
        return self.mct.gumbel_batch

    @property
    def gumbel_full(self):
        """the full Gumbel search: the paper's v_mix and its deterministic selection below the root (False: the root only)"""
        return self.mct.gumbel_full

    @property
    def symmetry(self):
        """the symmetries every leaf evaluation is averaged over (alphazero_amd.symmetry; None: off)"""
        return self.mct.symmetry

    @property
    def leaf_batch(self):
        """simulations per lock-step, kept apart by virtual loss (None / 1: the sequential search)"""
        return self.mct.leaf_batch

    def clone(self):
        return AlphaZeroPlayer(n_sim=self.n_sim, compute_time=self.compute_time,
                               nn=self.mct.nn.clone() if self.mct.nn is not None else None,
                               dirichlet_alpha=self.mct.dirichlet_alpha, dirichlet_epsilon=self.mct.dirichlet_epsilon,
                               verbose=self.verbose, symmetry=self.mct.symmetry, leaf_batch=self.mct.leaf_batch,
                               gumbel=self.mct.gumbel, gumbel_batch=self.mct.gumbel_batch, gumbel_full=self.mct.gumbel_full,
                               exact_endgame=self.mct.exact_endgame, proof_backup=self.mct.proof_backup, puct=self.mct.puct)

    def reset(self):
        old = self.mct
        self.mct = MCT(eval_method="neural", nn=old.nn, dirichlet_alpha=old.dirichlet_alpha,
                       dirichlet_epsilon=old.dirichlet_epsilon, symmetry=old.symmetry, leaf_batch=old.leaf_batch, gumbel=old.gumbel,
                       gumbel_batch=old.gumbel_batch, gumbel_full=old.gumbel_full, exact_endgame=old.exact_endgame,
                       proof_backup=old.proof_backup, puct=old.puct)
        # keep the uploaded weights and the device tree storage: a reset only drops the tree
        self.mct._hipnet, self.mct._engine, self.mct._engine_board = old._hipnet, old._engine, old._engine_board
        self.mct._engine_lb, self.mct._engine_gumbel, self.mct._engine_gb = old._engine_lb, old._engine_gumbel, old._engine_gb
        self.mct._engine_gf = old._engine_gf
        self.mct._engine_exact = old._engine_exact
        self.mct._engine_proof = old._engine_proof
        self.mct._engine_puct = old._engine_puct
        self.mct._evaluator = old._evaluator  # the carried engine calls it (external evaluation, evaluators.route)
        if self.mct._engine is not None:
            self.mct._plies = 0


def _root_key(board):
    """the position a device root stands for: the key MCT._sync_device_root compares"""
    return (board.grid.astype(np.int8).tobytes(), int(board.player))


class BatchedMCTSPlayer(Player):
    """MCTSPlayer (players.py:126-191) for up to n_slots games at once: UCT with random playouts, every tree in a slot of one
    device engine.  get_moves searches all the boards in one call and reads all the roots back with one kernel launch;
    apply_moves is Board.play_move + MCT.change_root for all of them.  Slot i holds the game of boards[i]: keep a game at its
    index from call to call (None where a game is finished or has nothing to ask) and the trees are reused.  Reuse is all or
    nothing -- if any board differs from the position its slot's root stands for, every tree restarts from its board."""
    _eval_method = "rollout"

    def __init__(self, n_sim=None, n_slots=1, seed=None, verbose=False):
        super().__init__(verbose=verbose)
        if n_sim is None:
            raise ValueError(f"{type(self).__name__} needs to have n_sim specified.")
        if int(n_slots) < 1:
            raise ValueError("n_slots must be a positive integer")
        self.n_sim, self.n_slots = int(n_sim), int(n_slots)
        self.nn, self.dirichlet_alpha, self.dirichlet_epsilon, self.symmetry, self.leaf_batch = None, None, None, None, None
        self.gumbel, self.gumbel_batch, self.gumbel_full = None, 1, False
        self.exact_endgame = None
        self.proof_backup = False
        self.puct = None
        self._seed = int(np.random.randint(0, 2**31 - 1)) if seed is None else int(seed)
        self._engine = None           # n_slots device trees
        self._engine_board = None     # (game, H, W) the engine was built for
        self._hipnet = None
        self._evaluator = None        # external evaluator of a network the HIP net does not serve (evaluators.route)
        self._keys = None             # per slot: _root_key of the position its root stands for (None: no game there)
        self._boards = None           # per slot: that position as a Board
        self._tie_mode = None         # tests: engine.TIE_LOWEST (None: ties are drawn among equals, utils.py:28-34)

    def reset(self):
        """drops the trees, keeps the device storage"""
        self._keys, self._boards = None, None

    def close(self):
        if self._engine is not None:
            self._engine.close()
        self._engine, self._keys, self._boards = None, None, None

    # ------------------------------------------------------------------ checks without device work
    def _check(self, boards):
        from .evaluators import check_game, check_normalizer
        boards = list(boards)
        if len(boards) > self.n_slots:
            raise ValueError(f"{self}: {len(boards)} boards for {self.n_slots} slots")
        live = [b for b in boards if b is not None]
        if not live:
            raise ValueError(f"{self}: no board to search")
        for b in live:
            check_game(b)
            if (b.game, b.grid.shape) != (live[0].game, live[0].grid.shape):
                raise ValueError(f"{self}: all boards must be of one game and size")
            if b.is_game_over():
                raise ValueError(f"{self}.get_move was called with a board in game over state...")
        if self._eval_method == "neural":
            if self.nn is None:
                raise ValueError("The MCT has no neural network to evaluate positions with.")
            check_normalizer(self.nn)
        return boards, live[0]

    @staticmethod
    def _temps(temps, n):
        t = np.asarray(temps, np.float64)
        t = np.full(n, float(t)) if t.ndim == 0 else t.reshape(-1)
        if len(t) != n:
            raise ValueError(f"{len(t)} temperatures for {n} boards")
        return t

    # ------------------------------------------------------------------ device trees
    def _build(self, first):
        from .engine import (EVAL_EXTERNAL, EVAL_NET, EVAL_ROLLOUT, GAME_IDS, NOISE_OFF, NOISE_PHILOX, TIE_RANDOM, SelfPlayEngine)
        from .evaluators import make_evaluator, route
        from .symmetry import members, parse
        H, W = first.grid.shape
        if self._engine is not None and self._engine_board != (first.game, H, W):
            self._engine.close()  # built for another board: rebuild rather than search with the wrong rules
            self._engine, self._hipnet, self._evaluator, self._keys, self._boards = None, None, None, None, None
        if self._engine is not None:
            return
        neural = self._eval_method == "neural"
        external = neural and route(self.nn) != "hip"  # evaluates the leaves itself, as in BatchedArena._engine
        sym = members(first.game, H, W, check_symmetry(self.symmetry, self.nn if neural else None))
        lb = check_leaf_batch(self.leaf_batch, self.nn if neural else None, self.symmetry, neural)
        gb = check_gumbel_batch(self.gumbel_batch, self.gumbel if neural else None, self.symmetry)
        gf = check_gumbel_full(self.gumbel_full, self.gumbel if neural else None)
        if neural and not external:
            # every slot's leaf in each of its twins, or every slot's leaf_batch / gumbel_batch walkers (a random spec evaluates one
            # twin per leaf)
            rnd = parse(self.symmetry)[1]
            self._hipnet = self.nn.to_hip(max_batch=max(1, 1 if rnd else len(sym), lb, gb) * self.n_slots)
        noisy = self.dirichlet_alpha is not None and self.dirichlet_epsilon is not None
        self._engine = SelfPlayEngine(GAME_IDS[first.game], H, W, n_slots=self.n_slots, n_sim=self.n_sim,
                                      net=self._hipnet if neural and not external else None,
                                      dirichlet_alpha=self.dirichlet_alpha, dirichlet_epsilon=self.dirichlet_epsilon,
                                      temp_max_step=-1, temp_min_step=0, tie_mode=TIE_RANDOM if self._tie_mode is None else self._tie_mode,
                                      noise_mode=NOISE_PHILOX if noisy else NOISE_OFF,
                                      evaluator=EVAL_EXTERNAL if external else (EVAL_NET if neural else EVAL_ROLLOUT),
                                      seed=self._seed, max_plies=4 * H * W + 16, sample_capacity=16)
        if external:
            self._evaluator = make_evaluator(self.nn, first.game, H, W)
            self._engine.set_evaluator(self._evaluator)
        if sym:
            self._engine.set_symmetry(("random", sym) if parse(self.symmetry)[1] else sym)
        if lb > 1:
            self._engine.set_leaf_batch(lb)
        if neural and self.gumbel is not None:
            check_gumbel(self.gumbel, self.nn, self.leaf_batch)
            self._engine.set_gumbel(self.gumbel)
            if gb > 1:
                self._engine.set_gumbel_batch(gb)
            if gf:
                self._engine.set_gumbel_full(True)
        if neural and self.exact_endgame is not None:
            self._engine.set_exact_endgame(check_exact_endgame(self.exact_endgame, self.nn, self.symmetry, self.leaf_batch, self.gumbel))
        if neural and check_proof_backup(self.proof_backup, self.nn, self.symmetry, self.leaf_batch, self.gumbel):
            self._engine.set_proof_backup(True)
        if neural and puct_is_on(check_puct(self.puct, self.nn, self.symmetry, self.leaf_batch, self.gumbel, self.exact_endgame, self.proof_backup)):
            self._engine.set_puct(self.puct)
        self._engine_board = (first.game, H, W)

    def _sync(self, boards, first):
        self._build(first)
        keys = [None if b is None else _root_key(b) for b in boards]
        kept = (self._keys is not None and len(keys) == len(self._keys)
                and all(k is None or k == mine for k, mine in zip(keys, self._keys)))
        if kept:
            return
        # all or nothing: every tree restarts from its board.  A slot without a board gets a filler position that nobody reads.
        fill = [first if b is None else b for b in boards]
        base = int(np.random.randint(0, 2**31 - 1))
        self._engine.set_roots(np.stack([b.grid.astype(np.int8) for b in fill]), np.array([b.player for b in fill], np.int8),
                               game_ids=((base + np.arange(len(fill), dtype=np.uint64)) & 0xFFFFFFFF).astype(np.uint32))
        self._keys = keys
        self._boards = [None if b is None else b.clone() for b in boards]

    def _search(self, boards, first, temps, pv_len=0):
        self._sync(boards, first)
        try:
            self._engine.search(self.n_sim)
        except BaseException:
            self._keys = None  # a failed evaluation leaves unevaluated leaves in the trees: the next call starts them afresh
            raise
        r = self._engine.root_readout(temps=temps, pv_len=pv_len, n=len(boards))
        return r, {k: v.cpu().numpy() for k, v in r.items()}

    # ------------------------------------------------------------------ the players' surface, many boards at a time
    def get_moves(self, boards, temps=0):
        """Player.get_move (players.py:158-191) for every board: a list of (move, action_probs, visit_counts, prior_probs), None
        for a None entry.  `temps`: one temperature or one per board.  The move is the device's draw: the most visited child
        at temperature 0 (ties as the engine breaks them), else sampled from action_probs."""
        boards, first = self._check(boards)
        temps = self._temps(temps, len(boards))
        _, h = self._search(boards, first, temps)
        neural = self._eval_method == "neural"
        out = []
        for i, b in enumerate(boards):
            if b is None:
                out.append(None)
                continue
            a = int(h["action"][i])
            if a < 0:
                raise RuntimeError(f"{self}: slot {i} has no searched root")
            acts = np.flatnonzero(h["child"][i])
            counts = {_move_of(b, int(x)): int(h["visits"][i, x]) for x in acts}
            priors = {_move_of(b, int(x)): (float(h["P"][i, x]) if neural else None) for x in acts}
            move = _move_of(b, a)
            probs = {move: 1} if temps[i] == 0 else {_move_of(b, int(x)): float(h["pi"][i, x]) for x in acts}
            out.append((move, probs, counts, priors))
        return out

    def apply_moves(self, moves):
        """Board.play_move + MCT.change_root (mcts.py:118-125) in every game; moves[i] is None where game i gets no move"""
        if self._engine is None or self._keys is None:
            return  # no device trees yet: the next search starts from the boards it is given
        moves = list(moves)
        if len(moves) > len(self._keys):
            raise ValueError(f"{self}: {len(moves)} moves for {len(self._keys)} games")
        actions = np.full(len(moves), -1, np.int32)
        after = {}
        for i, m in enumerate(moves):
            if m is None:
                continue
            if self._boards[i] is None:
                raise ValueError(f"{self}: a move for slot {i}, which holds no game")
            b = self._boards[i].clone()
            b.play_move(m)  # raises ValueError for an illegal move, like the engine would
            actions[i] = _action_of(self._boards[i], m)
            after[i] = b
        if not after:
            return
        self._engine.play(actions)
        for i, b in after.items():
            self._boards[i], self._keys[i] = b, _root_key(b)

    def analyze(self, boards, pv_len=8):
        """what the search thinks of every board: (readout, lines) -- the raw root readout (a dict of CUDA tensors, one row per
        board: visits, pi at temperature 0, Q, P, child, action, root_N, pv) and the principal line of every board as a list of moves"""
        boards, first = self._check(boards)
        r, h = self._search(boards, first, self._temps(0, len(boards)), pv_len=pv_len)
        lines = []
        for i, b in enumerate(boards):
            lines.append(None if b is None else [_move_of(b, int(a)) for a in (h["pv"][i] if pv_len > 0 else []) if a >= 0])
        return r, lines


class BatchedAlphaZeroPlayer(BatchedMCTSPlayer):
    """AlphaZeroPlayer (players.py:194-247) for up to n_slots games at once: PUCT with the network `nn` (the HIP network for a shipped
    architecture, else the network's own evaluate / predict through an external evaluator), optional root Dirichlet noise and an
    optional ensemble over the board's symmetries (`symmetry`: "all", a mask or transform codes; HIP network only) or one symmetry
    drawn per evaluation (`symmetry`: "random" or ("random", members); combines with `leaf_batch`)"""
    _eval_method = "neural"

    def __init__(self, n_sim=None, nn=None, n_slots=1, dirichlet_alpha=None, dirichlet_epsilon=None, seed=None, verbose=False,
                 symmetry=None, leaf_batch=None, gumbel=None, gumbel_batch=1, gumbel_full=False, exact_endgame=None, proof_backup=False,
                 puct=None):
        super().__init__(n_sim=n_sim, n_slots=n_slots, seed=seed, verbose=verbose)
        self.nn, self.dirichlet_alpha, self.dirichlet_epsilon = nn, dirichlet_alpha, dirichlet_epsilon
        # leaf evaluations averaged over the board's symmetries (alphazero_amd.symmetry; None: off); HIP-routed networks only
        self.symmetry = symmetry
        check_symmetry(symmetry, nn)
        # simulations per lock-step and game, kept apart by virtual loss (None / 1: the sequential search); HIP-routed networks only
        self.leaf_batch = leaf_batch
        check_leaf_batch(leaf_batch, nn, symmetry)
        # the Gumbel root search (alphazero_amd.gumbel: None = off, an int m or a dict): get_moves then returns its move and, at a
        # temperature other than 0, its improved policy; HIP-routed networks at leaf_batch 1 only
        self.gumbel = gumbel
        check_gumbel(gumbel, nn, leaf_batch)
        # Sequential Halving leaves per lock-step and game of the Gumbel root search (1: one); needs `gumbel`, not symmetry "all"
        self.gumbel_batch = gumbel_batch
        check_gumbel_batch(gumbel_batch, gumbel, symmetry)
        # the full Gumbel search: the paper's v_mix and its deterministic selection below the root; needs `gumbel`
        self.gumbel_full = gumbel_full
        check_gumbel_full(gumbel_full, gumbel)
        # exact endgames (alphazero_amd.endgame: None = off, or E in 1..10): a leaf with at most E empty cells is solved, not evaluated;
        # the plain PUCT search on HIP-routed networks only
        self.exact_endgame = exact_endgame
        check_exact_endgame(exact_endgame, nn, symmetry, leaf_batch, gumbel)
        # proof backup (alphazero_amd.proof: a bool): proven wins, losses and draws are backed up the tree; get_moves then returns the
        # move and the policy on the counts the proofs leave; the plain PUCT search on HIP-routed networks only
        self.proof_backup = proof_backup
        check_proof_backup(proof_backup, nn, symmetry, leaf_batch, gumbel)
        # the PUCT exploration settings (alphazero_amd.puct: None, c_init or a dict of c_init, c_base, fpu); the plain PUCT search on
        # HIP-routed networks only
        self.puct = puct
        check_puct(puct, nn, symmetry, leaf_batch, gumbel, exact_endgame, proof_backup)


PLAYERS_SET = {"human", "random", "greedy", "mcts", "alphazero"}
PLAYERS_REGISTER = {"random": RandomPlayer, "greedy": GreedyPlayer, "mcts": MCTSPlayer, "alphazero": AlphaZeroPlayer}
