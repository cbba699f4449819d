"""Host side of the MI355X self-play engine: thin Python over the C ABI (include/az_amd.h).

torch is used for device memory and streams only; all computation is in libaz_amd.so.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import (EVAL_EXTERNAL, EVAL_FAKE, EVAL_NET, EVAL_ROLLOUT, GAME_IDS, NOISE_HASH, NOISE_OFF, NOISE_PHILOX, TIE_LOWEST,  # noqa: F401
                   TIE_RANDOM, EngineCfg, EngineStats, AzError, check, lib)


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def game_shape(game, board_size=None, board_width=7, board_height=6):
    """(game id, H, W, action size) for the reference's game names / config fields"""
    if game == "othello":
        n = 6 if board_size is None else board_size  # OthelloConfig.board_size default (othello.py:22)
        return GAME_IDS[game], n, n, n * n + 1
    if game == "connect4":
        return GAME_IDS[game], board_height, board_width, board_width
    if game == "tictactoe":
        return GAME_IDS[game], 3, 3, 9
    raise ValueError(f"unknown game {game!r}")


class _DevView:
    """exposes a raw device pointer through __cuda_array_interface__ so torch can wrap it without a copy"""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner


def _wrap(ptr, shape, dtype, owner):
    typestr = {torch.int8: "|i1", torch.float32: "<f4", torch.int32: "<i4", torch.uint8: "|u1", torch.float64: "<f8"}[dtype]
    if int(np.prod(shape)) == 0:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return torch.as_tensor(_DevView(ptr, shape, typestr, owner), device="cuda")


# ---------------------------------------------------------------------------------------------- rules
def legal_batch(game_id, H, W, grids, players, for_player=None):
    """Board.get_moves for n positions: uint8 [n, A] legality table (device tensors in, device tensor out)."""
    n = players.numel()
    A = H * W + 1 if game_id == 0 else (W if game_id == 1 else 9)
    assert grids.dtype == torch.int8 and players.dtype == torch.int8 and grids.is_cuda and grids.is_contiguous()
    out = torch.empty((n, A), dtype=torch.uint8, device=grids.device)
    fp = for_player.data_ptr() if for_player is not None else None
    check(lib().az_board_legal_batch(game_id, H, W, grids.data_ptr(), players.data_ptr(), fp, n, out.data_ptr(), _stream_ptr()))
    return out


def play_batch(game_id, H, W, grids, players, actions):
    """Board.play_move for n positions; status[i] = 0 or AZ_EILLEGAL (the reference raises ValueError)."""
    n = players.numel()
    assert actions.dtype == torch.int32 and grids.is_contiguous()
    og, op = torch.empty_like(grids), torch.empty_like(players)
    st = torch.empty(n, dtype=torch.int32, device=grids.device)
    check(lib().az_board_play_batch(game_id, H, W, grids.data_ptr(), players.data_ptr(), actions.data_ptr(), n,
                                    og.data_ptr(), op.data_ptr(), st.data_ptr(), _stream_ptr()))
    return og, op, st


def status_batch(game_id, H, W, grids, players):
    """(is_game_over uint8, get_winner int8 [2 where not over], sum(player*grid) int32) for n positions."""
    n = players.numel()
    over = torch.empty(n, dtype=torch.uint8, device=grids.device)
    win = torch.empty(n, dtype=torch.int8, device=grids.device)
    score = torch.empty(n, dtype=torch.int32, device=grids.device)
    check(lib().az_board_status_batch(game_id, H, W, grids.data_ptr(), players.data_ptr(), n, over.data_ptr(),
                                      win.data_ptr(), score.data_ptr(), _stream_ptr()))
    return over, win, score


def solve_batch(game_id, H, W, grids, players, max_empties=_lib.SOLVE_MAX_EMPTIES, node_budget=0, with_nodes=False):
    """Exact endgames for n positions (az_solve_batch): (winner int8, action int32[, nodes int64]) device tensors.  winner = the
    outcome under optimal play as an absolute player id, action = the lowest action index that keeps it; a finished game reports its
    winner and action -1; a position with more than max_empties empty cells, or one that spent node_budget, reports
    (_lib.UNSOLVED, -1)."""
    n = players.numel()
    assert grids.dtype == torch.int8 and players.dtype == torch.int8 and grids.is_cuda and grids.is_contiguous()
    win = torch.empty(n, dtype=torch.int8, device=grids.device)
    act = torch.empty(n, dtype=torch.int32, device=grids.device)
    nodes = torch.empty(n, dtype=torch.int64, device=grids.device) if with_nodes else None
    check(lib().az_solve_batch(game_id, H, W, grids.data_ptr(), players.data_ptr(), n, int(max_empties), int(node_budget), win.data_ptr(),
                               act.data_ptr(), nodes.data_ptr() if with_nodes else None, _stream_ptr()))
    return (win, act, nodes) if with_nodes else (win, act)


def augment_samples(game_id, H, W, samples):
    """symmetry twins of the samples with move_idx >= 2, in the reference's order (trainer.py:275-284).
    samples: dict of CUDA tensors (state int8 [S,H,W], pi float32 [S,A], z int8 [S], meta int32 [S,4]).
    Returns the twins as a dict of the same form; meta[:, 3] is the transformation code 1..7."""
    st, pi, z, meta = (samples[k].contiguous() for k in ("state", "pi", "z", "meta"))
    S, A = z.shape[0], pi.shape[1]
    n = C.c_int64()
    check(lib().az_augment_count(game_id, meta.data_ptr() if S else None, S, C.byref(n), _stream_ptr()))
    N = n.value
    out = {"state": torch.empty((N, H, W), dtype=torch.int8, device=st.device), "pi": torch.empty((N, A), dtype=torch.float32, device=st.device),
           "z": torch.empty(N, dtype=torch.int8, device=st.device), "meta": torch.empty((N, 4), dtype=torch.int32, device=st.device)}
    if N:
        check(lib().az_augment(game_id, H, W, st.data_ptr(), pi.data_ptr(), z.data_ptr(), meta.data_ptr(), S, out["state"].data_ptr(),
                               out["pi"].data_ptr(), out["z"].data_ptr(), out["meta"].data_ptr(), N, _stream_ptr()))
    return out


TRANSFORM_NAMES = [None, "reflection_horizontal", "rotation_90", "reflection_horizontal+rotation_90", "rotation_180",
                   "reflection_horizontal+rotation_180", "rotation_270", "reflection_horizontal+rotation_270"]


# ---------------------------------------------------------------------------------------------- network
class HipNet:
    """Device policy-value network built from a reference state_dict (eval-mode BN folded at upload)."""

    def __init__(self, game_id, H, W, state_dict, max_batch=4096):
        self.game_id, self.H, self.W, self.max_batch = game_id, H, W, max_batch
        h = C.c_void_p()
        check(lib().az_net_create(game_id, H, W, max_batch, C.byref(h)))
        self.h = h
        self.A = lib().az_net_action_size(self.h)
        self.load_state_dict(state_dict)

    def load_state_dict(self, state_dict):
        """weights in (update_network, trainer.py:383-387).  CUDA tensors never leave the device: BatchNorm is folded and
        the weights are re-tiled by device kernels (az_net_commit_device); host tensors / numpy arrays take the host fold."""
        items = [(k, v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")]
        if items and all(isinstance(v, torch.Tensor) and v.is_cuda for _, v in items):
            keep = []
            for k, v in items:
                t = v.detach().to(torch.float32).contiguous()
                keep.append(t)  # alive until the copies have been queued on this stream
                check(lib().az_net_set_tensor_device(self.h, k.encode(), t.data_ptr(), t.numel(), _stream_ptr()))
            check(lib().az_net_commit_device(self.h, _stream_ptr()))
            return
        for k, v in items:
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            check(lib().az_net_set_tensor(self.h, k.encode(), a.ctypes.data, a.size))
        check(lib().az_net_commit(self.h, _stream_ptr()))

    def forward(self, x):
        """x: float32 CUDA tensor [B, H*W] of canonical boards (player*grid). Returns (probs [B,A], v [B])."""
        x = x.contiguous().view(-1, self.H * self.W)
        assert x.is_cuda and x.dtype == torch.float32
        B = x.shape[0]
        probs = torch.empty((B, self.A), dtype=torch.float32, device=x.device)
        v = torch.empty(B, dtype=torch.float32, device=x.device)
        check(lib().az_net_forward(self.h, x.data_ptr(), B, probs.data_ptr(), v.data_ptr(), _stream_ptr()))
        return probs, v

    def forward_dyn(self, x, count, probs=None, v=None):
        """az_net_forward_dyn: evaluates only the first min(count[0], B) rows of x; `count` is an int32 CUDA tensor (the engine's
        leaf counter on the hot path: the launch is sized for B, the rows really present are read on the device).  Rows beyond
        the count are left as they were in `probs` / `v`."""
        x = x.contiguous().view(-1, self.H * self.W)
        assert x.is_cuda and x.dtype == torch.float32 and count.is_cuda and count.dtype == torch.int32
        B = x.shape[0]
        if probs is None:
            probs = torch.empty((B, self.A), dtype=torch.float32, device=x.device)
        if v is None:
            v = torch.empty(B, dtype=torch.float32, device=x.device)
        check(lib().az_net_forward_dyn(self.h, x.data_ptr(), count.data_ptr(), B, probs.data_ptr(), v.data_ptr(), _stream_ptr()))
        return probs, v

    def forward_sym(self, x, symmetry="all"):
        """forward() averaged over the board's symmetries (az_net_forward_sym): `symmetry` is "all", None (off), a mask or an
        iterable of transform codes (alphazero_amd.symmetry).  Needs len(members) * B <= max_batch."""
        from .symmetry import resolve
        x = x.contiguous().view(-1, self.H * self.W)
        assert x.is_cuda and x.dtype == torch.float32
        B = x.shape[0]
        probs = torch.empty((B, self.A), dtype=torch.float32, device=x.device)
        v = torch.empty(B, dtype=torch.float32, device=x.device)
        check(lib().az_net_forward_sym(self.h, x.data_ptr(), B, resolve(symmetry), probs.data_ptr(), v.data_ptr(), _stream_ptr()))
        return probs, v

    def forward_sym_codes(self, x, codes):
        """forward() with row r evaluated in the one orientation codes[r] (az_net_forward_sym_codes): the row's twin goes through
        the network and its policy is mapped back, copies only.  `codes`: one transform code per row (alphazero_amd.symmetry), a
        sequence, numpy array or tensor; a code the board does not have is a ValueError."""
        from .symmetry import members
        x = x.contiguous().view(-1, self.H * self.W)
        assert x.is_cuda and x.dtype == torch.float32
        B = x.shape[0]
        c = torch.as_tensor(codes).reshape(-1)
        if c.dtype.is_floating_point or c.dtype == torch.bool or c.numel() != B:
            raise ValueError(f"codes: {B} integer transform codes expected, one per row")
        if B and (int(c.min()) < 0 or int(c.max()) > 7):
            raise ValueError("codes: transform codes are the integers 0..7")
        members({v: k for k, v in GAME_IDS.items()}[self.game_id], self.H, self.W, sorted(set(c.tolist())))  # ValueError: not this board's
        c = c.to(device=x.device, dtype=torch.uint8).contiguous()
        probs = torch.empty((B, self.A), dtype=torch.float32, device=x.device)
        v = torch.empty(B, dtype=torch.float32, device=x.device)
        check(lib().az_net_forward_sym_codes(self.h, x.data_ptr(), B, c.data_ptr(), probs.data_ptr(), v.data_ptr(), _stream_ptr()))
        return probs, v

    def flops_per_board(self):
        return int(lib().az_net_flops_per_board(self.h))

    def time_stage(self, stage, B, iters=20):
        ms = C.c_float()
        check(lib().az_net_time_stage(self.h, stage, B, iters, _stream_ptr(), C.byref(ms)))
        return float(ms.value)

    def stage_kernel(self, stage, B):
        """name of the kernel stage 0..3 launches for B boards (az_net_stage_kernel)"""
        buf = C.create_string_buffer(64)
        check(lib().az_net_stage_kernel(self.h, stage, B, buf, 64))
        return buf.value.decode()

    def trunk_prefetch(self, B, beside):
        """True where the trunk of a launch of B boards (beside: az_net_forward_lane's flag) runs k_trunk_quad's prefetching form"""
        return bool(lib().az_net_trunk_prefetch(self.h, B, int(beside)))

    def stage_plan(self, stage, B, beside):
        """the plan of stage 0..3 of a launch of B boards as text: kernel and the plan's fields for it (az_net_stage_plan)"""
        buf = C.create_string_buffer(128)
        check(lib().az_net_stage_plan(self.h, stage, B, int(beside), buf, 128))
        return buf.value.decode()

    def gemm_rows(self, stage, B, beside, count):
        """rows per block of fc1 / fc2 of a launch of B boards whose device count is `count`: 16 / 32 / 64 on k_gemm's 64 x 64 tile,
        the tile's height on its other tiles, 0 on another kernel (az_net_gemm_rows)"""
        return int(lib().az_net_gemm_rows(self.h, stage, B, int(beside), int(count)))

    def trunk_stores(self, B, beside):
        """True where that trunk runs the prefetching form with vector stores of conv3's planes and conv4's features"""
        return bool(lib().az_net_trunk_stores(self.h, B, int(beside)))

    def profile(self, enable=True):
        """bracket every stage launch of the following forwards with HIP events (az_net_profile)"""
        check(lib().az_net_profile(self.h, 1 if enable else 0))

    def profile_read(self):
        """-> {kernel: (total ms, launches)} since profile(True)"""
        ms, n = (C.c_double * 8)(), (C.c_int64 * 8)()
        check(lib().az_net_profile_read(self.h, ms, n))
        return {k: (ms[i], n[i]) for i, k in enumerate(PROFILE_SLOTS)}

    def profile_overhead_ms(self):
        """correction to subtract per launch from profile_read totals: 0 since every launch carries its own start / stop events
        (rounds 1-3 recorded events between the launches and calibrated an empty interval)"""
        ms = C.c_double()
        check(lib().az_net_profile_overhead(self.h, C.byref(ms)))
        return float(ms.value)

    def close(self):
        if getattr(self, "h", None):
            lib().az_net_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass


# az_net_profile_read's slots: one per kernel family (a slot's mean is what rocprofv3 lists for that kernel)
PROFILE_SLOTS = ["k_trunk2", "k_gemm fc1", "k_gemm fc2", "k_heads", "k_trunk", "small fc1", "small fc2", "k_trunk_q"]


# ---------------------------------------------------------------------------------------------- engine
class ExternalBatch:
    """what an EVAL_EXTERNAL engine hands its evaluator per root-prior pass / lock-step: zero-copy views of the engine's own
    buffers, valid during the call only.  Rows [0, count[0]) are pending; `cap` bounds them (rows beyond are scratch).
      x       float32 [cap, H, W]  player * grid (PolicyValueNetwork.evaluate's input, base.py:363)
      grids   int8    [cap, H, W]  Board.grid       players int8 [cap]  Board.player       slots int32 [cap]  engine slot
      probs   float32 [cap, A]     out: what predict() returns (exp(log_softmax)); the engine renormalises over the legal moves
      value   float32 [cap]        out: predict()'s value, side-to-move frame (evaluate()'s v times Board.player)"""
    __slots__ = ("cap", "H", "W", "A", "game_id", "count", "x", "grids", "players", "slots", "probs", "value")


class SelfPlayEngine:
    """n_slots concurrent self-play games in lock-step on one GPU (AlphaZeroTrainer.self_play, trainer.py:215-273)."""

    def __init__(self, game_id, H, W, n_slots, n_sim, net=None, dirichlet_alpha=0.03, dirichlet_epsilon=0.25,
                 temp_max_step=4, temp_min_step=4, tie_mode=TIE_RANDOM, noise_mode=NOISE_PHILOX, evaluator=EVAL_NET,
                 seed=0, node_capacity=None, max_plies=None, sample_capacity=None, groups=None):
        cells = H * W
        if max_plies is None:
            max_plies = 2 * cells if game_id == 0 else cells + 1
        if node_capacity is None:
            # per pool: the subtree kept at a move + everything one search allocates (the tree is compacted
            # into the slot's other pool at every move); exhaustion is reported, never silent
            node_capacity = max(4096, min(1 << 17, 96 * n_sim))
        if sample_capacity is None:
            sample_capacity = n_slots * max_plies
        self.cfg = EngineCfg(game_id, H, W, n_slots, n_sim,
                             -1.0 if dirichlet_alpha is None else dirichlet_alpha,
                             -1.0 if dirichlet_epsilon is None else dirichlet_epsilon,
                             temp_max_step, temp_min_step, tie_mode, noise_mode, evaluator, seed, node_capacity, max_plies,
                             sample_capacity)
        self.net = net
        self.A = H * W + 1 if game_id == 0 else (W if game_id == 1 else 9)
        self.cells = cells
        h = C.c_void_p()
        check(lib().az_engine_create(C.byref(self.cfg), net.h if net is not None else None, _stream_ptr(), C.byref(h)))
        self.h = h
        self._eval_cb = None     # the ctypes trampoline of set_evaluator: alive as long as the engine
        self._eval_exc = None    # an exception the evaluator raised, re-raised by the engine call that ran it
        self._eval_views = {}    # device pointer -> full-size view (the rows are sliced per call)
        self._eval_streams = {}
        self._sym_mode = None    # which symmetry mode set_symmetry last put in force: None, "ensemble" or "random"
        if groups is not None:
            self.set_groups(groups)

    # ---------------------------------------------------------------------------------------- external evaluator
    def set_evaluator(self, fn):
        """EVAL_EXTERNAL engines: fn(batch) evaluates the pending rows of every root-prior pass and lock-step (an ExternalBatch),
        inside torch.cuda.stream(the engine's stream).  An exception raised by fn fails the engine call that ran it and is
        re-raised from there unchanged (chained with the engine's message); the trees then need set_roots / run."""
        if self.cfg.evaluator != EVAL_EXTERNAL:
            raise ValueError(f"set_evaluator needs an engine created with evaluator=EVAL_EXTERNAL (this one: {self.cfg.evaluator})")

        engine = weakref.ref(self)  # the engine holds the trampoline, not the other way round

        def trampoline(user, batch, stream):
            eng = engine()
            try:
                views = eng._batch_views(batch.contents, stream)
                with torch.cuda.stream(eng._eval_streams[stream]):
                    fn(views)
                return 0
            except BaseException as exc:  # ctypes would print and drop it: keep it for the engine call
                eng._eval_exc = exc
                return 1
        cb = _lib.EVAL_FN(trampoline)
        check(lib().az_engine_set_evaluator(self.h, cb, None))
        self._eval_cb = cb

    def _view(self, ptr, shape, dtype):
        key = (ptr, dtype)
        v = self._eval_views.get(key)
        if v is None:
            v = self._eval_views[key] = _wrap(ptr, shape, dtype, None)  # the engine owns the memory and these views
        return v

    def _batch_views(self, b, stream):
        G, H, W, A = self.cfg.n_slots, b.H, b.W, b.A
        out = ExternalBatch()
        out.cap, out.H, out.W, out.A, out.game_id = b.cap, H, W, A, self.cfg.game
        out.count = self._view(b.d_count, (1,), torch.int32)
        out.x = self._view(b.d_input, (G, H, W), torch.float32)[: b.cap]
        out.grids = self._view(b.d_grids, (G, H, W), torch.int8)[: b.cap]
        out.players = self._view(b.d_players, (G,), torch.int8)[: b.cap]
        out.slots = self._view(b.d_slots, (G,), torch.int32)[: b.cap]
        out.probs = self._view(b.d_probs, (G, A), torch.float32)[: b.cap]
        out.value = self._view(b.d_value, (G,), torch.float32)[: b.cap]
        if stream not in self._eval_streams:
            self._eval_streams[stream] = torch.cuda.ExternalStream(stream)
        return out

    def _evaluated(self, rc):
        """check() for the calls that may run the evaluator: its own exception first, chained with the engine's message"""
        exc, self._eval_exc = self._eval_exc, None
        if exc is not None and rc != 0:
            try:
                check(rc)
            except AzError as err:
                raise exc from err
        check(rc)

    def set_symmetry(self, symmetry):
        """every leaf evaluation of this engine (EVAL_NET only) averaged over the board's symmetries: "all", None (off), a mask
        or an iterable of transform codes (alphazero_amd.symmetry).  The network needs max_batch >= len(members) * n_slots.
        "random" / ("random", members): every leaf in ONE member drawn per evaluation instead (az_engine_set_symmetry_random): the
        rows of the plain search, composes with set_leaf_batch.  The two modes exclude each other: the other one is switched off."""
        from .symmetry import parse
        mask, rnd = parse(symmetry)
        if rnd:
            if self._sym_mode == "ensemble":
                check(lib().az_engine_set_symmetry(self.h, 0))
                self._sym_mode = None
            check(lib().az_engine_set_symmetry_random(self.h, mask))
            self._sym_mode = "random" if mask != 0 else None
        else:
            if self._sym_mode == "random":
                check(lib().az_engine_set_symmetry_random(self.h, 0))
                self._sym_mode = None
            check(lib().az_engine_set_symmetry(self.h, mask))
            self._sym_mode = "ensemble" if mask != 0 else None

    def set_groups(self, n):
        """run() plays the slots as n contiguous slot groups, each a launch chain of its own on its own stream, so that one group's
        tree kernels overlap another's network kernels (az_engine_set_groups; 1, 2 or 4; None / 0: the measured default).  The
        samples are the same rows in another order.  Plain search of EVAL_NET / EVAL_FAKE engines only: anything else with n > 1
        is a ValueError that names the mode."""
        check(lib().az_engine_set_groups(self.h, int(n or 0)))

    def groups(self):
        """the slot groups the next run() would play with (1 under HipNet.profile and in every mode groups are not served for)"""
        n = C.c_int32()
        check(lib().az_engine_groups(self.h, C.byref(n)))
        return n.value

    def set_leaf_batch(self, k):
        """k simulations per slot and lock-step, kept apart by virtual loss (az_engine_set_leaf_batch; 1: the plain search, the
        default).  EVAL_NET / EVAL_FAKE engines without a symmetry ensemble (the random symmetry mode combines); the network needs
        max_batch >= k * n_slots."""
        check(lib().az_engine_set_leaf_batch(self.h, int(k)))

    def collisions(self):
        """walkers that landed on the pending leaf of an earlier walker of their lock-step, since the engine was created"""
        n = C.c_int64()
        check(lib().az_engine_collisions(self.h, C.byref(n)))
        return n.value

    def set_playout_cap(self, cap):
        """playout cap randomization (az_engine_set_playout_cap): None = off, or (n_fast, p_full) -- a ply is searched
        in full (n_sim simulations, root noise, recorded) with probability p_full and fast otherwise (n_fast simulations, no noise,
        played but not recorded), by a coin of (seed, game id, ply).  Plain search of EVAL_NET / EVAL_FAKE engines; any other mode
        is a ValueError that names it."""
        from .playout_cap import parse
        cap = parse(cap)
        check(lib().az_engine_set_playout_cap(self.h, *((0, 1.0) if cap is None else cap)))

    def playout_cap_stats(self):
        """{"full_plies", "fast_plies"}: the plies played after a full / a fast search since the last run() / set_roots(), counted
        while the playout cap is on (both 0 with it off)"""
        full, fast = C.c_int64(), C.c_int64()
        check(lib().az_engine_playout_cap_stats(self.h, C.byref(full), C.byref(fast)))
        return {"full_plies": full.value, "fast_plies": fast.value}

    @staticmethod
    def playout_cap_full(seed, game_id, ply, p_full):
        """the playout cap's coin of (seed, game id, ply): True = a full ply (az_playout_cap_full: host code, the kernels' arithmetic)"""
        return bool(lib().az_playout_cap_full(int(seed) & 0xFFFFFFFF, int(game_id) & 0xFFFFFFFF, int(ply), float(p_full)))

    def set_resign(self, resign):
        """resignation in run() (az_engine_set_resign): None = off, or a dict of threshold, consecutive, min_ply,
        holdout (alphazero_amd.resign) -- a side whose value max(v_mean, v_best) stayed below the threshold for `consecutive` tested
        plies resigns, except in the holdout share of the games, which are played out and only note the trigger.  holdout = 1.0
        records the game log and changes no sample.  Served by run() in every search mode; advance() never resigns."""
        from .resign import parse
        r = parse(resign)
        if r is None:
            check(lib().az_engine_set_resign(self.h, float("nan"), 0, 0, 0.0))
        else:
            check(lib().az_engine_set_resign(self.h, r["threshold"], r["consecutive"], r["min_ply"], r["holdout"]))

    def resign_stats(self):
        """{"resigned", "holdout_games", "holdout_triggered", "holdout_false_positives"} of the games ended since the last run() /
        set_roots(); all 0 with the mode off"""
        v = [C.c_int64() for _ in range(4)]
        check(lib().az_engine_resign_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("resigned", "holdout_games", "holdout_triggered", "holdout_false_positives"), (x.value for x in v)))

    GAME_LOG_COLUMNS = ("game_id", "plies", "winner", "ended", "holdout", "trigger_ply", "trigger_player")

    def game_log(self):
        """the game log of the last run() as a dict of CUDA tensors (copies): one entry per game at index game id - first_game_id --
        the int32 [n] columns game_id, plies, winner, ended (0 the rules / 1 resignation), holdout, trigger_ply (-1: none),
        trigger_player (0: none), the rows themselves as "rows" int32 [n, 8], and "low" float64 [n, 2] (column 0 player +1, column 1
        player -1; 2.0: the window was never full).  n = 0 when that run had resignation off."""
        n, rows, low = C.c_int64(), C.c_void_p(), C.c_void_p()
        check(lib().az_engine_game_log(self.h, C.byref(n), C.byref(rows), C.byref(low)))
        r = _wrap(rows.value, (n.value, 8), torch.int32, self).clone()
        out = {k: r[:, i].contiguous() for i, k in enumerate(self.GAME_LOG_COLUMNS)}
        out["rows"] = r
        out["low"] = _wrap(low.value, (n.value, 2), torch.float64, self).clone()
        return out

    def resign_values(self):
        """float64 [n_slots] on the device: the resignation rule's value max(v_mean, v_best) of every slot's root as it stands, NaN
        where the root's children hold no visit or the slot holds no game (az_engine_resign_values; one launch, reads only)"""
        out = torch.empty(self.cfg.n_slots, dtype=torch.float64, device="cuda")
        check(lib().az_engine_resign_values(self.h, out.data_ptr()))
        return out

    @staticmethod
    def resign_value(N, Q):
        """the rule's value of a root whose children, in child order, have visit counts N and values Q; NaN when no child was visited
        (az_resign_value: host code, the kernels' arithmetic)"""
        N = np.ascontiguousarray(N, np.int32)
        Q = np.ascontiguousarray(Q, np.float64)
        if not (N.ndim == Q.ndim == 1 and len(N) == len(Q)):
            raise ValueError("resign_value: N and Q are one-dimensional and of one length")
        v = C.c_double()
        check(lib().az_resign_value(len(N), N.ctypes.data, Q.ctypes.data, C.byref(v)))
        return v.value

    @staticmethod
    def resign_holdout(seed, game_id, p):
        """the holdout coin of (seed, game id): True = the game is played out whatever the rule says (az_resign_holdout: host code)"""
        return bool(lib().az_resign_holdout(int(seed) & 0xFFFFFFFF, int(game_id) & 0xFFFFFFFF, float(p)))

    def set_forced_playouts(self, k):
        """forced playouts and policy target pruning (az_engine_set_forced_playouts): None = off, or k in (0, 64]
        (KataGo: 2) -- on a fully searched ply every visited root child gets at least sqrt(k P N_root) playouts, and the recorded
        policy (and the move drawn from it) leaves out the forced playouts PUCT would not have spent.  Plain search of EVAL_NET /
        EVAL_FAKE engines, with the playout cap or without; any other mode is a ValueError that names it."""
        from .forced_playouts import parse
        k = parse(k)
        check(lib().az_engine_set_forced_playouts(self.h, 0.0 if k is None else k))

    def forced_playouts_stats(self):
        """{"forced_picks", "pruned_playouts"}: the root selections with a forced child (folded in when the ply's move is played) and
        the playouts pruned from the recorded policy targets since the last run() / set_roots(); both 0 with the mode off"""
        picks, pruned = C.c_int64(), C.c_int64()
        check(lib().az_engine_forced_playouts_stats(self.h, C.byref(picks), C.byref(pruned)))
        return {"forced_picks": picks.value, "pruned_playouts": pruned.value}

    def set_exact_endgame(self, max_empties):
        """exact endgames (az_engine_set_exact_endgame): None = off, or E in [1, 10] -- a leaf of the search with at
        most E empty cells is solved by alpha-beta on the device and becomes a terminal node whose winner is the outcome under
        optimal play; it takes no row of the network batch.  Plain search of EVAL_NET / EVAL_FAKE engines (one leaf per lock-step, no
        playout cap, no forced playouts); any other mode is a ValueError that names it.  A change over searched trees is refused:
        set_roots() / run() first."""
        from .endgame import parse
        e = parse(max_empties)
        check(lib().az_engine_set_exact_endgame(self.h, 0 if e is None else e))

    def exact_endgame_stats(self):
        """{"solved_leaves", "solver_nodes"}: the leaves solved (each node once) and the positions the solver entered for them since
        the last run() / set_roots(); both 0 with the mode off"""
        solved, nodes = C.c_int64(), C.c_int64()
        check(lib().az_engine_exact_endgame_stats(self.h, C.byref(solved), C.byref(nodes)))
        return {"solved_leaves": solved.value, "solver_nodes": nodes.value}

    def set_proof_backup(self, on):
        """proof backup, MCTS-Solver (az_engine_set_proof_backup): a node is proven as soon as its children decide
        it -- some child a proven win for its mover, or every child proven -- proven nodes are not searched again, and the move
        and the policy target leave out proven losses (or keep the proven wins alone).  Plain search of EVAL_NET / EVAL_FAKE engines,
        with exact endgames, the evaluation cache and slot groups or without; any other mode is a ValueError that names it.  A
        change over searched trees is refused: set_roots() / run() first."""
        check(lib().az_engine_set_proof_backup(self.h, 1 if on else 0))

    def proof_backup_stats(self):
        """{"proven_nodes", "proof_stops", "pruned_plies"}: interior nodes marked proven, walks that ended on one, and plies whose
        policy counts the proofs changed, since the last run() / set_roots(); all 0 with the mode off"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().az_engine_proof_backup_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"proven_nodes": a.value, "proof_stops": b.value, "pruned_plies": c.value}

    def root_proofs(self):
        """int8 [n_slots] on the device: the proven outcome (-1, 0, +1: an absolute player id) of every slot's root, endgame.UNSOLVED
        (2) for a root that is not decided and for a slot without a game (az_engine_root_proofs; one launch)"""
        out = torch.empty(self.cfg.n_slots, dtype=torch.int8, device="cuda")
        check(lib().az_engine_root_proofs(self.h, out.data_ptr()))
        return out

    def set_puct(self, spec=None, c_base=None, fpu=None):
        """the PUCT exploration settings (az_engine_set_puct): `spec` as alphazero_amd.puct takes it -- None (off: the
        reference's PUCT), a number (c_init) or a dict of c_init, c_base, fpu -- or the three values themselves,
        set_puct(c_init, c_base, fpu) (fpu None or negative: off).  The exploration constant of a node with N visits is c_init +
        log((1 + N + c_base) / c_base) (c_base 0: c_init), an unvisited child's Q is the parent's value - fpu * sqrt(the prior mass of
        the visited children).  (1.0, 0, off) is the mode off.  Plain search of EVAL_NET / EVAL_FAKE engines, with slot groups and the
        evaluation cache or without; any other mode is a ValueError that names it.  The settings may change between two searches."""
        from .puct import parse
        if c_base is not None or fpu is not None:
            spec = {"c_init": 1.0 if spec is None else spec, "c_base": 0.0 if c_base is None else c_base, "fpu": fpu}
        c_init, c_base, fpu = parse(spec)
        check(lib().az_engine_set_puct(self.h, c_init, c_base, fpu))

    @property
    def puct(self):
        """(c_init, c_base, fpu) in force; fpu -1.0: off.  (1.0, 0.0, -1.0) is the mode off"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(lib().az_engine_puct(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return (a.value, b.value, c.value)

    def set_eval_cache(self, mode=None, capacity=0, stone_limit=0):
        """the leaf evaluation cache of run() (az_engine_set_eval_cache): each slot group keeps the network's
        outputs by exact position, so a leaf another game of the wave already sent through the network takes no batch row; the
        samples do not change by a bit.  mode None = the measured rule, False = off, True = on wherever it is served (run() of an
        EVAL_NET engine in the plain search; any other mode is a ValueError that names it).  capacity: entries per group, a power
        of two (0: 2^18); stone_limit: only positions with at most that many stones are cached (0: 12)."""
        m = -1 if mode is None else (1 if mode else 0)
        check(lib().az_engine_set_eval_cache(self.h, m, int(capacity), int(stone_limit)))

    def eval_cache_stats(self):
        """{"in_force", "cache_hits"}: whether the next run() would cache, and the leaves answered from the cache since the last
        run() began (they count in stats()["net_evals"] too: net_evals - cache_hits rows went through the network)"""
        on, hits = C.c_int32(), C.c_int64()
        check(lib().az_engine_eval_cache_stats(self.h, C.byref(on), C.byref(hits)))
        return {"in_force": bool(on.value), "cache_hits": hits.value}

    def step_heads(self):
        """{"in_force", "used"}: whether the next run() would compute the policy / value heads inside its step kernels (k_step_heads;
        AZ_ENGINE_STEP_HEADS, read when the engine is created: unset = the measured rule, 0 = never, 1 = wherever served), and whether
        the last run() did"""
        on, used = C.c_int32(), C.c_int32()
        check(lib().az_engine_step_heads(self.h, C.byref(on), C.byref(used)))
        return {"in_force": bool(on.value), "used": bool(used.value)}

    @staticmethod
    def forced_playout(n, p, root_n, k):
        """the forced test of a root child with n visits and prior p under a root of root_n visits: True = forced (az_forced_playout:
        host code, the kernels' arithmetic)"""
        return bool(lib().az_forced_playout(int(n), float(p), int(root_n), float(k)))

    @staticmethod
    def forced_prune(N, Q, P, root_n, k):
        """the pruned visit counts (int32 array) of a root's children given in child order (az_forced_prune: host code, the kernels'
        arithmetic)"""
        N = np.ascontiguousarray(N, np.int32)
        Q = np.ascontiguousarray(Q, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        if not (N.ndim == Q.ndim == P.ndim == 1 and len(N) == len(Q) == len(P)):
            raise ValueError("forced_prune: N, Q and P are one-dimensional and of one length")
        out = np.empty_like(N)
        check(lib().az_forced_prune(len(N), N.ctypes.data, Q.ctypes.data, P.ctypes.data, int(root_n), float(k), out.ctypes.data))
        return out

    def set_gumbel(self, gumbel):
        """the Gumbel root search (az_engine_set_gumbel; alphazero_amd.gumbel.parse: None = off, an int m or a dict of m, c_visit,
        c_scale, gumbel_scale): Sequential Halving over m root actions sampled with Gumbel noise, the move and the policy target
        from the completed Q-values.  EVAL_NET / EVAL_FAKE engines at leaf_batch 1; combines with the symmetry modes."""
        from .gumbel import parse
        g = parse(gumbel)
        m, cv, cs, gs = (0, 0.0, 0.0, 0.0) if g is None else g
        check(lib().az_engine_set_gumbel(self.h, m, cv, cs, gs))

    def set_gumbel_batch(self, k):
        """k Sequential Halving leaves per slot and lock-step of the Gumbel root search (az_engine_set_gumbel_batch; DESIGN section
        17; 1: one, the default).  Accepted with the mode on or off, in force while it is on; not with a symmetry ensemble; the
        network needs max_batch >= k * n_slots."""
        from .gumbel import check_gumbel_batch
        check(lib().az_engine_set_gumbel_batch(self.h, check_gumbel_batch(k, gumbel=True)))

    def set_gumbel_full(self, on):
        """the full Gumbel search (az_engine_set_gumbel_full): every evaluated node keeps its network value, v_mix
        is the paper's (the node's own value mixed with its visited children), and below the root the child is chosen
        deterministically by pi' - N / (1 + sum N) instead of PUCT.  Accepted with the Gumbel mode on or off, in force while it is
        on.  It cannot come into force on trees that were searched without it: set_roots (or a reset of the player) first."""
        from .gumbel import check_gumbel_full
        check(lib().az_engine_set_gumbel_full(self.h, int(check_gumbel_full(on, gumbel=True))))

    def root_value(self, slot=0):
        """the network value stored for the slot's root, in the frame of the player to move there (float32 as a Python float); an
        error unless set_gumbel_full is in force and the root is evaluated"""
        v = C.c_float()
        check(lib().az_engine_root_value(self.h, int(slot), C.byref(v)))
        return v.value

    def considered(self, slot=0):
        """the root children the slot's Sequential Halving considers now, as ascending child indices ([]: none chosen yet, which
        reads as all children)"""
        mask = C.c_uint64()
        check(lib().az_engine_gumbel_considered(self.h, int(slot), C.byref(mask)))
        return [i for i in range(64) if (mask.value >> i) & 1]

    def run(self, n_games, first_game_id=0):
        """plays n_games to completion; returns the samples as a dict of CUDA tensors (copies)."""
        self._evaluated(lib().az_engine_run(self.h, first_game_id, n_games))
        return self.samples()

    def samples(self, copy=True):
        n = C.c_int64()
        ps = [C.c_void_p() for _ in range(5)]
        check(lib().az_engine_samples(self.h, C.byref(n), *[C.byref(p) for p in ps]))
        S = n.value
        H, W = self.cfg.H, self.cfg.W
        out = {"state": _wrap(ps[0].value, (S, H, W), torch.int8, self), "pi": _wrap(ps[1].value, (S, self.A), torch.float32, self),
               "z": _wrap(ps[2].value, (S,), torch.int8, self), "meta": _wrap(ps[3].value, (S, 4), torch.int32, self),
               "visits": _wrap(ps[4].value, (S, self.A), torch.int32, self)}
        return {k: v.clone() for k, v in out.items()} if copy else out

    def stats(self):
        st = EngineStats()
        check(lib().az_engine_get_stats(self.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    # finer-grained control ------------------------------------------------------------------
    def set_roots(self, grids, players, game_ids=None, plies=None):
        g = np.ascontiguousarray(grids, np.int8).reshape(-1, self.cells)
        p = np.ascontiguousarray(players, np.int8)
        gi = np.ascontiguousarray(game_ids, np.uint32) if game_ids is not None else None
        pl = np.ascontiguousarray(plies, np.int32) if plies is not None else None
        check(lib().az_engine_set_roots(self.h, g.ctypes.data, p.ctypes.data, gi.ctypes.data if gi is not None else None,
                                        pl.ctypes.data if pl is not None else None, len(p)))

    def search(self, n_sim):
        self._evaluated(lib().az_engine_search(self.h, n_sim))

    def search_begin(self, n_sim):
        """queues the search and returns; search_end() waits for it (another engine may search in between: the arena's two players)"""
        self._evaluated(lib().az_engine_search_begin(self.h, n_sim))

    def pair_with(self, other):
        """puts `other`'s stream on a hardware queue of its own so that overlapped searches of the two engines run side by side"""
        check(lib().az_engine_pair(self.h, other.h))

    def search_end(self):
        check(lib().az_engine_search_end(self.h))

    def advance(self):
        check(lib().az_engine_advance(self.h))

    def play(self, actions):
        """Board.play_move + MCT.change_root with externally chosen moves for slots 0..len(actions)-1"""
        a = np.ascontiguousarray(actions, np.int32)
        st = np.zeros(len(a), np.int32)
        check(lib().az_engine_play(self.h, a.ctypes.data, len(a), st.ctypes.data))

    # arena support -------------------------------------------------------------------------------
    def set_sides(self, sides):
        s = np.ascontiguousarray(sides, np.int8)
        check(lib().az_engine_set_sides(self.h, s.ctypes.data, len(s)))

    def best_moves(self):
        a = np.zeros(self.cfg.n_slots, np.int32)
        check(lib().az_engine_best_moves(self.h, a.ctypes.data))
        return a

    def player_moves(self, temp=0.0):
        """the move every slot's player plays now (az_engine_player_moves): root_readout(temps=temp)["action"] as a host int32 vector,
        what advance() would play at that temperature -- the Gumbel move in the Gumbel mode, whatever `temp` is; best_moves() stays
        visit-based in every mode.  -1 for a slot this engine does not search now or whose root is not expanded.  Reads only."""
        a = np.zeros(self.cfg.n_slots, np.int32)
        check(lib().az_engine_player_moves(self.h, float(temp), a.ctypes.data))
        return a

    def baseline_moves(self, kind, seed=0):
        a = np.zeros(self.cfg.n_slots, np.int32)
        check(lib().az_engine_baseline_moves(self.h, {"random": 0, "greedy": 1}[kind], seed, a.ctypes.data))
        return a

    def root_status(self):
        G = self.cfg.n_slots
        pl = np.zeros(G, np.int8); ov = np.zeros(G, np.uint8); wi = np.zeros(G, np.int8); sc = np.zeros(G, np.int32)
        check(lib().az_engine_root_status(self.h, pl.ctypes.data, ov.ctypes.data, wi.ctypes.data, sc.ctypes.data))
        return pl, ov.astype(bool), wi, sc

    def root_children(self, slot):
        a = np.zeros(65, np.int32); n = np.zeros(65, np.int32); q = np.zeros(65, np.float64); p = np.zeros(65, np.float64)
        k, rn = C.c_int32(), C.c_int32()
        check(lib().az_engine_root_children(self.h, slot, a.ctypes.data, n.ctypes.data, q.ctypes.data, p.ctypes.data,
                                            C.byref(k), C.byref(rn)))
        k = k.value
        return a[:k].copy(), n[:k].copy(), q[:k].copy(), p[:k].copy(), rn.value

    _READOUT = (("visits", torch.int32, True), ("pi", torch.float32, True), ("Q", torch.float64, True), ("P", torch.float64, True),
                ("child", torch.uint8, True), ("action", torch.int32, False), ("root_N", torch.int32, False))

    def root_readout(self, temps=None, pv_len=0, n=None, out=None):
        """Player.get_move's results (players.py:158-191) for slots 0..n-1 (default: all) in one kernel launch: a dict of CUDA tensors
        visits int32 [n, A], pi float32 [n, A], Q / P float64 [n, A], child uint8 [n, A] (1: the root holds a child for the action),
        action int32 [n], root_N int32 [n] and, when pv_len > 0, pv int32 [n, pv_len] (the principal line, -1 padded).  pi and action
        are what advance() would record and play now at the slot's temperature: `temps` (one number or one per slot; 0 = most
        visited under the engine's tie mode), or the engine's scheduler at the slot's ply when None.  A slot this engine does not
        search now, or whose root is not expanded, reads action -1 and zeros.  Nothing in the engine changes.  `out` may bring
        tensors to fill (same names, at least n rows: rows beyond n stay as they are); what it lacks is allocated."""
        G, A = self.cfg.n_slots, self.A
        n = G if n is None else int(n)
        rows = max(n, 0)
        res, ro = {}, _lib.RootReadout()
        shapes = [(k, dt, (rows, A) if wide else (rows,)) for k, dt, wide in self._READOUT]
        if pv_len > 0 or (out is not None and "pv" in out):
            shapes.append(("pv", torch.int32, (rows, max(int(pv_len), 0))))
        for k, dt, shape in shapes:
            t = out.get(k) if out is not None else None
            if t is None:
                t = torch.empty(shape, dtype=dt, device="cuda")
            elif k == "pv" and pv_len <= 0 and t.is_cuda and t.dtype == dt:
                pass  # a line buffer without a length: the library refuses it
            elif not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.shape[0] >= rows and tuple(t.shape[1:]) == shape[1:]):
                raise ValueError(f"root_readout: out[{k!r}] must be a contiguous CUDA {dt} tensor of shape {shape} (or more rows)")
            res[k] = t
            setattr(ro, "d_" + k, t.data_ptr() if t.numel() else None)
        ro.pv_len = int(pv_len)
        tp = None
        if temps is not None:
            t = np.asarray(temps, np.float64)
            t = np.full(rows, float(t), np.float64) if t.ndim == 0 else np.ascontiguousarray(t.reshape(-1))
            if len(t) != rows:
                raise ValueError(f"root_readout: {len(t)} temperatures for {rows} slots")
            tp = t.ctypes.data
        check(lib().az_engine_root_readout(self.h, tp, n, C.byref(ro)))
        return res

    def nodes_used(self, slot=0):
        n = C.c_int32()
        check(lib().az_engine_nodes_used(self.h, slot, C.byref(n)))
        return n.value

    def grow_pools(self, node_capacity):
        """re-allocates the tree pools with a larger capacity; the trees are kept"""
        check(lib().az_engine_grow_pools(self.h, node_capacity))
        self.cfg.node_capacity = node_capacity

    def close(self):
        if getattr(self, "h", None):
            lib().az_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
