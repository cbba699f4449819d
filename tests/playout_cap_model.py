"""Host model of playout cap randomization (az_engine_set_playout_cap): a plain restatement of the contract on
leaf_batch_model.Model at K = 1 (its hash noise, both tie modes), for tests.  Not a conftest, not a test module.

Contract -- the mode is default off; setting: n_fast in [1, n_sim), p_full in (0, 1], n_fast = 0 switches it off.
  coin       per (game id, ply): r = philox4x32(seed, game_id, ply, 0xFFFF, P_PLAYOUT_CAP = 10, 0), u = u53(r[0], r[1]); the ply is FULL
             iff u < p_full (1.0: every ply).  Never a function of the slot, the slot group, the batch or the games resident.
  full ply   today's behaviour: every simulation of the search call, root noise under the engine's noise mode, the sample recorded.
  fast ply   a search call of n simulations walks the local simulation indices s < min(n, n_fast) only (every call again); no root
             noise, the root is not marked noised; a fresh root is still evaluated first.  The move is chosen and played as ever
             (temperature schedule, the P_MOVE_SAMPLE / P_TIE_MOVE draws, re-rooting), but NO sample is recorded.  The tree under
             the played move is kept: a full ply that follows inherits it.
  counters   plies counts every ply; full_plies / fast_plies count the two kinds: samples == full_plies, plies == full + fast.
The coin is restated here from closed_form.philox4x32 and u53, independently of the library."""
import numpy as np

from alphazero_amd.gumbel import det_exp, det_log
from leaf_batch_model import Model, action_size, make_board
from tools import closed_form as cf

P_PLAYOUT_CAP = 10


def coin_full(seed, game_id, ply, p_full):
    r = cf.philox4x32(int(seed) & 0xFFFFFFFF, int(game_id) & 0xFFFFFFFF, int(ply) & 0xFFFFFFFF, 0xFFFF, P_PLAYOUT_CAP, 0)
    return cf.u53(r[0], r[1]) < float(p_full)


def is_full(cap, seed, game_id, ply):
    """cap: None (off: every ply is full) or (n_fast, p_full)"""
    return cap is None or coin_full(seed, game_id, ply, cap[1])


def linear_temp(step, tmax, tmin):
    """schedulers.py:33-40 as k_move restates it"""
    if step <= tmax:
        return 1.0
    if step >= tmin:
        return 0.0
    return 1.0 - float(step - tmax) / float(tmin - tmax)


def _pow(n, temp, inv):
    if temp == 1.0:
        return float(n)
    return det_exp(det_log(float(n)) * inv) if n > 0 else 0.0  # az_det_pow


def move_policy(m, temp):
    """move_policy of the engine on the model's root: (index of the chosen child, pi float32 [A])"""
    ch = m.root.children
    pi = np.zeros(m.A, np.float32)
    if temp == 0.0:
        best = max(c.N for c in ch)
        ties = [i for i, c in enumerate(ch) if c.N == best]
        k = 0
        if m.tie == "random" and len(ties) > 1:
            k = (cf.philox4x32(m.seed, m.gid, m.ply, 0xFFFF, cf.P_TIE_MOVE, 0)[0] * len(ties)) >> 32
        pi[ch[ties[k]].act] = 1.0
        return ties[k], pi
    inv = 1.0 / temp
    total = 0.0
    for c in ch:
        total += _pow(c.N, temp, inv)
    u = cf.move_sample_u(m.seed, m.gid, m.ply) if len(ch) > 1 else 2.0
    cum, chosen, last, found = 0.0, 0, 0, False
    for i, c in enumerate(ch):
        p = _pow(c.N, temp, inv) / total
        pi[c.act] = np.float32(p)
        if p > 0.0:
            last = i
        cum += p
        if not found and u < cum:
            chosen, found = i, True
    if not found:
        chosen = 0 if len(ch) == 1 else last
    return chosen, pi


def search_call(m, n, cap, noise):
    """one search call of n simulations on the model's root under the cap: the ply's noise and budget; returns True on a full ply"""
    full = is_full(cap, m.seed, m.gid, m.ply)
    m.noise = noise if full else None
    walked = n if full else min(n, cap[0])
    m.search(walked)
    m.sim_base += n - walked  # the engine's simulation counter moves by the call's n, whatever a slot walked
    return full


def reroot(m, idx):
    new = m.root.children[idx]
    m._board(new)
    new.parent = None
    m.root, m.ply, m.sim_base = new, m.ply + 1, 0
    return new.act


def advance(m, tmax, tmin, full):
    """k_move on the model: the sample of a full ply (None on a fast one), the move, the re-rooting"""
    b = m._board(m.root)
    idx, pi = move_policy(m, linear_temp(m.ply, tmax, tmin))
    smp = None
    if full:
        vis = np.zeros(m.A, np.int32)
        for c in m.root.children:
            vis[c.act] = c.N
        smp = {"state": (b.player * b.grid).astype(np.int8), "pi": pi, "visits": vis, "root_N": m.root.N,
               "meta": np.array([m.gid, m.ply, b.player, m.root.children[idx].act], np.int64).astype(np.uint32).view(np.int32)}
    reroot(m, idx)
    return smp


def play_game(game, H, W, seed, game_id, n_sim, cap, noise, tie, tmax, tmin):
    """one self-play game: (samples of its full plies with z, counters)"""
    m = Model(make_board(game, H, W), K=1, noise=None, tie=tie, seed=seed, game_id=game_id)
    samples, full_plies, fast_plies = [], 0, 0
    while True:
        full = search_call(m, n_sim, cap, noise)
        smp = advance(m, tmax, tmin, full)
        full_plies += 1 if full else 0
        fast_plies += 0 if full else 1
        if smp is not None:
            samples.append(smp)
        b = m.root.board
        if b.is_game_over():
            w = int(b.get_winner())
            for s in samples:
                s["z"] = np.int8(w * int(s["meta"][2]))
            break
    return samples, {"full_plies": full_plies, "fast_plies": fast_plies, "rows": m.rows}


def play_wave(game, H, W, seed, first_game_id, n_games, n_sim, cap, noise, tie, tmax, tmin):
    """az_engine_run on the model: the samples as arrays sorted by (game id, move idx), and the counters"""
    A = action_size(make_board(game, H, W))
    out = {"state": [], "pi": [], "visits": [], "meta": [], "z": [], "root_N": []}
    ctr = {"full_plies": 0, "fast_plies": 0, "rows": 0}
    for g in range(first_game_id, first_game_id + n_games):
        smp, c = play_game(game, H, W, seed, g, n_sim, cap, noise, tie, tmax, tmin)
        for k in ctr:
            ctr[k] += c[k]
        for s in smp:
            for k in out:
                out[k].append(s[k])
    S = len(out["z"])
    arr = {"state": np.array(out["state"], np.int8).reshape(S, H, W), "pi": np.array(out["pi"], np.float32).reshape(S, A),
           "visits": np.array(out["visits"], np.int32).reshape(S, A), "meta": np.array(out["meta"], np.int32).reshape(S, 4),
           "z": np.array(out["z"], np.int8).reshape(S), "root_N": np.array(out["root_N"], np.int64).reshape(S)}
    ctr.update(samples=S, plies=ctr["full_plies"] + ctr["fast_plies"], games_done=n_games)
    return arr, ctr
