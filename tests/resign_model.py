"""Host model of resignation in self-play (az_engine_set_resign): a plain restatement of the contract on
playout_cap_model / leaf_batch_model.Model at K = 1 (its hash noise, both tie modes), for tests.  Not a conftest, not a test module.

Contract -- the mode is default off; settings: v_resign in [-1, 0), consecutive = k in [1, 4], min_ply >= 0, p_holdout in [0, 1].
  value      of a ply, from the root's children after the ply's search, in child order: S_N = sum N_i; S_Q = sum over N_i > 0 of
             float(N_i) * Q_i in that order in float64; v_mean = S_Q / S_N; v_best = Q of the child with the greatest N (the lowest
             index among equals); v = v_best if v_best > v_mean else v_mean.  S_N == 0: the ply is untested.  Raw N and Q only.
  tested     after the ply is recorded and played as ever, and only if the rules have not ended the game.  A ply p < min_ply and a
             fast ply of the playout cap are untested.  A tested ply pushes v into the mover's window of its last k tested values
             (one per side and game).  m = the maximum of a full window; low[side] = the minimum of m over the game, 2.0 while the
             window was never full.  The side triggers at the first ply where m < v_resign.
  holdout    per game: r = philox4x32(seed, game_id, 0, 0xFFFF, P_RESIGN = 11, 0), u = u53(r[0], r[1]); holdout iff u < p_holdout.
  trigger    not a holdout: the mover resigns, the game ends now with winner -mover, z from that winner; the ply just played stays
             recorded and counted.  A holdout: only the first trigger is noted (ply, player), the game goes on, low keeps updating.
  counters   resigned, holdout_games, holdout_triggered, holdout_false_positives (a holdout game with a trigger and
             winner * trigger_player >= 0).
  log        per game: [game_id, plies, winner, ended (0 rules / 1 resignation), holdout, trigger_ply (-1), trigger_player (0), 0]
             and low = [low of player +1, low of player -1].
The coin is restated here from closed_form.philox4x32 and u53, independently of the library."""
import numpy as np

import playout_cap_model as M
from leaf_batch_model import Model, action_size, make_board
from tools import closed_form as cf

P_RESIGN = 11


def value(N, Q):
    """the value of a ply from the children's visit counts and values in child order; None when no child was visited"""
    sn, sq, best, vbest = 0, 0.0, -1, 0.0
    for n, q in zip(N, Q):
        n, q = int(n), float(q)
        if n > 0:
            sn += n
            sq += float(n) * q
        if n > best:
            best, vbest = n, q
    if sn == 0:
        return None
    vmean = sq / float(sn)
    return vbest if vbest > vmean else vmean


def root_value(m):
    return value([c.N for c in m.root.children], [c.Q for c in m.root.children])


def holdout(seed, game_id, p):
    r = cf.philox4x32(int(seed) & 0xFFFFFFFF, int(game_id) & 0xFFFFFFFF, 0, 0xFFFF, P_RESIGN, 0)
    return cf.u53(r[0], r[1]) < float(p)


def play_game(game, H, W, seed, game_id, n_sim, resign, cap, noise, tie, tmax, tmin):
    """one self-play game under resign = (v_resign, k, min_ply, p_holdout) and the playout cap `cap` (None: off): (samples with z,
    counters, the game's log row as a list of 8 ints, [low of +1, low of -1])"""
    thr, k, min_ply, p_hold = resign
    m = Model(make_board(game, H, W), K=1, noise=None, tie=tie, seed=seed, game_id=game_id)
    ho = holdout(seed, game_id, p_hold)
    windows, low = {1: [], -1: []}, {1: 2.0, -1: 2.0}
    samples, full_plies, fast_plies = [], 0, 0
    trig_ply, trig_player, ended = -1, 0, 0
    while True:
        full = M.search_call(m, n_sim, cap, noise)
        ply, mover = m.ply, int(m._board(m.root).player)
        v = root_value(m)  # the children the search left: the move below does not change them
        smp = M.advance(m, tmax, tmin, full)
        full_plies += 1 if full else 0
        fast_plies += 0 if full else 1
        if smp is not None:
            samples.append(smp)
        b = m.root.board
        if b.is_game_over():
            w = int(b.get_winner())
            break
        if ply < min_ply or not full or v is None:
            continue
        windows[mover].append(v)
        if len(windows[mover]) < k:
            continue
        mx = max(windows[mover][-k:])
        if mx < low[mover]:
            low[mover] = mx
        if mx < thr and trig_ply < 0:
            trig_ply, trig_player = ply, mover
            if not ho:
                w, ended = -mover, 1
                break
    for s in samples:
        s["z"] = np.int8(w * int(s["meta"][2]))
    fp = 1 if ho and trig_ply >= 0 and w * trig_player >= 0 else 0
    ctr = {"full_plies": full_plies, "fast_plies": fast_plies, "rows": m.rows, "resigned": ended, "holdout_games": int(ho),
           "holdout_triggered": int(ho and trig_ply >= 0), "holdout_false_positives": fp}
    gid32 = int(np.array([game_id], np.int64).astype(np.uint32).view(np.int32)[0])
    row = [gid32, m.ply, w, ended, int(ho), trig_ply, trig_player, 0]
    return samples, ctr, row, [low[1], low[-1]]


def play_wave(game, H, W, seed, first_game_id, n_games, n_sim, resign, cap, noise, tie, tmax, tmin):
    """az_engine_run on the model: the samples as arrays sorted by (game id, move idx), the counters, the log rows int32 [n, 8] and
    low float64 [n, 2]"""
    A = action_size(make_board(game, H, W))
    out = {"state": [], "pi": [], "visits": [], "meta": [], "z": [], "root_N": []}
    ctr = {"full_plies": 0, "fast_plies": 0, "rows": 0, "resigned": 0, "holdout_games": 0, "holdout_triggered": 0, "holdout_false_positives": 0}
    rows, lows = [], []
    for g in range(first_game_id, first_game_id + n_games):
        smp, c, row, low = play_game(game, H, W, seed, g, n_sim, resign, cap, noise, tie, tmax, tmin)
        for k in ctr:
            ctr[k] += c[k]
        rows.append(row)
        lows.append(low)
        for s in smp:
            for k in out:
                out[k].append(s[k])
    S = len(out["z"])
    arr = {"state": np.array(out["state"], np.int8).reshape(S, H, W), "pi": np.array(out["pi"], np.float32).reshape(S, A),
           "visits": np.array(out["visits"], np.int32).reshape(S, A), "meta": np.array(out["meta"], np.int32).reshape(S, 4),
           "z": np.array(out["z"], np.int8).reshape(S), "root_N": np.array(out["root_N"], np.int64).reshape(S)}
    ctr.update(samples=S, plies=ctr["full_plies"] + ctr["fast_plies"], games_done=n_games)
    return arr, ctr, np.array(rows, np.int32).reshape(n_games, 8), np.array(lows, np.float64).reshape(n_games, 2)
