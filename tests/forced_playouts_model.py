"""Host model of forced playouts and policy target pruning (az_engine_set_forced_playouts): a plain restatement of the
contract on leaf_batch_model.Model at K = 1 and on playout_cap_model's coin, move_policy and wave loop, for tests.  Not a conftest,
not a test module.  Rules 3 - 5 are restated here in Python floats (IEEE doubles, one operation at a time), independently of the
library.

Contract -- the mode is default off; k > 0 switches it on (KataGo: 2), k = 0 off; k finite and in [0, 64].
  forced ply  a ply that is full in the playout cap's sense with the mode on: every ply with the cap off, with it on the plies whose
              coin says full.  Fast plies take no forced playouts and no pruning.
  selection   (rule 3) at depth 0 of the walk on a forced ply only.  R.N = the root's visit count as PUCT's square root takes it.
              Child c is forced iff c.N > 0 and float(c.N) * float(c.N) < (k * c.P) * float(R.N), c.P the stored prior with root
              noise.  A forced child's key is +inf, the others keep their PUCT keys, the maximum is chosen as ever: several forced
              children are an ordinary tie (random: the P_TIE_SELECT draw of (ply, sim, depth 0); lowest: the lowest index).  A
              fresh root has R.N = 0 and forces nothing; an inherited root applies the rule to the counts it inherited.
  pruning     (rule 4) wherever move_policy runs on a forced ply at a temperature other than 0.  c* = the child with the greatest N
              (lowest index among equals); sq = sqrt(float(R.N)); star = c*.Q + (c*.P * sq) / float(1 + c*.N).  N' = N for c* and
              for N = 0; else nf = int(sqrt((k * c.P) * float(R.N))), gap = star - c.Q, need = c.N if gap <= 0.0, otherwise
              want = (c.P * sq) / gap - 1.0 and need = c.N if want >= float(c.N) else int(floor(want)) + 1;
              N' = min(c.N, max(c.N - nf, need, 0)); if N' < c.N and N' <= 1 then N' = 0.  The temperature formula takes N' for pi
              and for the move drawn from it (the same P_MOVE_SAMPLE draw).  Temperature 0 and the visits rows keep the raw counts.
  counters    (rule 5) forced_picks = the root selections with at least one forced child, folded in per ply when the move is played;
              pruned_playouts = the sum of N - N' over the recorded plies."""
import math

import numpy as np

import playout_cap_model as PC
from leaf_batch_model import Model, action_size, make_board
from tools import closed_form as cf


def forced(n, p, root_n, k):
    """rule 3: is a root child with n visits and stored prior p forced under a root of root_n visits?"""
    return n > 0 and float(n) * float(n) < (k * p) * float(root_n)


def prune(N, Q, P, root_n, k):
    """rule 4: the pruned counts N' of a root's children given in child order"""
    if not N:
        return []
    star_i = 0
    for i in range(1, len(N)):
        if N[i] > N[star_i]:
            star_i = i
    sq = math.sqrt(float(root_n))
    star = Q[star_i] + (P[star_i] * sq) / float(1 + N[star_i])
    out = []
    for i, (n, q, p) in enumerate(zip(N, Q, P)):
        if i == star_i or n == 0:
            out.append(n)
            continue
        nf = int(math.sqrt((k * p) * float(root_n)))
        gap = star - q
        if gap <= 0.0:
            need = n
        else:
            want = (p * sq) / gap - 1.0
            need = n if want >= float(n) else int(math.floor(want)) + 1
        m = min(n, max(n - nf, need, 0))
        if m < n and m <= 1:
            m = 0
        out.append(m)
    return out


class ForcedModel(Model):
    """leaf_batch_model.Model at K = 1 whose root selection applies rule 3 while self.kf > 0 (set per search call: the ply's k or 0)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        assert self.K == 1
        self.kf = 0.0
        self.picks = 0          # forced root selections since the last move (the engine's per-slot count)
        self.high_picks = 0     # ... of them the ones that chose a child of index >= 16 (for the test of a wide root)

    def _pick(self, parent, earlier, sim, depth):
        if depth != 0 or not self.kf > 0.0:
            return super()._pick(parent, earlier, sim, depth)
        sq = math.sqrt(float(parent.N))
        keys = []
        any_forced = False
        for c in parent.children:
            if forced(c.N, c.P, parent.N, self.kf):
                keys.append(math.inf)
                any_forced = True
            else:
                keys.append(c.Q + (c.P * sq) / float(1 + c.N))
        best = max(keys)
        ties = [i for i, key in enumerate(keys) if key == best]
        j = 0
        if self.tie == "random" and len(ties) > 1:
            r = cf.philox4x32(self.seed, self.gid, self.ply, (sim + self.sim_base) & 0xFFFFFFFF, cf.P_TIE_SELECT, 0)
            j = (r[0] * len(ties)) >> 32
        if any_forced:
            self.picks += 1
            self.high_picks += 1 if ties[j] >= 16 else 0
        return parent.children[ties[j]]


def is_forced_ply(k, cap, seed, game_id, ply):
    return k is not None and k > 0.0 and PC.is_full(cap, seed, game_id, ply)


def pruned_counts(m, k):
    ch = m.root.children
    return prune([c.N for c in ch], [c.Q for c in ch], [c.P for c in ch], m.root.N, k)


def move_policy(m, temp, k):
    """move_policy of the engine on the model's root under the mode: (chosen child index, pi float32 [A], pruned playouts).
    k: the ply's k, or None / 0 when it is not a forced ply -- then playout_cap_model.move_policy as it is."""
    if not k or temp == 0.0:
        idx, pi = PC.move_policy(m, temp)
        return idx, pi, 0
    ch = m.root.children
    cnt = pruned_counts(m, k)
    pi = np.zeros(m.A, np.float32)
    inv = 1.0 / temp
    total = 0.0
    for n in cnt:
        total += PC._pow(n, temp, inv)
    u = cf.move_sample_u(m.seed, m.gid, m.ply) if len(ch) > 1 else 2.0
    cum, chosen, last, found = 0.0, 0, 0, False
    for i, c in enumerate(ch):
        p = PC._pow(cnt[i], temp, inv) / total
        pi[c.act] = np.float32(p)
        if p > 0.0:
            last = i
        cum += p
        if not found and u < cum:
            chosen, found = i, True
    if not found:
        chosen = 0 if len(ch) == 1 else last
    return chosen, pi, sum(c.N for c in ch) - sum(cnt)


def search_call(m, n, k, cap, noise):
    """one search call of n simulations under the mode (and the cap, or None); returns True on a full ply"""
    m.kf = k if is_forced_ply(k, cap, m.seed, m.gid, m.ply) else 0.0
    return PC.search_call(m, n, cap, noise)


def advance(m, tmax, tmin, full, k):
    """k_move on the model: (the sample of a full ply or None, the forced picks folded in, the playouts pruned from the record)"""
    b = m._board(m.root)
    kk = k if (full and k) else None
    idx, pi, cut = move_policy(m, PC.linear_temp(m.ply, tmax, tmin), kk)
    smp = None
    if full:
        vis = np.zeros(m.A, np.int32)
        for c in m.root.children:
            vis[c.act] = c.N
        raw = PC.move_policy(m, PC.linear_temp(m.ply, tmax, tmin))[1]
        smp = {"state": (b.player * b.grid).astype(np.int8), "pi": pi, "visits": vis, "root_N": m.root.N, "raw_pi": raw,
               "meta": np.array([m.gid, m.ply, b.player, m.root.children[idx].act], np.int64).astype(np.uint32).view(np.int32)}
    picks, m.picks = m.picks, 0
    PC.reroot(m, idx)
    return smp, picks, (cut if full else 0)


def play_game(game, H, W, seed, game_id, n_sim, k, cap, noise, tie, tmax, tmin):
    m = ForcedModel(make_board(game, H, W), K=1, noise=None, tie=tie, seed=seed, game_id=game_id)
    samples = []
    ctr = {"full_plies": 0, "fast_plies": 0, "forced_picks": 0, "pruned_playouts": 0}
    while True:
        full = search_call(m, n_sim, k, cap, noise)
        smp, picks, cut = advance(m, tmax, tmin, full, k)
        ctr["full_plies" if full else "fast_plies"] += 1
        ctr["forced_picks"] += picks
        ctr["pruned_playouts"] += cut
        if smp is not None:
            samples.append(smp)
        b = m.root.board
        if b.is_game_over():
            w = int(b.get_winner())
            for s in samples:
                s["z"] = np.int8(w * int(s["meta"][2]))
            break
    ctr["rows"] = m.rows
    return samples, ctr


def play_wave(game, H, W, seed, first_game_id, n_games, n_sim, k, cap, noise, tie, tmax, tmin):
    """az_engine_run on the model: the samples as arrays sorted by (game id, move idx) -- raw_pi is the unpruned policy of the same
    counts, for the tests' preconditions -- and the counters"""
    A = action_size(make_board(game, H, W))
    out = {"state": [], "pi": [], "visits": [], "meta": [], "z": [], "root_N": [], "raw_pi": []}
    ctr = {"full_plies": 0, "fast_plies": 0, "forced_picks": 0, "pruned_playouts": 0, "rows": 0}
    for g in range(first_game_id, first_game_id + n_games):
        smp, c = play_game(game, H, W, seed, g, n_sim, k, cap, noise, tie, tmax, tmin)
        for key in ctr:
            ctr[key] += c[key]
        for s in smp:
            for key in out:
                out[key].append(s[key])
    S = len(out["z"])
    arr = {"state": np.array(out["state"], np.int8).reshape(S, H, W), "pi": np.array(out["pi"], np.float32).reshape(S, A),
           "visits": np.array(out["visits"], np.int32).reshape(S, A), "meta": np.array(out["meta"], np.int32).reshape(S, 4),
           "z": np.array(out["z"], np.int8).reshape(S), "root_N": np.array(out["root_N"], np.int64).reshape(S),
           "raw_pi": np.array(out["raw_pi"], np.float32).reshape(S, A)}
    ctr.update(samples=S, plies=ctr["full_plies"] + ctr["fast_plies"], games_done=n_games)
    return arr, ctr


# ---- the waves tests/test_gpu_forced_playouts.py plays, and tests/test_forced_playouts_host.py checks the preconditions of
GAMES = {"othello6": ("othello", 0, 6, 6), "connect4": ("connect4", 1, 6, 7), "tictactoe": ("tictactoe", 2, 3, 3)}
N_SIMS = {"othello6": 12, "connect4": 24, "tictactoe": 24}
K, CAP, NOISE, TMAX, TMIN = 2.0, (4, 0.4), (0.5, 0.25), 2, 7  # temperatures 1, 0.8, 0.6, 0.4, 0.2, 0 over plies 2 .. 7
SEED, FIRST, N_GAMES, N_SLOTS = 11, 1000, 28, 20
_WAVES = {}


def wave(tag, tie, cap, n_games=N_GAMES):
    """the model's wave of a (game, tie mode), with the playout cap (CAP) or without (None); computed once per process"""
    key = (tag, tie, cap, n_games)
    if key not in _WAVES:
        game, _, H, W = GAMES[tag]
        _WAVES[key] = play_wave(game, H, W, SEED, FIRST, n_games, N_SIMS[tag], K, cap, NOISE, tie, TMAX, TMIN)
    return _WAVES[key]
