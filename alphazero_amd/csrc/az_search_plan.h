// The launch sequence of one search, decided once per search as a value: which step kernel family an engine's mode launches, how many
// lock-steps, and every launch's arguments.  az_engine.hip enqueues from the plan (enqueue_search, launch_step), counts lock-steps
// from it and keys its captured graphs by it; tests/search_plan_table.cpp prints it without a GPU.  With it the host arithmetic that
// sizes a search's network batch and splits the slots into groups.  Plain C++17, no HIP.
#pragma once
#include <tuple>

#include "../../include/az_amd.h"

#define AZ_SLOT_BLOCK 16  // games per 256-thread block of the step kernels (az_engine.hip: GPB): a slot group is whole blocks

// what a plan depends on (az_engine.hip: search_mode fills it from a chain's device view)
struct SearchMode {
    bool rollout;  // AZ_EVAL_ROLLOUT: no network
    int gm;        // the Gumbel root search's m (0: off)
    int K;         // walkers per slot and lock-step in force
    bool full;     // the Gumbel mode keeps the network's values (az_engine_set_gumbel_full in force)
    bool cap;      // the playout cap's budgets are in force
    bool forced;   // forced playouts are on
    int exact;     // exact endgames: the empties limit of a solved leaf (az_engine_set_exact_endgame; 0: off)
    bool proof;    // proof backup is on (az_engine_set_proof_backup)
    bool puct;     // the exploration settings are not the neutral (1.0, 0, off) (az_engine_set_puct)
};

// the kernel family of a search's lock-steps
enum SearchFamily { SF_ROLLOUT, SF_STEP, SF_STEP_CAP, SF_STEP_FORCED, SF_STEP_CAP_FORCED, SF_STEP_MULTI, SF_STEP_GUMBEL, SF_STEP_GUMBEL_MULTI, SF_STEP_EXACT, SF_STEP_PROOF, SF_STEP_PUCT };

inline const char *search_family_name(SearchFamily f) {
    static const char *const name[] = {"k_rollout_step", "k_step", "k_step_cap", "k_step_forced", "k_step_cap_forced", "k_step_multi", "k_step_gumbel", "k_step_gumbel_multi", "k_step_exact", "k_step_proof", "k_step_puct"};
    return name[f];
}

// Lmax(n, m, K) of the Gumbel mode with K walkers (the contract above k_step_gumbel_multi; gumbel.locksteps in Python): the longest
// per-slot plan of any m0 in 1 .. m.  A pure function of its arguments: the launch sequence of a search captures as a graph.
inline int gumbel_locksteps(int n, int m, int K) {
    int best = 0;
    for (int m0 = 1; m0 <= m; ++m0) {
        int L = 0, mp = m0, end = 0, steps = 0;
        for (int b = m0 - 1; b > 0; b >>= 1) ++L;  // ceil(log2 m0)
        for (int s = 0; s < n;) {
            while (end <= s) {  // the phase that holds s
                if (m0 == 1) { end = n; break; }
                int v = n / (L * mp);
                end += mp * (v < 1 ? 1 : v);
                mp = mp / 2 < 2 ? 2 : mp / 2;
            }
            const int stop = end < n ? end : n;
            s += stop - s < K ? stop - s : K;
            ++steps;
        }
        best = steps > best ? steps : best;
    }
    return best;
}

// One search: the root-prior pass (k_root_prep, the network, k_root_init; empty unless a slot holds a fresh root), then L lock-steps
// of [backup + select -> network] and the last backup.  A rollout engine has no network: n_sim launches of k_rollout_step, nothing else.
struct SearchPlan {
    SearchFamily family;
    bool full;       // the <.., true> instantiation of the two Gumbel families (no run-time branch inside the walk)
    bool root_pass;  // false only for rollout
    int L;           // lock-steps that are followed by a forward
    int launches;    // step-kernel launches: what one search adds to the engine's lockstep_iters
    bool exact;      // SF_STEP_PROOF only: the family's kernels that carry the solver (k_step_proof_exact); the cache is, as for every
                     // one-leaf family, a property of the chain (its table pointers), not of the plan
};

inline SearchPlan plan_search(const SearchMode &m, int n_sim) {
    SearchPlan p = {SF_STEP, m.full, true, n_sim, 0, false};
    if (m.rollout) { p.family = SF_ROLLOUT; p.root_pass = false; p.L = 0; p.launches = n_sim; return p; }  // one launch per simulation
    if (m.gm > 0 && m.K > 1) { p.family = SF_STEP_GUMBEL_MULTI; p.L = gumbel_locksteps(n_sim, m.gm, m.K); }  // Sequential Halving with K walkers: cut per slot by its own cursor
    else if (m.K > 1) { p.family = SF_STEP_MULTI; p.L = (n_sim + m.K - 1) / m.K; }  // up to K walkers per slot and lock-step
    else if (m.gm > 0) p.family = SF_STEP_GUMBEL;
    else if (m.forced) p.family = m.cap ? SF_STEP_CAP_FORCED : SF_STEP_FORCED;
    else if (m.cap) p.family = SF_STEP_CAP;  // a slot past its budget idles: no walk, no row
    else if (m.proof) { p.family = SF_STEP_PROOF; p.exact = m.exact > 0; }  // one family: exact endgames under it are a property of the plan
    else if (m.exact > 0) p.family = SF_STEP_EXACT;  // the plain search alone (exact_endgame_refusal): a late leaf is solved, not evaluated
    else if (m.puct) p.family = SF_STEP_PUCT;  // the plain search alone (puct_refusal): k_step's lock-steps with puct_key's scores
    p.launches = p.L + 1;
    return p;
}

// Launch t of the plan's `launches` (t = L: the last backup; rollout: simulation t, nothing else set).  The families with a slot range
// take (t, g0, g1) -- the Gumbel one (t, n_sim, g0, g1) -- with the chain's g0 / g1; k_step_multi takes (t, kb, kt),
// k_step_gumbel_multi (t, n_sim).  Where `select` is set the network follows on the rows counted in batch counter `ctr`, as lock-step
// t, with kt leaves per slot (0: one).
struct StepArgs {
    bool backup, select;  // the kernel's template pair: t > 0, t < L
    int t;                // the simulation / lock-step index: the kernel's first argument and the forward's step
    int kb, kt;           // k_step_multi: walkers to back up, walkers to send out; kt also the forward's
    int ctr;
};

inline StepArgs plan_step(const SearchPlan &p, int n_sim, int K, int t) {
    StepArgs a = {t > 0, t < p.L, t, 0, 0, t & 1};
    const int left = n_sim - t * K;  // k_step_multi: simulations not yet sent out
    if (p.family == SF_STEP_MULTI) { a.kb = t == 0 ? 0 : (a.select ? K : left + K); a.kt = a.select ? (left < K ? left : K) : 0; }
    if (p.family == SF_STEP_GUMBEL_MULTI) a.kt = a.select ? K : 0;
    return a;
}

// network rows of a search over W slots, up to K leaves each per lock-step; `active` bounds the slots still searching (0: not known)
inline int search_batch_cap(int W, int K, int active) { return (active > 0 && active < W ? active : W) * K; }

// The cap a captured search is launched with, of R = W * K rows: launch parameters must not change from search to search, so the cap
// moves in steps of 512 rows -- and only from 4096 rows on, below which the network picks other kernels (an exact cap of 4095 --
// one game of 4096 over, as happens from ply ~11 on: Othello has early wipe-outs -- would hand the trunk to the one-board-per-wave
// kernel for the rest of the wave).
inline int quantised_cap(int R, int cap) { return (R >= 4096 && cap < 4096) ? (cap + 511) / 512 * 512 : R; }

// group i of n over G slots: [g0, g1) in whole blocks (trailing groups may be empty: 40 slots in 4 groups are 16, 16, 8, 0)
inline void group_range(int G, int i, int n, int *g0, int *g1) {
    const int blocks = (G + AZ_SLOT_BLOCK - 1) / AZ_SLOT_BLOCK, per = (blocks + n - 1) / n;
    const int a = i * per * AZ_SLOT_BLOCK, b = (i + 1) * per * AZ_SLOT_BLOCK;
    *g0 = a < G ? a : G; *g1 = b < G ? b : G;
}

// The measured rule (profiles/r14_groups.txt): the groups az_engine_run plays with where nothing was asked for.  A
// shape has n > 1 only where the worst of three grouped runs beat the best of three runs of the build before by more than that
// build's own spread; every shape that was not measured plays as one group.
inline int groups_auto(int evaluator, int game, int H, int W, int G) {
    if (evaluator != AZ_EVAL_NET) return 1;  // the fake evaluator has no network kernels to run beside
    if (game == AZ_GAME_OTHELLO && H == 8) {
        if (G >= 4096 && G < 8192) return 2;  // 4096 slots: 2 x 2048 +4.5 %; 4 x 1024 loses (-14 %)
        if (G >= 32768) return 2;             // 32768 slots: 2 x 16384 +1.3 %
        return 1;                             // 512 slots: +0.4 %, not worth a second chain; 8192 .. 32767: not measured
    }
    if (game == AZ_GAME_CONNECT4 && H == 6 && W == 7) return G >= 8192 ? 4 : 1;  // 8192 slots: 4 x 2048 +9.4 %, 2 x 4096 +0.2 %
    return 1;
}

// ---- the leaf evaluation cache (az_engine_set_eval_cache) ----------------------------------------------------------
// A slot group's table of network outputs by exact position.  The arithmetic of its keys lives here so that the step kernels and the
// host test (tests/eval_cache_table.cpp) share it.
#if defined(__HIPCC__)
#define AZ_PLAN_HD __host__ __device__ inline
#else
#define AZ_PLAN_HD inline
#endif
#define AZ_EC_PROBE 4                    // entries a lookup looks at: the bucket and the three behind it (one lane each)
#define AZ_EC_DEFAULT_CAPACITY (1 << 18) // entries per slot group: 108 568 distinct positions of <= 12 stones in 1024 games (tools/eval_cache_count.py)
#define AZ_EC_DEFAULT_LIMIT 12           // stones: keeps 4.54 of the 4.74 plies' worth of repeats per game
#define AZ_EC_MAX_CAPACITY (1 << 22)

// the bucket hash of a position: a 64-bit mix of the three key words, folded to 32 bits
AZ_PLAN_HD uint32_t ec_hash(uint64_t p1, uint64_t m1, int player) {
    uint64_t x = p1 * 0x9E3779B97F4A7C15ull ^ (m1 + (player > 0 ? 0x632BE59BD9B4E019ull : 0xD6E8FEB86659FD93ull));
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 29; x *= 0x9E3779B97F4A7C15ull; x ^= x >> 32;
    return (uint32_t)x;
}
// probe j of a lookup in a table of `capacity` entries (a power of two)
AZ_PLAN_HD uint32_t ec_bucket(uint32_t hash, int j, uint32_t capacity) { return (hash + (uint32_t)j) & (capacity - 1u); }
// only positions with at most `limit` stones are looked up or inserted
AZ_PLAN_HD bool ec_in_limit(uint64_t p1, uint64_t m1, int limit) { return __builtin_popcountll(p1 | m1) <= limit; }
// The stamp of a step kernel: the group's serial word (advanced by the ply's last backup) and the kernel's simulation index; never 0,
// and greater in every later kernel of the group's stream.  An entry's tag word is its claimer's stamp over the hash: 0 = empty.
AZ_PLAN_HD uint32_t ec_stamp(uint32_t serial, int sim) { return serial + (uint32_t)sim + 1u; }
AZ_PLAN_HD uint64_t ec_tag(uint32_t hash, uint32_t stamp) { return ((uint64_t)stamp << 32) | hash; }
AZ_PLAN_HD uint32_t ec_tag_stamp(uint64_t tag) { return (uint32_t)(tag >> 32); }
AZ_PLAN_HD uint32_t ec_tag_hash(uint64_t tag) { return (uint32_t)tag; }
// row_of_slot of a slot whose leaf was found in the table: the entry, as a negative row (batch rows are >= 0)
AZ_PLAN_HD int ec_row_of_entry(int entry) { return -(1 + entry); }
AZ_PLAN_HD bool ec_row_is_entry(int row) { return row < 0; }
AZ_PLAN_HD int ec_entry_of_row(int row) { return -(row + 1); }
// floats of an entry's payload: A priors and the value, in whole 16-byte words
AZ_PLAN_HD int ec_stride(int A) { return (A + 1 + 3) & ~3; }

// capacity and stone limit as az_engine_set_eval_cache takes them: 0 = the default; the capacity a power of two
inline bool ec_capacity_ok(int capacity) { return capacity == 0 || (capacity >= 1 && capacity <= AZ_EC_MAX_CAPACITY && (capacity & (capacity - 1)) == 0); }
inline bool ec_limit_ok(int limit) { return limit >= 0 && limit <= 64; }

// Where the cache is served at all: az_engine_run's plain PUCT search of a network engine, the net not under az_net_profile (the
// profiled step divides FLOPs x net_evals by kernel time and must keep describing full launches).  `beyond_plain`: az_engine.hip's
// beyond_plain_search is not null (external / rollout evaluator, a symmetry mode, leaf_batch > 1, the Gumbel search).
inline bool eval_cache_served(int evaluator, bool beyond_plain, bool profiled) { return evaluator == AZ_EVAL_NET && !beyond_plain && !profiled; }

// The measured rule (profiles/r26_eval_cache.txt): the shapes az_engine_run caches at where nothing was asked
// for.  As groups_auto: on only where the slowest of three cached runs beat the fastest of three uncached ones by more than their
// spread; every shape that was not measured, or did not pass, plays without.
inline bool eval_cache_auto(int evaluator, int game, int H, int W, int G) {
    if (evaluator != AZ_EVAL_NET) return false;
    if (game == AZ_GAME_OTHELLO && H == 8 && W == 8) return G >= 512;   // 512 slots +1.4 %, 4096 (2 x 2048) +2.5 %, 32768 (2 x 16384) +7.7 %
    if (game == AZ_GAME_CONNECT4 && H == 6 && W == 7) return G >= 8192;  // 8192 slots (4 x 2048), 200 sims: +11.6 %
    return false;                                                        // everything else: not measured
}

// request: AZ_EVAL_CACHE_AUTO (the rule), _OFF, _ON (wherever served)
inline bool eval_cache_in_force(int request, int evaluator, int game, int H, int W, int G, bool beyond_plain, bool profiled) {
    if (!eval_cache_served(evaluator, beyond_plain, profiled) || request == AZ_EVAL_CACHE_OFF) return false;
    return request == AZ_EVAL_CACHE_ON || eval_cache_auto(evaluator, game, H, W, G);
}

// ---- the heads inside the step kernel (k_step_heads) ---------------------------------------------------------------
// Where the form is served at all: az_engine_run's plain PUCT search of a network engine -- one leaf per slot and lock-step, no
// symmetry mode, no playout cap, forced playouts, exact endgames, proof backup or PUCT settings (`plain`: none of them; the external,
// fake and rollout evaluators and the Gumbel search are beyond the plain search already) -- a net whose heads k_heads2 has an
// instantiation for (`heads2_shape`), and never under az_net_profile: the profiled step keeps describing the five separate launches.
inline bool step_heads_served(int evaluator, bool plain, bool heads2_shape, bool profiled) { return evaluator == AZ_EVAL_NET && plain && heads2_shape && !profiled; }

// The measured rule (profiles/r30_step_heads.txt): the shapes az_engine_run runs the form at where nothing was asked for.  As
// groups_auto: on only where the slowest of three fused runs beat the fastest of three unfused ones by more than their spread; every
// shape that was not measured, or did not pass, keeps the five launches.
inline bool step_heads_auto(int evaluator, int game, int H, int W, int G) {
    if (evaluator != AZ_EVAL_NET) return false;
    // 512 slots (one group) +2.3 %, 4096 (2 x 2048) +2.0 %; 32768 (2 x 16384: 1024 blocks per step launch, no idle CU to fill) -0.1 %: off.
    // 8192 .. 32767 were not measured and stay off, as in groups_auto.
    if (game == AZ_GAME_OTHELLO && H == 8 && W == 8) return G >= 512 && G < 8192;
    return false;  // everything else: not measured
}

// request: AZ_ENGINE_STEP_HEADS -- -1 unset (the rule), 0 never, 1 wherever served
inline bool step_heads_in_force(int request, int evaluator, int game, int H, int W, int G, bool plain, bool heads2_shape, bool profiled) {
    if (!step_heads_served(evaluator, plain, heads2_shape, profiled) || request == 0) return false;
    return request == 1 || step_heads_auto(evaluator, game, H, W, G);
}

// ---- exact endgames (az_engine_set_exact_endgame) -----------------------------------------------------------------
// (AZ_EXACT_MAX_EMPTIES, the largest empties limit of a solved leaf, is the frame count of k_step_exact's solver stack: az_solve.h)
inline bool exact_endgame_ok(int max_empties) { return max_empties >= 0 && max_empties <= AZ_EXACT_MAX_EMPTIES; }
// Where the mode is served: the plain PUCT search of a network or fake engine, one leaf per slot and lock-step, without the playout cap
// and forced playouts (the hook is orthogonal to those two, their composed host models are not written).  The mode that refuses, as
// the setters name it, or null.
inline const char *exact_endgame_refusal(int evaluator, bool sym, bool sym_random, int leaf_batch, int gm, bool cap, bool forced) {
    if (evaluator == AZ_EVAL_EXTERNAL) return "an AZ_EVAL_EXTERNAL engine (external evaluator)";
    if (evaluator == AZ_EVAL_ROLLOUT) return "a rollout engine (AZ_EVAL_ROLLOUT)";
    if (sym) return "the symmetry ensemble (az_engine_set_symmetry)";
    if (sym_random) return "the random symmetry mode (az_engine_set_symmetry_random)";
    if (leaf_batch > 1) return "leaf_batch > 1 (az_engine_set_leaf_batch)";
    if (gm > 0) return "the Gumbel search (az_engine_set_gumbel)";
    if (cap) return "the playout cap (az_engine_set_playout_cap)";
    if (forced) return "forced playouts (az_engine_set_forced_playouts)";
    return nullptr;
}

// ---- proof backup (az_engine_set_proof_backup) --------------------------------------------------------------------
// Where the mode is served: where exact endgames are -- the plain PUCT search of a network or fake engine, one leaf per slot and
// lock-step, without the playout cap and forced playouts (their composed host models are not written).  It composes with exact
// endgames, the evaluation cache and slot groups.  The mode that refuses, as the setters name it, or null.
inline const char *proof_backup_refusal(int evaluator, bool sym, bool sym_random, int leaf_batch, int gm, bool cap, bool forced) {
    return exact_endgame_refusal(evaluator, sym, sym_random, leaf_batch, gm, cap, forced);
}

// ---- PUCT exploration settings (az_engine_set_puct) ----------------------------------------------------------------
// The ranges of the three settings, and the triple that is the mode off: c_init = 1.0, c_base = 0 (no growth), fpu negative (off).
inline bool puct_c_init_ok(double c_init) { return c_init > 0.0 && c_init <= 64.0; }                       // NaN fails every compare
inline bool puct_c_base_ok(double c_base) { return c_base == 0.0 || (c_base >= 1.0 && c_base <= 1e9); }
inline bool puct_fpu_ok(double fpu) { return fpu < 0.0 || (fpu >= 0.0 && fpu <= 4.0); }
inline bool puct_neutral(double c_init, double c_base, double fpu) { return c_init == 1.0 && c_base == 0.0 && fpu < 0.0; }
// Where the mode is served: the plain PUCT search of a network or fake engine, one leaf per slot and lock-step, with slot groups and
// the evaluation cache or without.  Every other mode is a follow-up (their composed host models are not written): the mode that
// refuses, as the setters name it, or null.
inline const char *puct_refusal(int evaluator, bool sym, bool sym_random, int leaf_batch, int gm, bool cap, bool forced, int exact, bool proof) {
    if (const char *why = exact_endgame_refusal(evaluator, sym, sym_random, leaf_batch, gm, cap, forced)) return why;
    if (exact > 0) return "exact endgames (az_engine_set_exact_endgame)";
    if (proof) return "proof backup (az_engine_set_proof_backup)";
    return nullptr;
}

// What a captured search is keyed by.  (A proof search is SF_STEP_PROOF whatever exact endgames say: the family keeps its graphs apart
// from the plain and the exact ones, and a change of the empties limit under it drops every graph like any other.)  (What else travels in the launch arguments -- K, m, the playout cap's n_fast and p_full, forced
// playouts' k, the empties limit of exact endgames, the pools -- drops every graph when it changes: az_engine.hip, drop_graphs.)
typedef std::tuple<int, bool, int, int, int, int> SearchKey;
inline SearchKey search_key(const SearchPlan &p, int n_sim, int cap, int g0, int g1) { return SearchKey((int)p.family, p.full, n_sim, cap, g0, g1); }
