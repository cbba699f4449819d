// az_engine.hip -- lock-step batched MCTS self-play on MI355X (gfx950).
//
// G concurrent games each advance ONE simulation per lock-step; the G pending leaves form one
// batch for the policy-value network.  Every tree still sees strictly sequential simulations, so
// per-game semantics equal the reference's MCT.search (mcts.py:226-269) exactly -- no virtual loss.  (Opt-in, default off:
// az_engine_set_leaf_batch walks K simulations per game and lock-step with virtual loss -- k_step_multi below, another search.)
// (Opt-in, default off: az_engine_set_playout_cap searches most plies with a few simulations and records the fully searched ones only --
// k_step_cap below, k_step with a per-slot simulation budget.)
// (Opt-in, default off: az_engine_set_forced_playouts gives every visited root child of a fully searched ply at least sqrt(k P N_root)
// playouts and takes the ones PUCT would not have spent out of the policy target again -- k_step_forced below, forced_playout /
// forced_pruned and move_policy.)
// (Opt-in, default off: az_engine_set_gumbel replaces the root's PUCT pick by Sequential Halving over actions sampled with Gumbel
// noise and reads the root out by the completed Q-values -- k_step_gumbel below, another search again; az_engine_set_gumbel_batch
// walks up to K simulations of a Sequential Halving phase per game and lock-step -- k_step_gumbel_multi.)
// (By a measured rule: az_engine_set_eval_cache.  The games of an az_engine_run wave start from one position under one set of weights,
// so a slot group keeps the network's outputs by exact position -- ec_lookup_grp, leaf_output -- and a leaf found there takes no batch
// row; the bits a slot backs up are the ones the forward would have written.)
// (Opt-in, default off: az_engine_set_proof_backup backs proven wins, losses and draws up the tree -- MCTS-Solver: a node is proven as
// soon as its children decide it, walks stop on proven nodes, selection and the policy target respect the proofs -- k_step_proof below,
// propagate_proofs_grp, proof_mode / proof_count in move_policy.)
// (Opt-in, default off: az_engine_set_puct frees PUCT's exploration constant, its growth with the parent's visits and the Q an
// unvisited child is assumed to have (first-play urgency) -- k_step_puct below, puct_c / puct_fpu_q / puct_key.)
//
// HBM layout
//   boards   : 2 x u64 bitboards + int8 side-to-move per slot (root and current leaf), SoA over slots
//   tree     : per slot two pools of `C` 32-byte nodes (one node = two 16-byte accesses; a node's children
//              are contiguous, so 16 lanes read 16 children as one 512-byte run).  Nodes are bump-allocated
//              during a search; at every move the kept subtree is copied breadth-first into the other pool
//              (change_root, mcts.py:118-125), so a game's live tree stays a few hundred KB, contiguous:
//              { f64 Q, f64 P, i32 N, i32 parent, i32 first_child, u8 n_children, u8 action, u8 flags, i8 winner }
//   net i/o  : nn_in[G][cells] f32 canonical leaf boards, probs[G][A] f32, value[G] f32
//   samples  : state i8[S][cells], pi f32[S][A], z i8[S], meta i32[S][4], visits i32[S][A]
//
// Mapping: 16 lanes per game (4 games per wavefront, 16 per 256-thread block).  PUCT scoring, prior
// renormalisation, child creation and Dirichlet draws are spread over the 16 lanes (one child
// each); arg-max / tie counting use width-16 shuffles and wave ballots; the board of the walk is
// replicated in the group's registers and advanced with bitboard shifts.
//
// Lazy expansion (mcts.py:151-160) is kept observable-equivalent with eager allocation: when a leaf
// is evaluated its children are created at once from the renormalised priors but stay invisible
// (flag F_EXPANDED clear) until the node's next visit, which is when the reference materialises
// them.  This stores n_children priors per evaluated node instead of the raw probs[A] vector.
#include <string.h>

#include <map>
#include <vector>

#include "az_device.h"
#include "az_solve.h"
#include "az_host.h"
#include "az_search_plan.h"  // up here for the evaluation cache's key arithmetic, which the step kernels share with the host (ec_*)
#include "az_heads_block.h"  // the heads of one block's 16 rows (k_step_heads)

#define F_EXPANDED 1
#define F_TERMINAL 2
#define F_PF32 4
#define F_NOISED 8
#define F_EVALUATED 16
#define F_SOLVED 32  // az_engine_set_exact_endgame: with F_TERMINAL, the winner was computed by the solver, not read off a finished board
#define F_PROVEN 64  // az_engine_set_proof_backup: an expanded node whose children decide it; `win` holds the outcome

#define LS_NONE 0
#define LS_EVAL 1
#define LS_TERM 2
#define LS_DUP 16  // leaf_batch > 1 only: LS_DUP + i = the walker landed on the pending (LS_EVAL) leaf of walker i of the same lock-step

#define ERR_NODE_POOL 1
#define ERR_SAMPLE_CAP 2
#define ERR_PLY_CAP 4
#define ERR_INTERNAL 8
#define ERR_RNG 16  // the Gamma rejection sampler of the root noise gave up (p < 1e-38 per draw): reported, never papered over
#define ERR_EVAL 32  // an external evaluator wrote a prior that is negative / not finite or a value that is not finite (k_ext_check)

#define LPG 16          // lanes per game
#define GPB (256 / LPG) // games per 256-thread block

enum { CTR_SAMPLES = 0, CTR_GAMES_DONE, CTR_NET_EVALS, CTR_NEXT_GAME, CTR_TOTAL_GAMES, CTR_FIRST_ID, CTR_PLIES,
       CTR_FULL_PLIES, CTR_FAST_PLIES,  // az_engine_set_playout_cap: the plies k_move played after a full / a fast search (counted while the mode is on)
       CTR_FORCED_PICKS, CTR_PRUNED,    // az_engine_set_forced_playouts: root selections with a forced child / playouts pruned from the recorded targets
       CTR_CACHE_HITS,                  // az_engine_set_eval_cache: leaves answered from the group's table (they count in CTR_NET_EVALS too)
       CTR_RESIGNED, CTR_HOLDOUT_GAMES, CTR_HOLDOUT_TRIG, CTR_HOLDOUT_FP,  // az_engine_set_resign: counted by k_move when a game ends
       CTR_COUNT };
// entries beyond CTR_COUNT live as long as the engine (k_reset_all clears [0, CTR_COUNT) only)
enum { CTR_COLLISIONS = CTR_COUNT, CTR_ALLOC };
#define MLB AZ_MAX_LEAF_BATCH  // walkers per slot and lock-step: one per lane of the game's group
static_assert(MLB == LPG, "walker j's pending leaf is kept by lane j of the game's group");

struct __attribute__((aligned(16))) Node {
    double Q, P;
    int N, parent, first;
    uint8_t nch, act, flags;
    int8_t win;
};
static_assert(sizeof(Node) == 32, "node is two 16-byte accesses");

struct EngDev {
    GameDesc gd;
    int G, C, A, max_plies;
    double alpha, eps;
    int tie_mode, noise_mode, tmax, tmin;
    u32 sim_base;  // simulations already run on the current roots: keeps Philox counters distinct across repeated az_engine_search calls
    int rollout;  // 1: TreeEval.ROLLOUT (plain UCT + random playouts, mcts.py:38-42, 152-154, 173-180), no network
    u32 seed;
    long long sample_cap;
    u64 *root_p1, *root_m1; int8_t *root_player;
    int *root, *n_nodes, *ply; u32 *game_id; uint8_t *active, *root_fresh;
    int8_t *side;  // arena: the colour this engine searches for in the slot (0 = both, self-play)
    int *leaf; u64 *leaf_p1, *leaf_m1; int8_t *leaf_player, *leaf_status, *leaf_winner;
    int *path, *path_len;  // root..leaf node indices of the pending simulation ([G][LPG]; longer paths chase parents)
    Node *nodes;        // [G][2][C]
    uint8_t *pool_sel;  // which of the slot's two pools holds the live tree
    float *nn_in, *probs, *value;
    int *row_of_slot;  // network batch row holding the slot's pending leaf (leaves are compacted)
    int *evals;        // per-slot network evaluations since the last move (folded into ctr[] once per ply)
    int *batch_cnt;    // [3] rows filled: two alternating lock-step counters + the root-prior pass (a slot group's own three)
    int *live;         // slots still holding a game after the ply's move (counted by k_reroot; a slot group's own word)
    int *samp_idx;
    int8_t *o_state; float *o_pi; int8_t *o_z; int *o_meta, *o_visits;
    unsigned long long *ctr;
    int *err, *max_nodes;
    int *max_path;  // longest root..leaf path (nodes) of any simulation, recorded only beyond LPG (the parent-chasing backup)
    // az_engine_set_leaf_batch (k_step_multi): K walkers per slot and lock-step; their pending leaves, [G][MLB] (m_path [G][MLB][LPG]).
    // nn_in / probs / value then hold K * G rows.  K == 1: k_step and the fields above, these stay unallocated.
    int K;
    int *m_leaf; u64 *m_leaf_p1, *m_leaf_m1; int8_t *m_leaf_player, *m_leaf_status, *m_leaf_winner;
    int *m_row, *m_path, *m_path_len;
    // az_engine_set_gumbel (k_step_gumbel): gm = the actions sampled at the root (0: off, the PUCT search), the constants of sigma
    // and the scale of the Gumbel draw; gmask [G] = the root children the slot's Sequential Halving still considers (0: all).
    int gm;
    double g_cvisit, g_cscale, g_scale;
    u64 *gmask;
    // az_engine_set_gumbel_batch (k_step_gumbel_multi; then K above = its walkers): the slot's cursor = the simulations of the search
    // call already dealt, and the cursor at the start of the slot's current lock-step, [G] each
    int *gcur, *gstart;
    // az_engine_set_gumbel_full: the network value of every evaluated node, [G][2][C] like nodes, in the frame of the player to move at
    // the node.  Null unless the switch is in force (on, and the Gumbel mode on): then no kernel touches it.
    float *nval;
    // az_engine_set_playout_cap (k_step_cap): cap_nfast = the simulations of a fast ply (0: off), cap_pfull = the share of full plies;
    // budget [G] = the simulations the slot walks in a search call, written by k_root_prep from the coin of the slot's (game id, ply):
    // CAP_FULL for a full ply, cap_nfast for a fast one.  Null unless the mode is on: then no kernel touches it.
    int cap_nfast;
    double cap_pfull;
    int *budget;
    // az_engine_set_forced_playouts (k_step_forced, move_policy): kforced = KataGo's k (0: off); fpicks [G] = the slot's root selections
    // with a forced child since its last move (k_move folds them into ctr[], as evals).  Null unless the mode is on: then no kernel touches it.
    double kforced;
    int *fpicks;
    // az_engine_set_eval_cache (step_grp): the slot group's table of network outputs by exact position -- ec_hdr
    // [ec_mask + 1] tag and key, ec_pay [ec_mask + 1][ec_stride] the A priors and the value -- and the group's serial word, from which
    // a step kernel forms its stamp; ec_claim [G] = the entry the slot's pending leaf claimed (-1: none), ec_hits [G] = the slot's
    // leaves answered from the table in this ply (the ply's last backup folds them into ctr[]).  Positions of at most ec_limit
    // stones only.  Null unless the cache is in force (az_engine_run alone sets them): then no kernel touches it.
    struct EcHdr *ec_hdr;
    float *ec_pay;
    u32 *ec_serial;
    int *ec_claim, *ec_hits;
    u32 ec_mask;
    int ec_limit, ec_stride;
    // az_engine_set_exact_endgame (k_step_exact): exact_max = the empties limit of a solved leaf (0: off); x_solved / x_nodes [G] = the
    // slot's leaves solved and the positions the solver entered for them since the last k_reset_all (the slot's own words, summed when
    // the stats are read).  Null unless the mode is on: then no kernel touches them.
    int exact_max;
    int *x_solved;
    unsigned long long *x_nodes;
    // az_engine_set_proof_backup (k_step_proof, move_policy): pf [3][G] = per slot the interior nodes marked F_PROVEN, the walks that
    // ended on such a node and the plies whose policy counts the proofs changed, since the last k_reset_all (the slot's own words,
    // summed when the stats are read).  Null unless the mode is on: then no kernel touches them.  (Last: the fields above keep their place.)
    int *pf;
    // az_engine_set_puct (k_step_puct): the exploration constant's c_init and c_base (0: no growth) and first-play
    // urgency's reduction (negative: off).  Read by the k_step_puct kernels alone, which are launched only while the triple is not the
    // neutral (1.0, 0, off).  (After pf: the fields above keep their place.)
    double puct_cinit, puct_cbase, puct_fpu;
    // the heads inside the step kernel (k_step_heads): the chain's fc2 rows (the net lane's h2), the head matrix in
    // k_heads2's fragment order and the padded bias; sh_nt = the 16-column tiles of the padded logits (5 or 3).  Null unless the form is
    // in force (az_engine_run alone sets them): then no kernel touches them.  (Last: the fields above keep their place.)
    const float *sh_h2, *sh_wq, *sh_hb;
    int sh_nt;
    // az_engine_set_resign (k_move): the settings, the per-slot windows and the game log, in device memory.  One
    // pointer, not the fields themselves: EngDev, an argument of every kernel, grows by eight bytes, and off is one null test.  (The
    // mode-off headline measured 0.2 % under the parent's with the fields here and with the pointer alike; the cause is not found:
    // DESIGN section 37.)  Null unless the mode is on AND the launch is az_engine_run's (rs_attach): k_move, and reset_slot under it and under
    // k_reset_all, read it and no other kernel does.  (Last: the fields above keep their place.)
    const struct ResignDev *rs;
};
// rs_k = the window length, rs_v = v_resign, rs_minply, rs_phold = the holdout share.  rs_win [G][2][AZ_RESIGN_MAX_K] = per slot and
// side the last tested values as a ring, rs_cnt [G][2] = how many were pushed; gl_rows [gl_n][8] / gl_low [gl_n][2] = the game log of
// the run, indexed by game id - first game id.
struct ResignDev {
    double rs_v, rs_phold;
    int rs_k, rs_minply;
    double *rs_win;
    int *rs_cnt;
    int *gl_rows;
    double *gl_low;
    int gl_n;
};
#define AZ_RESIGN_MAX_K 4
// tag = ec_tag(hash, the claimer's stamp), 0 = empty: claimed by one device-scope compare-and-swap, never rewritten within a run; the
// key is written by the claimer in the same kernel, the payload in the group's next one
struct __attribute__((aligned(16))) EcHdr { u64 tag, p1, m1; long long player; };
static_assert(sizeof(EcHdr) == 32, "an entry's tag and key are two 16-byte accesses");
#define CAP_FULL 0x7fffffff  // the budget of a full ply: every simulation of any search call, and the mark root noise asks for

// ---------------------------------------------------------------------------------------------
// node access (two 16-byte transactions) and 16-lane group primitives
// ---------------------------------------------------------------------------------------------
// a node's last word: n_children | action << 8 | flags << 16 | winner << 24
AZ_D u32 node_tail(const Node &n) { return (u32)n.nch | ((u32)n.act << 8) | ((u32)n.flags << 16) | ((u32)(uint8_t)n.win << 24); }
AZ_D void set_node_tail(Node &n, u32 w) {
    n.nch = (uint8_t)(w & 0xff); n.act = (uint8_t)((w >> 8) & 0xff); n.flags = (uint8_t)((w >> 16) & 0xff);
    n.win = (int8_t)(w >> 24);
}

AZ_D Node load_node(const Node *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 a = q[0], b = q[1];
    Node n;
    n.Q = __longlong_as_double((long long)(((u64)a.y << 32) | a.x));
    n.P = __longlong_as_double((long long)(((u64)a.w << 32) | a.z));
    n.N = (int)b.x; n.parent = (int)b.y; n.first = (int)b.z;
    set_node_tail(n, b.w);
    return n;
}

AZ_D void store_node(Node *p, const Node &n) {
    u64 q = (u64)__double_as_longlong(n.Q), pp = (u64)__double_as_longlong(n.P);
    uint4 a = make_uint4((u32)q, (u32)(q >> 32), (u32)pp, (u32)(pp >> 32));
    uint4 b = make_uint4((u32)n.N, (u32)n.parent, (u32)n.first, node_tail(n));
    uint4 *d = reinterpret_cast<uint4 *>(p);
    d[0] = a; d[1] = b;
}

AZ_D Node fresh_node(int action, int parent, double P, int flags) {
    Node n;
    n.Q = 0.0; n.P = P; n.N = 0; n.parent = parent; n.first = -1; n.nch = 0; n.act = (uint8_t)action;
    n.flags = (uint8_t)flags; n.win = 0;
    return n;
}

AZ_D Node *pool_of(const EngDev &E, int g) { return E.nodes + ((size_t)g * 2 + E.pool_sel[g]) * E.C; }
// the stored network values of a pool's nodes (az_engine_set_gumbel_full in force only): nval is laid out like nodes
AZ_D float *nval_of(const EngDev &E, const Node *pool) { return E.nval + (pool - E.nodes); }

// does this engine search slot g now? (active, and in arena mode only when its colour is to move)
AZ_D bool searches(const EngDev &E, int g) { return E.active[g] && (E.side[g] == 0 || E.side[g] == E.root_player[g]); }

AZ_D u32 grp_ballot(bool p) { return (u32)(__ballot(p) >> (threadIdx.x & 48)) & 0xFFFFu; }
AZ_D double grp_max(double v) {  // over the game's 16 lanes, by DPP (az_device.h: the same maximum in every lane as the shuffle butterfly gave)
    v = fmax(v, __longlong_as_double((long long)az_dpp64<AZ_DPP_SWAP1>((u64)__double_as_longlong(v))));
    v = fmax(v, __longlong_as_double((long long)az_dpp64<AZ_DPP_SWAP2>((u64)__double_as_longlong(v))));
    v = fmax(v, __longlong_as_double((long long)az_dpp64<AZ_DPP_HMIRROR>((u64)__double_as_longlong(v))));
    v = fmax(v, __longlong_as_double((long long)az_dpp64<AZ_DPP_MIRROR>((u64)__double_as_longlong(v))));
    return v;
}
// The sum over the game's 16 lanes as a pairwise tree with strides 1, 2, 4, 8, by grp_max's DPP steps: after the two quad steps the four
// lanes of a quad hold one value, so the half mirror (lane 7 - i: the other quad) hands over what lane i ^ 4 holds, and the row mirror
// what lane i ^ 8 does.  Double addition commutes: every lane ends with the same bits (az_engine_set_puct's vis).
AZ_D double grp_sum_f64(double v) {
    v = v + __longlong_as_double((long long)az_dpp64<AZ_DPP_SWAP1>((u64)__double_as_longlong(v)));
    v = v + __longlong_as_double((long long)az_dpp64<AZ_DPP_SWAP2>((u64)__double_as_longlong(v)));
    v = v + __longlong_as_double((long long)az_dpp64<AZ_DPP_HMIRROR>((u64)__double_as_longlong(v)));
    v = v + __longlong_as_double((long long)az_dpp64<AZ_DPP_MIRROR>((u64)__double_as_longlong(v)));
    return v;
}
AZ_D u64 grp_sum_u64(u64 v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += (u64)__shfl_xor((long long)v, m, LPG);
    return v;
}
AZ_D int kth_set_bit(u32 mask, int k) {
    for (int i = 0; i < k; ++i) mask &= mask - 1;
    return __ffs((int)mask) - 1;
}

// next free row of the network batch for this group (lane 0 draws it, the group gets it by shuffle)
AZ_D int alloc_row_grp(int *counter, int sub) {
    int row = 0;
    if (sub == 0) row = atomicAdd(counter, 1);
    return __shfl(row, 0, LPG);
}

AZ_D void start_position(const GameDesc &gd, BB &b) {
    b.p1 = 0; b.m1 = 0; b.player = 1;
    if (gd.game == AZ_OTHELLO) {  // othello.py:102-109
        int h = gd.H / 2;
        b.p1 = (1ULL << ((h - 1) * 8 + (h - 1))) | (1ULL << (h * 8 + h));
        b.m1 = (1ULL << ((h - 1) * 8 + h)) | (1ULL << (h * 8 + (h - 1)));
    }
}

// base.py:363 : player * grid, spread over the group's lanes (coalesced row of `cells` floats)
AZ_D void write_nn_input_grp(const EngDev &E, int row, const BB &b, int sub) {
    float *dst = E.nn_in + (size_t)row * E.gd.cells;
    for (int i = sub; i < E.gd.cells; i += LPG) dst[i] = (float)(b.player * az_cell_value(b, i / E.gd.W, i % E.gd.W));
}

// get_normalized_probs (othello.py:384-402, connect4.py:414-428, tictactoe.py:318-334) + add_child,
// one lane per legal action bit.  `fc` = the slot's bump pointer (first free node); returns the number of
// children created, or -1 on pool exhaustion.
AZ_D int create_children_grp(const EngDev &E, int g, Node *pool, int fc, int node, const BB &bb, const float *pr, int sub) {
    const GameDesc &gd = E.gd;
    u64 bits = az_legal_bits_grp(gd, bb, bb.player, sub);
    bool pass = (gd.game == AZ_OTHELLO && bits == 0);
    int k = pass ? 1 : __popcll(bits);
    if (k <= 0 || fc + k > E.C) { if (sub == 0) atomicOr(E.err, k <= 0 ? ERR_INTERNAL : ERR_NODE_POOL); return -1; }
    // priors of this lane's (up to 4) legal actions: independent loads, one round trip for the whole row
    float myp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int bit = r * LPG + sub;
        myp[r] = (!pass && ((bits >> bit) & 1ULL)) ? pr[az_bit_to_action(gd, bit)] : 0.0f;
    }
    const float ppass = pass ? pr[gd.A - 1] : 0.0f;
    // float32 running sum in ASCENDING action order, as the reference accumulates it: the operands come from
    // their lanes by shuffle, so the order is kept without a dependent global load per action
    float s = 0.0f;
    if (pass) s += ppass;
    else
        for (u64 m = bits; m; m &= m - 1) {
            const int bit = __ffsll((long long)m) - 1, r = bit >> 4;
            const float mine = r == 0 ? myp[0] : (r == 1 ? myp[1] : (r == 2 ? myp[2] : myp[3]));
            s += __shfl(mine, bit & 15, LPG);
        }
    bool uniform = s < 1e-6f;
    if (pass) {
        if (sub == 0) store_node(pool + fc, fresh_node(gd.A - 1, node, uniform ? 1.0 : (double)(ppass / s), uniform ? 0 : F_PF32));
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int bit = r * LPG + sub;
            if ((bits >> bit) & 1ULL) {
                int idx = __popcll(bits & ((1ULL << bit) - 1ULL));
                int a = az_bit_to_action(gd, bit);
                store_node(pool + fc + idx, fresh_node(a, node, uniform ? 1.0 / (double)k : (double)(myp[r] / s), uniform ? 0 : F_PF32));
            }
        }
    }
    if (sub == 0) {
        E.n_nodes[g] = fc + k;
        pool[node].first = fc;
        pool[node].nch = (uint8_t)k;
        pool[node].flags |= F_EVALUATED;
    }
    return k;
}

// az_engine_set_proof_backup: the proven outcome of a node by its visit count and last word -- a finished or solved position
// (F_TERMINAL) or an interior node its children decide (F_PROVEN), once it has been backed up -- or AZ_UNSOLVED.
AZ_D int proven_outcome(int N, u32 tail) {
    return (N > 0 && ((tail >> 16) & (F_TERMINAL | F_PROVEN))) ? (int)(int8_t)(tail >> 24) : AZ_UNSOLVED;
}

// The children one lane scores, one per round of 16: [r] is child r * LPG + sub of the parent, its score and what the walk needs of
// its header (N, first child, last word).
struct Scored {
    double key[4];
    int N[4], first[4];
    u32 tail[4];
};

// Round r of a scorer: marks the lane's child absent (key -inf), or loads it into c and keeps its header (the scorer then sets key[r]).
AZ_D bool load_child_grp(const Node *pool, const Node &parent, int r, int sub, Scored &s, Node &c) {
    s.key[r] = -__builtin_inf();
    s.N[r] = 0; s.first[r] = -1; s.tail[r] = 0;
    const int i = r * LPG + sub;
    if (i >= parent.nch) return false;
    c = load_node(pool + parent.first + i);
    s.N[r] = c.N; s.first[r] = c.first; s.tail[r] = node_tail(c);
    return true;
}

AZ_D int pick4(int v0, int v1, int v2, int v3, int r) { return r == 0 ? v0 : (r == 1 ? v1 : (r == 2 ? v2 : v3)); }

// fair_max (utils.py:28-34) among the children a group has scored: one lane per child, 16 children per round.  Children [0, nvote)
// take part in the ballot; when none of them holds the maximum, `none_err` (0: nothing) is raised.  `gid` is read only where a tie is
// drawn.  The chosen child's header is handed back by shuffle from the lane that scored it (no second memory trip); returns the
// child's index among the parent's children.  DRAW false: ties go to the lowest index whatever tie_mode says, no Philox draw.
// MASKED (az_engine_set_proof_backup): bit r of `skip` takes this lane's child of round r out of the ballot (its key is -inf already,
// so it does not set the maximum either; a voter mask, not a key: absent lanes carry -inf too and would win a ballot at -inf).
// CARRYQ (az_engine_set_puct): cq0 .. cq3 = the Q of this lane's child of round 0 .. 3 (by value, as the picks below); the chosen
// child's comes back in chosen.Q by one more 64-bit shuffle (first-play urgency reads the parent's Q at the next level).
template <bool DRAW = true, bool MASKED = false, bool CARRYQ = false>
AZ_D int choose_max_grp(const EngDev &E, const u32 &gid, int ply, int sim, int depth, const Scored &s, int nvote, int none_err,
                        int sub, Node &chosen, int skip = 0, double cq0 = 0.0, double cq1 = 0.0, double cq2 = 0.0, double cq3 = 0.0) {
    double best = grp_max(fmax(fmax(s.key[0], s.key[1]), fmax(s.key[2], s.key[3])));
    u32 mask[4];
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mask[r] = grp_ballot((r * LPG + sub) < nvote && (!MASKED || !((skip >> r) & 1)) && s.key[r] == best);
        cnt += __popc(mask[r]);
    }
    if (none_err && cnt == 0 && sub == 0) atomicOr(E.err, none_err);
    int k = 0;
    if (DRAW && E.tie_mode == AZ_TIE_RANDOM && cnt > 1) {  // with a single maximum the draw cannot change the result
        Philox4 rr = az_philox(E.seed, gid, (u32)ply, (u32)sim + E.sim_base, AZ_P_TIE_SELECT, (u32)depth);
        k = (int)(((u64)rr.x * (u64)cnt) >> 32);
    }
    int rsel = 0, lsel = 0;
    bool found = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int pc = __popc(mask[r]);
        if (!found) {
            if (k < pc) { rsel = r; lsel = kth_set_bit(mask[r], k); found = true; }
            else k -= pc;
        }
    }
    // by value: picked as lvalues, the compiler selects the ADDRESS, indexes s dynamically and moves it to scratch
    chosen.N = __shfl(pick4(s.N[0], s.N[1], s.N[2], s.N[3], rsel), lsel, LPG);
    chosen.first = __shfl(pick4(s.first[0], s.first[1], s.first[2], s.first[3], rsel), lsel, LPG);
    set_node_tail(chosen, (u32)__shfl(pick4((int)s.tail[0], (int)s.tail[1], (int)s.tail[2], (int)s.tail[3], rsel), lsel, LPG));
    chosen.Q = 0.0; chosen.P = 0.0; chosen.parent = 0;  // not needed by the walk
    if (CARRYQ) chosen.Q = __shfl(rsel == 0 ? cq0 : (rsel == 1 ? cq1 : (rsel == 2 ? cq2 : cq3)), lsel, LPG);
    return rsel * LPG + lsel;
}

// ---------------------------------------------------------------------------------------------
// Forced playouts and policy target pruning (az_engine_set_forced_playouts; KataGo: Wu 2019, section 3.2).
// Every operation is one IEEE double operation in the order written (-ffp-contract=off), sqrt the correctly rounded one of PUCT.
//   switch      k > 0 on (KataGo: 2), k = 0 off; finite and in [0, 64].
//   forced ply  a ply of a slot this engine searches, the mode on, that is full in the playout cap's sense: every ply with the cap
//               off, the plies whose coin playout_cap_full(seed, game id, ply, p_full) says full with it on.
//   selection   at depth 0 of the walk on a forced ply only.  R.N = the root's visit count as PUCT's square root takes it there.
//               Child c is FORCED iff c.N > 0 && (double)c.N * (double)c.N < (k * c.P) * (double)R.N  (c.P the stored prior, root
//               noise included; no square root).  A forced child's key is +inf, every other child keeps its PUCT key, and
//               choose_max_grp runs unchanged: several forced children are an ordinary tie (AZ_TIE_RANDOM: the AZ_P_TIE_SELECT
//               draw of that (ply, sim, depth 0); AZ_TIE_LOWEST: the lowest index).  A fresh root has R.N = 0: nothing is forced.
//               A root inherited through k_reroot applies the rule to the counts it inherited.  Below the root nothing changes.
//   pruning     wherever move_policy runs on a forced ply at a temperature other than 0.  c* = the child with the greatest N
//               (lowest index among equals, no draw); sq = sqrt((double)R.N); star = c*.Q + (c*.P * sq) / (double)(1 + c*.N).
//               N' = N for c* and for children with N = 0.  Every other child:
//                 nf = (int)sqrt((k * c.P) * (double)R.N);  gap = star - c.Q;
//                 need = c.N if gap <= 0.0; else want = (c.P * sq) / gap - 1.0, need = c.N if want >= (double)c.N,
//                 else (int)floor(want) + 1;
//                 N' = min(c.N, max(c.N - nf, need, 0));  if N' < c.N && N' <= 1 then N' = 0.
//               The temperature formula takes N' in place of N for the recorded pi and the move drawn from it (the same
//               AZ_P_MOVE_SAMPLE draw).  Temperature 0 (fair_max on the raw counts, one-hot pi), the visits rows and the Gumbel
//               branch do not change.
//   counters    forced_picks = the root selections in which at least one child was forced (counted per slot in fpicks[g], folded by
//               k_move once per ply); pruned_playouts = the sum of N - N' over the plies k_move recorded.  Both 0 with the mode off.
// The two rules as host-callable arithmetic (az_forced_playout / az_forced_prune are these on the host):
// ---------------------------------------------------------------------------------------------
AZ_HD bool forced_playout(int n, double p, int root_n, double k) {
    return n > 0 && (double)n * (double)n < (k * p) * (double)root_n;
}
// the pruned count of a child that is not c*: sq and star as above
AZ_HD int forced_pruned(int n, double q, double p, int root_n, double sq, double star, double k) {
    if (n == 0) return 0;
    const int nf = (int)sqrt((k * p) * (double)root_n);
    const double gap = star - q;
    int need = n;
    if (!(gap <= 0.0)) {
        const double want = (p * sq) / gap - 1.0;
        need = want >= (double)n ? n : (int)floor(want) + 1;
    }
    int m = n - nf;
    m = need > m ? need : m;
    m = m < 0 ? 0 : m;
    m = m < n ? m : n;
    return (m < n && m <= 1) ? 0 : m;
}

// ---------------------------------------------------------------------------------------------
// PUCT exploration settings (az_engine_set_puct; the contract stands in include/az_amd.h).  Every operation is one
// IEEE double operation in the order written (-ffp-contract=off), sqrt the correctly rounded one, log az_det_log.  The two rules as
// host-callable arithmetic (az_puct_c / az_puct_key are these on the host):
//   c    the exploration constant under a parent of parent_n visits
//   qu   the Q an unvisited child is assumed to have under first-play urgency (fpu >= 0): parent_q the parent's stored Q, vis the prior
//        mass of the parent's visited children; one value per parent, so the kernel takes its square root once per tree level
//   key  a child's score: sq = sqrt((double)parent.N), c and qu as above (qu is read only where the child is unvisited and fpu >= 0)
// ---------------------------------------------------------------------------------------------
AZ_HD double puct_c(int parent_n, double c_init, double c_base) {
    return c_base > 0.0 ? c_init + az_det_log(((1.0 + (double)parent_n) + c_base) / c_base) : c_init;
}
AZ_HD double puct_fpu_q(double parent_q, double vis, double fpu) { return (-parent_q) - fpu * sqrt(vis); }
AZ_HD double puct_key(double q_child, double p_child, int n_child, double sq, double c, double qu, double fpu) {
    const double q = (n_child > 0 || fpu < 0.0) ? q_child : qu;
    return q + ((c * p_child) * sq) / (double)(1 + n_child);
}

// ---------------------------------------------------------------------------------------------
// PUCT selection (mcts.py:44-46, 137) for k_step and k_step_multi.  k_step is walker j = 0 of a lock-step of one: no virtual count.
// leaf_batch = K > 1 (az_engine_set_leaf_batch): K simulations per slot and lock-step, kept apart by virtual loss.
// The reference searches strictly one simulation after the other (mcts.py:127-171 select_node, 197-223 back_propagate,
// 254-262 the loop of search): this is a different search, opt-in.  Contract:
//   lock-step t runs the walkers j = 0 .. k_t - 1 of every searching slot, simulation index t * K + j, one after the other;
//   walker j scores a child c of parent p with v(x) = the number of walkers i < j of this lock-step whose recorded path holds x:
//     Q term   v(c) == 0 ? c.Q : ((double)c.N * c.Q - (double)v(c)) / (double)(c.N + v(c))
//     U term   (c.P * sqrt((double)(p.N + v(p)))) / (double)(1 + c.N + v(c))
//   (every v = 0: the reference's PUCT, bit for bit); break tests and flags use the real N; a path position at depth >= LPG
//   is not recorded and counts 0.  A walker that lands on the pending leaf of an earlier walker i is a duplicate of i: no network
//   row, and at backup it propagates i's outcome.  Backup runs in ascending j (the bump allocator advances in that order).
// Virtual counts are never stored in a node: lane d of the group keeps the d-th node of every earlier walker's path (vpath), and a
// child at depth d + 1 is compared with path_i[d + 1] fetched from lane d + 1 by shuffle.
// ---------------------------------------------------------------------------------------------
// FORCED (az_engine_set_forced_playouts; the k_step_forced kernels only): with kf > 0 -- the root of a forced ply -- a child that
// forced_playout names takes the key +inf, and *forced_pick is raised when there was one; everything behind the keys is unchanged.
// PROOF (az_engine_set_proof_backup; the k_step_proof kernels only): `mover` = the player to move at the parent.  A
// child proven as a loss for the mover is no candidate -- key -inf and no vote -- unless every child is one (a root only: a node below
// it whose children are all proven is proven itself and stops the walk); at the root a child proven as the mover's win takes +inf.
// PUCT (az_engine_set_puct; the k_step_puct kernels only): the keys are puct_key's under the engine's c_init, c_base
// and fpu; parent.Q is the parent's real Q, and the chosen child's travels on in chosen.Q.  One walker per lock-step (leaf_batch > 1 is
// refused): no virtual count.  The children are loaded first, all four rounds, because an unvisited child's key reads the prior mass
// of the visited ones: four additions in the lane, four DPP steps over the group.
template <bool FORCED = false, bool PROOF = false, bool PUCT = false>
AZ_D int pick_child_vl_grp(const EngDev &E, int g, const Node *pool, const Node &parent, int pnode, const int (&vpath)[MLB], int j,
                           int ply, int sim, int depth, int sub, Node &chosen, double kf = 0.0, bool *forced_pick = nullptr, int mover = 0) {
    const int fc = parent.first;
    if (PUCT) {
        const double sq = sqrt((double)parent.N);
        const double cc = puct_c(parent.N, E.puct_cinit, E.puct_cbase), fpu = E.puct_fpu;
        Scored s;
        Node c0, c1, c2, c3;  // named, not an array: nothing here is indexed by a variable (choose_max_grp's note on scratch)
        c0.Q = c1.Q = c2.Q = c3.Q = 0.0; c0.P = c1.P = c2.P = c3.P = 0.0;
        const bool h0 = load_child_grp(pool, parent, 0, sub, s, c0), h1 = load_child_grp(pool, parent, 1, sub, s, c1);
        const bool h2 = load_child_grp(pool, parent, 2, sub, s, c2), h3 = load_child_grp(pool, parent, 3, sub, s, c3);
        double qu = 0.0;
        if (fpu >= 0.0) {  // uniform over the engine
            double vis = 0.0;
            vis = vis + ((h0 && s.N[0] > 0) ? c0.P : 0.0);
            vis = vis + ((h1 && s.N[1] > 0) ? c1.P : 0.0);
            vis = vis + ((h2 && s.N[2] > 0) ? c2.P : 0.0);
            vis = vis + ((h3 && s.N[3] > 0) ? c3.P : 0.0);
            qu = puct_fpu_q(parent.Q, grp_sum_f64(vis), fpu);
        }
        if (h0) s.key[0] = puct_key(c0.Q, c0.P, s.N[0], sq, cc, qu, fpu);
        if (h1) s.key[1] = puct_key(c1.Q, c1.P, s.N[1], sq, cc, qu, fpu);
        if (h2) s.key[2] = puct_key(c2.Q, c2.P, s.N[2], sq, cc, qu, fpu);
        if (h3) s.key[3] = puct_key(c3.Q, c3.P, s.N[3], sq, cc, qu, fpu);
        return fc + choose_max_grp<true, false, true>(E, E.game_id[g], ply, sim, depth, s, 4 * LPG, ERR_INTERNAL, sub, chosen, 0,
                                                      c0.Q, c1.Q, c2.Q, c3.Q);
    }
    int vp = 0, vc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < MLB; ++i) {
        if (i < j) {  // uniform over the group
            const int pd = depth < LPG ? __shfl(vpath[i], depth & (LPG - 1), LPG) : -1;
            const int cd = depth + 1 < LPG ? __shfl(vpath[i], (depth + 1) & (LPG - 1), LPG) : -1;
            vp += pd == pnode ? 1 : 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) vc[r] += cd == fc + r * LPG + sub ? 1 : 0;
        }
    }
    const double sq = sqrt((double)(parent.N + vp));
    Scored s;
    bool forced = false;
    int loss = 0;       // PROOF: bit r = this lane's child of round r is a proven loss for the mover
    bool live = false;  // PROOF: this lane holds a child that is not
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        Node c;
        if (load_child_grp(pool, parent, r, sub, s, c)) {
            const double q = vc[r] == 0 ? c.Q : ((double)c.N * c.Q - (double)vc[r]) / (double)(c.N + vc[r]);
            s.key[r] = q + (c.P * sq) / (double)(1 + c.N + vc[r]);
            if (FORCED && kf > 0.0 && forced_playout(c.N, c.P, parent.N + vp, kf)) { s.key[r] = __builtin_inf(); forced = true; }
            if (PROOF) {
                const int cw = proven_outcome(s.N[r], s.tail[r]);
                if (cw == -mover) loss |= 1 << r; else live = true;
                if (depth == 0 && cw == mover) s.key[r] = __builtin_inf();
            }
        }
    }
    if (FORCED && kf > 0.0 && grp_ballot(forced) != 0) *forced_pick = true;  // kf is uniform over the group
    if (PROOF) {
        if (grp_ballot(live) == 0) loss = 0;  // every child loses: all of them stay candidates
#pragma unroll
        for (int r = 0; r < 4; ++r) if ((loss >> r) & 1) s.key[r] = -__builtin_inf();
        // NaN scores stay an error: they equal no maximum, and a group whose voters all hold NaN finds -inf without a voter
        return fc + choose_max_grp<true, true>(E, E.game_id[g], ply, sim, depth, s, 4 * LPG, ERR_INTERNAL, sub, chosen, loss);
    }
    // every lane votes, and NaN scores (a diverged network) are an error: no key equals the maximum
    return fc + choose_max_grp(E, E.game_id[g], ply, sim, depth, s, 4 * LPG, ERR_INTERNAL, sub, chosen);
}

// One walker on its way from the root to its leaf: the board, the node it stands on, and the path so far.
struct Walk {
    BB b;
    Node cur;
    int node, plen, my_path;  // lane i keeps the i-th node of the root..leaf path in my_path (-1: none); depth = plen - 1
    bool bad;
};

// the deterministic scorer of az_engine_set_gumbel_full (defined with the Gumbel root search below): pick_child_vl_grp's signature
AZ_D int pick_child_gumbel_grp(const EngDev &E, int g, const Node *pool, const Node &parent, int pnode, const int (&vpath)[MLB], int j,
                               int ply, int sim, int depth, int sub, Node &chosen);

// select_node's descent (mcts.py:127-171) of walker j, from wk (the root, or wherever wk stands) to its leaf.  GUMBEL: the children
// are scored by pick_child_gumbel_grp instead of PUCT (the full Gumbel kernels only; every other kernel takes the default).
// FORCED: the selection at depth 0 applies the forced-playout rule with kf (0: not a forced ply); below the root nothing changes.
// PROOF (az_engine_set_proof_backup): below the root the walk stops on an F_PROVEN node as on a terminal one, and the scorer prunes
// by the proofs; the mover at depth d is the root's player times (-1)^d (a pass is an action: the side to move alternates strictly).
// PUCT (az_engine_set_puct): the scorer is pick_child_vl_grp's PUCT one; wk.cur then carries every node's real Q down the walk.
template <bool GUMBEL = false, bool FORCED = false, bool PROOF = false, bool PUCT = false>
AZ_D void walk_grp(const EngDev &E, int g, Node *pool, const int (&vpath)[MLB], int j, int ply, int sim, int sub, Walk &wk,
                   double kf = 0.0, bool *forced_pick = nullptr) {
    const int root_player = wk.b.player;  // PROOF: wk stands on the root when the step kernel calls
    for (;;) {
        bool fresh = false;
        if (PROOF && wk.plen > 1 && (wk.cur.flags & F_PROVEN)) break;
        if (!(wk.cur.flags & F_EXPANDED)) {
            if (wk.cur.flags & F_TERMINAL) break;  // mcts.py:146-147
            if (!(wk.cur.flags & F_EVALUATED)) { wk.bad = true; break; }
            wk.cur.flags |= F_EXPANDED;  // mcts.py:151-160 : children become visible now, also to the walkers that follow
            if (sub == 0) pool[wk.node].flags = wk.cur.flags;
            fresh = true;
        }
        Node ch;
        const int c = GUMBEL ? pick_child_gumbel_grp(E, g, pool, wk.cur, wk.node, vpath, j, ply, sim, wk.plen - 1, sub, ch)
                             : pick_child_vl_grp<FORCED, PROOF, PUCT>(E, g, pool, wk.cur, wk.node, vpath, j, ply, sim, wk.plen - 1, sub, ch,
                                                                      FORCED && wk.plen == 1 ? kf : 0.0, forced_pick,
                                                                      PROOF ? (((wk.plen - 1) & 1) ? -root_player : root_player) : 0);
        wk.node = c; wk.cur = ch;
        if (sub == wk.plen) wk.my_path = c;
        ++wk.plen;
        az_play_grp(E.gd, wk.b, wk.cur.act, sub);
        if (fresh || wk.cur.N == 0) break;  // mcts.py:143-144
    }
}

// What the walk ended on: LS_NONE (an internal error, reported), LS_TERM (w = the winner; a node found terminal now is marked)
// or LS_EVAL (the leaf wants a row of the network batch).
// PROOF (az_engine_set_proof_backup): a walk that ended below the root on an F_PROVEN node is LS_TERM with the node's outcome, and
// *proof_stop is raised.
template <bool PROOF = false>
AZ_D int classify_leaf_grp(const EngDev &E, Node *pool, const Walk &wk, int &w, int sub, bool *proof_stop = nullptr) {
    if (wk.bad) {
        if (sub == 0) atomicOr(E.err, ERR_INTERNAL);
        return LS_NONE;
    }
    if (wk.cur.flags & F_TERMINAL) { w = wk.cur.win; return LS_TERM; }
    if (PROOF && wk.plen > 1 && (wk.cur.flags & F_PROVEN)) { w = wk.cur.win; *proof_stop = true; return LS_TERM; }
    if (az_status_grp(E.gd, wk.b, &w, sub)) {  // mcts.py:185-186
        if (sub == 0) { pool[wk.node].flags = wk.cur.flags | F_TERMINAL; pool[wk.node].win = (int8_t)w; }
        return LS_TERM;
    }
    return LS_EVAL;
}

// Rows of the network batch are handed out per BLOCK: one LDS count of the lanes that want one and one global atomic per 16 games,
// instead of one per game on a single hot address.  Three workgroup barriers: EVERY wave of the block calls this, the same number
// of times, whether its lanes want a row or not.  Returns the lane's row (meaningless for a lane that wanted none).
AZ_D int alloc_rows_block(int *counter, bool want) {
    __shared__ int s_need, s_base;
    if (threadIdx.x == 0) s_need = 0;
    __syncthreads();
    int rank = 0;
    if (want) rank = atomicAdd(&s_need, 1);  // LDS atomic
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_need > 0 ? atomicAdd(counter, s_need) : 0;
    __syncthreads();
    return s_base + rank;
}

// az_engine_set_eval_cache: the pending leaf `b` of a slot against its group's table, by the group's lanes sub < AZ_EC_PROBE with one
// entry each (tag and key come in one round trip).  `stamp` is this kernel's.  Returns the entry on a hit; else -1, with *claim = the
// entry this slot claimed for the position -- it writes the key here and the payload in the next kernel's backup -- or -1.
//   hit   : the full key is equal and the entry's stamp is older than this kernel's.  Such an entry was claimed in an earlier kernel of
//           this stream, so its key is complete (kernel boundary); its payload is written by the kernel after the claim -- at the latest
//           the one running -- and is read by the NEXT kernel's backup, behind another boundary.
//   claim : the first probed entry seen empty, by one device-scope atomicCAS (executed at the memory side, so exact whatever an XCD's
//           L2 holds).  A tag is written once per run, so a stale view of it is the empty one and ends in a lost CAS: a miss, no insert.
//   An entry of this very kernel (equal stamp) under the position's hash ends the lookup without a claim: most likely another slot's
//   claim of the same position.  Nothing loops, nothing waits for another workgroup.
AZ_D int ec_lookup_grp(const EngDev &E, const BB &b, u32 stamp, int sub, int *claim) {
    const u32 h = ec_hash(b.p1, b.m1, b.player);
    const int idx = (int)ec_bucket(h, sub & (AZ_EC_PROBE - 1), E.ec_mask + 1u);
    EcHdr *p = E.ec_hdr + idx;
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    const uint4 x = q[0], y = q[1];
    const u64 tag = ((u64)x.y << 32) | x.x, p1 = ((u64)x.w << 32) | x.z, m1 = ((u64)y.y << 32) | y.x;
    const bool lane = sub < AZ_EC_PROBE;
    const bool same = tag != 0 && ec_tag_hash(tag) == h, older = ec_tag_stamp(tag) < stamp;
    const u32 m_hit = grp_ballot(lane && same && older && p1 == b.p1 && m1 == b.m1 && (int)y.z == b.player);
    const u32 m_now = grp_ballot(lane && same && !older);
    const u32 m_free = grp_ballot(lane && tag == 0);
    *claim = -1;
    if (m_hit) return __shfl(idx, __ffs((int)m_hit) - 1, LPG);
    if (m_now || !m_free) return -1;
    const int first = __ffs((int)m_free) - 1;
    int won = 0;
    if (sub == first) {
        won = atomicCAS(&p->tag, 0ULL, ec_tag(h, stamp)) == 0ULL ? 1 : 0;
        if (won) { p->p1 = b.p1; p->m1 = b.m1; p->player = (long long)b.player; }
    }
    if (__shfl(won, first, LPG)) *claim = __shfl(idx, first, LPG);
    return -1;
}

// The network's output for the leaf a slot selected in the previous lock-step: row `row` of the batch, or the payload of the table
// entry the row stands for (ec_row_of_entry; only with az_engine_set_eval_cache in force).  *v = the value.  A third kind of row, in
// k_step_heads alone: blk_pr = the priors the block has just computed for the slot's batch row into its LDS, blk_v their value.
AZ_D const float *leaf_output(const EngDev &E, int row, float *v, const float *blk_pr = nullptr, float blk_v = 0.0f) {
    if (ec_row_is_entry(row)) {
        const float *pay = E.ec_pay + (size_t)ec_entry_of_row(row) * E.ec_stride;
        *v = pay[E.A];
        return pay;
    }
    if (blk_pr) { *v = blk_v; return blk_pr; }
    *v = E.value[row];
    return E.probs + (size_t)row * E.A;
}

AZ_D double log_gamma_draw(const EngDev &E, u32 gid, int ply, int sim, double alpha, u32 j) {
    double d = (alpha + 1.0) - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d), g = d;
    bool accepted = false;
    for (u32 att = 0; att < 64; ++att) {
        Philox4 r = az_philox(E.seed, gid, (u32)ply, (u32)sim, AZ_P_NOISE_NORMAL, j | (att << 8));
        Philox4 q = az_philox(E.seed, gid, (u32)ply, (u32)sim, AZ_P_NOISE_NORMAL, j | (att << 8) | 0x80000000u);
        double u1 = 2.0 * az_u53(r.x, r.y) - 1.0, u2 = 2.0 * az_u53(r.z, r.w) - 1.0;
        double s = u1 * u1 + u2 * u2;
        if (!(s < 1.0) || s == 0.0) continue;
        double x = u1 * sqrt(-2.0 * az_det_log(s) / s);
        double v = 1.0 + c * x;
        if (!(v > 0.0)) continue;
        v = v * v * v;
        double u = 1.0 - az_u53(q.x, q.y);
        if (az_det_log(u) < 0.5 * x * x + d - d * v + d * az_det_log(v)) { g = d * v; accepted = true; break; }
    }
    if (!accepted) atomicOr(E.err, ERR_RNG);
    Philox4 r = az_philox(E.seed, gid, (u32)ply, (u32)sim, AZ_P_NOISE_BOOST, j);
    double ub = 1.0 - az_u53(r.x, r.y);
    return az_det_log(g) + az_det_log(ub) / alpha;
}

AZ_D double sel4(const double (&v)[4], int r) { return r == 0 ? v[0] : (r == 1 ? v[1] : (r == 2 ? v[2] : v[3])); }

// mcts.py:235-240 : P <- (1-eps) P + eps eta over the root's children, one lane per child
AZ_D void apply_root_noise_grp(const EngDev &E, int g, Node *pool, int root, const Node &rn, const BB &rb, int ply, int sim, int sub) {
    const int fc = rn.first, k = rn.nch;
    double eta[4];
    Node ch[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { int i = r * LPG + sub; ch[r] = load_node(pool + fc + (i < k ? i : 0)); }
    if (E.noise_mode == AZ_NOISE_HASH) {
        u64 h = az_board_hash(E.gd, rb), w[4], tot = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int i = r * LPG + sub;
            w[r] = i < k ? 1 + (az_splitmix64(h + (u64)(ch[r].act + 1) * 0xBF58476D1CE4E5B9ULL) >> 54) : 0;
            tot += w[r];
        }
        tot = grp_sum_u64(tot);
#pragma unroll
        for (int r = 0; r < 4; ++r) eta[r] = (double)w[r] / (double)tot;
    } else {
        double lg[4], m = -__builtin_inf();
        const u32 gid = E.game_id[g];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int i = r * LPG + sub;
            lg[r] = i < k ? log_gamma_draw(E, gid, ply, sim, E.alpha, (u32)i) : -__builtin_inf();
            m = fmax(m, lg[r]);
        }
        m = grp_max(m);
#pragma unroll
        for (int r = 0; r < 4; ++r) eta[r] = (r * LPG + sub) < k ? az_det_exp(lg[r] - m) : 0.0;
        double s = 0.0;  // sequential sum in ascending child order, as in the CPU restatement
        for (int i = 0; i < k; ++i) s += __shfl(sel4(eta, i >> 4), i & 15, LPG);
#pragma unroll
        for (int r = 0; r < 4; ++r) eta[r] = eta[r] / s;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int i = r * LPG + sub;
        if (i < k) {
            double P = ch[r].P;
            double keep = (ch[r].flags & F_PF32) ? (double)((float)(1.0 - E.eps) * (float)P) : (1.0 - E.eps) * P;
            pool[fc + i].P = keep + E.eps * eta[r];
            pool[fc + i].flags = ch[r].flags & (uint8_t)~F_PF32;
        }
    }
    if (sub == 0) pool[root].flags = rn.flags | F_NOISED;
}

// back_propagate (mcts.py:197-223).  The select step recorded the root..leaf path, so every node on it
// is updated by its own lane in one memory round trip (reward sign alternates from the leaf up);
// paths longer than 16 nodes fall back to chasing parent pointers.  `mine` = this lane's path node (already
// loaded), returns true when the fast path ran (lane 0 then holds the root with its N already incremented).
// KEEPQ (az_engine_set_puct): `mine` takes the Q it has just written too (the forwarded root's real Q).
template <bool KEEPQ = false>
AZ_D bool back_propagate_grp(Node *pool, int len, int my_node, Node &mine, int leaf, int player_to_play, double outcome, int sub) {
    double reward;
    if (fabs(outcome) < 1e-4) reward = 0.0;
    else reward = ((double)player_to_play * outcome > 0.0) ? -fabs(outcome) : fabs(outcome);
    if (len <= LPG) {
        if (sub < len) {
            const int up = len - 1 - sub;  // edges above the leaf
            const double r = (reward == 0.0) ? 0.0 : ((up & 1) ? -reward : reward);
            pool[my_node].Q = ((double)mine.N * mine.Q + r) / (double)(mine.N + 1);
            pool[my_node].N = mine.N + 1;
            if (KEEPQ) mine.Q = ((double)mine.N * mine.Q + r) / (double)(mine.N + 1);
            mine.N += 1;
        }
        return true;
    }
    int node = leaf;
    while (node >= 0) {
        Node n = load_node(pool + node);  // same address in all 16 lanes: one broadcast transaction
        if (sub == 0) {
            pool[node].Q = ((double)n.N * n.Q + reward) / (double)(n.N + 1);
            pool[node].N = n.N + 1;
        }
        node = n.parent;
        reward = (reward == 0.0) ? 0.0 : -reward;
    }
    return false;
}

// az_engine_set_proof_backup: the proofs a backup of a terminal leaf brings about.  From the leaf's parent upward,
// one group-wide step per level: the node (one address, a broadcast), its children in four rounds of 16, three ballots.  A node of
// mover m is proven when some child is proven with outcome m (then m), or when every child is proven (0 with a drawn child, else -m);
// lane 0 marks it and the walk up goes on, the first node the rule does not prove ends it.  my_node = this lane's path node (paths of
// at most LPG nodes; longer ones chase parents from the leaf, as the backup does).  The loop's condition is uniform over the group.
// Returns the nodes newly marked; *root_win is set, and true returned in *root_marked, when the root (path position 0) is one of them.
AZ_D int propagate_proofs_grp(Node *pool, int plen, int my_node, int leaf, int root_player, int sub, bool *root_marked, int *root_win) {
    // the backup's stores (other lanes: the leaf's first visit among them) must be visible to the loads below
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    int marked = 0;
    int chase = plen > LPG ? load_node(pool + leaf).parent : -1;
    for (int pos = plen - 2; pos >= 0; --pos) {
        const int pn = plen <= LPG ? __shfl(my_node, pos, LPG) : chase;
        if (pn < 0) break;
        const Node p = load_node(pool + pn);
        if (p.nch == 0) break;  // a path node above the leaf always has children
        const int m = (pos & 1) ? -root_player : root_player;
        Scored s;
        bool win = false, open = false, draw = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Node c;
            if (load_child_grp(pool, p, r, sub, s, c)) {
                const int cw = proven_outcome(s.N[r], s.tail[r]);
                win |= cw == m; draw |= cw == 0; open |= cw == AZ_UNSOLVED;
            }
        }
        const bool any_win = grp_ballot(win) != 0, any_open = grp_ballot(open) != 0, any_draw = grp_ballot(draw) != 0;
        if (!any_win && any_open) break;
        const int out = any_win ? m : (any_draw ? 0 : -m);
        if (!(p.flags & F_PROVEN)) {
            ++marked;
            if (sub == 0) { pool[pn].flags = p.flags | F_PROVEN; pool[pn].win = (int8_t)out; }
            if (pos == 0) { *root_marked = true; *root_win = out; }
            // the mark must be visible to the next level's loads (this node is a child there) and to the SELECT half
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
        chase = p.parent;
    }
    return marked;
}

// Resignation in self-play (az_engine_set_resign; the contract is in include/az_amd.h and above its code in
// k_move).  The two pieces of arithmetic the host can call (az_resign_value / az_resign_holdout are these on the host):
//   the value of a ply, from the root's children in pool order i = 0 .. nc - 1 (N and Q each behind a byte stride: the kernels pass a
//   Node's two fields, the host two plain arrays):  S_N = sum N_i;  S_Q = sum over N_i > 0 of (double)N_i * Q_i, in that order in
//   float64;  v_mean = S_Q / (double)S_N;  v_best = Q of the child with the greatest N (the lowest index among equals);
//   v = v_best > v_mean ? v_best : v_mean.  false (and *v untouched) when S_N == 0: the ply is untested.
AZ_HD bool resign_value(int nc, const void *N, size_t n_stride, const void *Q, size_t q_stride, double *v) {
    long long sn = 0;
    double sq = 0.0, vbest = 0.0;
    int best = -1;
    for (int i = 0; i < nc; ++i) {
        const int n = *reinterpret_cast<const int *>(static_cast<const char *>(N) + (size_t)i * n_stride);
        const double q = *reinterpret_cast<const double *>(static_cast<const char *>(Q) + (size_t)i * q_stride);
        if (n > 0) { sn += n; sq += (double)n * q; }
        if (n > best) { best = n; vbest = q; }
    }
    if (sn == 0) return false;
    const double vmean = sq / (double)sn;
    *v = vbest > vmean ? vbest : vmean;
    return true;
}
//   the holdout coin of a game: one draw per (seed, game id), never a function of the slot, the slot group or the batch
#define AZ_P_RESIGN 11
AZ_HD bool resign_holdout(u32 seed, u32 gid, double p_holdout) {
    const Philox4 r = az_philox(seed, gid, 0u, 0xFFFFu, AZ_P_RESIGN, 0);
    return az_u53(r.x, r.y) < p_holdout;
}

// first_id: the first game id of the run (the game log's row of game_id is game_id - first_id)
AZ_D void reset_slot(const EngDev &E, int g, u32 game_id, u32 first_id) {
    BB b;
    start_position(E.gd, b);
    E.root_p1[g] = b.p1; E.root_m1[g] = b.m1; E.root_player[g] = (int8_t)b.player;
    E.root[g] = 0; E.n_nodes[g] = 1; E.ply[g] = 0; E.game_id[g] = game_id; E.active[g] = 1;
    E.leaf_status[g] = LS_NONE; E.evals[g] = 0; E.side[g] = 0; E.gmask[g] = 0;
    if (E.fpicks) E.fpicks[g] = 0;
    if (E.rs) {  // az_engine_set_resign: both windows empty, the game's log row opened with its holdout coin
        const ResignDev R = *E.rs;
        R.rs_cnt[2 * g] = 0; R.rs_cnt[2 * g + 1] = 0;
        const u32 at = game_id - first_id;
        if (at < (u32)R.gl_n) {
            int *row = R.gl_rows + (size_t)at * 8;
            row[0] = (int)game_id; row[1] = 0; row[2] = 0; row[3] = 0;
            row[4] = resign_holdout(E.seed, game_id, R.rs_phold) ? 1 : 0;
            row[5] = -1; row[6] = 0; row[7] = 0;
            R.gl_low[(size_t)at * 2] = 2.0; R.gl_low[(size_t)at * 2 + 1] = 2.0;
        }
    }
    store_node(pool_of(E, g), fresh_node(0, -1, 0.0, 0));
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
__global__ void k_reset_all(EngDev E, u32 first_id, int n_games) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) {
        for (int i = 0; i < CTR_COUNT; ++i) E.ctr[i] = 0;
        E.ctr[CTR_NEXT_GAME] = (unsigned long long)(n_games < E.G ? n_games : E.G);
        E.ctr[CTR_TOTAL_GAMES] = (unsigned long long)n_games;
        E.ctr[CTR_FIRST_ID] = first_id;
        *E.err = 0; *E.max_nodes = 0; *E.max_path = 0;
        for (int i = 0; i < 4 * AZ_MAX_GROUPS; ++i) E.batch_cnt[i] = 0;  // every slot group's counters (E is the whole engine's view)
    }
    if (g >= E.G) return;
    E.pool_sel[g] = 0;
    if (E.x_solved) { E.x_solved[g] = 0; E.x_nodes[g] = 0; }
    if (E.pf) { E.pf[g] = 0; E.pf[E.G + g] = 0; E.pf[2 * E.G + g] = 0; }
    if (g < n_games) reset_slot(E, g, first_id + (u32)g, first_id);
    else { E.active[g] = 0; E.leaf_status[g] = LS_NONE; }
}

// Playout cap randomization (az_engine_set_playout_cap): the coin of (game id, ply).  The same arithmetic on the host
// (az_playout_cap_full) and in the two kernels that draw it: k_root_prep for the search budget, k_move for the record.
#define AZ_P_PLAYOUT_CAP 10
AZ_HD bool playout_cap_full(u32 seed, u32 gid, int ply, double p_full) {
    const Philox4 r = az_philox(seed, gid, (u32)ply, 0xFFFFu, AZ_P_PLAYOUT_CAP, 0);
    return az_u53(r.x, r.y) < p_full;
}

// mcts.py:231-233 : a root without priors is evaluated first (value discarded)
// (no barrier in here: a group leaves as a whole, and the rows are drawn per group)
__global__ __launch_bounds__(256) void k_root_prep(EngDev E, int g0, int g1) {
    const int g = g0 + blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (g >= g1) return;
    // the playout cap's budget of this search call, once per slot and ply: one Philox draw on the group's first lane
    if (E.budget && sub == 0) E.budget[g] = playout_cap_full(E.seed, E.game_id[g], E.ply[g], E.cap_pfull) ? CAP_FULL : E.cap_nfast;
    uint8_t fresh = 0;
    if (searches(E, g)) {
        uint8_t f = pool_of(E, g)[E.root[g]].flags;
        if (!(f & (F_EVALUATED | F_TERMINAL))) {
            fresh = 1;
        }
    }
    if (fresh) {
        BB b = {E.root_p1[g], E.root_m1[g], E.root_player[g]};
        int row = alloc_row_grp(E.batch_cnt + 2, sub);
        write_nn_input_grp(E, row, b, sub);
        if (sub == 0) E.row_of_slot[g] = row;
    }
    if (sub == 0) E.root_fresh[g] = fresh;
}

__global__ __launch_bounds__(256) void k_root_init(EngDev E, int g0, int g1) {
    const int g = g0 + blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (g >= g1 || !E.root_fresh[g]) return;
    BB b = {E.root_p1[g], E.root_m1[g], E.root_player[g]};
    Node *pool = pool_of(E, g);
    const int k = create_children_grp(E, g, pool, E.n_nodes[g], E.root[g], b, E.probs + (size_t)E.row_of_slot[g] * E.A, sub);
    // the value is discarded for the backup, as the reference discards it; az_engine_set_gumbel_full keeps it for the root's v_mix
    if (E.nval && k > 0 && sub == 0) nval_of(E, pool)[E.root[g]] = E.value[E.row_of_slot[g]];
    if (sub == 0) E.evals[g] += 1;
}

#ifdef AZ_PROBE  // diagnostic build only (make PROBE=1)
__device__ unsigned long long az_step_probe[4096 * 8];
#define PSTAMP(i) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); pt[i] = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }
#else
#define PSTAMP(i)
#endif

// One lock-step of the search for every slot:
//   BACKUP : nn_evaluation bookkeeping (mcts.py:188-191) + back_propagate (mcts.py:197-223) of the
//            leaf selected in the previous step, whose policy/value the network has just produced
//   SELECT : root noise (mcts.py:235-240) + select_node (mcts.py:127-171) of simulation `sim`,
//            writing the next leaf's canonical board into the network's input batch
// CAP (az_engine_set_playout_cap, k_step_cap): the slot walks the simulations sim < budget[g] of the search call only (k_root_prep
// wrote the budget: CAP_FULL on a full ply, n_fast on a fast one) and takes root noise on a full ply only.  A slot past its budget
// stays an inert group for the SELECT half -- no walk, no row, leaf_status LS_NONE, so the next BACKUP does nothing for it -- and
// still reaches every barrier of alloc_rows_block; it is NOT deactivated.  CAP false is the kernel as it always was.
// FORCED (az_engine_set_forced_playouts, k_step_forced / k_step_cap_forced): on a full ply (budget == CAP_FULL) the root's selection
// is walk_grp's forced one with k = kforced, and the group's first lane counts the selections that had a forced child in fpicks[g],
// with the pending-leaf stores.  FORCED false is the kernel as it was.
// EC (az_engine_set_eval_cache, k_step_cached): the leaf is looked up in the slot group's table before it asks for a batch row, and a
// slot that claimed an entry fills it in its next backup.  EC false is the kernel as it was: none of that code is compiled in.
// EXACT (az_engine_set_exact_endgame, k_step_exact): a leaf that wants a network row and has at most exact_max empty cells is solved
// on the spot (az_solve.h; xstk = the block's frame store in LDS) and becomes a terminal node whose winner is the outcome.  Before the
// cache is consulted, and before the rows are handed out: the solver holds no barrier and the group leaves it as a whole.  EXACT false
// is the kernel as it was.
// PROOF (az_engine_set_proof_backup, k_step_proof): the backup of an LS_TERM leaf is followed by
// propagate_proofs_grp, the walk and its scorer take the proofs into account, and a walk that ends on an F_PROVEN node is LS_TERM: no
// row, no solve, no cache lookup.  PROOF false is the kernel as it was.
// PUCT (az_engine_set_puct, k_step_puct): the walk scores by puct_key, and the root this kernel's backup forwards to
// its own walk carries the Q that backup has just written (first-play urgency reads it).  PUCT false is the kernel as it was.
// HEADS (k_step_heads): the 16-column tiles of the net's padded logits, 0 = off.  The forward before this kernel
// stopped behind fc2: the block computes the heads of its own slots' rows (heads_block16) in front of the backup and reads priors and
// values from its LDS; E.probs / E.value are neither written nor read.  A slot brings a row if its leaf is LS_EVAL with a batch row
// (row_prev >= 0: not a cache hit); every thread of the block reaches the routine, whose barriers lie in front of every divergent
// branch below.  HEADS 0 is the kernel as it was.
template <bool BACKUP, bool SELECT, bool CAP, bool FORCED, bool EC = false, bool EXACT = false, bool PROOF = false, bool PUCT = false, int HEADS = 0>
AZ_D void step_grp(const EngDev &E, int sim, int g0, int g1, u64 *xstk = nullptr) {
    const int g = g0 + blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    // this step's leaves are compacted into rows [0, batch_cnt[sim & 1]); the other counter (read by the
    // previous step's network kernels, which have completed) is cleared for the next step
    // (a slot range is a slot group with counters of its own: its first block clears them)
    if (blockIdx.x == 0 && threadIdx.x == 0) { E.batch_cnt[(sim + 1) & 1] = 0; if (!SELECT) E.batch_cnt[2] = 0; }
#ifdef AZ_PROBE
    unsigned long long pt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    PSTAMP(0)
    // Groups beyond the last slot (the slot count need not fill the last wavefront / block) stay in the kernel as
    // inert groups: every __syncthreads() below must be reached by all waves of the block the same number of times, and
    // an early return -- or barriers in a divergent branch -- of SOME lanes of a wavefront breaks exactly that (the
    // wave would arrive twice per barrier: leaf rows were then handed out before all groups had asked for one).
    const bool in_range = g < g1;
    const int gs = in_range ? g : g1 - 1;  // a valid index for the (unused) loads of an inert group
    // ---- every per-slot word is fetched here, in one batch of independent loads: the kernel is bound by
    // ---- the number of DEPENDENT memory round trips (~1 us each), not by bytes
    Node *pool = pool_of(E, gs);
    const int st = (BACKUP && in_range) ? E.leaf_status[gs] : LS_NONE;
    const int leaf = BACKUP ? E.leaf[gs] : 0;
    const BB lb = {BACKUP ? E.leaf_p1[gs] : 0, BACKUP ? E.leaf_m1[gs] : 0, BACKUP ? E.leaf_player[gs] : 1};
    const int row_prev = BACKUP ? E.row_of_slot[gs] : 0;
    const int plen_prev = BACKUP ? E.path_len[gs] : 0;
    const int path_prev = BACKUP ? E.path[(size_t)gs * LPG + sub] : 0;
    const int lwin = BACKUP ? E.leaf_winner[gs] : 0;
    int n_nodes = E.n_nodes[gs];
    int evals = E.evals[gs];
    bool active = in_range && searches(E, gs);
    const int ply = E.ply[gs];
    BB b = {E.root_p1[gs], E.root_m1[gs], E.root_player[gs]};
    int node = E.root[gs];
    const int budget = CAP ? E.budget[gs] : CAP_FULL;  // with the loads above: no round trip of its own
    const int fpicks = (FORCED && SELECT) ? E.fpicks[gs] : 0;
    // az_engine_set_eval_cache: the entry the pending leaf claimed, and the group's serial word (uniform; this kernel's stamp with sim)
    // and, in the ply's last backup, the slot's hits of this ply, which that kernel folds into ctr[]
    const int ec_prev = (EC && BACKUP) ? E.ec_claim[gs] : -1;
    const u32 ec_serial = EC ? *E.ec_serial : 0u;
    const int ec_nhits = (EC && !SELECT) ? E.ec_hits[gs] : 0;
    Node fwd;
    bool have_root = false;
    PSTAMP(1)
    Node mine;
    const bool on_path = plen_prev <= LPG && sub < plen_prev;
    const float *blk_pr = nullptr;
    float blk_v = 0.0f;
    if (HEADS > 0) {
        // the path nodes are requested in front of the heads: their round trip runs beside the staging of the rows
        if (BACKUP && st != LS_NONE && on_path) mine = load_node(pool + path_prev);
        heads_block16<(HEADS > 0 ? HEADS : 1)>(E.sh_h2, (BACKUP && st == LS_EVAL && row_prev >= 0) ? row_prev : -1, E.sh_wq, E.sh_hb, E.A, &blk_pr, &blk_v);
    }
    if (BACKUP && st != LS_NONE) {
        // path nodes and the network row are fetched together (second round trip)
        if (HEADS == 0 && on_path) mine = load_node(pool + path_prev);
        double outcome;
        bool ok = true;
        if (st == LS_EVAL) {
            float v = 0.0f;
            const float *pr = HEADS > 0 ? nullptr : E.probs + (size_t)row_prev * E.A;
            if (HEADS > 0) pr = leaf_output(E, row_prev, &v, blk_pr, blk_v);
            else if (EC) pr = leaf_output(E, row_prev, &v);
            else v = E.value[row_prev];
            int k = create_children_grp(E, g, pool, n_nodes, leaf, lb, pr, sub);
            if (EC && ec_prev >= 0) {  // the slot won its claim in the previous kernel: its batch row becomes the entry's payload
                float *pay = E.ec_pay + (size_t)ec_prev * E.ec_stride;
                for (int i = sub; i <= E.A; i += LPG) pay[i] = i < E.A ? pr[i] : v;
            }
            ok = k > 0;
            n_nodes += ok ? k : 0;
            outcome = (double)lb.player * (double)v;  // base.py:366
            if (ok) evals += 1;
            else { active = false; if (sub == 0) E.active[g] = 0; }
        } else {
            outcome = (double)lwin;
        }
        PSTAMP(2)
        if (ok) {
            bool fast = back_propagate_grp<PUCT>(pool, plen_prev, path_prev, mine, leaf, lb.player, outcome, sub);
            if (fast && SELECT) {  // lane 0 holds the root (path[0]) with its new visit count: forward it
                fwd.N = __shfl(mine.N, 0, LPG);
                fwd.first = __shfl(mine.first, 0, LPG);
                set_node_tail(fwd, (u32)__shfl((int)node_tail(mine), 0, LPG));
                fwd.Q = 0.0; fwd.P = 0.0; fwd.parent = -1;
                if (PUCT) fwd.Q = __shfl(mine.Q, 0, LPG);
                // the root itself may be the leaf that just got its children (first visit of an unexpanded root)
                have_root = (leaf != node) || st != LS_EVAL;
            }
            if (PROOF && st == LS_TERM) {  // only a terminal leaf's backup can decide a node: the dependent round trips are paid here alone
                bool root_marked = false;
                int root_win = 0;
                const int marked = propagate_proofs_grp(pool, plen_prev, path_prev, leaf, b.player, sub, &root_marked, &root_win);
                // the forwarded root was read before the walk up: it carries what the propagation has just written
                if (root_marked && fast && SELECT) { fwd.flags |= F_PROVEN; fwd.win = (int8_t)root_win; }
                if (marked && sub == 0) E.pf[g] += marked;
            }
        }
        if (sub == 0) E.leaf_status[g] = LS_NONE;
        // the group's own stores (other lanes) must be visible to the loads below
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    PSTAMP(3)
    if (BACKUP && sub == 0 && in_range) E.evals[g] = evals;
    if (!SELECT) {
        // the ply's last backup: no lookup in this kernel, so no block needs the serial word any more -- the next ply's stamps follow on
        if (EC && blockIdx.x == 0 && threadIdx.x == 0) *E.ec_serial = ec_stamp(ec_serial, sim);
        if (EC && sub == 0 && in_range && ec_nhits) { atomicAdd(&E.ctr[CTR_CACHE_HITS], (unsigned long long)ec_nhits); E.ec_hits[g] = 0; }
        return;
    }
    // From here on no group may leave early: the leaf rows are handed out per block (alloc_rows_block) behind workgroup barriers.
    int status = LS_NONE, w = 0;
    Walk wk = {b, Node(), node, 1, sub == 0 ? node : -1, false};
    const bool walks = active && (!CAP || sim < budget);  // uniform over the game's group
    bool forced_pick = false, proof_stop = false;
    if (walks) {
        if (have_root) wk.cur = fwd; else wk.cur = load_node(pool + node);
        const bool noise_ply = !CAP || budget == CAP_FULL;  // a fast ply takes no root noise and leaves F_NOISED clear
        if (noise_ply && E.noise_mode != AZ_NOISE_OFF && E.alpha >= 0.0 && E.eps >= 0.0 && (wk.cur.flags & F_EXPANDED) && !(wk.cur.flags & F_NOISED)) {
            apply_root_noise_grp(E, g, pool, node, wk.cur, b, ply, sim, sub);
            wk.cur.flags |= F_NOISED;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
        PSTAMP(4)
        const int no_walkers[MLB] = {};  // walker j = 0: nobody walked before it in this lock-step, every virtual count is 0
        if (FORCED) walk_grp<false, true>(E, g, pool, no_walkers, 0, ply, sim, sub, wk, budget == CAP_FULL ? E.kforced : 0.0, &forced_pick);
        else if (PROOF) walk_grp<false, false, true>(E, g, pool, no_walkers, 0, ply, sim, sub, wk);
        else if (PUCT) walk_grp<false, false, false, true>(E, g, pool, no_walkers, 0, ply, sim, sub, wk);
        else walk_grp(E, g, pool, no_walkers, 0, ply, sim, sub, wk);
        PSTAMP(5)
        E.path[(size_t)g * LPG + sub] = wk.my_path;
        if (sub == 0) { E.path_len[g] = wk.plen; if (wk.plen > LPG) atomicMax(E.max_path, wk.plen); }
        if (PROOF) status = classify_leaf_grp<true>(E, pool, wk, w, sub, &proof_stop);
        else status = classify_leaf_grp(E, pool, wk, w, sub);
        if (EXACT && status == LS_EVAL && wk.plen > 1 && __popcll(E.gd.valid & ~(wk.b.p1 | wk.b.m1)) <= E.exact_max) {
            int sw = 0, sa = -1;
            unsigned long long cnt = 0;
            if (az_solve_grp<AZ_EXACT_MAX_EMPTIES, 256>(E.gd, wk.b, sub, xstk + threadIdx.x, false, 0, &sw, &sa, &cnt) == AZ_SOLVE_OK) {
                w = sw;
                status = LS_TERM;
                if (sub == 0) {
                    pool[wk.node].flags = wk.cur.flags | F_TERMINAL | F_SOLVED; pool[wk.node].win = (int8_t)w;
                    E.x_solved[g] += 1; E.x_nodes[g] += cnt;
                }
            } else if (sub == 0) {
                atomicOr(E.err, ERR_INTERNAL);  // the solver's ceiling: reported, and the leaf goes to the network
            }
        }
    }
    // az_engine_set_eval_cache: a leaf within the stone limit is looked up first; a hit takes no batch row and writes no input, the next
    // backup reads the entry's payload through the negative row.  Beyond the limit the kernel pays this one compare.
    int ec_hit = -1, ec_claim = -1;
    if (EC && status == LS_EVAL && ec_in_limit(wk.b.p1, wk.b.m1, E.ec_limit)) ec_hit = ec_lookup_grp(E, wk.b, ec_stamp(ec_serial, sim), sub, &ec_claim);
    const int row = __shfl(alloc_rows_block(E.batch_cnt + (sim & 1), status == LS_EVAL && ec_hit < 0 && sub == 0), 0, LPG);
    if (status == LS_EVAL) {
        if (ec_hit < 0) write_nn_input_grp(E, row, wk.b, sub);
        if (sub == 0) E.row_of_slot[g] = ec_hit < 0 ? row : ec_row_of_entry(ec_hit);
    }
    if (sub == 0 && in_range) {
        if (walks) {
            E.leaf[g] = wk.node; E.leaf_p1[g] = wk.b.p1; E.leaf_m1[g] = wk.b.m1; E.leaf_player[g] = (int8_t)wk.b.player;
            E.leaf_winner[g] = (int8_t)w;
            if (FORCED && forced_pick) E.fpicks[g] = fpicks + 1;
            if (PROOF && proof_stop) E.pf[E.G + g] += 1;
        }
        E.leaf_status[g] = (int8_t)status;
        if (EC) {
            if (!BACKUP || ec_claim != ec_prev) E.ec_claim[g] = ec_claim;  // beyond the opening both are -1: no store
            if (ec_hit >= 0) atomicAdd(&E.ec_hits[g], 1);  // the slot's own word: no return value, no round trip
        }
    }
    PSTAMP(6)
#ifdef AZ_PROBE
    if (BACKUP && SELECT && sim == 50 && (threadIdx.x & 63) == 0 && blockIdx.x < 1024) {  // az_step_probe holds 1024 blocks x 4 waves
        unsigned long long *o = az_step_probe + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
        for (int i = 0; i < 7; ++i) o[i] = pt[i];
        o[7] = (unsigned long long)(wk.plen - 1);
    }
#endif
}

// the plain search's lock-step, under the name and with the code it always had, and the playout cap's
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step(EngDev E, int sim, int g0, int g1) { step_grp<BACKUP, SELECT, false, false>(E, sim, g0, g1); }
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_cap(EngDev E, int sim, int g0, int g1) { step_grp<BACKUP, SELECT, true, false>(E, sim, g0, g1); }
// and the two of az_engine_set_forced_playouts: the same lock-steps with the forced root selection, without and with the playout cap
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_forced(EngDev E, int sim, int g0, int g1) { step_grp<BACKUP, SELECT, false, true>(E, sim, g0, g1); }
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_cap_forced(EngDev E, int sim, int g0, int g1) { step_grp<BACKUP, SELECT, true, true>(E, sim, g0, g1); }
// and any of the four with the leaf evaluation cache in force (az_engine_set_eval_cache): launched only where E.ec_hdr is set, so the
// kernels above stay the code they were for every search that does not cache
template <bool BACKUP, bool SELECT, bool CAP, bool FORCED>
__global__ __launch_bounds__(256) void k_step_cached(EngDev E, int sim, int g0, int g1) { step_grp<BACKUP, SELECT, CAP, FORCED, true>(E, sim, g0, g1); }
// and the plain one-leaf lock-step with the heads computed inside, without the cache and with it: the two forms
// that hold a backup -- a ply's first step has none and stays k_step / k_step_cached.  NT: the tiles of the padded logits (5: 80, 3: 48)
template <bool SELECT, bool EC, int NT>
__global__ __launch_bounds__(256) void k_step_heads(EngDev E, int sim, int g0, int g1) { step_grp<true, SELECT, false, false, EC, false, false, false, NT>(E, sim, g0, g1); }
// and the plain lock-step with exact endgames (az_engine_set_exact_endgame), without and with the cache: the solver's frames, three u64
// per frame and lane, are the block's LDS (60 KiB: one block per CU's share of 64 KiB)
#define EXACT_STK_WORDS (AZ_EXACT_MAX_EMPTIES * AZ_SOLVE_FRAME_WORDS * 256)
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_exact(EngDev E, int sim, int g0, int g1) {
    __shared__ u64 s_xstk[EXACT_STK_WORDS];
    step_grp<BACKUP, SELECT, false, false, false, true>(E, sim, g0, g1, s_xstk);
}
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_exact_cached(EngDev E, int sim, int g0, int g1) {
    __shared__ u64 s_xstk[EXACT_STK_WORDS];
    step_grp<BACKUP, SELECT, false, false, true, true>(E, sim, g0, g1, s_xstk);
}

// and the plain lock-step with proof backup (az_engine_set_proof_backup), alone, with the cache, with exact endgames, with both: the
// exact ones carry the solver's LDS as k_step_exact does
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_proof(EngDev E, int sim, int g0, int g1) {
    step_grp<BACKUP, SELECT, false, false, false, false, true>(E, sim, g0, g1);
}
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_proof_cached(EngDev E, int sim, int g0, int g1) {
    step_grp<BACKUP, SELECT, false, false, true, false, true>(E, sim, g0, g1);
}
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_proof_exact(EngDev E, int sim, int g0, int g1) {
    __shared__ u64 s_xstk[EXACT_STK_WORDS];
    step_grp<BACKUP, SELECT, false, false, false, true, true>(E, sim, g0, g1, s_xstk);
}
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_proof_exact_cached(EngDev E, int sim, int g0, int g1) {
    __shared__ u64 s_xstk[EXACT_STK_WORDS];
    step_grp<BACKUP, SELECT, false, false, true, true, true>(E, sim, g0, g1, s_xstk);
}

// and the plain lock-step under exploration settings other than (1.0, 0, off) (az_engine_set_puct), without and with the cache
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_puct(EngDev E, int sim, int g0, int g1) {
    step_grp<BACKUP, SELECT, false, false, false, false, false, true>(E, sim, g0, g1);
}
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_puct_cached(EngDev E, int sim, int g0, int g1) {
    step_grp<BACKUP, SELECT, false, false, true, false, false, true>(E, sim, g0, g1);
}

// One lock-step of K walkers per slot: BACKUP of the kb walkers the previous lock-step selected (their rows are evaluated), then
// SELECT of kt walkers.  Lane j of the game's group owns walker j's pending words (loaded / stored coalesced, handed round by
// shuffle); the walkers themselves run one after the other on all 16 lanes, as a simulation of k_step does.
template <bool BACKUP, bool SELECT>
__global__ __launch_bounds__(256) void k_step_multi(EngDev E, int t, int kb, int kt) {
    const int g = blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) { E.batch_cnt[(t + 1) & 1] = 0; if (!SELECT) E.batch_cnt[2] = 0; }
    // groups beyond the last slot stay as inert groups: every __syncthreads() below is reached by every wave once (see k_step)
    const bool in_range = g < E.G;
    const int gs = in_range ? g : E.G - 1;
    Node *pool = pool_of(E, gs);
    const size_t wj = (size_t)gs * MLB + sub;  // this lane's walker
    // ---- every per-slot and per-walker word in one batch of independent loads
    const int p_st = (BACKUP && in_range && sub < kb) ? E.m_leaf_status[wj] : LS_NONE;
    const int p_leaf = BACKUP ? E.m_leaf[wj] : 0;
    const u64 p_p1 = BACKUP ? E.m_leaf_p1[wj] : 0, p_m1 = BACKUP ? E.m_leaf_m1[wj] : 0;
    const int p_pl = BACKUP ? E.m_leaf_player[wj] : 1, p_win = BACKUP ? E.m_leaf_winner[wj] : 0;
    const int p_row = BACKUP ? E.m_row[wj] : 0, p_plen = BACKUP ? E.m_path_len[wj] : 0;
    int path_cur = (BACKUP && kb > 0) ? E.m_path[(size_t)gs * MLB * LPG + sub] : 0;
    int n_nodes = E.n_nodes[gs];
    int evals = E.evals[gs];
    bool active = in_range && searches(E, gs);
    const int ply = E.ply[gs];
    const BB rb = {E.root_p1[gs], E.root_m1[gs], E.root_player[gs]};
    const int root = E.root[gs];
    if (BACKUP) {
        double p_out = 0.0;  // lane j: the outcome walker j propagated (a duplicate of j propagates it again)
        bool dead = false;
        for (int j = 0; j < kb; ++j) {
            // the next walker's path indices travel while this one is backed up
            const int path_next = (j + 1 < kb) ? E.m_path[((size_t)gs * MLB + j + 1) * LPG + sub] : 0;
            const int st = __shfl(p_st, j, LPG);
            if (st != LS_NONE && !dead) {
                const int leaf = __shfl(p_leaf, j, LPG), plen = __shfl(p_plen, j, LPG);
                const BB lb = {(u64)__shfl((long long)p_p1, j, LPG), (u64)__shfl((long long)p_m1, j, LPG), __shfl(p_pl, j, LPG)};
                Node mine;
                const bool on_path = plen <= LPG && sub < plen;
                if (on_path) mine = load_node(pool + path_cur);
                double outcome;
                bool ok = true;
                if (st == LS_EVAL) {
                    const int row = __shfl(p_row, j, LPG);
                    const float v = E.value[row];
                    int k = create_children_grp(E, g, pool, n_nodes, leaf, lb, E.probs + (size_t)row * E.A, sub);
                    ok = k > 0;
                    n_nodes += ok ? k : 0;
                    outcome = (double)lb.player * (double)v;  // base.py:366
                    if (ok) evals += 1;
                    if (sub == j) p_out = outcome;
                } else if (st >= LS_DUP) {
                    outcome = __shfl(p_out, st - LS_DUP, LPG);
                } else {
                    outcome = (double)__shfl(p_win, j, LPG);
                }
                if (ok) back_propagate_grp(pool, plen, path_cur, mine, leaf, lb.player, outcome, sub);
                else { dead = true; active = false; if (sub == 0) E.active[g] = 0; }
                // this walker's stores (other lanes) must be visible to the next walker's loads
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            }
            path_cur = path_next;
        }
        if (sub == 0 && in_range) E.evals[g] = evals;
        if (!SELECT && in_range) E.m_leaf_status[wj] = LS_NONE;
    }
    if (!SELECT) return;
    // From here on no group may leave early: all walks first, then the rows of the whole block (alloc_rows_block: one LDS count of the
    // LS_EVAL walkers, one global atomic).  No barrier inside the walker loop.
    int k_st = LS_NONE, k_leaf = 0, k_pl = 1, k_w = 0, k_plen = 0;  // lane j: walker j's pending leaf
    u64 k_p1 = 0, k_m1 = 0;
    int vpath[MLB];  // vpath[i]: the sub-th node of walker i's path (-1: none)
#pragma unroll
    for (int i = 0; i < MLB; ++i) vpath[i] = -1;
    if (active) {
        Node rootn = load_node(pool + root);
        int ndup = 0;
        for (int j = 0; j < kt; ++j) {
            const int sim = t * E.K + j;
            Walk wk = {rb, rootn, root, 1, sub == 0 ? root : -1, false};
            if (E.noise_mode != AZ_NOISE_OFF && E.alpha >= 0.0 && E.eps >= 0.0 && (wk.cur.flags & F_EXPANDED) && !(wk.cur.flags & F_NOISED)) {
                apply_root_noise_grp(E, g, pool, root, wk.cur, rb, ply, sim, sub);
                wk.cur.flags |= F_NOISED;
                rootn.flags = wk.cur.flags;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            }
            walk_grp(E, g, pool, vpath, j, ply, sim, sub, wk);
            if (wk.plen > 1) rootn.flags |= F_EXPANDED;  // a walk that left the root found or made its children visible
            E.m_path[((size_t)g * MLB + j) * LPG + sub] = wk.my_path;
#pragma unroll
            for (int i = 0; i < MLB; ++i) vpath[i] = i == j ? wk.my_path : vpath[i];
            if (wk.plen > LPG && sub == 0) atomicMax(E.max_path, wk.plen);
            int w = 0;
            int status = classify_leaf_grp(E, pool, wk, w, sub);
            if (status == LS_EVAL) {
                const u32 m = grp_ballot(sub < j && k_st == LS_EVAL && k_leaf == wk.node);  // pending leaf of an earlier walker?
                if (m) { status = LS_DUP + (__ffs((int)m) - 1); ++ndup; }
            }
            if (sub == j) { k_st = status; k_leaf = wk.node; k_p1 = wk.b.p1; k_m1 = wk.b.m1; k_pl = wk.b.player; k_w = w; k_plen = wk.plen; }
            // flag stores of this walker (F_EXPANDED, F_TERMINAL, the noised priors) must be visible to the next walker's loads
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
        if (ndup > 0 && sub == 0) atomicAdd(&E.ctr[CTR_COLLISIONS], (unsigned long long)ndup);
    }
    const int k_row = alloc_rows_block(E.batch_cnt + (t & 1), k_st == LS_EVAL);  // < K * G: at most one row per walker
    for (int j = 0; j < kt; ++j) {
        if (__shfl(k_st, j, LPG) == LS_EVAL) {
            const BB bj = {(u64)__shfl((long long)k_p1, j, LPG), (u64)__shfl((long long)k_m1, j, LPG), __shfl(k_pl, j, LPG)};
            write_nn_input_grp(E, __shfl(k_row, j, LPG), bj, sub);
        }
    }
    if (in_range) {
        E.m_leaf_status[wj] = (int8_t)k_st;
        if (k_st != LS_NONE) {
            E.m_leaf[wj] = k_leaf; E.m_leaf_p1[wj] = k_p1; E.m_leaf_m1[wj] = k_m1; E.m_leaf_player[wj] = (int8_t)k_pl;
            E.m_leaf_winner[wj] = (int8_t)k_w; E.m_row[wj] = k_row; E.m_path_len[wj] = k_plen;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Gumbel root search (az_engine_set_gumbel; "Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022): the root
// samples gm actions without replacement by Gumbel noise, deals the simulations of a search over them by Sequential Halving and
// is read out as the policy improved by the completed Q-values.  A different search from the reference's: opt-in, default off.
// Contract.  The root has children 0 .. nch - 1; float64, one operation at a time:
//   logit(a) = az_det_log(P(a))                                                  (-inf for P = 0)
//   g(a)     = gumbel_scale == 0 ? 0.0 (no draw) : gumbel_scale * (-az_det_log(-az_det_log(u))),
//              r = az_philox(seed, game_id, ply, 0xFFFF, AZ_P_GUMBEL, action(a)), u = az_u53(r.x, r.y), 2^-53 where that is 0:
//              one draw per (game, ply, action), the same in every phase and search call, no function of slot, row or batch
//   vmix     = (sum over N(b) > 0 of P(b) Q(b)) / (sum over N(b) > 0 of P(b)), child-index order; 0.0 when the divisor is 0
//   cq(a)    = N(a) > 0 ? Q(a) : vmix            maxN = max N(b)
//   sigma(a) = ((c_visit + (double)maxN) * c_scale) * cq(a)
//   score(a) = (g(a) + logit(a)) + sigma(a)
// Schedule of a search call of n simulations, m0 = min(gm, nch): m0 = 1 sends all to child 0; otherwise L = ceil(log2 m0), phase p
// considers m_p candidates (m_0 = m0, m_{p+1} = max(2, m_p / 2)) for v_p = max(1, n / (L m_p)) rounds, phases follow each other
// until n simulations are dealt (the phase of 2 repeats, the last one is cut).  At the first simulation of a phase the candidates
// become the m_p best by score of the previous set (phase 0: of all children), ties to the lowest index whatever tie_mode says;
// simulation i of a phase takes the (i mod m_p)-th candidate in ascending child index.  Below the root: the plain PUCT walk.
// No root noise.  Move = the best score among the slot's candidates on the final statistics; policy target = softmax(logit + sigma).
// ---------------------------------------------------------------------------------------------
#define AZ_P_GUMBEL 9

AZ_D double gumbel_g(const EngDev &E, u32 gid, int ply, int action) {
    if (E.g_scale == 0.0) return 0.0;
    const Philox4 r = az_philox(E.seed, gid, (u32)ply, 0xFFFFu, AZ_P_GUMBEL, (u32)action);
    double u = az_u53(r.x, r.y);
    if (u == 0.0) u = 1.0 / 9007199254740992.0;
    return E.g_scale * (-az_det_log(-az_det_log(u)));
}

// where simulation s of a search of n stands in the schedule: phase p of m_p candidates, i = its index inside the phase
AZ_D void gumbel_phase(int s, int n, int m0, int &p, int &mp, int &i) {
    p = 0; mp = m0; i = s;
    if (m0 <= 1) return;
    const int L = 32 - __clz(m0 - 1);  // ceil(log2 m0)
    int start = 0;
    for (;;) {
        int v = n / (L * mp);
        v = v < 1 ? 1 : v;
        if (s < start + mp * v) break;
        start += mp * v;
        mp = mp / 2 < 2 ? 2 : mp / 2;
        ++p;
    }
    i = s - start;
}

// The paper's v_mix of a node (az_engine_set_gumbel_full): vhat = the network value stored for the node, sumN = the
// sum of its children's real counts, num / den = the sums over its visited children of the contract above.
AZ_D double gumbel_vmix_full(double vhat, int sumN, double num, double den) {
    if (sumN == 0 || !(den > 0.0)) return vhat;
    const double wq = num / den;
    return (vhat + (double)sumN * wq) / (double)(1 + sumN);
}

AZ_D int kth_set_bit64(u64 mask, int k) {
    for (int i = 0; i < k; ++i) mask &= mask - 1;
    return mask ? __ffsll((long long)mask) - 1 : -1;
}
AZ_D u64 first_bits64(int n) { return n >= 64 ? ~0ULL : (1ULL << n) - 1ULL; }

// The mp best by score among the children `prev` of the root, one lane per child and round: N / Q / P [r] are child r * LPG + sub
// (absent: N = 0, P = 0).  At most 16 rounds of one group maximum each; a NaN score is an error (it equals no maximum).
// FULL (az_engine_set_gumbel_full): vmix is the paper's, with vhat = the root's stored network value.
template <bool FULL>
AZ_D u64 gumbel_rerank_grp(const EngDev &E, const int (&N)[4], const double (&Q)[4], const double (&P)[4], const uint8_t (&act)[4],
                           int nch, u64 prev, int mp, u32 gid, int ply, double vhat, int sub) {
    double pq[4], pp[4];
    int mx = 0, sn = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool vis = N[r] > 0;
        pq[r] = vis ? P[r] * Q[r] : 0.0;
        pp[r] = vis ? P[r] : 0.0;
        mx = N[r] > mx ? N[r] : mx;
        sn += N[r];
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) { const int o = __shfl_xor(mx, m, LPG); mx = o > mx ? o : mx; }
    if (FULL) {
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) sn += __shfl_xor(sn, m, LPG);
    }
    double num = 0.0, den = 0.0;  // sequential sums in child-index order (an unvisited child adds an exact 0.0)
    for (int i = 0; i < nch; ++i) {
        num += __shfl(sel4(pq, i >> 4), i & 15, LPG);
        den += __shfl(sel4(pp, i >> 4), i & 15, LPG);
    }
    const double vmix = FULL ? gumbel_vmix_full(vhat, sn, num, den) : (den > 0.0 ? num / den : 0.0);
    const double k = (E.g_cvisit + (double)mx) * E.g_cscale;
    double sc[4];
    bool nan = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc[r] = -__builtin_inf();
        if ((prev >> (r * LPG + sub)) & 1ULL) {
            sc[r] = (gumbel_g(E, gid, ply, act[r]) + az_det_log(P[r])) + k * (N[r] > 0 ? Q[r] : vmix);
            nan |= sc[r] != sc[r];
        }
    }
    if (grp_ballot(nan) != 0 && sub == 0) atomicOr(E.err, ERR_INTERNAL);
    u64 avail = prev, sel = 0;
    for (int t = 0; t < mp; ++t) {
        double mine = -__builtin_inf();
#pragma unroll
        for (int r = 0; r < 4; ++r) if ((avail >> (r * LPG + sub)) & 1ULL) mine = fmax(mine, sc[r]);
        const double best = grp_max(mine);
        int idx = -1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const u32 b = grp_ballot(((avail >> (r * LPG + sub)) & 1ULL) && sc[r] == best);
            if (idx < 0 && b) idx = r * LPG + __ffs((int)b) - 1;
        }
        if (idx < 0) break;  // nothing left that compares: NaN scores, reported above
        sel |= 1ULL << idx;
        avail &= ~(1ULL << idx);
    }
    return sel;
}

// The deterministic non-root selection of the paper (az_engine_set_gumbel_full) for walker j at parent p, depth >= 1.
// v(b) = the virtual count of child b (the walkers i < j of this lock-step whose recorded path holds b, pick_child_vl_grp's), vsum
// their sum; sumN, maxN, vmix(p) and pi' on the real counts only; float64, one operation at a time, sums in child-index order:
//   k      = (c_visit + (double)maxN) * c_scale          cq(b) = N(b) > 0 ? Q(b) : vmix(p)
//   x(b)   = az_det_log(P(b)) + k * cq(b)                e(b)  = az_det_exp(x(b) - max x)       pi'(b) = e(b) / sum e
//   key(b) = pi'(b) - (double)(N(b) + v(b)) / (double)(1 + sumN + vsum)
// The child is the maximum of key, the lowest index among equals whatever tie_mode says (no Philox draw); NaN keys are an error.
AZ_D int pick_child_gumbel_grp(const EngDev &E, int g, const Node *pool, const Node &parent, int pnode, const int (&vpath)[MLB], int j,
                               int ply, int sim, int depth, int sub, Node &chosen) {
    const int fc = parent.first, nch = parent.nch;
    int vc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < MLB; ++i) {
        if (i < j) {  // uniform over the group
            const int cd = depth + 1 < LPG ? __shfl(vpath[i], (depth + 1) & (LPG - 1), LPG) : -1;
#pragma unroll
            for (int r = 0; r < 4; ++r) vc[r] += cd == fc + r * LPG + sub ? 1 : 0;
        }
    }
    Scored s;
    double cQ[4], cP[4], pq[4], pp[4];
    int mx = 0, sn = 0, sv = 0;
    const float vhat = nval_of(E, pool)[pnode];  // one address for the group: a broadcast, in flight with the children
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        Node c;
        cQ[r] = 0.0; cP[r] = 0.0;
        if (load_child_grp(pool, parent, r, sub, s, c)) { cQ[r] = c.Q; cP[r] = c.P; }
        const bool vis = s.N[r] > 0;
        pq[r] = vis ? cP[r] * cQ[r] : 0.0;
        pp[r] = vis ? cP[r] : 0.0;
        mx = s.N[r] > mx ? s.N[r] : mx;
        sn += s.N[r];
        sv += r * LPG + sub < nch ? vc[r] : 0;  // a lane without a child may have matched a neighbouring block's node
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        const int o = __shfl_xor(mx, m, LPG);
        mx = o > mx ? o : mx;
        sn += __shfl_xor(sn, m, LPG);
        sv += __shfl_xor(sv, m, LPG);
    }
    double num = 0.0, den = 0.0;  // sequential sums in child-index order (an unvisited child adds an exact 0.0)
    for (int i = 0; i < nch; ++i) {
        num += __shfl(sel4(pq, i >> 4), i & 15, LPG);
        den += __shfl(sel4(pp, i >> 4), i & 15, LPG);
    }
    const double vmix = gumbel_vmix_full((double)vhat, sn, num, den);
    const double k = (E.g_cvisit + (double)mx) * E.g_cscale;
    double x[4], xm = -__builtin_inf();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        x[r] = -__builtin_inf();
        if (r * LPG + sub < nch) x[r] = az_det_log(cP[r]) + k * (s.N[r] > 0 ? cQ[r] : vmix);
        xm = fmax(xm, x[r]);
    }
    xm = grp_max(xm);
    double ex[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ex[r] = r * LPG + sub < nch ? az_det_exp(x[r] - xm) : 0.0;
    double sum = 0.0;
    for (int i = 0; i < nch; ++i) sum += __shfl(sel4(ex, i >> 4), i & 15, LPG);
    const double tot = (double)(1 + sn + sv);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r * LPG + sub < nch) s.key[r] = ex[r] / sum - (double)(s.N[r] + vc[r]) / tot;
    // every lane votes, and NaN keys (a diverged network) are an error: no key equals the maximum
    const u32 no_draw = 0;
    return fc + choose_max_grp<false>(E, no_draw, ply, sim, depth, s, 4 * LPG, ERR_INTERNAL, sub, chosen);
}

// One lock-step of the search in the Gumbel mode: k_step with the root's child taken from the Sequential Halving schedule instead
// of pick_child_vl_grp and without root noise.  BACKUP and everything from the root's child downwards are k_step's.
// FULL (az_engine_set_gumbel_full): an evaluated leaf keeps its network value, the re-ranking takes the paper's v_mix, and below the
// root the child is pick_child_gumbel_grp's.
template <bool BACKUP, bool SELECT, bool FULL>
__global__ __launch_bounds__(256) void k_step_gumbel(EngDev E, int sim, int n_sim, int g0, int g1) {
    const int g = g0 + blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0 && g0 == 0) { E.batch_cnt[(sim + 1) & 1] = 0; if (!SELECT) E.batch_cnt[2] = 0; }
    // inert groups beyond the last slot stay in the kernel: every barrier below is reached once by every wave (see k_step)
    const bool in_range = g < g1;
    const int gs = in_range ? g : g1 - 1;
    Node *pool = pool_of(E, gs);
    const int st = (BACKUP && in_range) ? E.leaf_status[gs] : LS_NONE;
    const int leaf = BACKUP ? E.leaf[gs] : 0;
    const BB lb = {BACKUP ? E.leaf_p1[gs] : 0, BACKUP ? E.leaf_m1[gs] : 0, BACKUP ? E.leaf_player[gs] : 1};
    const int row_prev = BACKUP ? E.row_of_slot[gs] : 0;
    const int plen_prev = BACKUP ? E.path_len[gs] : 0;
    const int path_prev = BACKUP ? E.path[(size_t)gs * LPG + sub] : 0;
    const int lwin = BACKUP ? E.leaf_winner[gs] : 0;
    int n_nodes = E.n_nodes[gs];
    int evals = E.evals[gs];
    bool active = in_range && searches(E, gs);
    const int ply = E.ply[gs];
    BB b = {E.root_p1[gs], E.root_m1[gs], E.root_player[gs]};
    int node = E.root[gs];
    u64 mask = SELECT ? E.gmask[gs] : 0;
    const u32 gid = E.game_id[gs];
    Node fwd;
    bool have_root = false;
    if (BACKUP && st != LS_NONE) {
        Node mine;
        const bool on_path = plen_prev <= LPG && sub < plen_prev;
        if (on_path) mine = load_node(pool + path_prev);
        double outcome;
        bool ok = true;
        if (st == LS_EVAL) {
            const float v = E.value[row_prev];
            int k = create_children_grp(E, g, pool, n_nodes, leaf, lb, E.probs + (size_t)row_prev * E.A, sub);
            ok = k > 0;
            n_nodes += ok ? k : 0;
            outcome = (double)lb.player * (double)v;  // base.py:366
            if (FULL && ok && sub == 0) nval_of(E, pool)[leaf] = v;
            if (ok) evals += 1;
            else { active = false; if (sub == 0) E.active[g] = 0; }
        } else {
            outcome = (double)lwin;
        }
        if (ok) {
            bool fast = back_propagate_grp(pool, plen_prev, path_prev, mine, leaf, lb.player, outcome, sub);
            if (fast && SELECT) {  // lane 0 holds the root (path[0]) with its new visit count: forward it
                fwd.N = __shfl(mine.N, 0, LPG);
                fwd.first = __shfl(mine.first, 0, LPG);
                set_node_tail(fwd, (u32)__shfl((int)node_tail(mine), 0, LPG));
                fwd.Q = 0.0; fwd.P = 0.0; fwd.parent = -1;
                have_root = (leaf != node) || st != LS_EVAL;
            }
        }
        if (sub == 0) E.leaf_status[g] = LS_NONE;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if (BACKUP && sub == 0 && in_range) E.evals[g] = evals;
    if (!SELECT) return;
    // From here on no group may leave early: the leaf rows are handed out per block (alloc_rows_block) behind workgroup barriers.
    int status = LS_NONE, w = 0;
    Walk wk = {b, Node(), node, 1, sub == 0 ? node : -1, false};
    if (active) {
        if (have_root) wk.cur = fwd; else wk.cur = load_node(pool + node);
        const float vroot = FULL ? nval_of(E, pool)[node] : 0.0f;  // in flight with the root; read where a phase starts
        // the root's step of select_node (walk_grp's first turn) with the scheduled child
        bool fresh = false, stop = false;
        if (!(wk.cur.flags & F_EXPANDED)) {
            if (wk.cur.flags & F_TERMINAL) stop = true;
            else if (!(wk.cur.flags & F_EVALUATED)) { wk.bad = true; stop = true; }
            else {
                wk.cur.flags |= F_EXPANDED;
                if (sub == 0) pool[wk.node].flags = wk.cur.flags;
                fresh = true;
            }
        }
        if (!stop && wk.cur.nch == 0) { wk.bad = true; stop = true; }  // an expanded node always has children
        if (!stop) {
            const int nch = wk.cur.nch;
            int p, mp, i;
            gumbel_phase(sim, n_sim, nch < E.gm ? nch : E.gm, p, mp, i);
            Scored s;
            double cQ[4], cP[4];
            uint8_t cact[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Node c;
                cQ[r] = 0.0; cP[r] = 0.0; cact[r] = 0;
                if (load_child_grp(pool, wk.cur, r, sub, s, c)) { cQ[r] = c.Q; cP[r] = c.P; cact[r] = c.act; }
            }
            const u64 all = first_bits64(nch);
            if (i == 0) {  // a phase starts: the candidates are ranked again
                mask = mp == 1 ? 1ULL : gumbel_rerank_grp<FULL>(E, s.N, cQ, cP, cact, nch, p == 0 ? all : (mask & all), mp, gid, ply, (double)vroot, sub);
                if (sub == 0) E.gmask[g] = mask;
            }
            int c = kth_set_bit64(mask & all, i % mp);
            if (c < 0) { c = 0; if (sub == 0) atomicOr(E.err, ERR_INTERNAL); }
            const int rsel = c >> 4, lsel = c & (LPG - 1);
            Node ch;  // the chosen child's header, from the lane that loaded it
            ch.N = __shfl(pick4(s.N[0], s.N[1], s.N[2], s.N[3], rsel), lsel, LPG);
            ch.first = __shfl(pick4(s.first[0], s.first[1], s.first[2], s.first[3], rsel), lsel, LPG);
            set_node_tail(ch, (u32)__shfl(pick4((int)s.tail[0], (int)s.tail[1], (int)s.tail[2], (int)s.tail[3], rsel), lsel, LPG));
            ch.Q = 0.0; ch.P = 0.0; ch.parent = 0;
            wk.node = wk.cur.first + c; wk.cur = ch;
            if (sub == wk.plen) wk.my_path = wk.node;
            ++wk.plen;
            az_play_grp(E.gd, wk.b, wk.cur.act, sub);
            if (!(fresh || wk.cur.N == 0)) {
                const int no_walkers[MLB] = {};
                walk_grp<FULL>(E, g, pool, no_walkers, 0, ply, sim, sub, wk);
            }
        }
        E.path[(size_t)g * LPG + sub] = wk.my_path;
        if (sub == 0) { E.path_len[g] = wk.plen; if (wk.plen > LPG) atomicMax(E.max_path, wk.plen); }
        status = classify_leaf_grp(E, pool, wk, w, sub);
    }
    const int row = __shfl(alloc_rows_block(E.batch_cnt + (sim & 1), status == LS_EVAL && sub == 0), 0, LPG);
    if (status == LS_EVAL) {
        write_nn_input_grp(E, row, wk.b, sub);
        if (sub == 0) E.row_of_slot[g] = row;
    }
    if (sub == 0 && in_range) {
        if (active) {
            E.leaf[g] = wk.node; E.leaf_p1[g] = wk.b.p1; E.leaf_m1[g] = wk.b.m1; E.leaf_player[g] = (int8_t)wk.b.player;
            E.leaf_winner[g] = (int8_t)w;
        }
        E.leaf_status[g] = (int8_t)status;
    }
}

// where the phase that holds simulation s of a search of n ends (first simulation of the next phase, at most n): gumbel_phase's walk
AZ_D int gumbel_phase_end(int s, int n, int m0) {
    if (m0 <= 1) return n;
    const int L = 32 - __clz(m0 - 1);
    int start = 0, mp = m0;
    for (;;) {
        int v = n / (L * mp);
        v = v < 1 ? 1 : v;
        start += mp * v;
        if (s < start) break;
        mp = mp / 2 < 2 ? 2 : mp / 2;
    }
    return start < n ? start : n;
}

// Several Sequential Halving leaves per network call (az_engine_set_gumbel_batch(K > 1) while the Gumbel mode is on; DESIGN
// section 17).  Everything not named here is the contract above k_step_gumbel.  The schedule depends on m0 = min(gm, nch) and that
// differs from slot to slot, so every searching slot keeps a cursor s = the simulations of this search call already dealt:
//   the search's first launch sets s = 0; a lock-step of the slot runs kt = min(K, end of the current phase - s, n - s) walkers
//   j = 0 .. kt - 1, walker j is simulation s + j (+ sim_base in every Philox counter), then s += kt.  No lock-step crosses a
//   phase boundary: a re-ranking (i == 0) can only fall on walker 0 and sees real statistics only, every earlier walker being
//   backed up.  A root without children, and m0 = 1, take the one phase of n: child 0, ceil(n / K) lock-steps.
//   The host enqueues Lmax(n, gm, K) = the longest plan of any m0 in 1 .. gm lock-steps (+ the backup-only launch); a slot whose
//   plan is shorter idles in the rest: kt = 0, LS_NONE for every walker, no rows.
//   The walkers of a lock-step run in ascending j, one after the other, as k_step_multi's.  Walker j makes k_step_gumbel's root
//   step -- first-visit expansion with the `fresh` break, child = the (i mod m_p)-th candidate, stop when fresh or the child's
//   real N == 0 -- with no virtual count (the pick is forced), then descends from depth 1 with pick_child_vl_grp's virtual counts
//   over the earlier walkers' recorded paths (the root's child is node 1 of a path).  Leaf status, duplicates (LS_DUP + i, counted
//   in collisions: with K > m_p several walkers share a root child and, while its real N is 0, its pending leaf), backup order,
//   the bump allocator's order and the fences are k_step_multi's.
// Every root grows by exactly n visits per search call; the result is a function of (seed, game id, gm, constants, K, n), never of
// the slot, the slot count or the block; K = 1 never comes here (k_step_gumbel).
// gcur [G] = the cursor, gstart [G] = its value at the start of the slot's current lock-step (k_sym_pick's simulation index and the
// number of walkers the next launch backs up: gcur - gstart).  Lane j of the group owns walker j's pending words, as in k_step_multi.
// FULL (az_engine_set_gumbel_full): as in k_step_gumbel; the virtual counts enter pick_child_gumbel_grp's subtracted term only.
template <bool BACKUP, bool SELECT, bool FULL>
__global__ __launch_bounds__(256) void k_step_gumbel_multi(EngDev E, int t, int n_sim) {
    const int g = blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) { E.batch_cnt[(t + 1) & 1] = 0; if (!SELECT) E.batch_cnt[2] = 0; }
    // groups beyond the last slot stay as inert groups: every __syncthreads() below is reached by every wave once (see k_step)
    const bool in_range = g < E.G;
    const int gs = in_range ? g : E.G - 1;
    Node *pool = pool_of(E, gs);
    const size_t wj = (size_t)gs * MLB + sub;  // this lane's walker
    // ---- every per-slot and per-walker word in one batch of independent loads
    const int cur = BACKUP ? E.gcur[gs] : 0;  // the search's first launch (no BACKUP) starts the cursor at 0
    int kb = BACKUP ? cur - E.gstart[gs] : 0;  // walkers the slot's previous lock-step selected
    kb = kb < 0 ? 0 : (kb > MLB ? MLB : kb);
    const int p_st = (BACKUP && in_range && sub < kb) ? E.m_leaf_status[wj] : LS_NONE;
    const int p_leaf = BACKUP ? E.m_leaf[wj] : 0;
    const u64 p_p1 = BACKUP ? E.m_leaf_p1[wj] : 0, p_m1 = BACKUP ? E.m_leaf_m1[wj] : 0;
    const int p_pl = BACKUP ? E.m_leaf_player[wj] : 1, p_win = BACKUP ? E.m_leaf_winner[wj] : 0;
    const int p_row = BACKUP ? E.m_row[wj] : 0, p_plen = BACKUP ? E.m_path_len[wj] : 0;
    int path_cur = (BACKUP && kb > 0) ? E.m_path[(size_t)gs * MLB * LPG + sub] : 0;
    int n_nodes = E.n_nodes[gs];
    int evals = E.evals[gs];
    bool active = in_range && searches(E, gs);
    const int ply = E.ply[gs];
    const BB rb = {E.root_p1[gs], E.root_m1[gs], E.root_player[gs]};
    const int root = E.root[gs];
    u64 mask = SELECT ? E.gmask[gs] : 0;
    const u32 gid = E.game_id[gs];
    if (BACKUP) {  // k_step_multi's, over the slot's own kb
        double p_out = 0.0;  // lane j: the outcome walker j propagated (a duplicate of j propagates it again)
        bool dead = false;
        for (int j = 0; j < kb; ++j) {
            const int path_next = (j + 1 < kb) ? E.m_path[((size_t)gs * MLB + j + 1) * LPG + sub] : 0;
            const int st = __shfl(p_st, j, LPG);
            if (st != LS_NONE && !dead) {
                const int leaf = __shfl(p_leaf, j, LPG), plen = __shfl(p_plen, j, LPG);
                const BB lb = {(u64)__shfl((long long)p_p1, j, LPG), (u64)__shfl((long long)p_m1, j, LPG), __shfl(p_pl, j, LPG)};
                Node mine;
                const bool on_path = plen <= LPG && sub < plen;
                if (on_path) mine = load_node(pool + path_cur);
                double outcome;
                bool ok = true;
                if (st == LS_EVAL) {
                    const int row = __shfl(p_row, j, LPG);
                    const float v = E.value[row];
                    int k = create_children_grp(E, g, pool, n_nodes, leaf, lb, E.probs + (size_t)row * E.A, sub);
                    ok = k > 0;
                    n_nodes += ok ? k : 0;
                    outcome = (double)lb.player * (double)v;  // base.py:366
                    if (FULL && ok && sub == 0) nval_of(E, pool)[leaf] = v;
                    if (ok) evals += 1;
                    if (sub == j) p_out = outcome;
                } else if (st >= LS_DUP) {
                    outcome = __shfl(p_out, st - LS_DUP, LPG);
                } else {
                    outcome = (double)__shfl(p_win, j, LPG);
                }
                if (ok) back_propagate_grp(pool, plen, path_cur, mine, leaf, lb.player, outcome, sub);
                else { dead = true; active = false; if (sub == 0) E.active[g] = 0; }
                // this walker's stores (other lanes) must be visible to the next walker's loads
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            }
            path_cur = path_next;
        }
        if (sub == 0 && in_range) E.evals[g] = evals;
        if (!SELECT && in_range) E.m_leaf_status[wj] = LS_NONE;
    }
    if (!SELECT) return;
    // From here on no group may leave early: all walks first, then the rows of the whole block (alloc_rows_block).  No barrier inside
    // the walker loop, whose length differs from group to group.
    int k_st = LS_NONE, k_leaf = 0, k_pl = 1, k_w = 0, k_plen = 0;  // lane j: walker j's pending leaf
    u64 k_p1 = 0, k_m1 = 0;
    int vpath[MLB];  // vpath[i]: the sub-th node of walker i's path (-1: none)
#pragma unroll
    for (int i = 0; i < MLB; ++i) vpath[i] = -1;
    int kt = 0;
    if (active && cur < n_sim) {
        Node rootn = load_node(pool + root);
        const float vroot = FULL ? nval_of(E, pool)[root] : 0.0f;  // in flight with the root; read where a phase starts
        // k_step_gumbel's tests at the root: the same for every walker of the lock-step but `fresh`, which only walker 0 can see
        const bool unexp = !(rootn.flags & F_EXPANDED);
        const bool root_term = unexp && (rootn.flags & F_TERMINAL);
        const bool root_bad = (unexp && !root_term && !(rootn.flags & F_EVALUATED)) || (!root_term && rootn.nch == 0);
        const bool stop = root_term || root_bad;
        const int nch = stop ? 0 : rootn.nch;
        const int m0 = nch < E.gm ? nch : E.gm;
        const int end = gumbel_phase_end(cur, n_sim, m0);
        kt = end - cur < E.K ? end - cur : E.K;
        int p = 0, mp = 1, i0 = 0;
        Scored s;
        if (!stop) {
            gumbel_phase(cur, n_sim, m0, p, mp, i0);
            double cQ[4], cP[4];
            uint8_t cact[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Node c;
                cQ[r] = 0.0; cP[r] = 0.0; cact[r] = 0;
                if (load_child_grp(pool, rootn, r, sub, s, c)) { cQ[r] = c.Q; cP[r] = c.P; cact[r] = c.act; }
            }
            if (i0 == 0) {  // a phase starts with walker 0: the candidates are ranked again, on real statistics
                const u64 all = first_bits64(nch);
                mask = mp == 1 ? 1ULL : gumbel_rerank_grp<FULL>(E, s.N, cQ, cP, cact, nch, p == 0 ? all : (mask & all), mp, gid, ply, (double)vroot, sub);
                if (sub == 0) E.gmask[g] = mask;
            }
            mask &= first_bits64(nch);
        }
        int ndup = 0;
        for (int j = 0; j < kt; ++j) {
            const int sim = cur + j;
            Walk wk = {rb, rootn, root, 1, sub == 0 ? root : -1, false};
            wk.bad = root_bad;
            if (!stop) {
                bool fresh = false;
                if (!(rootn.flags & F_EXPANDED)) {  // walker 0 of the root's first visit
                    rootn.flags |= F_EXPANDED;
                    if (sub == 0) pool[root].flags = rootn.flags;
                    fresh = true;
                }
                int c = kth_set_bit64(mask, (i0 + j) % mp);
                if (c < 0) { c = 0; if (sub == 0) atomicOr(E.err, ERR_INTERNAL); }
                const int rsel = c >> 4, lsel = c & (LPG - 1);
                Node ch;  // the chosen child's header, from the lane that loaded it
                ch.N = __shfl(pick4(s.N[0], s.N[1], s.N[2], s.N[3], rsel), lsel, LPG);
                ch.first = __shfl(pick4(s.first[0], s.first[1], s.first[2], s.first[3], rsel), lsel, LPG);
                set_node_tail(ch, (u32)__shfl(pick4((int)s.tail[0], (int)s.tail[1], (int)s.tail[2], (int)s.tail[3], rsel), lsel, LPG));
                ch.Q = 0.0; ch.P = 0.0; ch.parent = 0;
                wk.node = rootn.first + c;
                // an earlier walker of this lock-step went through the same child (K > m_p): its flag stores count, N is still the real one
                if (j >= mp) set_node_tail(ch, node_tail(load_node(pool + wk.node)));
                wk.cur = ch;
                if (sub == wk.plen) wk.my_path = wk.node;
                ++wk.plen;
                az_play_grp(E.gd, wk.b, wk.cur.act, sub);
                if (!(fresh || wk.cur.N == 0)) walk_grp<FULL>(E, g, pool, vpath, j, ply, sim, sub, wk);
            }
            E.m_path[((size_t)g * MLB + j) * LPG + sub] = wk.my_path;
#pragma unroll
            for (int i = 0; i < MLB; ++i) vpath[i] = i == j ? wk.my_path : vpath[i];
            if (wk.plen > LPG && sub == 0) atomicMax(E.max_path, wk.plen);
            int w = 0;
            int status = classify_leaf_grp(E, pool, wk, w, sub);
            if (status == LS_EVAL) {
                const u32 m = grp_ballot(sub < j && k_st == LS_EVAL && k_leaf == wk.node);  // pending leaf of an earlier walker?
                if (m) { status = LS_DUP + (__ffs((int)m) - 1); ++ndup; }
            }
            if (sub == j) { k_st = status; k_leaf = wk.node; k_p1 = wk.b.p1; k_m1 = wk.b.m1; k_pl = wk.b.player; k_w = w; k_plen = wk.plen; }
            // flag stores of this walker (F_EXPANDED, F_TERMINAL) must be visible to the next walker's loads
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
        if (ndup > 0 && sub == 0) atomicAdd(&E.ctr[CTR_COLLISIONS], (unsigned long long)ndup);
    }
    const int k_row = alloc_rows_block(E.batch_cnt + (t & 1), k_st == LS_EVAL);  // < K * G: at most one row per walker
    for (int j = 0; j < kt; ++j) {
        if (__shfl(k_st, j, LPG) == LS_EVAL) {
            const BB bj = {(u64)__shfl((long long)k_p1, j, LPG), (u64)__shfl((long long)k_m1, j, LPG), __shfl(k_pl, j, LPG)};
            write_nn_input_grp(E, __shfl(k_row, j, LPG), bj, sub);
        }
    }
    if (in_range) {
        E.m_leaf_status[wj] = (int8_t)k_st;
        if (k_st != LS_NONE) {
            E.m_leaf[wj] = k_leaf; E.m_leaf_p1[wj] = k_p1; E.m_leaf_m1[wj] = k_m1; E.m_leaf_player[wj] = (int8_t)k_pl;
            E.m_leaf_winner[wj] = (int8_t)k_w; E.m_row[wj] = k_row; E.m_path_len[wj] = k_plen;
        }
        if (sub == 0) { E.gstart[g] = cur; E.gcur[g] = cur + kt; }
    }
}

// ---------------------------------------------------------------------------------------------
// TreeEval.ROLLOUT (BASELINE config 1, the reference's default evaluation opponent): one whole simulation per
// launch -- UCT selection (mcts.py:38-42, 134-135), expansion with a uniformly random child (mcts.py:152-154,
// 163-165), random playout to the end of the game (mcts.py:173-180), back-propagation (mcts.py:197-223).
// np.log is restated by az_det_log (as in the CPU oracle).
// ---------------------------------------------------------------------------------------------
#define AZ_P_ROLLOUT_EXPAND 6
#define AZ_P_PLAYOUT 7

AZ_D int pick_child_uct_grp(const EngDev &E, u32 gid, const Node *pool, const Node &parent, int ply, int sim, int depth, int sub, Node &chosen) {
    const double lg = az_det_log((double)parent.N);
    Scored s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        Node c;
        if (load_child_grp(pool, parent, r, sub, s, c))
            s.key[r] = c.N == 0 ? __builtin_inf() : c.Q + 1.4142135623730951 * sqrt(lg / (double)c.N);
    }
    return parent.first + choose_max_grp(E, gid, ply, sim, depth, s, parent.nch, 0, sub, chosen);
}

__global__ __launch_bounds__(256) void k_rollout_step(EngDev E, int sim) {
    const int g = blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (g >= E.G || !searches(E, g)) return;
    const GameDesc &gd = E.gd;
    Node *pool = pool_of(E, g);
    const int ply = E.ply[g];
    const u32 gid = E.game_id[g];
    int n_nodes = E.n_nodes[g];
    BB b = {E.root_p1[g], E.root_m1[g], E.root_player[g]};
    int node = E.root[g];
    Node cur = load_node(pool + node);
    int depth = 0, plen = 1;
    int my_path = sub == 0 ? node : -1;
    bool reached_new = false;
    while (cur.flags & F_EXPANDED) {  // mcts.py:132-144
        Node ch;
        int c = pick_child_uct_grp(E, gid, pool, cur, ply, sim, depth++, sub, ch);
        node = c; cur = ch;
        if (sub == plen) my_path = c;
        ++plen;
        az_play_grp(gd, b, cur.act, sub);
        if (cur.N == 0) { reached_new = true; break; }
    }
    int w = 0;
    bool over = az_status_grp(gd, b, &w, sub);
    if (!reached_new && !over) {  // mcts.py:146-171 : expand with every legal move, step into a uniformly random child
        u64 bits = az_legal_bits_grp(gd, b, b.player, sub);
        const bool pass = (gd.game == AZ_OTHELLO && bits == 0);
        const int k = pass ? 1 : __popcll(bits);
        if (n_nodes + k > E.C) { if (sub == 0) { atomicOr(E.err, ERR_NODE_POOL); E.active[g] = 0; } return; }
        const int fc = n_nodes;
        if (pass) { if (sub == 0) store_node(pool + fc, fresh_node(gd.A - 1, node, 0.0, 0)); }
        else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int bit = r * LPG + sub;
                if ((bits >> bit) & 1ULL) store_node(pool + fc + __popcll(bits & ((1ULL << bit) - 1ULL)), fresh_node(az_bit_to_action(gd, bit), node, 0.0, 0));
            }
        }
        n_nodes += k;
        if (sub == 0) { pool[node].first = fc; pool[node].nch = (uint8_t)k; pool[node].flags = cur.flags | F_EXPANDED; E.n_nodes[g] = n_nodes; }
        Philox4 rr = az_philox(E.seed, gid, (u32)ply, (u32)sim + E.sim_base, AZ_P_ROLLOUT_EXPAND, (u32)depth);
        const int pick = (int)(((u64)rr.x * (u64)k) >> 32);
        int act;
        if (pass) act = gd.A - 1;
        else { u64 m = bits; for (int i = 0; i < pick; ++i) m &= m - 1; act = az_bit_to_action(gd, __ffsll((long long)m) - 1); }
        node = fc + pick;
        if (sub == plen) my_path = node;
        ++plen;
        az_play_grp(gd, b, act, sub);
        over = az_status_grp(gd, b, &w, sub);
    }
    const int player_to_play = b.player;  // mcts.py:243 : side to move at the selected node
    for (u32 step = 0; !over; ++step) {    // mcts.py:173-180 : uniformly random playout
        u64 bits = az_legal_bits_grp(gd, b, b.player, sub);
        int act;
        if (gd.game == AZ_OTHELLO && bits == 0) act = gd.A - 1;
        else {
            const int k = __popcll(bits);
            Philox4 rr = az_philox(E.seed, gid, (u32)ply, (u32)sim + E.sim_base, AZ_P_PLAYOUT, step);
            const int pick = (int)(((u64)rr.x * (u64)k) >> 32);
            u64 m = bits;
            for (int i = 0; i < pick; ++i) m &= m - 1;
            act = az_bit_to_action(gd, __ffsll((long long)m) - 1);
        }
        az_play_grp(gd, b, act, sub);
        over = az_status_grp(gd, b, &w, sub);
    }
    // back_propagate along the recorded path
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (plen > LPG && sub == 0) atomicMax(E.max_path, plen);
    Node mine;
    if (plen <= LPG && sub < plen) mine = load_node(pool + my_path);
    back_propagate_grp(pool, plen, my_path, mine, node, player_to_play, (double)w, sub);
}

AZ_D double linear_temp(int step, int tmax, int tmin) {  // schedulers.py:33-40
    if (step <= tmax) return 1.0;
    if (step >= tmin) return 0.0;
    return 1.0 - (double)(step - tmax) / (double)(tmin - tmax);
}

// get_action_probs (mcts.py:95-116) + the move choice (players.py:184-189) over the root's children pool[fc .. fc + nc): writes
// pi[action] of every child into the (already zeroed) row `pi` when one is given and returns the index of the chosen child.
// One lane; sum and running total in child-index order in float64.  In the Gumbel mode (az_engine_set_gumbel) move and policy are
// gumbel_move_policy's, whatever the temperature.  k_move (which then plays the move) and k_root_readout (which
// only reports it) both call this, so what a readout shows is what an advance would record and play.
// Gumbel mode (the contract above k_step_gumbel): the move is the best score among the candidates `gmask` (0: all children) on the
// statistics as they stand, pi the softmax of logit + sigma over all children; the temperature plays no part.
// vroot: the root's stored network value when az_engine_set_gumbel_full is in force (vmix is then the paper's), else null.
AZ_D int gumbel_move_policy(const EngDev &E, const Node *pool, int fc, int nc, u64 gmask, u32 gid, int ply, const float *vroot, float *pi) {
    double num = 0.0, den = 0.0;
    int maxN = 0, sumN = 0;
    for (int i = 0; i < nc; ++i) {
        const int n = pool[fc + i].N;
        if (n > 0) { const double P = pool[fc + i].P; num += P * pool[fc + i].Q; den += P; }
        maxN = n > maxN ? n : maxN;
        sumN += n;
    }
    const double vmix = vroot ? gumbel_vmix_full((double)*vroot, sumN, num, den) : (den > 0.0 ? num / den : 0.0);
    const double k = (E.g_cvisit + (double)maxN) * E.g_cscale;
    gmask &= first_bits64(nc);
    if (gmask == 0) gmask = first_bits64(nc);
    double xmax = -__builtin_inf(), best = -__builtin_inf();
    int pick = -1;
    bool nan = false;
    for (int i = 0; i < nc; ++i) {
        const double logit = az_det_log(pool[fc + i].P);
        const double sigma = k * (pool[fc + i].N > 0 ? pool[fc + i].Q : vmix);
        const double x = logit + sigma;
        nan |= x != x;
        xmax = fmax(xmax, x);
        if ((gmask >> i) & 1ULL) {
            const double sc = (gumbel_g(E, gid, ply, pool[fc + i].act) + logit) + sigma;
            if (sc != sc) nan = true;
            else if (pick < 0 || sc > best) { best = sc; pick = i; }
        }
    }
    if (nan || pick < 0) { atomicOr(E.err, ERR_INTERNAL); pick = pick < 0 ? 0 : pick; }
    if (pi) {
        double sum = 0.0;
        for (int i = 0; i < nc; ++i)
            sum += az_det_exp((az_det_log(pool[fc + i].P) + k * (pool[fc + i].N > 0 ? pool[fc + i].Q : vmix)) - xmax);
        for (int i = 0; i < nc; ++i)
            pi[pool[fc + i].act] = (float)(az_det_exp((az_det_log(pool[fc + i].P) + k * (pool[fc + i].N > 0 ? pool[fc + i].Q : vmix)) - xmax) / sum);
    }
    return pick;
}

// Is (gid, ply) a forced ply of az_engine_set_forced_playouts?  Its k, or 0: the mode on, and the ply full under the playout cap.
// k_root_readout and k_player_moves ask here; k_move has drawn the coin already and passes its own `fast`.
AZ_D double forced_ply_k(const EngDev &E, u32 gid, int ply) {
    return (E.kforced > 0.0 && (E.cap_nfast == 0 || playout_cap_full(E.seed, gid, ply, E.cap_pfull))) ? E.kforced : 0.0;
}

// az_engine_set_proof_backup: how the proofs among the root's children change the counts move and policy target
// are made of.  mover = the root's player.  1: some child is a proven win for the mover -- only such children keep their counts;
// 2: children proven as the mover's loss count 0; 0: the raw counts -- no proven child that matters, every child a proven loss, or
// (what the search's own pruning all but rules out) no visited child left that is not one.  *changed: some count is not the raw one.
AZ_D int proof_mode(const Node *pool, int fc, int nc, int mover, bool *changed) {
    bool any_win = false, any_loss = false, kept = false, cut = false;
    for (int i = 0; i < nc; ++i) {
        const int n = pool[fc + i].N, cw = proven_outcome(n, node_tail(pool[fc + i]));
        any_win |= cw == mover;
        if (cw == -mover) any_loss = true; else if (n > 0) kept = true;
        cut |= n > 0 && cw != mover;
    }
    const int mode = any_win ? 1 : ((any_loss && kept) ? 2 : 0);
    *changed = mode == 1 ? cut : mode == 2;
    return mode;
}
AZ_D int proof_count(const Node *pool, int fc, int i, int pmode, int mover) {
    const int n = pool[fc + i].N;
    if (pmode == 0) return n;
    const int cw = proven_outcome(n, node_tail(pool[fc + i]));
    return pmode == 1 ? (cw == mover ? n : 0) : (cw == -mover ? 0 : n);
}

// the count the temperature formula takes for child i: the raw N, or on a forced ply (kf > 0) the pruned one (no per-thread array:
// the second pass over the children computes it again), or under proof backup proof_count's (the two modes never meet)
AZ_D int policy_count(const Node *pool, int fc, int i, double kf, int root_n, int cstar, double sq, double star, int pmode = 0, int mover = 0) {
    if (pmode) return proof_count(pool, fc, i, pmode, mover);
    const int n = pool[fc + i].N;
    if (!(kf > 0.0) || i == cstar) return n;
    return forced_pruned(n, pool[fc + i].Q, pool[fc + i].P, root_n, sq, star, kf);
}

// kf: forced_ply_k of the ply (0: raw counts, the function as it always was); *pruned (when given): the sum of N - N' over the children.
// mover: under az_engine_set_proof_backup the root's player (0: the mode is off), the counts are then proof_count's at every
// temperature, 0 included; *proof_cut (when given): whether the proofs changed a count.
AZ_D int move_policy(const EngDev &E, const Node *pool, int root, int fc, int nc, double temp, u32 gid, int ply, u64 gmask, float *pi,
                     double kf = 0.0, int *pruned = nullptr, int mover = 0, bool *proof_cut = nullptr) {
    if (pruned) *pruned = 0;
    if (proof_cut) *proof_cut = false;
    if (E.gm > 0) return gumbel_move_policy(E, pool, fc, nc, gmask, gid, ply, E.nval ? nval_of(E, pool) + root : nullptr, pi);
    bool pcut = false;
    const int pmode = mover != 0 ? proof_mode(pool, fc, nc, mover, &pcut) : 0;
    if (proof_cut) *proof_cut = pcut;
    if (temp == 0.0) {  // fair_max by N
        int best = -1, cnt = 0, first = 0;
        for (int i = 0; i < nc; ++i) {
            int n = proof_count(pool, fc, i, pmode, mover);
            if (n > best) { best = n; cnt = 1; first = i; } else if (n == best) cnt++;
        }
        int pick = first;
        if (E.tie_mode == AZ_TIE_RANDOM && cnt > 1) {
            Philox4 r = az_philox(E.seed, gid, (u32)ply, 0xFFFFu, AZ_P_TIE_MOVE, 0);
            int k = (int)(((u64)r.x * (u64)cnt) >> 32);
            for (int i = 0; i < nc; ++i)
                if (proof_count(pool, fc, i, pmode, mover) == best) { if (k == 0) { pick = i; break; } --k; }
        }
        if (pi) pi[pool[fc + pick].act] = 1.0f;
        return pick;
    }
    const double inv_temp = 1.0 / temp;
    // policy target pruning (the contract above forced_playout): c*, sq and star once, then N' wherever a count is read
    int root_n = 0, cstar = 0;
    double sq = 0.0, star = 0.0;
    if (kf > 0.0) {
        root_n = pool[root].N;
        for (int i = 1; i < nc; ++i) if (pool[fc + i].N > pool[fc + cstar].N) cstar = i;
        sq = sqrt((double)root_n);
        star = pool[fc + cstar].Q + (pool[fc + cstar].P * sq) / (double)(1 + pool[fc + cstar].N);
    }
    double sum = 0.0;
    int cut = 0;
    for (int i = 0; i < nc; ++i) {
        const int ni = policy_count(pool, fc, i, kf, root_n, cstar, sq, star, pmode, mover);
        if (!pmode) cut += pool[fc + i].N - ni;  // forced playouts' own count
        double n = (double)ni;
        sum += (temp == 1.0) ? n : az_det_pow(n, inv_temp);
    }
    if (pruned) *pruned = cut;
    double u = 2.0, cum = 0.0;
    if (nc > 1) {
        Philox4 r = az_philox(E.seed, gid, (u32)ply, 0xFFFFu, AZ_P_MOVE_SAMPLE, 0);
        u = az_u53(r.x, r.y);
    }
    int chosen = 0, last = 0; bool found = false;
    for (int i = 0; i < nc; ++i) {
        double n = (double)policy_count(pool, fc, i, kf, root_n, cstar, sq, star, pmode, mover);
        double p = ((temp == 1.0) ? n : az_det_pow(n, inv_temp)) / sum;
        if (pi) pi[pool[fc + i].act] = (float)p;
        if (p > 0.0) last = i;
        cum += p;
        if (!found && u < cum) { chosen = i; found = true; }
    }
    if (!found) chosen = nc == 1 ? 0 : last;
    return chosen;
}

// get_action_probs (mcts.py:95-116) + move choice (players.py:184-189) + Sample (trainer.py:244-250)
// + play_move / change_root (trainer.py:253-256) + end-of-game bookkeeping (trainer.py:262-268).
// Once per ply: one thread per slot of [g0, g1).
__global__ void k_move(EngDev E, int g0, int g1) {
    int g = g0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= g1 || !E.active[g]) return;
    const GameDesc &gd = E.gd;
    Node *pool = pool_of(E, g);
    int ply = E.ply[g], root = E.root[g];
    u32 gid = E.game_id[g];
    BB b = {E.root_p1[g], E.root_m1[g], E.root_player[g]};
    int fc = pool[root].first, nc = pool[root].nch;
    if (nc == 0 || !(pool[root].flags & F_EXPANDED)) { atomicOr(E.err, ERR_INTERNAL); E.active[g] = 0; return; }
    double temp = linear_temp(ply, E.tmax, E.tmin);

    // az_engine_set_playout_cap: a fast ply plays its move like any other and records no sample (samp_idx -1, as the z patch expects)
    const bool fast = E.cap_nfast > 0 && !playout_cap_full(E.seed, gid, ply, E.cap_pfull);
    long long si = -1;
    if (!fast) {
        si = (long long)atomicAdd(&E.ctr[CTR_SAMPLES], 1ULL);
        if (si >= E.sample_cap) { atomicOr(E.err, ERR_SAMPLE_CAP); si = -1; }
    }
    if (ply >= E.max_plies) { atomicOr(E.err, ERR_PLY_CAP); E.active[g] = 0; return; }
    E.samp_idx[(size_t)g * E.max_plies + ply] = (int)si;
    float *pi = si >= 0 ? E.o_pi + (size_t)si * E.A : nullptr;
    int *vis = si >= 0 ? E.o_visits + (size_t)si * E.A : nullptr;
    if (si >= 0) for (int a = 0; a < E.A; ++a) { pi[a] = 0.0f; vis[a] = 0; }

    int pruned = 0;  // az_engine_set_forced_playouts: the playouts a forced ply's target lost (0 with the mode off, on a fast ply, at temperature 0)
    bool proof_cut = false;  // az_engine_set_proof_backup: the proofs changed the counts this ply's move and target are made of
    const int chosen = fc + move_policy(E, pool, root, fc, nc, temp, gid, ply, E.gmask[g], pi, fast ? 0.0 : E.kforced, &pruned,
                                        E.pf ? b.player : 0, &proof_cut);
    if (proof_cut) E.pf[2 * E.G + g] += 1;
    E.gmask[g] = 0;  // the candidates belong to the root that is left here
    int action = pool[chosen].act;
    if (si >= 0) {
        for (int i = 0; i < nc; ++i) vis[pool[fc + i].act] = pool[fc + i].N;
        int8_t *st = E.o_state + (size_t)si * gd.cells;
        for (int r = 0; r < gd.H; ++r)
            for (int c = 0; c < gd.W; ++c) st[r * gd.W + c] = (int8_t)(b.player * az_cell_value(b, r, c));
        int *m = E.o_meta + (size_t)si * 4;
        m[0] = (int)gid; m[1] = ply; m[2] = b.player; m[3] = action;
        E.o_z[si] = 0;
    }
    const int mover = b.player;  // az_engine_set_resign: whose value the root's children hold
    az_play(gd, b, action);
    E.root_p1[g] = b.p1; E.root_m1[g] = b.m1; E.root_player[g] = (int8_t)b.player;
    E.root[g] = chosen;
    pool[chosen].parent = -1;  // mcts.py:121-123
    // az_engine_set_exact_endgame: a solved node that becomes the root is an unevaluated, unexpanded root again (it keeps N and Q)
    if (pool[chosen].flags & F_SOLVED) pool[chosen].flags &= (uint8_t)~(F_TERMINAL | F_SOLVED);
    E.ply[g] = ply + 1;
    atomicAdd(&E.ctr[CTR_PLIES], 1ULL);
    if (E.cap_nfast > 0) atomicAdd(&E.ctr[fast ? CTR_FAST_PLIES : CTR_FULL_PLIES], 1ULL);
    atomicAdd(&E.ctr[CTR_NET_EVALS], (unsigned long long)E.evals[g]);
    E.evals[g] = 0;
    if (E.fpicks) {  // the forced root selections of this ply's searches, and what pruning took from the target it recorded
        if (E.fpicks[g]) atomicAdd(&E.ctr[CTR_FORCED_PICKS], (unsigned long long)E.fpicks[g]);
        E.fpicks[g] = 0;
        if (si >= 0 && pruned) atomicAdd(&E.ctr[CTR_PRUNED], (unsigned long long)pruned);
    }
    atomicMax(E.max_nodes, E.n_nodes[g]);
    int w = 0;
    bool over = az_status(gd, b, &w);
    // Resignation (az_engine_set_resign; the contract is in include/az_amd.h).  The ply above is recorded, counted and played as ever;
    // the test follows, and only if the rules have not ended the game.  A ply below rs_minply, a fast ply of the playout cap and a ply
    // whose root children hold no visit (S_N == 0) are untested: they leave the window alone.  A tested ply pushes its value
    // v = max(v_mean, v_best) (resign_value, from the raw N and Q of the children the search left under the old root: no pruning, no
    // proofs, no completed Q) into the mover's window of its last rs_k tested values -- one window per side and slot, emptied by
    // reset_slot.  m = the maximum of a full window; low[side] = the minimum of m over the game, 2.0 while the window was never full.
    // The side triggers at the first ply where m < rs_v, so it triggers at a threshold t exactly when low < t.  On a trigger: in a
    // holdout game (the coin of (seed, game id) in the log row, drawn by reset_slot) only the first one is noted -- ply and player --
    // and the game goes on, low with it; otherwise the mover resigns: the game ends here with winner -mover, through the very z patch,
    // CTR_GAMES_DONE and refill a finished game takes.  The log row is this slot's thread's alone: index game id - first id, no atomics.
    // E.rs is null unless the mode is on and the launch is az_engine_run's: az_engine_advance and the arena never resign.
    int *row = nullptr;
    u32 at = 0;
    ResignDev R = {};
    if (E.rs) {
        R = *E.rs;
        at = gid - (u32)E.ctr[CTR_FIRST_ID];
        if (at < (u32)R.gl_n) row = R.gl_rows + (size_t)at * 8;
    }
    if (row && !over && !fast && ply >= R.rs_minply) {
        double v;
        if (resign_value(nc, &pool[fc].N, sizeof(Node), &pool[fc].Q, sizeof(Node), &v)) {
            const int s = mover == 1 ? 0 : 1;
            double *win = R.rs_win + ((size_t)g * 2 + s) * AZ_RESIGN_MAX_K;
            const int cnt = R.rs_cnt[2 * g + s];
            win[cnt % R.rs_k] = v;
            R.rs_cnt[2 * g + s] = cnt + 1;
            if (cnt + 1 >= R.rs_k) {
                double m = win[0];
                for (int i = 1; i < R.rs_k; ++i) m = win[i] > m ? win[i] : m;
                double *low = R.gl_low + (size_t)at * 2 + s;
                if (m < *low) *low = m;
                if (m < R.rs_v && row[5] < 0) {
                    row[5] = ply; row[6] = mover;
                    if (!row[4]) { over = true; w = -mover; row[3] = 1; }
                }
            }
        }
    }
    if (over) {  // trainer.py:235, 262-265
        for (int p = 0; p <= ply; ++p) {
            int s2 = E.samp_idx[(size_t)g * E.max_plies + p];
            if (s2 >= 0) E.o_z[s2] = (int8_t)(w * E.o_meta[(size_t)s2 * 4 + 2]);
        }
        if (row) {
            row[1] = ply + 1; row[2] = w;
            if (row[3]) atomicAdd(&E.ctr[CTR_RESIGNED], 1ULL);
            if (row[4]) {
                atomicAdd(&E.ctr[CTR_HOLDOUT_GAMES], 1ULL);
                if (row[5] >= 0) {
                    atomicAdd(&E.ctr[CTR_HOLDOUT_TRIG], 1ULL);
                    if (w * row[6] >= 0) atomicAdd(&E.ctr[CTR_HOLDOUT_FP], 1ULL);  // the side that would have resigned did not lose
                }
            }
        }
        atomicAdd(&E.ctr[CTR_GAMES_DONE], 1ULL);
        unsigned long long nx = atomicAdd(&E.ctr[CTR_NEXT_GAME], 1ULL);
        if (nx < E.ctr[CTR_TOTAL_GAMES]) reset_slot(E, g, (u32)E.ctr[CTR_FIRST_ID] + (u32)nx, (u32)E.ctr[CTR_FIRST_ID]);
        else E.active[g] = 0;
    }
}

// change_root (mcts.py:118-125) as a compaction: the subtree under the new root (E.root[g], set by k_move) is
// copied breadth-first into the slot's other pool and becomes node 0.  While a node waits in the queue its
// `first` field still holds the OLD index of its children; when its level is processed the children are copied
// to a freshly bump-allocated block and `first` is rewritten.  16 lanes take 16 queue nodes per round.
// FULL (az_engine_set_gumbel_full in force): a node's network value travels with the node, to the same new index.
template <bool FULL>
__global__ __launch_bounds__(256) void k_reroot(EngDev E, int g0, int g1) {
    const int g = g0 + blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (g >= g1 || !E.active[g]) return;
    const int sel = E.pool_sel[g];
    const Node *src = E.nodes + ((size_t)g * 2 + sel) * E.C;
    Node *dst = E.nodes + ((size_t)g * 2 + (sel ^ 1)) * E.C;
    const float *vsrc = FULL ? nval_of(E, src) : nullptr;
    float *vdst = FULL ? nval_of(E, dst) : nullptr;
    if (sub == 0) {
        Node r = load_node(src + E.root[g]);
        r.parent = -1;
        store_node(dst, r);
        if (FULL) vdst[0] = vsrc[E.root[g]];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    int lo = 0, hi = 1, next = 1;
    bool overflow = false;
    while (lo < hi && !overflow) {
        for (int base = lo; base < hi; base += LPG) {
            const int i = base + sub;
            int cnt = 0, oldfc = 0;
            if (i < hi) { Node nd = load_node(dst + i); cnt = nd.nch; oldfc = nd.first; }
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < LPG; d <<= 1) { int y = __shfl_up(incl, d, LPG); if (sub >= d) incl += y; }
            const int total = __shfl(incl, LPG - 1, LPG);
            const int newfc = next + incl - cnt;
            if (next + total > E.C) { overflow = true; break; }
            if (cnt > 0) {
                // four children per trip: their eight 16-byte loads are in flight together (a load -> store -> load chain
                // paid the memory latency once per child: the kernel took ~0.4 ms per ply)
                for (int j = 0; j < cnt; j += 4) {
                    Node c[4];
                    float cv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int u = 0; u < 4; ++u) c[u] = load_node(src + oldfc + (j + u < cnt ? j + u : cnt - 1));
                    if (FULL) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) cv[u] = vsrc[oldfc + (j + u < cnt ? j + u : cnt - 1)];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (j + u < cnt) { c[u].parent = i; store_node(dst + newfc + j + u, c[u]); if (FULL) vdst[newfc + j + u] = cv[u]; }
                }
                dst[i].first = newfc;
            }
            next += total;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        lo = hi; hi = next;
    }
    if (sub == 0) {
        if (overflow) { atomicOr(E.err, ERR_NODE_POOL); E.active[g] = 0; }
        else atomicAdd(E.live, 1);
        E.root[g] = 0; E.n_nodes[g] = next; E.pool_sel[g] = (uint8_t)(sel ^ 1);
    }
}

// Board.play_move + MCT.change_root (mcts.py:118-125) for a move chosen OUTSIDE the engine (arena opponent,
// human): re-root at the child if the root's children are materialised and hold the action, otherwise start
// a fresh root.  status[g] = 0 or AZ_EILLEGAL (reference: ValueError, board untouched).  One thread per slot.
__global__ void k_apply_moves(EngDev E, const int *actions, int n, int *status) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || g >= E.G) return;
    const int a = actions[g];
    if (a < 0) { status[g] = AZ_OK; return; }  // no move for this slot
    if (!E.active[g]) { status[g] = AZ_ESTATE; return; }
    const GameDesc &gd = E.gd;
    Node *pool = pool_of(E, g);
    BB b = {E.root_p1[g], E.root_m1[g], E.root_player[g]};
    u64 bits = az_legal_bits(gd, b, b.player);
    bool ok = false;
    if (a >= 0 && a < gd.A) {
        if (gd.game == AZ_OTHELLO && a == gd.A - 1) ok = (bits == 0);
        else ok = (bits >> az_action_to_bit(gd, a)) & 1ULL;
    }
    if (!ok) { status[g] = AZ_EILLEGAL; return; }
    const int root = E.root[g];
    int chosen = -1;
    if (pool[root].flags & F_EXPANDED)
        for (int i = 0; i < pool[root].nch; ++i)
            if (pool[pool[root].first + i].act == a) chosen = pool[root].first + i;
    if (chosen < 0) { chosen = 0; store_node(pool, fresh_node(0, -1, 0.0, 0)); }  // mcts.py:124-125
    pool[chosen].parent = -1;
    if (pool[chosen].flags & F_SOLVED) pool[chosen].flags &= (uint8_t)~(F_TERMINAL | F_SOLVED);  // as k_move: a solved node kept as the root
    az_play(gd, b, a);
    E.root_p1[g] = b.p1; E.root_m1[g] = b.m1; E.root_player[g] = (int8_t)b.player;
    E.root[g] = chosen;
    E.ply[g] = E.ply[g] + 1;
    E.leaf_status[g] = LS_NONE;
    E.gmask[g] = 0;
    int w = 0;
    if (az_status(gd, b, &w)) E.active[g] = 0;  // finished: the board stays readable, the slot is no longer searched
    status[g] = AZ_OK;
}

// MCT.get_action_probs(temp=0) + fair_max (mcts.py:110-112): the most visited root child of every slot this
// engine is to move in; -1 elsewhere.  One thread per slot.
__global__ void k_best_moves(EngDev E, int *actions) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    actions[g] = -1;
    if (!searches(E, g)) return;
    Node *pool = pool_of(E, g);
    const int root = E.root[g], fc = pool[root].first, nc = pool[root].nch;
    if (nc == 0 || !(pool[root].flags & F_EXPANDED)) return;
    int best = -1, cnt = 0, first = 0;
    for (int i = 0; i < nc; ++i) {
        int n = pool[fc + i].N;
        if (n > best) { best = n; cnt = 1; first = i; } else if (n == best) cnt++;
    }
    int pick = first;
    if (E.tie_mode == AZ_TIE_RANDOM && cnt > 1) {
        Philox4 r = az_philox(E.seed, E.game_id[g], (u32)E.ply[g], 0xFFFFu, AZ_P_TIE_MOVE, 0);
        int k = (int)(((u64)r.x * (u64)cnt) >> 32);
        for (int i = 0; i < nc; ++i)
            if (pool[fc + i].N == best) { if (k == 0) { pick = i; break; } --k; }
    }
    actions[g] = pool[fc + pick].act;
}

// The move every slot's player plays now at temperature `temp` (az_engine_player_moves): move_policy's child for the slots k_root_readout
// serves (searched now, root expanded with children), -1 elsewhere.  In the Gumbel mode that is the Gumbel move over the slot's
// candidates; with the mode off and temp 0 it is k_best_moves' pick, draw for draw.  Reads only.  One thread per slot.
__global__ void k_player_moves(EngDev E, double temp, int *actions) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    actions[g] = -1;
    if (!searches(E, g)) return;
    const Node *pool = pool_of(E, g);
    const int root = E.root[g], fc = pool[root].first, nc = pool[root].nch;
    if (nc == 0 || !(pool[root].flags & F_EXPANDED)) return;
    actions[g] = pool[fc + move_policy(E, pool, root, fc, nc, temp, E.game_id[g], E.ply[g], E.gmask[g], nullptr, forced_ply_k(E, E.game_id[g], E.ply[g]),
                                       nullptr, E.pf ? (int)E.root_player[g] : 0)].act;
}

// Root readout for slots [0, n) in one launch: everything Player.get_move returns (players.py:158-191: the move, get_action_probs,
// the visit counts, get_prior_probs of mcts.py:95-116) plus Q and the principal line, as dense rows indexed by action.  Reads only:
// trees, boards, counters, sample buffers and the Philox state (a pure function of seed, game id and ply) stay as they are.
// 16 lanes per game: lane `sub` owns the actions sub, sub + 16, ... of every row (coalesced stores); the float64 policy arithmetic
// is move_policy in lane 0.  A slot is served when this engine searches it and its root is expanded with children; the rest get
// action -1, root_N 0, zero rows and an empty line.  Whole groups diverge together and the group steps are width-16 shuffles.
struct RootOut {
    int *visits; float *pi; double *Q, *P; uint8_t *child;
    int *action, *root_N, *pv;
    int pv_len;
};
#define RO_ROWS ((AZ_MAX_ACTIONS + LPG - 1) / LPG)  // dense-row entries per lane

AZ_D int sel4i(const int (&v)[4], int r) { return r == 0 ? v[0] : (r == 1 ? v[1] : (r == 2 ? v[2] : v[3])); }
AZ_D u64 grp_max_u64(u64 v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) { const u64 o = (u64)__shfl_xor((long long)v, m, LPG); v = o > v ? o : v; }
    return v;
}

__global__ __launch_bounds__(256) void k_root_readout(EngDev E, int n, const double *temps, RootOut o) {
    const int g = blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (g >= n) return;
    const int A = E.A;
    const Node *pool = pool_of(E, g);
    bool served = searches(E, g);
    Node rn = fresh_node(0, -1, 0.0, 0);
    if (served) {
        rn = load_node(pool + E.root[g]);  // one address for the group: a broadcast
        served = (rn.flags & F_EXPANDED) && rn.nch > 0;
    }
    const int fc = served ? rn.first : 0, nc = served ? rn.nch : 0;
    // which child holds each action this lane owns: the children's actions go round the group once
    int cact[4], idx[RO_ROWS];
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int i = r * LPG + sub; cact[r] = i < nc ? (int)pool[fc + i].act : -1; }
#pragma unroll
    for (int r = 0; r < RO_ROWS; ++r) idx[r] = -1;
    for (int i = 0; i < nc; ++i) {
        const int ai = __shfl(sel4i(cact, i >> 4), i & 15, LPG);
#pragma unroll
        for (int r = 0; r < RO_ROWS; ++r) if (ai == r * LPG + sub) idx[r] = i;
    }
#pragma unroll
    for (int r = 0; r < RO_ROWS; ++r) {
        const int a = r * LPG + sub;
        if (a >= A) continue;
        const bool has = idx[r] >= 0;
        Node c = fresh_node(0, -1, 0.0, 0);
        if (has) c = load_node(pool + fc + idx[r]);
        const size_t at = (size_t)g * A + a;
        if (o.visits) o.visits[at] = has ? c.N : 0;
        if (o.Q) o.Q[at] = has ? c.Q : 0.0;
        if (o.P) o.P[at] = has ? c.P : 0.0;
        if (o.child) o.child[at] = has ? 1 : 0;
        if (o.pi) o.pi[at] = 0.0f;
    }
    // lane 0 writes pi[action] over the zeros the other lanes have just stored: those stores must have landed
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (sub == 0) {
        int act = -1;
        if (served && (o.pi || o.action)) {
            const int ply = E.ply[g];
            const double temp = temps ? temps[g] : linear_temp(ply, E.tmax, E.tmin);
            act = pool[fc + move_policy(E, pool, E.root[g], fc, nc, temp, E.game_id[g], ply, E.gmask[g], o.pi ? o.pi + (size_t)g * A : nullptr, forced_ply_k(E, E.game_id[g], ply),
                                        nullptr, E.pf ? (int)E.root_player[g] : 0)].act;
        }
        if (o.action) o.action[g] = act;
        if (o.root_N) o.root_N[g] = served ? rn.N : 0;
    }
    if (!o.pv) return;
    // principal line: from the root, the child with the greatest N (lowest action among equals) while there is one with N > 0
    bool on = served;
    int nf = fc, nn = nc;
    for (int step = 0; step < o.pv_len; ++step) {
        int out = -1;
        if (on) {
            u64 key = 0;  // N | 255 - action | child index: the maximum is the most visited child, the lowest action among equals
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = r * LPG + sub;
                if (i < nn) {
                    const Node c = load_node(pool + nf + i);
                    const u64 k = ((u64)(u32)c.N << 16) | ((u64)(255 - c.act) << 8) | (u64)i;
                    if (c.N > 0 && k > key) key = k;
                }
            }
            key = grp_max_u64(key);
            on = key != 0;
            if (on) {
                out = 255 - (int)((key >> 8) & 255);
                const Node c = load_node(pool + nf + (int)(key & 255));
                on = (c.flags & F_EXPANDED) && c.nch > 0;
                nf = c.first; nn = c.nch;
            }
        }
        if (sub == 0) o.pv[(size_t)g * o.pv_len + step] = out;
    }
}

// TicTacToeBoard.get_score (tictactoe.py:119-126) is +inf when the side to move holds two cells of an alignment whose
// third cell is free, else 0
AZ_D bool ttt_can_win_at_once(const BB &b) {
    const u64 own = b.player > 0 ? b.p1 : b.m1, occ = b.p1 | b.m1;
    const u64 L[8] = {0x7ULL, 0x7ULL << 8, 0x7ULL << 16, 0x010101ULL, 0x010101ULL << 1, 0x010101ULL << 2,
                      (1ULL | (1ULL << 9) | (1ULL << 18)), ((1ULL << 2) | (1ULL << 9) | (1ULL << 16))};
    bool threat = false;
    for (int l = 0; l < 8; ++l) threat |= (__popcll(own & L[l]) == 2 && __popcll(occ & L[l]) == 2);
    return threat;
}

// RandomPlayer / GreedyPlayer (players.py:76-123) for the slots where the OTHER colour is to move:
// kind 0 = uniform legal move, kind 1 = best immediate -get_score() of the position after the move, ties uniform.
__global__ void k_baseline_moves(EngDev E, int kind, u32 seed, int *actions) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    actions[g] = -1;
    if (!E.active[g] || E.side[g] == 0 || E.side[g] == E.root_player[g]) return;
    const GameDesc &gd = E.gd;
    BB b = {E.root_p1[g], E.root_m1[g], E.root_player[g]};
    u64 bits = az_legal_bits(gd, b, b.player);
    if (gd.game == AZ_OTHELLO && bits == 0) { actions[g] = gd.A - 1; return; }  // forced pass
    int n = __popcll(bits);
    if (n == 0) return;
    u64 cand = bits;
    if (kind == 1) {  // greedy: keep the moves with the best score
        int best = -1000000;
        cand = 0;
        for (u64 m = bits; m; m &= m - 1) {
            int bit = __ffsll((long long)m) - 1;
            BB c = b;
            az_play(gd, c, az_bit_to_action(gd, bit));
            int sc;
            if (gd.game == AZ_TICTACTOE) {  // -get_score(): -inf when the opponent can complete a line at once (tictactoe.py:119-126)
                sc = ttt_can_win_at_once(c) ? -1 : 0;
            } else {
                sc = -(c.player * (__popcll(c.p1) - __popcll(c.m1)));  // -sum(player*grid) after the move
            }
            if (sc > best) { best = sc; cand = 1ULL << bit; } else if (sc == best) cand |= 1ULL << bit;
        }
        n = __popcll(cand);
    }
    int k = 0;  // greedy under the deterministic tie-break (tests against the reference's patched fair_max): lowest action
    if (kind == 0 || E.tie_mode == AZ_TIE_RANDOM) {
        Philox4 r = az_philox(seed, E.game_id[g], (u32)E.ply[g], 0xFFFEu, AZ_P_TIE_MOVE, (u32)kind);
        k = (int)(((u64)r.x * (u64)n) >> 32);
    }
    for (int i = 0; i < k; ++i) cand &= cand - 1;
    actions[g] = az_bit_to_action(gd, __ffsll((long long)cand) - 1);
}

__global__ void k_root_status(EngDev E, int8_t *players, uint8_t *over, int8_t *winner, int *score) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    BB b = {E.root_p1[g], E.root_m1[g], E.root_player[g]};
    int w = 2;
    bool o = az_status(E.gd, b, &w);
    players[g] = (int8_t)b.player; over[g] = o ? 1 : 0; winner[g] = (int8_t)(o ? w : 2);
    // Board.get_score from the side to move's viewpoint; TicTacToe's +inf is reported as 32767
    score[g] = E.gd.game == AZ_TICTACTOE ? (ttt_can_win_at_once(b) ? 32767 : 0) : b.player * (__popcll(b.p1) - __popcll(b.m1));
}

// closed-form fake network (tests): reads the canonical board back from nn_in
__global__ void k_fakenet(EngDev E, const int *cnt) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G * E.K || g >= *cnt) return;
    const float *in = E.nn_in + (size_t)g * E.gd.cells;
    u64 h = 0x9E3779B97F4A7C15ULL;
    for (int i = 0; i < E.gd.cells; ++i) h = (h ^ (u64)((int)in[i] + 1)) * 0x100000001B3ULL;
    h = az_splitmix64(h);
    float *pr = E.probs + (size_t)g * E.A;
    for (int a = 0; a < E.A; ++a) {
        u64 w = 1 + (az_splitmix64(h + (u64)(a + 1) * 0x9E3779B97F4A7C15ULL) >> 58);
        pr[a] = (float)w / 4096.0f;
    }
    u64 t = az_splitmix64(h ^ 0xD1B54A32D192ED03ULL);
    int sel = (int)((t >> 10) & 15);
    float v = ((float)(int)(t & 1023) - 512.0f) / 512.0f;
    if (sel == 0) v = 0.0f;
    if (sel == 1) v = 6.103515625e-05f;
    E.value[g] = v;
}

// ---- AZ_EVAL_EXTERNAL: the caller evaluates the pending rows (az_engine_set_evaluator) ---------------------------------------
// Before the callback: the absolute board (Board.grid, Board.player) and the slot of every pending row, so that the host can
// rebuild the reference's Board.  Root pass: the fresh roots (k_root_prep); lock-step: the leaves k_step selected for evaluation.
__global__ __launch_bounds__(256) void k_ext_export(EngDev E, int root_pass, int8_t *grids, int8_t *players, int *slots) {
    const int g = blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (g >= E.G) return;
    BB b;
    if (root_pass) {
        if (!E.root_fresh[g]) return;
        b = {E.root_p1[g], E.root_m1[g], E.root_player[g]};
    } else {
        if (E.leaf_status[g] != LS_EVAL) return;
        b = {E.leaf_p1[g], E.leaf_m1[g], E.leaf_player[g]};
    }
    const int row = E.row_of_slot[g];  // < G: rows are handed out once per pending slot
    int8_t *dst = grids + (size_t)row * E.gd.cells;
    for (int i = sub; i < E.gd.cells; i += LPG) dst[i] = (int8_t)az_cell_value(b, i / E.gd.W, i % E.gd.W);
    if (sub == 0) { players[row] = (int8_t)b.player; slots[row] = g; }
}

// After the callback: outputs from outside the program are validated, never repaired.  A negative or non-finite prior or a
// non-finite value raises ERR_EVAL and records the lowest offending slot.
__global__ __launch_bounds__(256) void k_ext_check(EngDev E, const int *cnt, const int *slots, int *bad_slot) {
    const int row = blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (row >= E.G || row >= *cnt) return;
    const float *pr = E.probs + (size_t)row * E.A;
    bool bad = false;
    for (int a = sub; a < E.A; a += LPG) bad |= !(pr[a] >= 0.0f) || __builtin_isinf(pr[a]);
    if (sub == 0) bad |= !__builtin_isfinite(E.value[row]);
    if (bad) { atomicOr(E.err, ERR_EVAL); atomicMin(bad_slot, slots[row]); }
}

// ---- one randomly drawn board symmetry per evaluation (az_engine_set_symmetry_random) ----------------------------
// Every pending row is evaluated in ONE member of the candidate mask.  members = the mask's codes in ascending order, n of them:
//   r = az_philox(seed, game_id[slot], ply[slot], s, AZ_P_SYMMETRY, 0),  m = (u32)(((u64)r.x * n) >> 32),  code = members[m]
// s = (u32)(sim + sim_base) for the leaf of simulation sim (leaf_batch K: walker j of lock-step t has sim = t * K + j, k_step_multi's
// own index), 0xFFFFFFFF for the root-prior pass; ply is the root's.  A function of the game alone: never of the slot, the row, the
// batch shape or the GPU.  The kernel is slot-major (only the slot knows its game id and ply) with the pending predicate and the
// row of k_ext_export; slots that do not search hold root_fresh 0 (k_root_prep), LS_NONE (k_step) and LS_NONE for every walker
// (k_step_multi) -- all three are written for every slot of the engine, arena mode (az_engine_set_sides) included.  It writes the
// twin of nn_in[row] to sym_in[row] (out of place) and the code to sym_code[row]; k_sym_unpick (az_symmetry.hip) maps the network's
// answer back.  No barrier: groups without a pending row leave at once.
#define AZ_P_SYMMETRY 8
#define SYM_ROOT_PASS 0xFFFFFFFFu

AZ_D int sym_draw(const EngDev &E, int g, u32 ply, u32 s, int mask, int n) {
    const Philox4 r = az_philox(E.seed, E.game_id[g], ply, s, AZ_P_SYMMETRY, 0);
    return kth_set_bit((u32)mask, (int)(((u64)r.x * (u64)n) >> 32));
}

AZ_D void sym_pick_row_grp(const EngDev &E, int row, int code, float *sym_in, uint8_t *sym_code, int sub) {
    const float *src = E.nn_in + (size_t)row * E.gd.cells;
    float *dst = sym_in + (size_t)row * E.gd.cells;
    for (int i = sub; i < E.gd.cells; i += LPG) {
        int rr, cc;
        aug_source(code, E.gd.H, E.gd.W, i / E.gd.W, i % E.gd.W, &rr, &cc);
        dst[i] = src[rr * E.gd.W + cc];
    }
    if (sub == 0) sym_code[row] = (uint8_t)code;
}

// step: -1 the root-prior pass; K == 1: the simulation index k_step was launched with; K > 1: the lock-step t of k_step_multi and its kt;
// Gumbel mode with K > 1 (k_step_gumbel_multi): kt = K, walker j of a slot is simulation gstart[slot] + j, walkers the slot did not run hold LS_NONE
__global__ __launch_bounds__(256) void k_sym_pick(EngDev E, int mask, int n, int step, int kt, float *sym_in, uint8_t *sym_code) {
    const int g = blockIdx.x * GPB + (threadIdx.x >> 4), sub = threadIdx.x & (LPG - 1);
    if (g >= E.G) return;
    if (step < 0 || E.K == 1) {
        if (step < 0 ? !E.root_fresh[g] : E.leaf_status[g] != LS_EVAL) return;
        const int code = sym_draw(E, g, (u32)E.ply[g], step < 0 ? SYM_ROOT_PASS : (u32)step + E.sim_base, mask, n);
        sym_pick_row_grp(E, E.row_of_slot[g], code, sym_in, sym_code, sub);
        return;
    }
    // lane j: walker j's status, row and draw; the rows are then permuted one after the other by the whole group
    const size_t wj = (size_t)g * MLB + sub;
    const bool mine = sub < kt && E.m_leaf_status[wj] == LS_EVAL;
    const int my_row = mine ? E.m_row[wj] : -1;
    const int sim0 = E.gm > 0 ? E.gstart[g] : step * E.K;
    const int my_code = mine ? sym_draw(E, g, (u32)E.ply[g], (u32)(sim0 + sub) + E.sim_base, mask, n) : 0;
    for (int j = 0; j < kt; ++j) {
        const int row = __shfl(my_row, j, LPG), code = __shfl(my_code, j, LPG);
        if (row >= 0) sym_pick_row_grp(E, row, code, sym_in, sym_code, sub);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#include "az_search_plan.h"  // the launch sequence of a search as a value, the batch caps, the slot groups' ranges and measured rule
static_assert(GPB == AZ_SLOT_BLOCK, "a slot group is whole blocks of the step kernels");

struct az_engine {
    az_engine_cfg cfg;
    EngDev d;
    az_net *net;
    hipStream_t stream;
    std::vector<void *> allocs;
    unsigned long long *h_ctr;  // pinned [AZ_MAX_GROUPS][CTR_ALLOC]: a slot group reads the shared counters into its own copy ([0]: every other caller)
    int *h_err;                 // pinned [AZ_MAX_GROUPS][4] : err, max_nodes, max_path, the group's live slots
    long long lockstep_iters[AZ_MAX_GROUPS];  // per slot group; the stats report the largest (a ply's lock-steps count once, not once per group)
    u32 sim_base = 0;
    // The engine runs on a stream of its own (graph capture is not allowed on the legacy default stream); every entry
    // point first orders it behind the caller's stream and returns only after its own stream has drained.
    hipStream_t user_stream = nullptr;
    bool search_open = false;  // between az_engine_search_begin and _end
    hipEvent_t ev_in = nullptr;
    // One search = 1 + 5 n_sim kernel launches: captured once per (kernel family, n_sim, batch cap, slot range) as a HIP graph and replayed
    std::map<SearchKey, hipGraphExec_t> graphs;
    std::map<SearchKey, int> graph_seen;
    bool graphs_ok = true;
    long long graph_replays = 0;
    int *scr_a = nullptr, *scr_b = nullptr;  // [G] int scratch of the arena entry points (moves in/out, status, scores)
    char *scr_c = nullptr;                   // [3 G] bytes
    int active_bound = 0;  // upper bound on the slots still searching (known per ply): caps the network batch, which picks the kernels
    // AZ_EVAL_EXTERNAL only: the caller's evaluator and the rows it is shown besides nn_in
    az_eval_fn ext_fn = nullptr;
    void *ext_user = nullptr;
    int8_t *ext_grids = nullptr, *ext_players = nullptr;
    int *ext_slots = nullptr, *ext_bad = nullptr;  // ext_bad: lowest slot k_ext_check rejected
    bool in_callback = false;  // the evaluator is running: calls into this engine are refused
    bool unevaluated = false;  // a failed evaluation left leaves in the trees that were never evaluated (until set_roots / run)
    double *ro_temps = nullptr;  // [G] per-slot temperatures of az_engine_root_readout (allocated at its first use)
    // az_engine_set_symmetry: the transform codes every leaf is averaged over (0: off) and the twins' rows, [sym_rows] each
    int sym_mask = 0, sym_n = 0, sym_rows = 0;
    float *sym_in = nullptr, *sym_p = nullptr, *sym_v = nullptr;
    int *sym_cnt = nullptr;  // sym_n * the pending count, written by k_sym_expand for az_net_forward_dyn
    // az_engine_set_symmetry_random: the candidate codes one of which is drawn per evaluation (0: off; never together with sym_mask)
    // and the code of every pending row, [sym_rows] bytes; the twins and their outputs use sym_in / sym_p / sym_v, K * G rows
    int symr_mask = 0, symr_n = 0;
    uint8_t *sym_code = nullptr;
    // az_engine_set_leaf_batch: walkers per slot and lock-step (1: k_step) and the rows nn_in / probs / value hold
    int leaf_batch = 1, net_rows = 0;
    // az_engine_set_gumbel_batch: the walkers of the Gumbel mode, in force (d.K) only while d.gm > 0
    int gumbel_batch = 1;
    // az_engine_set_gumbel_full: the switch and the per-node network values, [G][2][C], allocated when it first goes on; in force
    // (d.nval == nval) only while d.gm > 0, else d.nval is null
    int gumbel_full = 0;
    float *nval = nullptr;
    // az_engine_set_groups: the request (0: auto) and whether AZ_ENGINE_GROUPS made it; the later groups' streams (group 0 runs on
    // `stream`), made at the first grouped run; the event that orders them behind `stream`
    // az_engine_set_playout_cap: the per-slot budgets, [G], allocated when the mode first goes on; in force (d.budget == cap_budget,
    // d.cap_nfast > 0) only while it is on, else d.budget is null
    int *cap_budget = nullptr;
    // az_engine_set_forced_playouts: the per-slot counts of forced root selections, [G], allocated when the mode first goes on; in
    // force (d.fpicks == forced_picks, d.kforced > 0) only while it is on, else d.fpicks is null
    int *forced_picks = nullptr;
    // az_engine_set_eval_cache: the request (AZ_EVAL_CACHE_*) and whether AZ_ENGINE_EVAL_CACHE made it; entries per group and the stone
    // limit; the groups' tables, their serial words and the per-slot words, allocated by the first run that caches.  d.ec_* point at
    // them only inside az_engine_run (ec_attach): every other entry point launches with null pointers.  graphs_ec: the captured
    // searches carry the tables' pointers (a search with the other setting drops them first).
    int ec_req = AZ_EVAL_CACHE_AUTO;
    bool ec_env = false;
    int ec_capacity = AZ_EC_DEFAULT_CAPACITY, ec_limit = AZ_EC_DEFAULT_LIMIT;
    EcHdr *ec_hdr[AZ_MAX_GROUPS] = {nullptr, nullptr, nullptr, nullptr};
    float *ec_pay[AZ_MAX_GROUPS] = {nullptr, nullptr, nullptr, nullptr};
    u32 *ec_serial = nullptr;
    int *ec_claim = nullptr, *ec_hits = nullptr;
    bool graphs_ec = false;
    // the heads inside the step kernel: the request of AZ_ENGINE_STEP_HEADS (-1: unset, the measured rule; 0: never;
    // 1: wherever served), whether the last az_engine_run ran the form, and the pointers the captured searches of each chain carry by
    // value (a search with other ones drops every graph first)
    int sh_req = -1;
    bool sh_used = false;
    const void *graphs_sh[AZ_MAX_GROUPS][3] = {};
    // az_engine_set_exact_endgame: the per-slot counts of solved leaves and solver positions, [G] each, allocated when the mode first
    // goes on; in force (d.x_solved == exact_solved, d.exact_max > 0) only while it is on, else d.x_solved is null
    int *exact_solved = nullptr;
    unsigned long long *exact_nodes = nullptr, *exact_sums = nullptr;  // exact_sums [2]: where k_exact_stats leaves the two totals
    // az_engine_set_proof_backup: the per-slot counter words, [3][G], allocated when the mode first goes on; in force (d.pf == proof_ctr)
    // only while it is on, else d.pf is null; proof_sums [3]: where k_proof_stats leaves the totals
    int *proof_ctr = nullptr;
    unsigned long long *proof_sums = nullptr;
    // az_engine_set_resign: the settings live in rs (rs.rs_k == 0: off) and reach the device as *rs_dev, written at every run.  The
    // per-slot windows and counts, [G][2][AZ_RESIGN_MAX_K] and [G][2], and rs_dev are allocated when the mode first goes on; the game
    // log -- gl_rows [gl_cap][8], gl_low [gl_cap][2], memory of their own because a run with more games grows them -- at the run, for
    // its n_games; gl_n = the rows of the last az_engine_run (0: it ran with the mode off).  d.rs == rs_dev only inside az_engine_run
    // (rs_attach): every other entry
    // point launches k_move with null pointers.  No captured search holds k_move, and no kernel of one reads these fields.
    ResignDev rs = {};
    ResignDev *rs_dev = nullptr;
    double *rs_win = nullptr;
    int *rs_cnt = nullptr;
    int *gl_rows = nullptr;
    double *gl_low = nullptr;
    int gl_cap = 0, gl_n = 0;
    int groups_req = 0;
    bool groups_env = false;
    hipStream_t gstream[AZ_MAX_GROUPS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_grp = nullptr;
};

// One launch chain of a search: the whole engine on its stream, or one slot group of az_engine_run -- slots [g0, g1) on the group's
// stream, with d = the engine's device view whose network rows, row counters and live word are the group's own.
struct Chain {
    EngDev d;
    int g0, g1, idx;
    hipStream_t st;
    bool beside;  // another chain runs next to this one (az_net_forward_lane)
    int live;     // a slot group: the slots that hold a game (exact: counted by the group's own last ply); bounds its network batch
};
static Chain whole_chain(const az_engine *e) { return Chain{e->d, 0, e->d.G, 0, e->stream, false, 0}; }

int az_make_game_desc(int game, int H, int W, GameDesc *gd) {
    AZ_REQUIRE(game >= 0 && game <= 2, AZ_EINVAL, "unknown game id %d", game);
    if (game == AZ_OTHELLO) {
        AZ_REQUIRE(H == W && H >= 4 && H <= 8, AZ_EINVAL, "Othello board must be n x n with 4 <= n <= 8, got %dx%d", H, W);
        AZ_REQUIRE(H % 2 == 0, AZ_EINVAL, "Board size must be even but got n=%d", H);  // othello.py:87-88
    } else if (game == AZ_CONNECT4) {
        AZ_REQUIRE(H >= 4 && W >= 4, AZ_EINVAL, "Borad size must be at least 4x4, got %dx%d", W, H);  // connect4.py:90-91
        AZ_REQUIRE(H <= 8 && W <= 8, AZ_EINVAL, "Connect4 board larger than 8x8 is not supported (%dx%d)", W, H);
    } else {
        AZ_REQUIRE(H == 3 && W == 3, AZ_EINVAL, "TicTacToe board is 3x3");
    }
    gd->game = game; gd->H = H; gd->W = W; gd->cells = H * W;
    gd->A = game == AZ_OTHELLO ? H * W + 1 : (game == AZ_CONNECT4 ? W : 9);
    u64 v = 0;
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) v |= 1ULL << (r * 8 + c);
    gd->valid = v;
    return AZ_OK;
}

template <typename T>
static int dev_alloc(az_engine *e, T **p, size_t n) {
    void *q = nullptr;
    AZ_HIP(hipMalloc(&q, n * sizeof(T)));
    AZ_HIP(hipMemsetAsync(q, 0, n * sizeof(T), e->stream));
    e->allocs.push_back(q);
    *p = (T *)q;
    return AZ_OK;
}

#define AZ_TRY(x) do { int _rc = (x); if (_rc != AZ_OK) return _rc; } while (0)

static inline dim3 grid_for(int n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }
#define TB 64

// between az_engine_search_begin and _end the search's launches are in flight and its error flags unread: every other entry point of
// the engine (they reorder host-side state -- sim_base, active_bound, the graph cache -- or read device state the search is writing)
// refuses until the search has been ended
#define AZ_NO_OPEN_SEARCH(e, who) AZ_REQUIRE(!(e)->search_open, AZ_ESTATE, who ": a search begun with az_engine_search_begin has not been ended (az_engine_search_end)")
// AZ_EVAL_EXTERNAL: no call from inside the evaluator; none but set_roots / run (and destroy) after a failed evaluation
#define AZ_NOT_IN_CALLBACK(e, who) AZ_REQUIRE(!(e)->in_callback, AZ_ESTATE, who ": called from inside the engine's own evaluator")
#define AZ_USABLE(e, who) do { AZ_NOT_IN_CALLBACK(e, who); \
    AZ_REQUIRE(!(e)->unevaluated, AZ_ESTATE, who ": an evaluation failed and left unevaluated leaves in the trees; az_engine_set_roots or az_engine_run resets the slots"); } while (0)
// how every az_engine_set_* of a search mode opens
#define AZ_SETTER(e, who) do { AZ_REQUIRE(e, AZ_EINVAL, "null engine"); AZ_NO_OPEN_SEARCH(e, who); AZ_NOT_IN_CALLBACK(e, who); } while (0)

extern "C" int az_engine_create(const az_engine_cfg *cfg, az_net *net, void *stream, az_engine **out) {
    AZ_REQUIRE(cfg && out, AZ_EINVAL, "null argument");
    GameDesc gd;
    AZ_TRY(az_make_game_desc(cfg->game, cfg->H, cfg->W, &gd));
    AZ_REQUIRE(cfg->n_slots > 0 && cfg->n_sim > 0, AZ_EINVAL, "n_slots and n_sim must be positive");
    AZ_REQUIRE(cfg->node_capacity >= 2 * AZ_MAX_ACTIONS, AZ_EINVAL, "node_capacity too small");
    AZ_REQUIRE(cfg->max_plies > 0 && cfg->sample_capacity > 0, AZ_EINVAL, "max_plies / sample_capacity must be positive");
    AZ_REQUIRE(cfg->temp_min_step >= cfg->temp_max_step, AZ_EINVAL,
               "temp_min_step should be greater than temp_max_step for linear scheduler.");  // schedulers.py:29-30
    AZ_REQUIRE(cfg->evaluator >= AZ_EVAL_NET && cfg->evaluator <= AZ_EVAL_EXTERNAL, AZ_EINVAL, "unknown evaluator %d", cfg->evaluator);
    AZ_REQUIRE(cfg->evaluator != AZ_EVAL_NET || net != nullptr, AZ_ESTATE, "a network is required for AZ_EVAL_NET");
    if (cfg->evaluator == AZ_EVAL_NET)
        AZ_REQUIRE(az_net_action_size(net) == gd.A, AZ_EINVAL, "network action size %d != game action size %d",
                   az_net_action_size(net), gd.A);
    az_engine *e = new az_engine();
    e->h_ctr = nullptr; e->h_err = nullptr;
    e->cfg = *cfg; e->net = net; e->user_stream = (hipStream_t)stream; e->stream = nullptr;
    for (int i = 0; i < AZ_MAX_GROUPS; ++i) e->lockstep_iters[i] = 0;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming) != hipSuccess) {
        az_engine_destroy(e);
        az_set_error("could not create the engine's stream");
        return AZ_EHIP;
    }
    { const char *g = getenv("AZ_ENGINE_GRAPHS"); if (g && atoi(g) == 0) e->graphs_ok = false; }
    EngDev &d = e->d;
    d.gd = gd; d.G = cfg->n_slots; d.C = cfg->node_capacity; d.A = gd.A; d.max_plies = cfg->max_plies;
    d.alpha = cfg->dirichlet_alpha; d.eps = cfg->dirichlet_epsilon; d.tie_mode = cfg->tie_mode;
    d.rollout = cfg->evaluator == AZ_EVAL_ROLLOUT ? 1 : 0;
    d.noise_mode = cfg->noise_mode; d.tmax = cfg->temp_max_step; d.tmin = cfg->temp_min_step; d.seed = cfg->seed;
    d.sample_cap = cfg->sample_capacity;
    d.K = 1; e->net_rows = d.G;
    d.gm = 0; d.g_cvisit = 0.0; d.g_cscale = 0.0; d.g_scale = 0.0;
    d.nval = nullptr;
    d.cap_nfast = 0; d.cap_pfull = 1.0; d.budget = nullptr;
    d.kforced = 0.0; d.fpicks = nullptr;
    d.ec_hdr = nullptr; d.ec_pay = nullptr; d.ec_serial = nullptr; d.ec_claim = nullptr; d.ec_hits = nullptr;
    d.ec_mask = 0; d.ec_limit = 0; d.ec_stride = 0;
    d.exact_max = 0; d.x_solved = nullptr; d.x_nodes = nullptr;
    d.pf = nullptr;
    d.puct_cinit = 1.0; d.puct_cbase = 0.0; d.puct_fpu = -1.0;
    d.sh_h2 = nullptr; d.sh_wq = nullptr; d.sh_hb = nullptr; d.sh_nt = 0;
    d.rs = nullptr;
    size_t G = d.G, NC = G * (size_t)d.C, S = (size_t)cfg->sample_capacity;
    int rc = AZ_OK;
#define A_(p, n) if (rc == AZ_OK) rc = dev_alloc(e, &d.p, (n))
    A_(root_p1, G); A_(root_m1, G); A_(root_player, G); A_(root, G); A_(n_nodes, G); A_(ply, G); A_(game_id, G);
    A_(active, G); A_(root_fresh, G); A_(side, G); A_(leaf, G); A_(leaf_p1, G); A_(leaf_m1, G); A_(leaf_player, G);
    A_(leaf_status, G); A_(leaf_winner, G); A_(path, G * LPG); A_(path_len, G);
    A_(nodes, 2 * NC); A_(pool_sel, G);
    A_(nn_in, G * gd.cells); A_(probs, G * gd.A); A_(value, G); A_(row_of_slot, G); A_(evals, G); A_(batch_cnt, 4 * AZ_MAX_GROUPS); A_(live, AZ_MAX_GROUPS);
    A_(samp_idx, G * (size_t)d.max_plies);
    A_(o_state, S * gd.cells); A_(o_pi, S * gd.A); A_(o_z, S); A_(o_meta, S * 4); A_(o_visits, S * gd.A);
    A_(ctr, CTR_ALLOC); A_(err, 1); A_(max_nodes, 1); A_(max_path, 1);
    A_(gmask, G); A_(gcur, G); A_(gstart, G);
#undef A_
    if (rc == AZ_OK) rc = dev_alloc(e, &e->scr_a, G);
    if (rc == AZ_OK) rc = dev_alloc(e, &e->scr_b, G);
    if (rc == AZ_OK) rc = dev_alloc(e, &e->scr_c, 3 * G);
    if (cfg->evaluator == AZ_EVAL_EXTERNAL) {
        if (rc == AZ_OK) rc = dev_alloc(e, &e->ext_grids, G * gd.cells);
        if (rc == AZ_OK) rc = dev_alloc(e, &e->ext_players, G);
        if (rc == AZ_OK) rc = dev_alloc(e, &e->ext_slots, G);
        if (rc == AZ_OK) rc = dev_alloc(e, &e->ext_bad, 1);
    }
    if (rc == AZ_OK && hipHostMalloc((void **)&e->h_ctr, sizeof(unsigned long long) * CTR_ALLOC * AZ_MAX_GROUPS) != hipSuccess) rc = AZ_EHIP;
    if (rc == AZ_OK && hipHostMalloc((void **)&e->h_err, sizeof(int) * 4 * AZ_MAX_GROUPS) != hipSuccess) rc = AZ_EHIP;
    if (rc == AZ_OK) {  // AZ_ENGINE_GROUPS: one build measured against itself; engines that do not serve groups ignore it (groups_in_force)
        const char *g = getenv("AZ_ENGINE_GROUPS");
        const int n = g ? atoi(g) : 0;
        if (n == 1 || n == 2 || n == 4) { e->groups_req = n; e->groups_env = true; }
    }
    if (rc == AZ_OK) {  // AZ_ENGINE_EVAL_CACHE, likewise: 0 = never, 1 = wherever the cache is served (eval_cache_in_force)
        const char *c = getenv("AZ_ENGINE_EVAL_CACHE");
        if (c && (c[0] == '0' || c[0] == '1') && c[1] == 0) { e->ec_req = c[0] == '1' ? AZ_EVAL_CACHE_ON : AZ_EVAL_CACHE_OFF; e->ec_env = true; }
    }
    if (rc == AZ_OK) {  // AZ_ENGINE_STEP_HEADS, likewise: 0 = never, 1 = wherever the form is served (step_heads_in_force)
        const char *c = getenv("AZ_ENGINE_STEP_HEADS");
        if (c && (c[0] == '0' || c[0] == '1') && c[1] == 0) e->sh_req = c[0] - '0';
    }
    if (rc != AZ_OK) { az_engine_destroy(e); return rc; }
    if (hipStreamSynchronize(e->stream) != hipSuccess) { az_engine_destroy(e); az_set_error("stream sync failed"); return AZ_EHIP; }
    *out = e;
    return AZ_OK;
}

static int fetch_counters(az_engine *e, const Chain *grp = nullptr);
static int check_err(az_engine *e, int idx = 0);
static void drop_graphs(az_engine *e);

// change_root for every active slot; with az_engine_set_gumbel_full in force the instantiation that moves the stored values too
static void launch_reroot(const Chain &c) {
    const EngDev &d = c.d;
    const dim3 gg((unsigned)((c.g1 - c.g0 + GPB - 1) / GPB)), gb(256);
    if (d.nval) hipLaunchKernelGGL((k_reroot<true>), gg, gb, 0, c.st, d, c.g0, c.g1);
    else hipLaunchKernelGGL((k_reroot<false>), gg, gb, 0, c.st, d, c.g0, c.g1);
}

extern "C" void az_engine_destroy(az_engine *e) {
    if (!e) return;
    if (e->in_callback) { fprintf(stderr, "az_engine_destroy: called from inside the engine's own evaluator; ignored\n"); return; }
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (int i = 1; i < AZ_MAX_GROUPS; ++i)
        if (e->gstream[i]) { (void)hipStreamSynchronize(e->gstream[i]); (void)hipStreamDestroy(e->gstream[i]); }
    if (e->ev_grp) (void)hipEventDestroy(e->ev_grp);
    if (e->search_open) {  // destroyed with a search still open: its errors would vanish with the engine -- say so
        e->search_open = false;
        if (fetch_counters(e) == AZ_OK && check_err(e) != AZ_OK)
            fprintf(stderr, "az_engine_destroy: the search that was never ended had failed: %s\n", az_last_error());
    }
    for (auto &kv : e->graphs) (void)hipGraphExecDestroy(kv.second);
    for (void *p : e->allocs) (void)hipFree(p);
    for (int i = 0; i < AZ_MAX_GROUPS; ++i) { if (e->ec_hdr[i]) (void)hipFree(e->ec_hdr[i]); if (e->ec_pay[i]) (void)hipFree(e->ec_pay[i]); }
    if (e->gl_rows) (void)hipFree(e->gl_rows);
    if (e->gl_low) (void)hipFree(e->gl_low);
    if (e->ev_in) (void)hipEventDestroy(e->ev_in);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->h_ctr) (void)hipHostFree(e->h_ctr);
    if (e->h_err) (void)hipHostFree(e->h_err);
    delete e;
}

// AZ_EVAL_EXTERNAL: export the pending rows' boards, call the caller's evaluator, validate what it wrote.  `step`: the lock-step
// index, -1 for the root-prior pass.  A failed callback ends the search here: nothing more is queued, the stream is drained.
static int forward_external(az_engine *e, const int *cnt, int cap, int step) {
    EngDev &d = e->d;
    dim3 gg((unsigned)((d.G + GPB - 1) / GPB)), gb(256);
    hipLaunchKernelGGL(k_ext_export, gg, gb, 0, e->stream, d, step < 0 ? 1 : 0, e->ext_grids, e->ext_players, e->ext_slots);
    AZ_HIP(hipGetLastError());
    az_eval_batch b;
    b.cap = cap; b.H = d.gd.H; b.W = d.gd.W; b.A = d.A;
    b.d_count = cnt; b.d_input = d.nn_in; b.d_grids = e->ext_grids; b.d_players = e->ext_players; b.d_slots = e->ext_slots;
    b.d_probs = d.probs; b.d_value = d.value;
    e->in_callback = true;
    const int rc = e->ext_fn(e->ext_user, &b, (void *)e->stream);
    e->in_callback = false;
    if (rc != 0) {
        e->unevaluated = true;
        (void)hipStreamSynchronize(e->stream);
        if (step < 0) az_set_error("external evaluator returned %d in the root-prior pass", rc);
        else az_set_error("external evaluator returned %d at lock-step %d", rc, step);
        return AZ_EEVAL;
    }
    hipLaunchKernelGGL(k_ext_check, gg, gb, 0, e->stream, d, cnt, (const int *)e->ext_slots, e->ext_bad);
    AZ_HIP(hipGetLastError());
    return AZ_OK;
}

// network over the compacted leaf rows [0, *cnt)
// (the external evaluator and the symmetry modes run as the whole engine's chain only: their buffers are per engine)
static int forward(az_engine *e, const Chain &c, const int *cnt, int cap, int step, int kt = 0) {
    const EngDev &d = c.d;
    if (e->cfg.evaluator == AZ_EVAL_EXTERNAL) return forward_external(e, cnt, cap, step);
    if (e->cfg.evaluator == AZ_EVAL_FAKE) {
        hipLaunchKernelGGL(k_fakenet, grid_for((c.g1 - c.g0) * d.K, TB), dim3(TB), 0, c.st, d, cnt);
        return AZ_OK;
    }
    if (e->symr_mask != 0) {  // one drawn member per pending row: twin -> the network on the same rows -> mapped back (copies)
        hipLaunchKernelGGL(k_sym_pick, dim3((unsigned)((d.G + GPB - 1) / GPB)), dim3(256), 0, e->stream, d, e->symr_mask, e->symr_n, step, kt, e->sym_in,
                           e->sym_code);
        AZ_HIP(hipGetLastError());
        AZ_TRY(az_net_forward_dyn(e->net, e->sym_in, cnt, cap, e->sym_p, e->sym_v, e->stream));
        return az_sym_unpick(&d.gd, e->sym_code, e->sym_p, e->sym_v, cnt, cap, d.probs, d.value, e->stream);
    }
    // k_step_heads follows a lock-step's forward: the forward stops behind fc2 (the root-prior pass keeps its heads: k_root_init reads them)
    if (d.sh_h2 && step >= 0) return az_net_forward_lane_fc2(e->net, c.idx, c.beside ? 1 : 0, d.nn_in, cnt, cap, c.st);
    if (e->sym_mask == 0) return az_net_forward_lane(e->net, c.idx, c.beside ? 1 : 0, d.nn_in, cnt, cap, d.probs, d.value, c.st);
    // ensemble over the board's symmetries: twins of the pending rows -> the network on sym_n * count rows -> mapped back and averaged
    AZ_TRY(az_sym_expand(&d.gd, e->sym_mask, d.nn_in, cnt, cap, e->sym_in, e->sym_cnt, e->stream));
    AZ_TRY(az_net_forward_dyn(e->net, e->sym_in, e->sym_cnt, e->sym_n * cap, e->sym_p, e->sym_v, e->stream));
    return az_sym_reduce(&d.gd, e->sym_mask, e->sym_p, e->sym_v, cnt, cap, d.probs, d.value, e->stream);
}

// az_engine_set_puct: the exploration settings are anything but the neutral (1.0, 0, off)
static bool puct_on(const EngDev &d) { return !puct_neutral(d.puct_cinit, d.puct_cbase, d.puct_fpu); }
static SearchMode search_mode(const EngDev &d) { return SearchMode{d.rollout != 0, d.gm, d.K, d.nval != nullptr, d.budget != nullptr, d.kforced > 0.0, d.exact_max, d.pf != nullptr, puct_on(d)}; }

// The one place that names the step kernels: launch `a` of the plan on chain c.  Each family is instantiated for three (backup, select)
// pairs -- the first step, the later ones, the last backup; never <false, false> -- and the two Gumbel families for `full` on and off.
// (the kernels without a slot range -- rollout, K walkers -- run as the whole engine's chain only: g0 = 0, g1 = G)
template <bool B, bool S>
static void launch_step_as(const SearchPlan &p, const Chain &c, int n_sim, const StepArgs &a) {
    const EngDev &d = c.d;
    const dim3 gg((unsigned)((c.g1 - c.g0 + GPB - 1) / GPB)), gb(256);
    switch (p.family) {
        case SF_ROLLOUT: hipLaunchKernelGGL(k_rollout_step, gg, gb, 0, c.st, d, a.t); break;
        // the four one-leaf families: with the evaluation cache's pointers set (az_engine_run alone sets them) their cached instantiation
        case SF_STEP:
            // with the heads' pointers set (az_engine_run alone sets them) the steps that hold a backup compute the heads themselves
            if (B && d.sh_h2) {
                if (d.sh_nt == 5) {
                    if (d.ec_hdr) hipLaunchKernelGGL((k_step_heads<S, true, 5>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
                    else hipLaunchKernelGGL((k_step_heads<S, false, 5>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
                } else {
                    if (d.ec_hdr) hipLaunchKernelGGL((k_step_heads<S, true, 3>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
                    else hipLaunchKernelGGL((k_step_heads<S, false, 3>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
                }
            }
            else if (d.ec_hdr) hipLaunchKernelGGL((k_step_cached<B, S, false, false>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            else hipLaunchKernelGGL((k_step<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            break;
        case SF_STEP_CAP:
            if (d.ec_hdr) hipLaunchKernelGGL((k_step_cached<B, S, true, false>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            else hipLaunchKernelGGL((k_step_cap<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            break;
        case SF_STEP_FORCED:
            if (d.ec_hdr) hipLaunchKernelGGL((k_step_cached<B, S, false, true>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            else hipLaunchKernelGGL((k_step_forced<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            break;
        case SF_STEP_CAP_FORCED:
            if (d.ec_hdr) hipLaunchKernelGGL((k_step_cached<B, S, true, true>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            else hipLaunchKernelGGL((k_step_cap_forced<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            break;
        case SF_STEP_EXACT:
            if (d.ec_hdr) hipLaunchKernelGGL((k_step_exact_cached<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            else hipLaunchKernelGGL((k_step_exact<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            break;
        case SF_STEP_PROOF:
            if (p.exact) {
                if (d.ec_hdr) hipLaunchKernelGGL((k_step_proof_exact_cached<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
                else hipLaunchKernelGGL((k_step_proof_exact<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            } else {
                if (d.ec_hdr) hipLaunchKernelGGL((k_step_proof_cached<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
                else hipLaunchKernelGGL((k_step_proof<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            }
            break;
        case SF_STEP_PUCT:
            if (d.ec_hdr) hipLaunchKernelGGL((k_step_puct_cached<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            else hipLaunchKernelGGL((k_step_puct<B, S>), gg, gb, 0, c.st, d, a.t, c.g0, c.g1);
            break;
        case SF_STEP_MULTI: hipLaunchKernelGGL((k_step_multi<B, S>), gg, gb, 0, c.st, d, a.t, a.kb, a.kt); break;
        case SF_STEP_GUMBEL:
            if (p.full) hipLaunchKernelGGL((k_step_gumbel<B, S, true>), gg, gb, 0, c.st, d, a.t, n_sim, c.g0, c.g1);
            else hipLaunchKernelGGL((k_step_gumbel<B, S, false>), gg, gb, 0, c.st, d, a.t, n_sim, c.g0, c.g1);
            break;
        case SF_STEP_GUMBEL_MULTI:
            if (p.full) hipLaunchKernelGGL((k_step_gumbel_multi<B, S, true>), gg, gb, 0, c.st, d, a.t, n_sim);
            else hipLaunchKernelGGL((k_step_gumbel_multi<B, S, false>), gg, gb, 0, c.st, d, a.t, n_sim);
            break;
    }
}
static void launch_step(const SearchPlan &p, const Chain &c, int n_sim, const StepArgs &a) {
    if (!a.backup) launch_step_as<false, true>(p, c, n_sim, a);
    else if (a.select) launch_step_as<true, true>(p, c, n_sim, a);
    else launch_step_as<true, false>(p, c, n_sim, a);
}

// MCT.search for every active slot: one root-prior pass (mcts.py:231-233; empty unless a slot holds a fresh root), then the plan's
// lock-steps of [backup+select -> network] and the last backup.
// the raw launch sequence of one search; `cap` bounds the network batch (leaf rows are compact: count <= searching slots)
static int enqueue_search(az_engine *e, const Chain &c, const SearchPlan &p, int n_sim, int cap) {
    const EngDev &d = c.d;
    if (p.root_pass) {
        const dim3 gg((unsigned)((c.g1 - c.g0 + GPB - 1) / GPB)), gb(256);
        hipLaunchKernelGGL(k_root_prep, gg, gb, 0, c.st, d, c.g0, c.g1);
        AZ_TRY(forward(e, c, d.batch_cnt + 2, cap, -1));
        hipLaunchKernelGGL(k_root_init, gg, gb, 0, c.st, d, c.g0, c.g1);
    }
    for (int t = 0; t < p.launches; ++t) {
        const StepArgs a = plan_step(p, n_sim, d.K, t);
        launch_step(p, c, n_sim, a);
        if (a.select) AZ_TRY(forward(e, c, d.batch_cnt + a.ctr, cap, a.t, a.kt));
    }
    AZ_HIP(hipGetLastError());
    return AZ_OK;
}

// queues one search on chain c (null: the whole engine on its stream; a slot group's chain: one search per root, sim_base 0)
static int do_search(az_engine *e, int n_sim, const Chain *grp = nullptr) {
    AZ_REQUIRE(e->cfg.evaluator != AZ_EVAL_EXTERNAL || e->ext_fn, AZ_ESTATE, "AZ_EVAL_EXTERNAL engine without an evaluator (az_engine_set_evaluator)");
    if (!grp) {
        e->d.sim_base = e->sim_base;
        e->sim_base += (u32)n_sim;
    }
    const Chain whole = whole_chain(e);
    const Chain &c = grp ? *grp : whole;
    const EngDev &d = c.d;
    const SearchPlan plan = plan_search(search_mode(d), n_sim);
    e->lockstep_iters[c.idx] += plan.launches;
    // network rows: every searching slot brings up to K leaves per lock-step (K = 1 unless az_engine_set_leaf_batch / _set_gumbel_batch)
    // (a group takes its own live count, not active_bound: the shared counters behind that are moving while another group plays its ply)
    const int W = c.g1 - c.g0;
    int cap = search_batch_cap(W, d.K, grp ? grp->live : e->active_bound);
    // graph replay needs launch parameters that do not change from search to search: the Philox counter base must be 0
    // (one search per root, as in self-play and the arena), no per-launch event recording, and a quantised batch cap
    const bool profiled = e->net && az_net_profiling(e->net);
    const bool graphable = e->graphs_ok && d.sim_base == 0 && !profiled && e->cfg.evaluator != AZ_EVAL_EXTERNAL;
    // the quantised cap of the graph path also when the search runs as plain launches under az_net_profile: the profiled step then
    // launches the kernels the timed (graph-replayed) steps launch
    if (graphable || (profiled && d.sim_base == 0)) cap = quantised_cap(W * d.K, cap);
    if (!graphable) return enqueue_search(e, c, plan, n_sim, cap);
    // another family, or the full instantiation of a Gumbel one, launches other kernels: the key keeps their graphs apart
    // (and a captured search holds the evaluation cache's pointers, or null ones, by value: one with the other setting replays none of them)
    if ((d.ec_hdr != nullptr) != e->graphs_ec) { drop_graphs(e); e->graphs_ec = d.ec_hdr != nullptr; }
    // and the heads' pointers of k_step_heads, or null ones: the lane's rows move with az_net_set_lanes, the form goes with the switch
    {
        const void **have = e->graphs_sh[c.idx];
        if (have[0] != d.sh_h2 || have[1] != d.sh_wq || have[2] != d.sh_hb) {
            drop_graphs(e);
            have[0] = d.sh_h2; have[1] = d.sh_wq; have[2] = d.sh_hb;
        }
    }
    const SearchKey key = search_key(plan, n_sim, cap, c.g0, c.g1);
    auto it = e->graphs.find(key);
    if (it != e->graphs.end()) {
        AZ_HIP(hipGraphLaunch(it->second, c.st));
        e->graph_replays++;
        return AZ_OK;
    }
    if (e->graph_seen[key]++ == 0) return enqueue_search(e, c, plan, n_sim, cap);  // first time: plain launches (kernel attributes get set)
    hipGraph_t g = nullptr;
    hipGraphExec_t ex = nullptr;
    if (hipStreamBeginCapture(c.st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        e->graphs_ok = false;
        return enqueue_search(e, c, plan, n_sim, cap);
    }
    const int rc = enqueue_search(e, c, plan, n_sim, cap);  // recorded, not executed
    const hipError_t er = hipStreamEndCapture(c.st, &g);
    if (rc != AZ_OK || er != hipSuccess || hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        e->graphs_ok = false;
        return enqueue_search(e, c, plan, n_sim, cap);
    }
    (void)hipGraphDestroy(g);
    e->graphs[key] = ex;
    AZ_HIP(hipGraphLaunch(ex, c.st));
    e->graph_replays++;
    return AZ_OK;
}

// orders the engine's stream behind whatever the caller has queued on the stream it handed to az_engine_create
static int enter(az_engine *e) {
    AZ_HIP(hipEventRecord(e->ev_in, e->user_stream));
    AZ_HIP(hipStreamWaitEvent(e->stream, e->ev_in, 0));
    return AZ_OK;
}

// set_roots / run reset every slot: the trees hold no unevaluated leaf any more
static int reset_external(az_engine *e) {
    e->unevaluated = false;
    if (e->ext_bad) AZ_HIP(hipMemsetAsync(e->ext_bad, 0x7f, sizeof(int), e->stream));
    return AZ_OK;
}

// the shared counters and error words, read behind everything queued on the chain's stream (null: the engine's) into the chain's own
// host copy; a slot group also reads its live word
static int fetch_counters(az_engine *e, const Chain *grp) {
    const int idx = grp ? grp->idx : 0;
    hipStream_t st = grp ? grp->st : e->stream;
    int *he = e->h_err + 4 * idx;
    AZ_HIP(hipMemcpyAsync(e->h_ctr + (size_t)CTR_ALLOC * idx, e->d.ctr, sizeof(unsigned long long) * CTR_ALLOC, hipMemcpyDeviceToHost, st));
    AZ_HIP(hipMemcpyAsync(&he[0], e->d.err, sizeof(int), hipMemcpyDeviceToHost, st));
    AZ_HIP(hipMemcpyAsync(&he[1], e->d.max_nodes, sizeof(int), hipMemcpyDeviceToHost, st));
    AZ_HIP(hipMemcpyAsync(&he[2], e->d.max_path, sizeof(int), hipMemcpyDeviceToHost, st));
    if (grp) {  // queued only: the host loop of az_engine_run waits for the group when its turn comes
        AZ_HIP(hipMemcpyAsync(&he[3], grp->d.live, sizeof(int), hipMemcpyDeviceToHost, st));
        return AZ_OK;
    }
    AZ_HIP(hipStreamSynchronize(st));
    return AZ_OK;
}

static int check_err(az_engine *e, int idx) {
    int f = e->h_err[4 * idx];
    if (f & ERR_EVAL) {  // first: the rejected rows were consumed by the step that followed
        e->unevaluated = true;
        int slot = -1;
        AZ_HIP(hipMemcpy(&slot, e->ext_bad, sizeof(int), hipMemcpyDeviceToHost));
        az_set_error("external evaluator: a prior that is negative or not finite, or a value that is not finite, for slot %d", slot);
        return AZ_EINVAL;
    }
    if (f & ERR_NODE_POOL) { az_set_error("tree node pool exhausted (node_capacity=%d)", e->cfg.node_capacity); return AZ_ECAPACITY; }
    if (f & ERR_SAMPLE_CAP) { az_set_error("sample buffer exhausted (sample_capacity=%lld)", (long long)e->cfg.sample_capacity); return AZ_ECAPACITY; }
    if (f & ERR_PLY_CAP) { az_set_error("game longer than max_plies=%d", e->cfg.max_plies); return AZ_ECAPACITY; }
    if (f & ERR_RNG) { az_set_error("Dirichlet noise: the Gamma rejection sampler did not accept within 64 attempts"); return AZ_ESTATE; }
    if (f & ERR_INTERNAL) { az_set_error("internal tree invariant violated (no selectable child: NaN priors or values?)"); return AZ_ESTATE; }
    return AZ_OK;
}

// ---- the modes served in the plain search only: slot groups, the playout cap, forced playouts -----------------------------------------
// The mode of this engine that leaves the plain PUCT search of a network or fake engine, or null.  Slot groups, the playout cap and
// forced playouts are served in that search only: their kernels are k_step's family, one leaf per slot and lock-step.  (For the groups
// besides: the external evaluator's export buffers and the symmetry modes' twin rows are per engine, a rollout engine has no network to
// overlap with, and the kernels of leaf_batch > 1 and of the Gumbel search take no slot range.)
static const char *beyond_plain_search(const az_engine *e) {
    if (e->cfg.evaluator == AZ_EVAL_EXTERNAL) return "an AZ_EVAL_EXTERNAL engine (external evaluator)";
    if (e->cfg.evaluator == AZ_EVAL_ROLLOUT) return "a rollout engine (AZ_EVAL_ROLLOUT)";
    if (e->sym_mask != 0) return "the symmetry ensemble (az_engine_set_symmetry)";
    if (e->symr_mask != 0) return "the random symmetry mode (az_engine_set_symmetry_random)";
    if (e->leaf_batch > 1) return "leaf_batch > 1 (az_engine_set_leaf_batch)";
    if (e->d.gm > 0) return "the Gumbel search (az_engine_set_gumbel)";
    return nullptr;
}

// the other way round: what the setter `who` of such a mode answers while the playout cap or forced playouts are on (`where`: what
// the mode would leave)
static int refuse_beside_cap_or_forced(const az_engine *e, const char *who, const char *where) {
    const EngDev &d = e->d;
    AZ_REQUIRE(d.cap_nfast == 0, AZ_EINVAL, "%s: the playout cap is on (az_engine_set_playout_cap, n_fast = %d) and is served %s only; switch it off first", who, d.cap_nfast, where);
    AZ_REQUIRE(d.kforced == 0.0, AZ_EINVAL, "%s: forced playouts are on (az_engine_set_forced_playouts, k = %g) and are served %s only; switch them off first", who, d.kforced, where);
    AZ_REQUIRE(d.exact_max == 0, AZ_EINVAL, "%s: exact endgames are on (az_engine_set_exact_endgame, max_empties = %d) and are served %s only; switch them off first", who, d.exact_max, where);
    AZ_REQUIRE(!d.pf, AZ_EINVAL, "%s: proof backup is on (az_engine_set_proof_backup) and is served %s only; switch it off first", who, where);
    AZ_REQUIRE(!puct_on(d), AZ_EINVAL, "%s: PUCT exploration settings are on (az_engine_set_puct, c_init = %g, c_base = %g, fpu = %g) and are served %s only; switch them off first", who, d.puct_cinit, d.puct_cbase, d.puct_fpu, where);
    return AZ_OK;
}

// ---- slot groups (az_engine_set_groups) ---------------------------------------------------------------------------------------
// groups of the next az_engine_run: the request (auto: the rule) where the mode is served and every group holds a block of slots
static int groups_in_force(const az_engine *e) {
    if (beyond_plain_search(e)) return 1;
    if (e->net && az_net_profiling(e->net)) return 1;  // the profiled run is today's launch sequence: full-width, un-overlapped kernels
    const int n = e->groups_req > 0 ? e->groups_req : groups_auto(e->cfg.evaluator, e->cfg.game, e->cfg.H, e->cfg.W, e->d.G);
    return e->d.G > GPB ? n : 1;  // a group is whole blocks of slots (group_range)
}

extern "C" int az_engine_set_groups(az_engine *e, int32_t n) {
    AZ_SETTER(e, "az_engine_set_groups");
    AZ_REQUIRE(n == 0 || n == 1 || n == 2 || n == 4, AZ_EINVAL, "az_engine_set_groups: %d groups (0 = auto, 1, 2 or 4)", n);
    const char *why = beyond_plain_search(e);
    AZ_REQUIRE(n <= 1 || !why, AZ_EINVAL, "az_engine_set_groups: %d slot groups are not served for %s", n, why);
    AZ_REQUIRE(n <= 1 || e->d.G > GPB, AZ_EINVAL, "az_engine_set_groups: %d groups of %d slots: a group is whole blocks of %d slots, this engine is less than a block to split", n, e->d.G, GPB);
    if (n == e->groups_req && !e->groups_env) return AZ_OK;
    AZ_TRY(enter(e));
    AZ_HIP(hipStreamSynchronize(e->stream));
    e->groups_req = n; e->groups_env = false;
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_groups(az_engine *e, int32_t *n) {
    AZ_REQUIRE(e && n, AZ_EINVAL, "null argument");
    *n = groups_in_force(e);
    return AZ_OK;
}

// group i of n: slots [g0, g1) in whole blocks, the group's stream, rows [g0, g1) of the network batch, counters 4 i .. and live word i
static int make_chain(az_engine *e, int i, int n, Chain *c) {
    const EngDev &d = e->d;
    int g0 = 0, g1 = 0;
    group_range(d.G, i, n, &g0, &g1);
    if (i > 0 && !e->gstream[i]) {  // from the other priority pool (az_engine_pair): streams of one priority may share a hardware queue
        int least = 0, greatest = 0;
        AZ_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        AZ_HIP(hipStreamCreateWithPriority(&e->gstream[i], hipStreamNonBlocking, greatest));
    }
    c->d = d; c->g0 = g0; c->g1 = g1; c->idx = i; c->st = i == 0 ? e->stream : e->gstream[i]; c->beside = true; c->live = 0;
    c->d.sim_base = 0;
    c->d.nn_in = d.nn_in + (size_t)g0 * d.gd.cells; c->d.probs = d.probs + (size_t)g0 * d.A; c->d.value = d.value + g0;
    c->d.batch_cnt = d.batch_cnt + 4 * i; c->d.live = d.live + i;
    // the group's own evaluation cache: the two groups' kernels are not ordered against each other, a table's producers and consumers are
    if (d.ec_hdr) { c->d.ec_hdr = e->ec_hdr[i]; c->d.ec_pay = e->ec_pay[i]; c->d.ec_serial = e->ec_serial + i; }
    return AZ_OK;
}

// one ply of a slot group: the search, the move, the re-root, and the counters on their way to the host
static int issue_ply(az_engine *e, const Chain &c) {
    AZ_TRY(do_search(e, e->cfg.n_sim, &c));
    AZ_HIP(hipMemsetAsync(c.d.live, 0, sizeof(int), c.st));
    hipLaunchKernelGGL(k_move, grid_for(c.g1 - c.g0, TB), dim3(TB), 0, c.st, c.d, c.g0, c.g1);
    launch_reroot(c);
    return fetch_counters(e, &c);
}

// az_engine_run as n slot groups.  The groups' chains are independent (what they share is touched by atomics or disjoint by slot), so
// each runs on its own stream and the host keeps one ply queued per group: wait for the oldest, read its counters, queue its next.
// A group without a live slot has nothing left to do -- only a slot's own finished game is refilled -- and is retired.
static int run_grouped(az_engine *e, int n, int32_t n_games, long long max_iters) {
    Chain ch[AZ_MAX_GROUPS];
    bool open[AZ_MAX_GROUPS] = {false, false, false, false};
    if (!e->ev_grp) AZ_HIP(hipEventCreateWithFlags(&e->ev_grp, hipEventDisableTiming));
    int widest = 0;
    for (int i = 0; i < n; ++i) {
        AZ_TRY(make_chain(e, i, n, &ch[i]));
        widest = ch[i].g1 - ch[i].g0 > widest ? ch[i].g1 - ch[i].g0 : widest;
    }
    if (e->cfg.evaluator == AZ_EVAL_NET) AZ_TRY(az_net_set_lanes(e->net, n, widest));
    if (e->d.sh_h2)  // k_step_heads reads the fc2 rows of its own chain's lane (they exist from here on)
        for (int i = 0; i < n; ++i) AZ_TRY(az_net_heads_view(e->net, i, &ch[i].d.sh_h2, nullptr, nullptr, nullptr, nullptr));
    AZ_HIP(hipEventRecord(e->ev_grp, e->stream));  // behind k_reset_all
    int rc = AZ_OK, n_open = 0;
    for (int i = 0; i < n && rc == AZ_OK; ++i) {
        if (i > 0) AZ_HIP(hipStreamWaitEvent(ch[i].st, e->ev_grp, 0));
        const int first = n_games - ch[i].g0;  // k_reset_all seats games 0 .. in slots 0 ..
        ch[i].live = first < 0 ? 0 : (first < ch[i].g1 - ch[i].g0 ? first : ch[i].g1 - ch[i].g0);
        if (ch[i].live == 0) continue;
        rc = issue_ply(e, ch[i]);
        open[i] = rc == AZ_OK;
        n_open += open[i] ? 1 : 0;
    }
    bool done = false;
    for (long long it = 0; rc == AZ_OK && n_open > 0 && !done; ++it) {
        if (it >= max_iters) { az_set_error("self-play did not finish within %lld plies", max_iters); rc = AZ_ESTATE; break; }
        for (int i = 0; i < n && rc == AZ_OK && !done; ++i) {
            if (!open[i]) continue;
            if (hipStreamSynchronize(ch[i].st) != hipSuccess) { az_set_error("HIP error: slot group %d: %s", i, hipGetErrorString(hipGetLastError())); rc = AZ_EHIP; break; }
            rc = check_err(e, i);
            if (rc != AZ_OK) break;
            ch[i].live = e->h_err[4 * i + 3];
            if (e->h_ctr[(size_t)CTR_ALLOC * i + CTR_GAMES_DONE] >= (unsigned long long)n_games) { done = true; break; }
            if (ch[i].live == 0) { open[i] = false; --n_open; continue; }
            rc = issue_ply(e, ch[i]);
        }
    }
    // nothing of any group may be in flight when the call returns, whatever ended it (a ply queued by a group that did not see the
    // last game end plays on empty slots)
    for (int i = 0; i < n; ++i) (void)hipStreamSynchronize(ch[i].st);
    if (rc != AZ_OK) return rc;
    AZ_TRY(fetch_counters(e));  // the final words, as every later reader expects them (slot 0 of the host copies)
    AZ_TRY(check_err(e));
    if (e->h_ctr[CTR_GAMES_DONE] >= (unsigned long long)n_games) return AZ_OK;
    az_set_error("self-play: every slot group is empty and %llu of %d games are done", e->h_ctr[CTR_GAMES_DONE], (int)n_games);
    return AZ_ESTATE;
}

// ---- leaf evaluation cache (az_engine_set_eval_cache) -----------------------------------------------------------
// whether the next az_engine_run caches: the request (auto: the rule) where the cache is served
static bool eval_cache_on(const az_engine *e) {
    return eval_cache_in_force(e->ec_req, e->cfg.evaluator, e->cfg.game, e->cfg.H, e->cfg.W, e->d.G, beyond_plain_search(e) != nullptr,
                               e->net && az_net_profiling(e->net));
}

// A run that caches: the tables of its n slot groups (allocated at their first use), cleared on the engine's stream -- every group's
// stream is ordered behind it (ev_grp) -- and the engine's device view pointing at group 0's until the run returns (ec_detach).
static int ec_attach(az_engine *e, int n) {
    EngDev &d = e->d;
    const size_t cap = (size_t)e->ec_capacity, stride = (size_t)ec_stride(d.A);
    if (!e->ec_serial) AZ_TRY(dev_alloc(e, &e->ec_serial, (size_t)AZ_MAX_GROUPS));
    if (!e->ec_claim) AZ_TRY(dev_alloc(e, &e->ec_claim, (size_t)d.G));
    if (!e->ec_hits) AZ_TRY(dev_alloc(e, &e->ec_hits, (size_t)d.G));
    for (int i = 0; i < n; ++i) {
        if (!e->ec_hdr[i]) AZ_HIP(hipMalloc((void **)&e->ec_hdr[i], cap * sizeof(EcHdr)));
        if (!e->ec_pay[i]) AZ_HIP(hipMalloc((void **)&e->ec_pay[i], cap * stride * sizeof(float)));
        AZ_HIP(hipMemsetAsync(e->ec_hdr[i], 0, cap * sizeof(EcHdr), e->stream));  // the tags (0 = empty) with their keys
    }
    AZ_HIP(hipMemsetAsync(e->ec_serial, 0, sizeof(u32) * AZ_MAX_GROUPS, e->stream));
    AZ_HIP(hipMemsetAsync(e->ec_hits, 0, sizeof(int) * (size_t)d.G, e->stream));
    d.ec_hdr = e->ec_hdr[0]; d.ec_pay = e->ec_pay[0]; d.ec_serial = e->ec_serial; d.ec_claim = e->ec_claim; d.ec_hits = e->ec_hits;
    d.ec_mask = (u32)cap - 1u; d.ec_limit = e->ec_limit; d.ec_stride = (int)stride;
    return AZ_OK;
}
static void ec_detach(az_engine *e) {
    EngDev &d = e->d;
    d.ec_hdr = nullptr; d.ec_pay = nullptr; d.ec_serial = nullptr; d.ec_claim = nullptr; d.ec_hits = nullptr;
    d.ec_mask = 0; d.ec_limit = 0; d.ec_stride = 0;
}

// ---- the heads inside the step kernel (k_step_heads) ---------------------------------------------------------------
// whether the next az_engine_run computes the heads in its step kernels: the request (unset: the rule) where the form is served
static bool step_heads_on(const az_engine *e) {
    const EngDev &d = e->d;
    int nh = 0, f2 = 0;
    const bool shape = e->cfg.evaluator == AZ_EVAL_NET && e->net && az_net_heads_view(e->net, 0, nullptr, nullptr, nullptr, &nh, &f2) == AZ_OK;
    const SearchMode m = search_mode(d);
    const bool plain = beyond_plain_search(e) == nullptr && !m.cap && !m.forced && m.exact == 0 && !m.proof && !m.puct;
    return step_heads_in_force(e->sh_req, e->cfg.evaluator, e->cfg.game, e->cfg.H, e->cfg.W, d.G, plain, shape, e->net && az_net_profiling(e->net));
}
// a run in that form: the engine's device view points at lane 0's rows and the net's head weights until the run returns (sh_detach)
static int sh_attach(az_engine *e) {
    EngDev &d = e->d;
    int nh = 0, f2 = 0;
    AZ_TRY(az_net_heads_view(e->net, 0, &d.sh_h2, &d.sh_wq, &d.sh_hb, &nh, &f2));
    d.sh_nt = nh / 16;
    return AZ_OK;
}
static void sh_detach(az_engine *e) {
    EngDev &d = e->d;
    d.sh_h2 = nullptr; d.sh_wq = nullptr; d.sh_hb = nullptr; d.sh_nt = 0;
}

// ---- resignation in self-play (k_move) ------------------------------------------------------------------------------
// A run with the mode on: the game log for its n_games (grown when this run has more games than any before; the engine's stream is
// idle here, every entry point drains it before it returns), cleared on the engine's stream -- k_reset_all follows on it and every
// group's stream is ordered behind that -- and the engine's device view pointing at the windows and the log until the run returns
// (rs_detach).  With the mode off the log is empty.
static int rs_attach(az_engine *e, int32_t n_games) {
    EngDev &d = e->d;
    e->gl_n = 0;
    if (e->rs.rs_k == 0) return AZ_OK;
    if (e->gl_cap < n_games) {
        AZ_HIP(hipStreamSynchronize(e->stream));
        if (e->gl_rows) { (void)hipFree(e->gl_rows); e->gl_rows = nullptr; }
        if (e->gl_low) { (void)hipFree(e->gl_low); e->gl_low = nullptr; }
        e->gl_cap = 0;
        AZ_HIP(hipMalloc((void **)&e->gl_rows, (size_t)n_games * 8 * sizeof(int)));
        AZ_HIP(hipMalloc((void **)&e->gl_low, (size_t)n_games * 2 * sizeof(double)));
        e->gl_cap = n_games;
    }
    AZ_HIP(hipMemsetAsync(e->gl_rows, 0, (size_t)n_games * 8 * sizeof(int), e->stream));
    AZ_HIP(hipMemsetAsync(e->gl_low, 0, (size_t)n_games * 2 * sizeof(double), e->stream));
    e->gl_n = n_games;
    e->rs.rs_win = e->rs_win; e->rs.rs_cnt = e->rs_cnt; e->rs.gl_rows = e->gl_rows; e->rs.gl_low = e->gl_low; e->rs.gl_n = n_games;
    AZ_HIP(hipMemcpy(e->rs_dev, &e->rs, sizeof(ResignDev), hipMemcpyHostToDevice));  // blocking: k_reset_all is launched after it
    d.rs = e->rs_dev;
    return AZ_OK;
}
static void rs_detach(az_engine *e) {
    EngDev &d = e->d;
    d.rs = nullptr;
}

static int run_games(az_engine *e, uint32_t first_game_id, int32_t n_games);

extern "C" int az_engine_run(az_engine *e, uint32_t first_game_id, int32_t n_games) {
    AZ_REQUIRE(e && n_games > 0, AZ_EINVAL, "bad arguments");
    AZ_NO_OPEN_SEARCH(e, "az_engine_run");
    AZ_NOT_IN_CALLBACK(e, "az_engine_run");
    const int rc = run_games(e, first_game_id, n_games);
    ec_detach(e);
    sh_detach(e);
    rs_detach(e);
    return rc;
}

static int run_games(az_engine *e, uint32_t first_game_id, int32_t n_games) {
    AZ_TRY(enter(e));
    EngDev &d = e->d;
    AZ_TRY(reset_external(e));
    for (int i = 0; i < AZ_MAX_GROUPS; ++i) e->lockstep_iters[i] = 0;
    const int n_groups = groups_in_force(e);
    if (e->groups_req > 1 && !e->groups_env && n_groups == 1 && beyond_plain_search(e)) {
        az_set_error("az_engine_run: %d slot groups were asked for (az_engine_set_groups) and are not served for %s", e->groups_req, beyond_plain_search(e));
        return AZ_EINVAL;
    }
    if (e->ec_req == AZ_EVAL_CACHE_ON && !e->ec_env && beyond_plain_search(e)) {
        az_set_error("az_engine_run: the evaluation cache was asked for (az_engine_set_eval_cache) and is not served for %s", beyond_plain_search(e));
        return AZ_EINVAL;
    }
    if (eval_cache_on(e)) AZ_TRY(ec_attach(e, n_groups));
    e->sh_used = step_heads_on(e);
    if (e->sh_used) AZ_TRY(sh_attach(e));
    AZ_TRY(rs_attach(e, n_games));
    hipLaunchKernelGGL(k_reset_all, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, (u32)first_game_id, (int)n_games);
    long long max_iters = ((long long)n_games / d.G + 2) * (long long)d.max_plies + 8;
    e->active_bound = n_games < d.G ? n_games : d.G;
    if (n_groups > 1) return run_grouped(e, n_groups, n_games, max_iters);
    const Chain whole = whole_chain(e);
    for (long long it = 0; it < max_iters; ++it) {
        e->sim_base = 0;
        AZ_TRY(do_search(e, e->cfg.n_sim));
        hipLaunchKernelGGL(k_move, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, 0, d.G);
        launch_reroot(whole);
        AZ_TRY(fetch_counters(e));
        AZ_TRY(check_err(e));
        if (e->h_ctr[CTR_GAMES_DONE] >= (unsigned long long)n_games) return AZ_OK;
        {
            unsigned long long started = e->h_ctr[CTR_NEXT_GAME] < e->h_ctr[CTR_TOTAL_GAMES] ? e->h_ctr[CTR_NEXT_GAME] : e->h_ctr[CTR_TOTAL_GAMES];
            e->active_bound = (int)(started - e->h_ctr[CTR_GAMES_DONE]);
        }
    }
    az_set_error("self-play did not finish within %lld plies", max_iters);
    return AZ_ESTATE;
}

extern "C" int az_engine_get_stats(az_engine *e, az_engine_stats *out) {
    AZ_REQUIRE(e && out, AZ_EINVAL, "null argument");
    AZ_USABLE(e, "az_engine_get_stats");
    AZ_TRY(enter(e));
    AZ_TRY(fetch_counters(e));
    out->games_done = (int64_t)e->h_ctr[CTR_GAMES_DONE];
    long long s = (long long)e->h_ctr[CTR_SAMPLES];
    out->samples = s < e->cfg.sample_capacity ? s : e->cfg.sample_capacity;
    out->net_evals = (int64_t)e->h_ctr[CTR_NET_EVALS];
    out->plies = (int64_t)e->h_ctr[CTR_PLIES];
    out->lockstep_iters = 0;  // a ply's lock-steps once: the group that played the most plies
    for (int i = 0; i < AZ_MAX_GROUPS; ++i) out->lockstep_iters = e->lockstep_iters[i] > out->lockstep_iters ? e->lockstep_iters[i] : out->lockstep_iters;
    out->max_nodes_used = e->h_err[1];
    out->error_flags = e->h_err[0];
    out->graph_replays = e->graph_replays;
    out->max_path_len = e->h_err[2];
    out->reserved = 0;
    out->cache_hits = (int64_t)e->h_ctr[CTR_CACHE_HITS];
    return AZ_OK;
}

extern "C" int az_engine_samples(az_engine *e, int64_t *n_samples, const int8_t **d_states, const float **d_pis,
                                 const int8_t **d_zs, const int32_t **d_meta, const int32_t **d_visits) {
    AZ_REQUIRE(e && n_samples, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_samples");
    AZ_USABLE(e, "az_engine_samples");
    AZ_TRY(fetch_counters(e));
    long long s = (long long)e->h_ctr[CTR_SAMPLES];
    *n_samples = s < e->cfg.sample_capacity ? s : e->cfg.sample_capacity;
    if (d_states) *d_states = e->d.o_state;
    if (d_pis) *d_pis = e->d.o_pi;
    if (d_zs) *d_zs = e->d.o_z;
    if (d_meta) *d_meta = e->d.o_meta;
    if (d_visits) *d_visits = e->d.o_visits;
    return AZ_OK;
}

extern "C" int az_engine_set_roots(az_engine *e, const int8_t *h_grids, const int8_t *h_players, const uint32_t *h_game_ids,
                                   const int32_t *h_plies, int32_t n_roots) {
    AZ_REQUIRE(e && h_grids && h_players, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_set_roots");
    AZ_NOT_IN_CALLBACK(e, "az_engine_set_roots");
    e->sim_base = 0;
    EngDev &d = e->d;
    AZ_REQUIRE(n_roots > 0 && n_roots <= d.G, AZ_EINVAL, "n_roots must be in [1, n_slots]");
    AZ_TRY(enter(e));
    AZ_TRY(reset_external(e));
    e->active_bound = n_roots;
    hipLaunchKernelGGL(k_reset_all, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, 0u, (int)n_roots);
    std::vector<u64> p1(n_roots), m1(n_roots);
    std::vector<u32> gid(n_roots);
    std::vector<int> ply(n_roots);
    for (int i = 0; i < n_roots; ++i) {
        u64 a = 0, b = 0;
        for (int r = 0; r < d.gd.H; ++r)
            for (int c = 0; c < d.gd.W; ++c) {
                int v = h_grids[(size_t)i * d.gd.cells + r * d.gd.W + c];
                AZ_REQUIRE(v >= -1 && v <= 1, AZ_EINVAL, "grid values must be -1, 0 or 1");
                if (v > 0) a |= 1ULL << (r * 8 + c);
                if (v < 0) b |= 1ULL << (r * 8 + c);
            }
        AZ_REQUIRE(h_players[i] == 1 || h_players[i] == -1, AZ_EINVAL, "player must be +1 or -1");
        p1[i] = a; m1[i] = b;
        gid[i] = h_game_ids ? h_game_ids[i] : (u32)i;
        ply[i] = h_plies ? h_plies[i] : 0;
    }
    AZ_HIP(hipMemcpyAsync(d.root_p1, p1.data(), sizeof(u64) * n_roots, hipMemcpyHostToDevice, e->stream));
    AZ_HIP(hipMemcpyAsync(d.root_m1, m1.data(), sizeof(u64) * n_roots, hipMemcpyHostToDevice, e->stream));
    AZ_HIP(hipMemcpyAsync(d.root_player, h_players, n_roots, hipMemcpyHostToDevice, e->stream));
    AZ_HIP(hipMemcpyAsync(d.game_id, gid.data(), sizeof(u32) * n_roots, hipMemcpyHostToDevice, e->stream));
    AZ_HIP(hipMemcpyAsync(d.ply, ply.data(), sizeof(int) * n_roots, hipMemcpyHostToDevice, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

extern "C" int az_engine_search(az_engine *e, int32_t n_sim) {
    AZ_REQUIRE(e && n_sim > 0, AZ_EINVAL, "bad arguments");
    AZ_NO_OPEN_SEARCH(e, "az_engine_search");
    AZ_USABLE(e, "az_engine_search");
    AZ_TRY(enter(e));
    AZ_TRY(do_search(e, n_sim));
    AZ_TRY(fetch_counters(e));
    return check_err(e);
}

// az_engine_search in two halves: _begin queues the search on the engine's stream and returns, _end waits for it and reports its
// errors.  Between the two the caller may start the search of ANOTHER engine (the arena's two players think at the same time on
// disjoint slots: two latency-bound launch chains side by side); no other entry point of THIS engine may be called in between.
extern "C" int az_engine_search_begin(az_engine *e, int32_t n_sim) {
    AZ_REQUIRE(e && n_sim > 0, AZ_EINVAL, "bad arguments");
    AZ_REQUIRE(!e->search_open, AZ_ESTATE, "az_engine_search_begin: the previous search has not been ended");
    AZ_USABLE(e, "az_engine_search_begin");
    AZ_TRY(enter(e));
    AZ_TRY(do_search(e, n_sim));
    e->search_open = true;
    return AZ_OK;
}

extern "C" int az_engine_search_end(az_engine *e) {
    AZ_REQUIRE(e, AZ_EINVAL, "null argument");
    AZ_REQUIRE(e->search_open, AZ_ESTATE, "az_engine_search_end without az_engine_search_begin");
    AZ_USABLE(e, "az_engine_search_end");
    e->search_open = false;
    AZ_TRY(fetch_counters(e));
    return check_err(e);
}

// Two engines whose searches are to overlap (az_engine_search_begin on both) need streams on DIFFERENT hardware queues.  The HIP
// runtime deals its few hardware queues (four by default) out to streams of one priority in turn, so two streams of a process that
// has made others (torch's, a trainer's) may share a queue and then run strictly one after the other (measured: an arena inside
// the trainer's process gained nothing from the overlap).  Queues of different priorities come from different pools: `b` gets a
// new stream of the highest priority.  Call before b's first search.
extern "C" int az_engine_pair(az_engine *a, az_engine *b) {
    AZ_REQUIRE(a && b && a != b, AZ_EINVAL, "two different engines are needed");
    AZ_USABLE(a, "az_engine_pair");
    AZ_USABLE(b, "az_engine_pair");
    AZ_REQUIRE(!a->search_open && !b->search_open, AZ_ESTATE, "az_engine_pair: a search is open");
    AZ_REQUIRE(b->graphs.empty(), AZ_ESTATE, "az_engine_pair must come before the second engine's searches");
    int least = 0, greatest = 0;  // numerically lower = higher priority
    AZ_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (least == greatest) return AZ_OK;  // no priorities on this device: nothing to do
    hipStream_t s = nullptr;
    AZ_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest));
    AZ_HIP(hipStreamSynchronize(b->stream));
    (void)hipStreamDestroy(b->stream);
    b->stream = s;
    return AZ_OK;
}

extern "C" int az_engine_advance(az_engine *e) {
    AZ_REQUIRE(e, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_advance");
    AZ_USABLE(e, "az_engine_advance");
    e->sim_base = 0;
    EngDev &d = e->d;
    // games that end here must not be refilled: cap the queue at what has been started
    hipLaunchKernelGGL(k_move, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, 0, d.G);
    launch_reroot(whole_chain(e));
    AZ_TRY(fetch_counters(e));
    return check_err(e);
}

extern "C" int az_engine_root_children(az_engine *e, int32_t slot, int32_t *h_actions, int32_t *h_N, double *h_Q,
                                       double *h_P, int32_t *count, int32_t *root_N) {
    AZ_REQUIRE(e && count, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_root_children");
    AZ_USABLE(e, "az_engine_root_children");
    EngDev &d = e->d;
    AZ_REQUIRE(slot >= 0 && slot < d.G, AZ_EINVAL, "slot out of range");
    AZ_HIP(hipStreamSynchronize(e->stream));
    int root = 0;
    uint8_t sel = 0;
    AZ_HIP(hipMemcpy(&sel, d.pool_sel + slot, 1, hipMemcpyDeviceToHost));
    size_t base = ((size_t)slot * 2 + sel) * d.C;
    AZ_HIP(hipMemcpy(&root, d.root + slot, sizeof(int), hipMemcpyDeviceToHost));
    Node rn;
    AZ_HIP(hipMemcpy(&rn, d.nodes + base + root, sizeof(Node), hipMemcpyDeviceToHost));
    if (root_N) *root_N = rn.N;
    int nc = (rn.flags & F_EXPANDED) ? rn.nch : 0;  // children not materialised yet in the reference's tree
    *count = nc;
    if (nc == 0) return AZ_OK;
    std::vector<Node> ch(nc);
    AZ_HIP(hipMemcpy(ch.data(), d.nodes + base + rn.first, sizeof(Node) * nc, hipMemcpyDeviceToHost));
    for (int i = 0; i < nc; ++i) {
        if (h_actions) h_actions[i] = ch[i].act;
        if (h_N) h_N[i] = ch[i].N;
        if (h_Q) h_Q[i] = ch[i].Q;
        if (h_P) h_P[i] = ch[i].P;
    }
    return AZ_OK;
}

// Player.get_move's results (players.py:158-191; MCT.get_action_probs / get_prior_probs, mcts.py:95-116) for slots [0, n) at once:
// one launch of k_root_readout into the caller's device buffers, no per-slot host copy (az_engine_root_children is the one-slot form).
extern "C" int az_engine_root_readout(az_engine *e, const double *h_temps, int32_t n, const az_root_readout *out) {
    AZ_REQUIRE(e && out, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_root_readout");
    AZ_USABLE(e, "az_engine_root_readout");
    EngDev &d = e->d;
    AZ_REQUIRE(n >= 1 && n <= d.G, AZ_EINVAL, "n must be in [1, n_slots], got %d", n);
    AZ_REQUIRE(out->pv_len >= 0 && out->pv_len <= 16, AZ_EINVAL, "pv_len must be in [0, 16], got %d", out->pv_len);
    AZ_REQUIRE(!(out->d_pv && out->pv_len == 0), AZ_EINVAL, "d_pv given with pv_len 0");
    if (h_temps)
        for (int i = 0; i < n; ++i)
            AZ_REQUIRE(h_temps[i] >= 0.0 && h_temps[i] <= 1.7976931348623157e308, AZ_EINVAL,
                       "temperature of slot %d is negative or not finite (%g)", i, h_temps[i]);
    AZ_TRY(enter(e));
    if (h_temps) {
        if (!e->ro_temps) AZ_TRY(dev_alloc(e, &e->ro_temps, (size_t)d.G));
        AZ_HIP(hipMemcpyAsync(e->ro_temps, h_temps, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
    }
    RootOut o;
    o.visits = out->d_visits; o.pi = out->d_pi; o.Q = out->d_Q; o.P = out->d_P; o.child = out->d_child;
    o.action = out->d_action; o.root_N = out->d_root_N; o.pv = out->pv_len > 0 ? out->d_pv : nullptr; o.pv_len = out->pv_len;
    hipLaunchKernelGGL(k_root_readout, dim3((unsigned)((n + GPB - 1) / GPB)), dim3(256), 0, e->stream, d, (int)n,
                       (const double *)(h_temps ? e->ro_temps : nullptr), o);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

// Nodes the slot's live pool holds (bump allocator top): what a caller that keeps searching one root (MCT.search called again
// and again without a move, mcts.py:226-269) checks before the next search.
extern "C" int az_engine_nodes_used(az_engine *e, int32_t slot, int32_t *n_nodes) {
    AZ_REQUIRE(e && n_nodes, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_nodes_used");
    AZ_USABLE(e, "az_engine_nodes_used");
    AZ_REQUIRE(slot >= 0 && slot < e->d.G, AZ_EINVAL, "slot out of range");
    AZ_HIP(hipStreamSynchronize(e->stream));
    AZ_HIP(hipMemcpy(n_nodes, e->d.n_nodes + slot, sizeof(int), hipMemcpyDeviceToHost));
    return AZ_OK;
}

// Re-allocates the tree pools with `node_capacity` nodes each and moves every slot's trees over (node links are pool-relative).
// The reference's tree grows without bound; here the pools are sized per search and grown on demand by the single-game MCT.
extern "C" int az_engine_grow_pools(az_engine *e, int32_t node_capacity) {
    AZ_REQUIRE(e, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_grow_pools");
    AZ_USABLE(e, "az_engine_grow_pools");
    EngDev &d = e->d;
    AZ_REQUIRE(node_capacity >= d.C, AZ_EINVAL, "pools can only grow (%d < %d)", node_capacity, d.C);
    if (node_capacity == d.C) return AZ_OK;
    AZ_TRY(enter(e));
    const size_t rows = 2 * (size_t)d.G;
    Node *fresh = nullptr;
    AZ_HIP(hipMalloc((void **)&fresh, rows * (size_t)node_capacity * sizeof(Node)));
    hipError_t er = hipMemsetAsync(fresh, 0, rows * (size_t)node_capacity * sizeof(Node), e->stream);
    if (er == hipSuccess)
        er = hipMemcpy2DAsync(fresh, (size_t)node_capacity * sizeof(Node), d.nodes, (size_t)d.C * sizeof(Node), (size_t)d.C * sizeof(Node), rows,
                              hipMemcpyDeviceToDevice, e->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    float *fresh_v = nullptr;  // the stored network values (az_engine_set_gumbel_full) are laid out like the nodes and move with them
    if (er == hipSuccess && e->nval) {
        er = hipMalloc((void **)&fresh_v, rows * (size_t)node_capacity * sizeof(float));
        if (er == hipSuccess) er = hipMemsetAsync(fresh_v, 0, rows * (size_t)node_capacity * sizeof(float), e->stream);
        if (er == hipSuccess)
            er = hipMemcpy2DAsync(fresh_v, (size_t)node_capacity * sizeof(float), e->nval, (size_t)d.C * sizeof(float), (size_t)d.C * sizeof(float), rows,
                                  hipMemcpyDeviceToDevice, e->stream);
        if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    }
    if (er != hipSuccess) {
        (void)hipFree(fresh);
        if (fresh_v) (void)hipFree(fresh_v);
        az_set_error("growing the node pools failed: %s", hipGetErrorString(er));
        return AZ_EHIP;
    }
    for (auto &p : e->allocs) if (p == (void *)d.nodes) p = (void *)fresh;
    (void)hipFree(d.nodes);
    d.nodes = fresh;
    if (fresh_v) {
        for (auto &p : e->allocs) if (p == (void *)e->nval) p = (void *)fresh_v;
        (void)hipFree(e->nval);
        if (d.nval) d.nval = fresh_v;
        e->nval = fresh_v;
    }
    d.C = node_capacity;
    e->cfg.node_capacity = node_capacity;
    drop_graphs(e);  // captured searches hold the old pool pointer and capacity by value
    return AZ_OK;
}

extern "C" int az_engine_play(az_engine *e, const int32_t *h_actions, int32_t n, int32_t *h_status) {
    AZ_REQUIRE(e && h_actions && h_status, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_play");
    AZ_USABLE(e, "az_engine_play");
    e->sim_base = 0;
    EngDev &d = e->d;
    AZ_REQUIRE(n > 0 && n <= d.G, AZ_EINVAL, "n must be in [1, n_slots]");
    int *d_act = e->scr_a, *d_st = e->scr_b;
    AZ_HIP(hipMemcpyAsync(d_act, h_actions, sizeof(int) * n, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_apply_moves, grid_for(n, TB), dim3(TB), 0, e->stream, d, d_act, (int)n, d_st);
    launch_reroot(whole_chain(e));
    AZ_HIP(hipMemcpyAsync(h_status, d_st, sizeof(int) * n, hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n; ++i)
        if (h_status[i] == AZ_EILLEGAL) { az_set_error("Illegal move %d for slot %d", h_actions[i], i); return AZ_EILLEGAL; }
    AZ_TRY(fetch_counters(e));
    return check_err(e);
}

#ifdef AZ_PROBE
extern "C" int az_debug_read_step_probe(unsigned long long *h_out, int n_words) {
    AZ_HIP(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(az_step_probe), sizeof(unsigned long long) * (size_t)n_words));
    return AZ_OK;
}
#endif

// ---- arena support ---------------------------------------------------------------
extern "C" int az_engine_set_sides(az_engine *e, const int8_t *h_sides, int32_t n) {
    AZ_REQUIRE(e && h_sides && n > 0 && n <= e->d.G, AZ_EINVAL, "bad arguments");
    AZ_NO_OPEN_SEARCH(e, "az_engine_set_sides");
    AZ_USABLE(e, "az_engine_set_sides");
    AZ_HIP(hipMemcpyAsync(e->d.side, h_sides, (size_t)n, hipMemcpyHostToDevice, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

static int moves_out(az_engine *e, int32_t *h_actions, int which, int kind, uint32_t seed) {
    EngDev &d = e->d;
    int *d_act = e->scr_a;
    if (which == 0) hipLaunchKernelGGL(k_best_moves, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, d_act);
    else hipLaunchKernelGGL(k_baseline_moves, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, kind, (u32)seed, d_act);
    AZ_HIP(hipMemcpyAsync(h_actions, d_act, sizeof(int) * d.G, hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

extern "C" int az_engine_best_moves(az_engine *e, int32_t *h_actions) {
    AZ_REQUIRE(e && h_actions, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_best_moves");
    AZ_USABLE(e, "az_engine_best_moves");
    return moves_out(e, h_actions, 0, 0, 0);
}

// what az_engine_advance would play now at temperature `temp`, per slot, as host ints: d_action of az_engine_root_readout with every
// temperature `temp`, without its device rows (the arena's loop works on host int vectors)
extern "C" int az_engine_player_moves(az_engine *e, double temp, int32_t *h_actions) {
    AZ_REQUIRE(e && h_actions, AZ_EINVAL, "null argument");
    AZ_REQUIRE(temp >= 0.0 && temp <= 1.7976931348623157e308, AZ_EINVAL, "az_engine_player_moves: the temperature is negative or not finite (%g)", temp);
    AZ_NO_OPEN_SEARCH(e, "az_engine_player_moves");
    AZ_USABLE(e, "az_engine_player_moves");
    EngDev &d = e->d;
    int *d_act = e->scr_a;
    hipLaunchKernelGGL(k_player_moves, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, temp, d_act);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(h_actions, d_act, sizeof(int) * d.G, hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

extern "C" int az_engine_baseline_moves(az_engine *e, int32_t kind, uint32_t seed, int32_t *h_actions) {
    AZ_REQUIRE(e && h_actions && (kind == 0 || kind == 1), AZ_EINVAL, "bad arguments (kind: 0 random, 1 greedy)");
    AZ_NO_OPEN_SEARCH(e, "az_engine_baseline_moves");
    AZ_USABLE(e, "az_engine_baseline_moves");
    return moves_out(e, h_actions, 1, kind, seed);
}

extern "C" int az_engine_root_status(az_engine *e, int8_t *h_players, uint8_t *h_over, int8_t *h_winner, int32_t *h_score) {
    AZ_REQUIRE(e && h_players && h_over && h_winner && h_score, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_root_status");
    AZ_USABLE(e, "az_engine_root_status");
    EngDev &d = e->d;
    char *buf = e->scr_c;
    size_t G = d.G;
    int8_t *pl = (int8_t *)buf; uint8_t *ov = (uint8_t *)(buf + G); int8_t *wi = (int8_t *)(buf + 2 * G);
    int *sc = e->scr_a;
    hipLaunchKernelGGL(k_root_status, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, pl, ov, wi, sc);
    AZ_HIP(hipMemcpyAsync(h_players, pl, G, hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipMemcpyAsync(h_over, ov, G, hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipMemcpyAsync(h_winner, wi, G, hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipMemcpyAsync(h_score, sc, G * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

// ---- leaf evaluation over the board's symmetries (az_symmetry.hip; forward() above) --------------------------
// the scratch rows of both symmetry modes (twins, their outputs, the per-row codes); smaller ones stay allocated until the engine goes
static int sym_reserve(az_engine *e, int rows) {
    EngDev &d = e->d;
    if (rows <= e->sym_rows) return AZ_OK;
    AZ_TRY(dev_alloc(e, &e->sym_in, (size_t)rows * d.gd.cells));
    AZ_TRY(dev_alloc(e, &e->sym_p, (size_t)rows * d.A));
    AZ_TRY(dev_alloc(e, &e->sym_v, (size_t)rows));
    AZ_TRY(dev_alloc(e, &e->sym_code, (size_t)rows));
    if (!e->sym_cnt) AZ_TRY(dev_alloc(e, &e->sym_cnt, 1));
    AZ_HIP(hipStreamSynchronize(e->stream));
    e->sym_rows = rows;
    return AZ_OK;
}

static void drop_graphs(az_engine *e) {
    for (auto &kv : e->graphs) (void)hipGraphExecDestroy(kv.second);
    e->graphs.clear();
    e->graph_seen.clear();
}

extern "C" int az_engine_set_symmetry(az_engine *e, int32_t mask) {
    AZ_SETTER(e, "az_engine_set_symmetry");
    EngDev &d = e->d;
    AZ_REQUIRE(e->cfg.evaluator == AZ_EVAL_NET, AZ_EINVAL, "az_engine_set_symmetry needs an engine created with evaluator = AZ_EVAL_NET (this one: %d)",
               e->cfg.evaluator);
    int n = 0;
    AZ_TRY(az_sym_resolve(&d.gd, mask, &mask, &n));
    AZ_REQUIRE(mask == 0 || e->symr_mask == 0, AZ_EINVAL, "az_engine_set_symmetry: the engine draws one symmetry per evaluation (az_engine_set_symmetry_random, mask 0x%x); switch that mode off first", (unsigned)e->symr_mask);
    AZ_REQUIRE(mask == 0 || e->leaf_batch == 1, AZ_EINVAL, "az_engine_set_symmetry: the symmetry ensemble does not combine with leaf_batch %d > 1 (az_engine_set_leaf_batch)", e->leaf_batch);
    AZ_REQUIRE(mask == 0 || e->gumbel_batch == 1, AZ_EINVAL, "az_engine_set_symmetry: the symmetry ensemble does not combine with gumbel_batch %d > 1 (az_engine_set_gumbel_batch)", e->gumbel_batch);
    if (mask != 0) AZ_TRY(refuse_beside_cap_or_forced(e, "az_engine_set_symmetry", "in the plain search"));
    AZ_REQUIRE((long long)n * d.G <= az_net_max_batch(e->net), AZ_EINVAL,
               "%d symmetries of %d slots are %lld rows, the network's max_batch is %d", n, d.G, (long long)n * d.G, az_net_max_batch(e->net));
    if (mask == e->sym_mask) return AZ_OK;
    AZ_TRY(enter(e));
    AZ_TRY(sym_reserve(e, n * d.G));
    e->sym_mask = mask; e->sym_n = n;
    // the launch sequence of a search changes: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

// one member of `mask`, drawn per evaluation (k_sym_pick above): the rows of the plain search, so it composes with leaf_batch
extern "C" int az_engine_set_symmetry_random(az_engine *e, int32_t mask) {
    AZ_SETTER(e, "az_engine_set_symmetry_random");
    EngDev &d = e->d;
    AZ_REQUIRE(e->cfg.evaluator == AZ_EVAL_NET, AZ_EINVAL, "az_engine_set_symmetry_random needs an engine created with evaluator = AZ_EVAL_NET (this one: %d)",
               e->cfg.evaluator);
    int n = 0;
    AZ_TRY(az_sym_resolve(&d.gd, mask, &mask, &n));
    AZ_REQUIRE(mask == 0 || e->sym_mask == 0, AZ_EINVAL, "az_engine_set_symmetry_random: the engine averages over a symmetry mask (az_engine_set_symmetry, mask 0x%x); switch the ensemble off first", (unsigned)e->sym_mask);
    if (mask != 0) AZ_TRY(refuse_beside_cap_or_forced(e, "az_engine_set_symmetry_random", "in the plain search"));
    AZ_REQUIRE((long long)d.K * d.G <= az_net_max_batch(e->net), AZ_EINVAL,
               "leaf_batch %d of %d slots are %lld rows, the network's max_batch is %d", d.K, d.G, (long long)d.K * d.G, az_net_max_batch(e->net));
    if (mask == e->symr_mask) return AZ_OK;
    AZ_TRY(enter(e));
    if (mask != 0) AZ_TRY(sym_reserve(e, d.K * d.G));  // d.K: the walkers in force (leaf_batch, or gumbel_batch while the Gumbel mode is on)
    e->symr_mask = mask; e->symr_n = n;
    drop_graphs(e);
    return AZ_OK;
}

// ---- external evaluator (AZ_EVAL_EXTERNAL) ----------------------------------------------------------------
extern "C" int az_engine_set_evaluator(az_engine *e, az_eval_fn fn, void *user) {
    AZ_REQUIRE(e, AZ_EINVAL, "null argument");
    AZ_REQUIRE(e->cfg.evaluator == AZ_EVAL_EXTERNAL, AZ_EINVAL, "az_engine_set_evaluator: the engine was created with evaluator %d, not AZ_EVAL_EXTERNAL", e->cfg.evaluator);
    AZ_REQUIRE(!e->search_open, AZ_EINVAL, "az_engine_set_evaluator: a search begun with az_engine_search_begin has not been ended");
    AZ_USABLE(e, "az_engine_set_evaluator");
    e->ext_fn = fn;
    e->ext_user = user;
    return AZ_OK;
}

// ---- several leaves per slot and lock-step, kept apart by virtual loss (k_step_multi) --------------------------------
// K walkers per slot and lock-step come into force (az_engine_set_leaf_batch; az_engine_set_gumbel_batch while the Gumbel mode is on):
// the walkers' pending words at the first K > 1, K * G network rows, the twins of the random symmetry mode.  The caller has entered.
static int set_walkers(az_engine *e, int k) {
    EngDev &d = e->d;
    if (k == d.K) return AZ_OK;
    const long long rows = (long long)k * d.G;
    if (k > 1 && !d.m_leaf) {  // the walkers' pending leaves, at the first k > 1
        const size_t W = (size_t)d.G * MLB;
        AZ_TRY(dev_alloc(e, &d.m_leaf, W)); AZ_TRY(dev_alloc(e, &d.m_leaf_p1, W)); AZ_TRY(dev_alloc(e, &d.m_leaf_m1, W));
        AZ_TRY(dev_alloc(e, &d.m_leaf_player, W)); AZ_TRY(dev_alloc(e, &d.m_leaf_status, W)); AZ_TRY(dev_alloc(e, &d.m_leaf_winner, W));
        AZ_TRY(dev_alloc(e, &d.m_row, W)); AZ_TRY(dev_alloc(e, &d.m_path, W * LPG)); AZ_TRY(dev_alloc(e, &d.m_path_len, W));
    }
    if (rows > e->net_rows) {  // K * G rows for the network (the smaller buffers stay allocated until the engine goes: e->allocs)
        AZ_TRY(dev_alloc(e, &d.nn_in, (size_t)rows * d.gd.cells));
        AZ_TRY(dev_alloc(e, &d.probs, (size_t)rows * d.A));
        AZ_TRY(dev_alloc(e, &d.value, (size_t)rows));
        e->net_rows = (int)rows;
    }
    if (e->symr_mask != 0) AZ_TRY(sym_reserve(e, (int)rows));  // the twins of the random symmetry mode follow K * G
    AZ_HIP(hipStreamSynchronize(e->stream));
    d.K = k;
    // the launch sequence of a search changes: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_set_leaf_batch(az_engine *e, int32_t k) {
    AZ_SETTER(e, "az_engine_set_leaf_batch");
    EngDev &d = e->d;
    AZ_REQUIRE(k >= 1 && k <= AZ_MAX_LEAF_BATCH, AZ_EINVAL, "leaf_batch must be in [1, %d], got %d", AZ_MAX_LEAF_BATCH, k);
    AZ_REQUIRE(e->cfg.evaluator != AZ_EVAL_EXTERNAL, AZ_EINVAL, "az_engine_set_leaf_batch: an AZ_EVAL_EXTERNAL engine searches one leaf per lock-step (external evaluator)");
    AZ_REQUIRE(e->cfg.evaluator != AZ_EVAL_ROLLOUT, AZ_EINVAL, "az_engine_set_leaf_batch: a rollout engine (AZ_EVAL_ROLLOUT) evaluates no leaf with a network");
    AZ_REQUIRE(e->sym_mask == 0, AZ_EINVAL, "az_engine_set_leaf_batch: the engine evaluates over a symmetry mask (0x%x); the ensemble does not combine with leaf_batch", e->sym_mask);
    AZ_REQUIRE(k == 1 || d.gm == 0, AZ_EINVAL, "az_engine_set_leaf_batch: the Gumbel root search is on (az_engine_set_gumbel, m = %d) and searches one leaf per lock-step; switch it off first", d.gm);
    if (k > 1) AZ_TRY(refuse_beside_cap_or_forced(e, "az_engine_set_leaf_batch", "at one leaf per lock-step"));
    const long long rows = (long long)k * d.G;
    if (e->cfg.evaluator == AZ_EVAL_NET)
        AZ_REQUIRE(rows <= az_net_max_batch(e->net), AZ_EINVAL, "leaf_batch %d of %d slots are %lld rows, the network's max_batch is %d", k, d.G,
                   rows, az_net_max_batch(e->net));
    if (k == e->leaf_batch) return AZ_OK;
    AZ_TRY(enter(e));
    AZ_TRY(set_walkers(e, k));
    e->leaf_batch = k;
    return AZ_OK;
}

extern "C" int az_engine_collisions(az_engine *e, int64_t *n) {
    AZ_REQUIRE(e && n, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_collisions");
    AZ_USABLE(e, "az_engine_collisions");
    AZ_TRY(enter(e));
    AZ_TRY(fetch_counters(e));
    *n = (int64_t)e->h_ctr[CTR_COLLISIONS];
    return AZ_OK;
}

// ---- Gumbel root search (k_step_gumbel, gumbel_move_policy) -------------------------------------------------------------
// az_engine_set_gumbel_full comes into force (the switch goes on while the mode is on, or the mode with the switch on): from then on
// v_mix reads the stored value of every evaluated node it meets, so no active slot may hold a tree that was evaluated without
// storing.  A fresh root (not evaluated: after az_engine_set_roots, a reset slot of az_engine_run) has no such node.
__global__ void k_count_evaluated_roots(EngDev E, int *out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G || !E.active[g]) return;
    if (pool_of(E, g)[E.root[g]].flags & F_EVALUATED) atomicAdd(out, 1);
}

static int full_needs_fresh_roots(az_engine *e, const char *who) {
    EngDev &d = e->d;
    int n = 0;
    AZ_HIP(hipMemsetAsync(e->scr_a, 0, sizeof(int), e->stream));
    hipLaunchKernelGGL(k_count_evaluated_roots, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, e->scr_a);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(&n, e->scr_a, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    AZ_REQUIRE(n == 0, AZ_ESTATE, "%s: gumbel_full would come into force while %d active slot(s) hold evaluated nodes whose network value was "
               "never stored; start the trees afresh first (az_engine_set_roots / az_engine_run; Python: set_roots, reset)", who, n);
    return AZ_OK;
}

extern "C" int az_engine_set_gumbel(az_engine *e, int32_t m, double c_visit, double c_scale, double gumbel_scale) {
    AZ_SETTER(e, "az_engine_set_gumbel");
    EngDev &d = e->d;
    AZ_REQUIRE(m >= 0 && m <= AZ_MAX_GUMBEL, AZ_EINVAL, "az_engine_set_gumbel: m must be in [0, %d], got %d", AZ_MAX_GUMBEL, m);
    if (m == 0 && d.gm == 0) return AZ_OK;
    if (m > 0) {
        AZ_REQUIRE(c_visit >= 0.0 && c_visit <= 1.79769313486231570815e308 && c_scale >= 0.0 && c_scale <= 1.79769313486231570815e308 &&
                   gumbel_scale >= 0.0 && gumbel_scale <= 1.79769313486231570815e308, AZ_EINVAL,
                   "az_engine_set_gumbel: c_visit, c_scale and gumbel_scale must be finite and >= 0, got %g, %g, %g", c_visit, c_scale, gumbel_scale);
        AZ_REQUIRE(e->cfg.evaluator != AZ_EVAL_ROLLOUT, AZ_EINVAL, "az_engine_set_gumbel: a rollout engine (AZ_EVAL_ROLLOUT) has no priors to sample the root's actions from");
        AZ_REQUIRE(e->cfg.evaluator != AZ_EVAL_EXTERNAL, AZ_EINVAL, "az_engine_set_gumbel: an AZ_EVAL_EXTERNAL engine searches with the PUCT root only");
        AZ_REQUIRE(e->leaf_batch == 1, AZ_EINVAL, "az_engine_set_gumbel: leaf_batch %d > 1 is in force (az_engine_set_leaf_batch); the Gumbel root search takes one leaf per lock-step", e->leaf_batch);
        AZ_TRY(refuse_beside_cap_or_forced(e, "az_engine_set_gumbel", "in the PUCT search"));
    }
    if (m > 0 && e->gumbel_batch > 1 && e->cfg.evaluator == AZ_EVAL_NET)
        AZ_REQUIRE((long long)e->gumbel_batch * d.G <= az_net_max_batch(e->net), AZ_EINVAL, "az_engine_set_gumbel: gumbel_batch %d of %d slots are %lld rows, the network's max_batch is %d",
                   e->gumbel_batch, d.G, (long long)e->gumbel_batch * d.G, az_net_max_batch(e->net));
    AZ_TRY(enter(e));
    if (m > 0 && d.gm == 0 && e->gumbel_full) AZ_TRY(full_needs_fresh_roots(e, "az_engine_set_gumbel"));  // the switch comes into force with the mode
    AZ_HIP(hipMemsetAsync(d.gmask, 0, sizeof(u64) * (size_t)d.G, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    AZ_TRY(set_walkers(e, m > 0 ? e->gumbel_batch : e->leaf_batch));  // gumbel_batch is in force only while the mode is on
    d.gm = m;
    d.nval = (m > 0 && e->gumbel_full) ? e->nval : nullptr;
    d.g_cvisit = m > 0 ? c_visit : 0.0; d.g_cscale = m > 0 ? c_scale : 0.0; d.g_scale = m > 0 ? gumbel_scale : 0.0;
    // the launch sequence of a search changes: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

// several Sequential Halving leaves per slot and lock-step (k_step_gumbel_multi): accepted with the mode on or off, in force while it is on
extern "C" int az_engine_set_gumbel_batch(az_engine *e, int32_t k) {
    AZ_SETTER(e, "az_engine_set_gumbel_batch");
    EngDev &d = e->d;
    AZ_REQUIRE(k >= 1 && k <= AZ_MAX_LEAF_BATCH, AZ_EINVAL, "gumbel_batch must be in [1, %d], got %d", AZ_MAX_LEAF_BATCH, k);
    AZ_REQUIRE(k == 1 || e->sym_mask == 0, AZ_EINVAL, "az_engine_set_gumbel_batch: the engine evaluates over a symmetry mask (az_engine_set_symmetry, 0x%x); the ensemble does not combine with gumbel_batch", (unsigned)e->sym_mask);
    if (d.gm > 0 && e->cfg.evaluator == AZ_EVAL_NET)
        AZ_REQUIRE((long long)k * d.G <= az_net_max_batch(e->net), AZ_EINVAL, "gumbel_batch %d of %d slots are %lld rows, the network's max_batch is %d", k, d.G,
                   (long long)k * d.G, az_net_max_batch(e->net));
    if (k == e->gumbel_batch) return AZ_OK;
    if (d.gm > 0) {
        AZ_TRY(enter(e));
        AZ_TRY(set_walkers(e, k));
    }
    e->gumbel_batch = k;
    return AZ_OK;
}

extern "C" int az_gumbel_locksteps(int32_t n_sim, int32_t m, int32_t k) {
    if (n_sim < 0 || m < 1 || m > AZ_MAX_GUMBEL || k < 1 || k > AZ_MAX_LEAF_BATCH) return -1;
    return gumbel_locksteps(n_sim, m, k);
}

extern "C" int az_engine_gumbel_considered(az_engine *e, int32_t slot, uint64_t *mask) {
    AZ_REQUIRE(e && mask, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_gumbel_considered");
    AZ_USABLE(e, "az_engine_gumbel_considered");
    AZ_REQUIRE(slot >= 0 && slot < e->d.G, AZ_EINVAL, "slot %d outside [0, %d)", slot, e->d.G);
    AZ_TRY(enter(e));
    AZ_HIP(hipMemcpyAsync(mask, e->d.gmask + slot, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

// the paper's v_mix and deterministic non-root selection on top of the Gumbel mode: accepted with the mode on or
// off, in force while it is on
extern "C" int az_engine_set_gumbel_full(az_engine *e, int32_t on) {
    AZ_SETTER(e, "az_engine_set_gumbel_full");
    EngDev &d = e->d;
    AZ_REQUIRE(on == 0 || on == 1, AZ_EINVAL, "gumbel_full must be 0 or 1, got %d", on);
    if (on == e->gumbel_full) return AZ_OK;
    AZ_TRY(enter(e));
    if (on) {
        if (d.gm > 0) AZ_TRY(full_needs_fresh_roots(e, "az_engine_set_gumbel_full"));
        if (!e->nval) {
            AZ_TRY(dev_alloc(e, &e->nval, 2 * (size_t)d.G * (size_t)d.C));
            AZ_HIP(hipStreamSynchronize(e->stream));
        }
    }
    e->gumbel_full = on;
    d.nval = (on && d.gm > 0) ? e->nval : nullptr;
    // the Gumbel kernels of a search change: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_root_value(az_engine *e, int32_t slot, float *v) {
    AZ_REQUIRE(e && v, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_root_value");
    AZ_USABLE(e, "az_engine_root_value");
    EngDev &d = e->d;
    AZ_REQUIRE(slot >= 0 && slot < d.G, AZ_EINVAL, "slot %d outside [0, %d)", slot, d.G);
    AZ_REQUIRE(d.nval, AZ_ESTATE, "az_engine_root_value: no network values are kept (az_engine_set_gumbel_full is off, or the Gumbel mode is)");
    AZ_TRY(enter(e));
    AZ_HIP(hipStreamSynchronize(e->stream));
    int root = 0;
    uint8_t sel = 0, active = 0;
    AZ_HIP(hipMemcpy(&sel, d.pool_sel + slot, 1, hipMemcpyDeviceToHost));
    AZ_HIP(hipMemcpy(&active, d.active + slot, 1, hipMemcpyDeviceToHost));
    AZ_HIP(hipMemcpy(&root, d.root + slot, sizeof(int), hipMemcpyDeviceToHost));
    const size_t at = ((size_t)slot * 2 + sel) * d.C + root;
    Node rn;
    AZ_HIP(hipMemcpy(&rn, d.nodes + at, sizeof(Node), hipMemcpyDeviceToHost));
    AZ_REQUIRE(active && (rn.flags & F_EVALUATED), AZ_ESTATE, "az_engine_root_value: the root of slot %d has not been evaluated (or the slot holds no game)", slot);
    AZ_HIP(hipMemcpy(v, d.nval + at, sizeof(float), hipMemcpyDeviceToHost));
    return AZ_OK;
}

// ---- playout cap randomization (k_step_cap, k_root_prep, k_move) -----------------------------------------------
extern "C" int az_engine_set_playout_cap(az_engine *e, int32_t n_fast, double p_full) {
    AZ_SETTER(e, "az_engine_set_playout_cap");
    EngDev &d = e->d;
    if (n_fast == 0) {  // off: p_full is not looked at
        if (d.cap_nfast == 0) return AZ_OK;
    } else {
        AZ_REQUIRE(n_fast >= 1 && n_fast < e->cfg.n_sim, AZ_EINVAL, "az_engine_set_playout_cap: n_fast must be in [1, n_sim = %d) (0 = off), got %d", e->cfg.n_sim, n_fast);
        AZ_REQUIRE(p_full > 0.0 && p_full <= 1.0, AZ_EINVAL, "az_engine_set_playout_cap: p_full must be in (0, 1], got %g", p_full);
        const char *why = beyond_plain_search(e);
        AZ_REQUIRE(!why, AZ_EINVAL, "az_engine_set_playout_cap: the playout cap is not served for %s", why);
        AZ_REQUIRE(d.exact_max == 0, AZ_EINVAL, "az_engine_set_playout_cap: exact endgames are on (az_engine_set_exact_endgame, max_empties = %d) and do not combine with the playout cap; switch them off first", d.exact_max);
        AZ_REQUIRE(!d.pf, AZ_EINVAL, "az_engine_set_playout_cap: proof backup is on (az_engine_set_proof_backup) and does not combine with the playout cap; switch it off first");
        AZ_REQUIRE(!puct_on(d), AZ_EINVAL, "az_engine_set_playout_cap: PUCT exploration settings are on (az_engine_set_puct) and do not combine with the playout cap; switch them off first");
        if (n_fast == d.cap_nfast && p_full == d.cap_pfull) return AZ_OK;
    }
    AZ_TRY(enter(e));
    if (n_fast > 0 && !e->cap_budget) AZ_TRY(dev_alloc(e, &e->cap_budget, (size_t)d.G));
    AZ_HIP(hipStreamSynchronize(e->stream));
    d.cap_nfast = n_fast; d.cap_pfull = n_fast > 0 ? p_full : 1.0;
    d.budget = n_fast > 0 ? e->cap_budget : nullptr;
    // other kernels, and n_fast / p_full are launch arguments: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_playout_cap_stats(az_engine *e, int64_t *full_plies, int64_t *fast_plies) {
    AZ_REQUIRE(e && full_plies && fast_plies, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_playout_cap_stats");
    AZ_USABLE(e, "az_engine_playout_cap_stats");
    AZ_TRY(enter(e));
    AZ_TRY(fetch_counters(e));
    *full_plies = (int64_t)e->h_ctr[CTR_FULL_PLIES];
    *fast_plies = (int64_t)e->h_ctr[CTR_FAST_PLIES];
    return AZ_OK;
}

extern "C" int az_playout_cap_full(uint32_t seed, uint32_t game_id, int32_t ply, double p_full) {
    return playout_cap_full(seed, game_id, ply, p_full) ? 1 : 0;
}

// ---- resignation in self-play (k_move, k_resign_value) ---------------------------------------------------------------
extern "C" int az_engine_set_resign(az_engine *e, double v_resign, int32_t consecutive, int32_t min_ply, double p_holdout) {
    AZ_SETTER(e, "az_engine_set_resign");
    EngDev &d = e->d;
    const bool on = v_resign == v_resign;  // a NaN threshold is the mode off: the other three are then not looked at
    if (!on) {
        if (e->rs.rs_k == 0) return AZ_OK;
    } else {
        AZ_REQUIRE(v_resign >= -1.0 && v_resign < 0.0, AZ_EINVAL, "az_engine_set_resign: v_resign must be in [-1, 0) (NaN = off), got %g", v_resign);
        AZ_REQUIRE(consecutive >= 1 && consecutive <= AZ_RESIGN_MAX_K, AZ_EINVAL, "az_engine_set_resign: consecutive must be in [1, %d], got %d", AZ_RESIGN_MAX_K, consecutive);
        AZ_REQUIRE(min_ply >= 0, AZ_EINVAL, "az_engine_set_resign: min_ply must be >= 0, got %d", min_ply);
        AZ_REQUIRE(p_holdout >= 0.0 && p_holdout <= 1.0, AZ_EINVAL, "az_engine_set_resign: p_holdout must be in [0, 1], got %g", p_holdout);
        if (e->rs.rs_k == consecutive && e->rs.rs_v == v_resign && e->rs.rs_minply == min_ply && e->rs.rs_phold == p_holdout) return AZ_OK;
    }
    AZ_TRY(enter(e));
    if (on && !e->rs_win) AZ_TRY(dev_alloc(e, &e->rs_win, (size_t)d.G * 2 * AZ_RESIGN_MAX_K));
    if (on && !e->rs_cnt) AZ_TRY(dev_alloc(e, &e->rs_cnt, (size_t)d.G * 2));
    if (on && !e->rs_dev) AZ_TRY(dev_alloc(e, &e->rs_dev, (size_t)1));
    AZ_HIP(hipStreamSynchronize(e->stream));
    e->rs.rs_k = on ? consecutive : 0; e->rs.rs_v = on ? v_resign : 0.0; e->rs.rs_minply = on ? min_ply : 0; e->rs.rs_phold = on ? p_holdout : 0.0;
    // the settings are k_move's arguments alone, and k_move is launched, never captured: no cached search graph holds them
    return AZ_OK;
}

extern "C" int az_engine_resign_stats(az_engine *e, int64_t *resigned, int64_t *holdout_games, int64_t *holdout_triggered, int64_t *holdout_false_positives) {
    AZ_REQUIRE(e && resigned && holdout_games && holdout_triggered && holdout_false_positives, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_resign_stats");
    AZ_USABLE(e, "az_engine_resign_stats");
    AZ_TRY(enter(e));
    AZ_TRY(fetch_counters(e));
    *resigned = (int64_t)e->h_ctr[CTR_RESIGNED];
    *holdout_games = (int64_t)e->h_ctr[CTR_HOLDOUT_GAMES];
    *holdout_triggered = (int64_t)e->h_ctr[CTR_HOLDOUT_TRIG];
    *holdout_false_positives = (int64_t)e->h_ctr[CTR_HOLDOUT_FP];
    return AZ_OK;
}

// device views of the last az_engine_run's game log: n rows (0, and null pointers: that run had the mode off, or there was none)
extern "C" int az_engine_game_log(az_engine *e, int64_t *n, const int32_t **d_rows, const double **d_low) {
    AZ_REQUIRE(e && n, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_game_log");
    AZ_USABLE(e, "az_engine_game_log");
    AZ_TRY(enter(e));
    AZ_HIP(hipStreamSynchronize(e->stream));
    *n = e->gl_n;
    if (d_rows) *d_rows = e->gl_n > 0 ? e->gl_rows : nullptr;
    if (d_low) *d_low = e->gl_n > 0 ? e->gl_low : nullptr;
    return AZ_OK;
}

// the value of a ply (resign_value) for every slot's root as it stands: NaN where the slot holds no game, the root is not expanded
// or its children hold no visit.  One thread per slot; reads only.
__global__ void k_resign_value(EngDev E, double *out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    double v = __builtin_nan("");
    if (E.active[g]) {
        const Node *pool = pool_of(E, g);
        const int root = E.root[g];
        if (pool[root].flags & F_EXPANDED) {
            const int fc = pool[root].first, nc = pool[root].nch;
            double r;
            if (nc > 0 && resign_value(nc, &pool[fc].N, sizeof(Node), &pool[fc].Q, sizeof(Node), &r)) v = r;
        }
    }
    out[g] = v;
}

extern "C" int az_engine_resign_values(az_engine *e, double *d_v) {
    AZ_REQUIRE(e && d_v, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_resign_values");
    AZ_USABLE(e, "az_engine_resign_values");
    AZ_TRY(enter(e));
    hipLaunchKernelGGL(k_resign_value, grid_for(e->d.G, TB), dim3(TB), 0, e->stream, e->d, d_v);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

extern "C" int az_resign_value(int32_t n_children, const int32_t *N, const double *Q, double *v) {
    AZ_REQUIRE(n_children >= 0 && v && (n_children == 0 || (N && Q)), AZ_EINVAL, "az_resign_value: null argument or a negative count");
    for (int i = 0; i < n_children; ++i) AZ_REQUIRE(N[i] >= 0, AZ_EINVAL, "az_resign_value: N[%d] = %d is negative", i, N[i]);
    double r = 0.0;
    *v = resign_value(n_children, N, sizeof(int32_t), Q, sizeof(double), &r) ? r : __builtin_nan("");
    return AZ_OK;
}

extern "C" int az_resign_holdout(uint32_t seed, uint32_t game_id, double p_holdout) {
    return resign_holdout(seed, game_id, p_holdout) ? 1 : 0;
}

// ---- forced playouts and policy target pruning (k_step_forced, move_policy) -------------------------------------
extern "C" int az_engine_set_forced_playouts(az_engine *e, double k) {
    AZ_SETTER(e, "az_engine_set_forced_playouts");
    EngDev &d = e->d;
    AZ_REQUIRE(k >= 0.0 && k <= 64.0, AZ_EINVAL, "az_engine_set_forced_playouts: k must be finite and in [0, 64] (0 = off), got %g", k);
    if (k > 0.0) {
        const char *why = beyond_plain_search(e);
        AZ_REQUIRE(!why, AZ_EINVAL, "az_engine_set_forced_playouts: forced playouts are not served for %s", why);
        AZ_REQUIRE(d.exact_max == 0, AZ_EINVAL, "az_engine_set_forced_playouts: exact endgames are on (az_engine_set_exact_endgame, max_empties = %d) and do not combine with forced playouts; switch them off first", d.exact_max);
    }
    if (k > 0.0) AZ_REQUIRE(!d.pf, AZ_EINVAL, "az_engine_set_forced_playouts: proof backup is on (az_engine_set_proof_backup) and does not combine with forced playouts; switch it off first");
    if (k > 0.0) AZ_REQUIRE(!puct_on(d), AZ_EINVAL, "az_engine_set_forced_playouts: PUCT exploration settings are on (az_engine_set_puct) and do not combine with forced playouts; switch them off first");
    if (k == d.kforced) return AZ_OK;
    AZ_TRY(enter(e));
    if (k > 0.0 && !e->forced_picks) AZ_TRY(dev_alloc(e, &e->forced_picks, (size_t)d.G));
    // a count left by searches that were never followed by a move must not reach a later ply's fold
    if (k > 0.0 && d.kforced == 0.0) AZ_HIP(hipMemsetAsync(e->forced_picks, 0, sizeof(int) * (size_t)d.G, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    d.kforced = k > 0.0 ? k : 0.0;
    d.fpicks = k > 0.0 ? e->forced_picks : nullptr;
    // other kernels, and k is a launch argument: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_forced_playouts_stats(az_engine *e, int64_t *forced_picks, int64_t *pruned_playouts) {
    AZ_REQUIRE(e && forced_picks && pruned_playouts, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_forced_playouts_stats");
    AZ_USABLE(e, "az_engine_forced_playouts_stats");
    AZ_TRY(enter(e));
    AZ_TRY(fetch_counters(e));
    *forced_picks = (int64_t)e->h_ctr[CTR_FORCED_PICKS];
    *pruned_playouts = (int64_t)e->h_ctr[CTR_PRUNED];
    return AZ_OK;
}

// ---- exact endgames (k_step_exact, az_solve.h) ------------------------------------------------------------------
// the slots' own counts, summed: one block, the sums in out[0] (solved leaves) and out[1] (solver positions)
__global__ __launch_bounds__(256) void k_exact_stats(EngDev E, unsigned long long *out) {
    __shared__ unsigned long long s_sum[2];
    if (threadIdx.x == 0) { s_sum[0] = 0; s_sum[1] = 0; }
    __syncthreads();
    unsigned long long a = 0, b = 0;
    for (int g = threadIdx.x; g < E.G; g += blockDim.x) { a += (unsigned long long)E.x_solved[g]; b += E.x_nodes[g]; }
    if (a) atomicAdd(&s_sum[0], a);
    if (b) atomicAdd(&s_sum[1], b);
    __syncthreads();
    if (threadIdx.x == 0) { out[0] = s_sum[0]; out[1] = s_sum[1]; }
}

extern "C" int az_engine_set_exact_endgame(az_engine *e, int32_t max_empties) {
    AZ_SETTER(e, "az_engine_set_exact_endgame");
    EngDev &d = e->d;
    AZ_REQUIRE(exact_endgame_ok(max_empties), AZ_EINVAL, "az_engine_set_exact_endgame: max_empties must be in [0, %d] (0 = off), got %d", AZ_EXACT_MAX_EMPTIES, max_empties);
    if (max_empties > 0) {
        const char *why = exact_endgame_refusal(e->cfg.evaluator, e->sym_mask != 0, e->symr_mask != 0, e->leaf_batch, d.gm, d.cap_nfast > 0, d.kforced > 0.0);
        AZ_REQUIRE(!why, AZ_EINVAL, "az_engine_set_exact_endgame: exact endgames are not served for %s", why);
        AZ_REQUIRE(!puct_on(d), AZ_EINVAL, "az_engine_set_exact_endgame: PUCT exploration settings are on (az_engine_set_puct) and do not combine with exact endgames; switch them off first");
    }
    if (max_empties == d.exact_max) return AZ_OK;
    AZ_USABLE(e, "az_engine_set_exact_endgame");
    AZ_TRY(enter(e));
    {   // the leaves of a searched tree were classified under the old value: as az_engine_set_gumbel_full, fresh roots only
        int n = 0;
        AZ_HIP(hipMemsetAsync(e->scr_a, 0, sizeof(int), e->stream));
        hipLaunchKernelGGL(k_count_evaluated_roots, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, e->scr_a);
        AZ_HIP(hipGetLastError());
        AZ_HIP(hipMemcpyAsync(&n, e->scr_a, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        AZ_HIP(hipStreamSynchronize(e->stream));
        AZ_REQUIRE(n == 0, AZ_ESTATE, "az_engine_set_exact_endgame: max_empties would change from %d to %d while %d active slot(s) hold searched trees; "
                   "start the trees afresh first (az_engine_set_roots / az_engine_run; Python: set_roots, reset)", d.exact_max, max_empties, n);
    }
    if (max_empties > 0 && !e->exact_solved) {
        AZ_TRY(dev_alloc(e, &e->exact_solved, (size_t)d.G));
        AZ_TRY(dev_alloc(e, &e->exact_nodes, (size_t)d.G));
        AZ_TRY(dev_alloc(e, &e->exact_sums, 2));
    }
    // counts of an earlier spell of the mode must not show up in this one
    if (max_empties > 0 && d.exact_max == 0) {
        AZ_HIP(hipMemsetAsync(e->exact_solved, 0, sizeof(int) * (size_t)d.G, e->stream));
        AZ_HIP(hipMemsetAsync(e->exact_nodes, 0, sizeof(unsigned long long) * (size_t)d.G, e->stream));
    }
    AZ_HIP(hipStreamSynchronize(e->stream));
    d.exact_max = max_empties;
    d.x_solved = max_empties > 0 ? e->exact_solved : nullptr;
    d.x_nodes = max_empties > 0 ? e->exact_nodes : nullptr;
    // other kernels, and max_empties is a launch argument: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_exact_endgame_stats(az_engine *e, int64_t *solved_leaves, int64_t *solver_nodes) {
    AZ_REQUIRE(e && solved_leaves && solver_nodes, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_exact_endgame_stats");
    AZ_USABLE(e, "az_engine_exact_endgame_stats");
    *solved_leaves = 0; *solver_nodes = 0;
    if (!e->d.x_solved) return AZ_OK;  // off: both 0
    AZ_TRY(enter(e));
    unsigned long long h[2] = {0, 0};
    hipLaunchKernelGGL(k_exact_stats, dim3(1), dim3(256), 0, e->stream, e->d, e->exact_sums);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(h, e->exact_sums, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    *solved_leaves = (int64_t)h[0]; *solver_nodes = (int64_t)h[1];
    return AZ_OK;
}

// ---- proof backup (k_step_proof, propagate_proofs_grp, move_policy) ---------------------------------------------
// the slots' own counts, summed: one block, out[0] = nodes marked, out[1] = walks stopped on a proven node, out[2] = plies pruned
__global__ __launch_bounds__(256) void k_proof_stats(EngDev E, unsigned long long *out) {
    __shared__ unsigned long long s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long a[3] = {0, 0, 0};
    for (int g = threadIdx.x; g < E.G; g += blockDim.x)
        for (int i = 0; i < 3; ++i) a[i] += (unsigned long long)E.pf[(size_t)i * E.G + g];
    for (int i = 0; i < 3; ++i) if (a[i]) atomicAdd(&s_sum[i], a[i]);
    __syncthreads();
    if (threadIdx.x < 3) out[threadIdx.x] = s_sum[threadIdx.x];
}

// the proven outcome of every slot's root: a slot that holds a game whose root is decided (F_PROVEN; F_TERMINAL) has its outcome, every
// other slot AZ_UNSOLVED.  Reads only; one thread per slot.
__global__ void k_root_proofs(EngDev E, int8_t *out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    int w = AZ_UNSOLVED;
    if (E.active[g]) {
        const Node r = load_node(pool_of(E, g) + E.root[g]);
        if (r.flags & (F_TERMINAL | F_PROVEN)) w = r.win;
    }
    out[g] = (int8_t)w;
}

extern "C" int az_engine_set_proof_backup(az_engine *e, int32_t on) {
    AZ_SETTER(e, "az_engine_set_proof_backup");
    EngDev &d = e->d;
    AZ_REQUIRE(on == 0 || on == 1, AZ_EINVAL, "az_engine_set_proof_backup: on must be 0 or 1, got %d", on);
    if (on) {
        const char *why = proof_backup_refusal(e->cfg.evaluator, e->sym_mask != 0, e->symr_mask != 0, e->leaf_batch, d.gm, d.cap_nfast > 0, d.kforced > 0.0);
        AZ_REQUIRE(!why, AZ_EINVAL, "az_engine_set_proof_backup: proof backup is not served for %s", why);
        AZ_REQUIRE(!puct_on(d), AZ_EINVAL, "az_engine_set_proof_backup: PUCT exploration settings are on (az_engine_set_puct) and do not combine with proof backup; switch them off first");
    }
    if ((on != 0) == (d.pf != nullptr)) return AZ_OK;
    AZ_USABLE(e, "az_engine_set_proof_backup");
    AZ_TRY(enter(e));
    {   // a searched tree holds the marks of the old setting, or none where the new one expects them: fresh roots only
        int n = 0;
        AZ_HIP(hipMemsetAsync(e->scr_a, 0, sizeof(int), e->stream));
        hipLaunchKernelGGL(k_count_evaluated_roots, grid_for(d.G, TB), dim3(TB), 0, e->stream, d, e->scr_a);
        AZ_HIP(hipGetLastError());
        AZ_HIP(hipMemcpyAsync(&n, e->scr_a, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        AZ_HIP(hipStreamSynchronize(e->stream));
        AZ_REQUIRE(n == 0, AZ_ESTATE, "az_engine_set_proof_backup: proof backup would go %s while %d active slot(s) hold searched trees; "
                   "start the trees afresh first (az_engine_set_roots / az_engine_run; Python: set_roots, reset)", on ? "on" : "off", n);
    }
    if (on && !e->proof_ctr) {
        AZ_TRY(dev_alloc(e, &e->proof_ctr, 3 * (size_t)d.G));
        AZ_TRY(dev_alloc(e, &e->proof_sums, 3));
    }
    // counts of an earlier spell of the mode must not show up in this one
    if (on) AZ_HIP(hipMemsetAsync(e->proof_ctr, 0, sizeof(int) * 3 * (size_t)d.G, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    d.pf = on ? e->proof_ctr : nullptr;
    // other kernels: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_proof_backup_stats(az_engine *e, int64_t *proven_nodes, int64_t *proof_stops, int64_t *pruned_plies) {
    AZ_REQUIRE(e && proven_nodes && proof_stops && pruned_plies, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_proof_backup_stats");
    AZ_USABLE(e, "az_engine_proof_backup_stats");
    *proven_nodes = 0; *proof_stops = 0; *pruned_plies = 0;
    if (!e->d.pf) return AZ_OK;  // off: all 0
    AZ_TRY(enter(e));
    unsigned long long h[3] = {0, 0, 0};
    hipLaunchKernelGGL(k_proof_stats, dim3(1), dim3(256), 0, e->stream, e->d, e->proof_sums);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(h, e->proof_sums, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
    *proven_nodes = (int64_t)h[0]; *proof_stops = (int64_t)h[1]; *pruned_plies = (int64_t)h[2];
    return AZ_OK;
}

extern "C" int az_engine_root_proofs(az_engine *e, int8_t *d_out) {
    AZ_REQUIRE(e && d_out, AZ_EINVAL, "null argument");
    AZ_NO_OPEN_SEARCH(e, "az_engine_root_proofs");
    AZ_USABLE(e, "az_engine_root_proofs");
    AZ_TRY(enter(e));
    hipLaunchKernelGGL(k_root_proofs, grid_for(e->d.G, TB), dim3(TB), 0, e->stream, e->d, d_out);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipStreamSynchronize(e->stream));
    return AZ_OK;
}

// ---- PUCT exploration settings (k_step_puct, puct_c, puct_key) ---------------------------------------------------
extern "C" int az_engine_set_puct(az_engine *e, double c_init, double c_base, double fpu) {
    AZ_SETTER(e, "az_engine_set_puct");
    EngDev &d = e->d;
    AZ_REQUIRE(puct_c_init_ok(c_init), AZ_EINVAL, "az_engine_set_puct: c_init must be finite and in (0, 64], got %g", c_init);
    AZ_REQUIRE(puct_c_base_ok(c_base), AZ_EINVAL, "az_engine_set_puct: c_base must be 0 (no growth) or finite and in [1, 1e9], got %g", c_base);
    AZ_REQUIRE(puct_fpu_ok(fpu), AZ_EINVAL, "az_engine_set_puct: fpu must be negative (off) or finite and in [0, 4], got %g", fpu);
    if (fpu < 0.0) fpu = -1.0;  // the canonical off
    if (!puct_neutral(c_init, c_base, fpu)) {
        const char *why = puct_refusal(e->cfg.evaluator, e->sym_mask != 0, e->symr_mask != 0, e->leaf_batch, d.gm, d.cap_nfast > 0, d.kforced > 0.0,
                                       d.exact_max, d.pf != nullptr);
        AZ_REQUIRE(!why, AZ_EINVAL, "az_engine_set_puct: PUCT exploration settings are not served for %s", why);
    }
    if (c_init == d.puct_cinit && c_base == d.puct_cbase && fpu == d.puct_fpu) return AZ_OK;
    AZ_TRY(enter(e));
    AZ_HIP(hipStreamSynchronize(e->stream));
    d.puct_cinit = c_init; d.puct_cbase = c_base; d.puct_fpu = fpu;
    // other kernels, and the three settings travel by value in the launch arguments: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_puct(az_engine *e, double *c_init, double *c_base, double *fpu) {
    AZ_REQUIRE(e && c_init && c_base && fpu, AZ_EINVAL, "null argument");
    *c_init = e->d.puct_cinit; *c_base = e->d.puct_cbase; *fpu = e->d.puct_fpu;
    return AZ_OK;
}

extern "C" double az_puct_c(int32_t parent_n, double c_init, double c_base) { return puct_c(parent_n, c_init, c_base); }

extern "C" double az_puct_key(double q_child, double p_child, int32_t n_child, int32_t parent_n, double parent_q, double vis,
                              double c_init, double c_base, double fpu) {
    return puct_key(q_child, p_child, n_child, sqrt((double)parent_n), puct_c(parent_n, c_init, c_base),
                    fpu >= 0.0 ? puct_fpu_q(parent_q, vis, fpu) : 0.0, fpu);
}

// ---- leaf evaluation cache (k_step_cached) ------------------------------------------------------------------------
extern "C" int az_engine_set_eval_cache(az_engine *e, int32_t mode, int32_t capacity, int32_t stone_limit) {
    AZ_SETTER(e, "az_engine_set_eval_cache");
    AZ_REQUIRE(mode == AZ_EVAL_CACHE_AUTO || mode == AZ_EVAL_CACHE_OFF || mode == AZ_EVAL_CACHE_ON, AZ_EINVAL,
               "az_engine_set_eval_cache: mode %d (AZ_EVAL_CACHE_AUTO = -1, _OFF = 0, _ON = 1)", mode);
    AZ_REQUIRE(ec_capacity_ok(capacity), AZ_EINVAL, "az_engine_set_eval_cache: capacity must be a power of two in [1, %d] (0 = the default, %d), got %d", AZ_EC_MAX_CAPACITY, AZ_EC_DEFAULT_CAPACITY, capacity);
    AZ_REQUIRE(ec_limit_ok(stone_limit), AZ_EINVAL, "az_engine_set_eval_cache: stone_limit must be in [1, 64] (0 = the default, %d), got %d", AZ_EC_DEFAULT_LIMIT, stone_limit);
    if (mode == AZ_EVAL_CACHE_ON) {
        AZ_REQUIRE(e->cfg.evaluator == AZ_EVAL_NET, AZ_EINVAL, "az_engine_set_eval_cache: the evaluation cache is not served for %s", e->cfg.evaluator == AZ_EVAL_FAKE ? "the fake evaluator (AZ_EVAL_FAKE)" : beyond_plain_search(e));
        const char *why = beyond_plain_search(e);
        AZ_REQUIRE(!why, AZ_EINVAL, "az_engine_set_eval_cache: the evaluation cache is not served for %s", why);
    }
    const int cap = capacity > 0 ? capacity : AZ_EC_DEFAULT_CAPACITY, lim = stone_limit > 0 ? stone_limit : AZ_EC_DEFAULT_LIMIT;
    if (mode == e->ec_req && !e->ec_env && cap == e->ec_capacity && lim == e->ec_limit) return AZ_OK;
    AZ_TRY(enter(e));
    AZ_HIP(hipStreamSynchronize(e->stream));
    if (cap != e->ec_capacity)  // tables of another size: the next caching run allocates them
        for (int i = 0; i < AZ_MAX_GROUPS; ++i) {
            if (e->ec_hdr[i]) (void)hipFree(e->ec_hdr[i]);
            if (e->ec_pay[i]) (void)hipFree(e->ec_pay[i]);
            e->ec_hdr[i] = nullptr; e->ec_pay[i] = nullptr;
        }
    e->ec_req = mode; e->ec_env = false; e->ec_capacity = cap; e->ec_limit = lim;
    // the tables' pointers, the mask and the limit are launch arguments: nothing captured before may be replayed
    drop_graphs(e);
    return AZ_OK;
}

extern "C" int az_engine_eval_cache_stats(az_engine *e, int32_t *in_force, int64_t *hits) {
    AZ_REQUIRE(e && in_force && hits, AZ_EINVAL, "null argument");
    AZ_USABLE(e, "az_engine_eval_cache_stats");  // as az_engine_get_stats, whose net_evals the hits are a part of
    AZ_TRY(enter(e));
    AZ_TRY(fetch_counters(e));
    *in_force = eval_cache_on(e) ? 1 : 0;
    *hits = (int64_t)e->h_ctr[CTR_CACHE_HITS];
    return AZ_OK;
}

// whether the next az_engine_run would compute the heads in its step kernels, and whether the last one did
extern "C" int az_engine_step_heads(az_engine *e, int32_t *in_force, int32_t *used) {
    AZ_REQUIRE(e && in_force && used, AZ_EINVAL, "null argument");
    *in_force = step_heads_on(e) ? 1 : 0;
    *used = e->sh_used ? 1 : 0;
    return AZ_OK;
}

extern "C" int az_forced_playout(int32_t n, double p, int32_t root_n, double k) {
    return (k > 0.0 && forced_playout(n, p, root_n, k)) ? 1 : 0;
}

extern "C" int az_forced_prune(int32_t n_children, const int32_t *N, const double *Q, const double *P, int32_t root_n, double k, int32_t *out_N) {
    AZ_REQUIRE(n_children >= 0 && (n_children == 0 || (N && Q && P && out_N)), AZ_EINVAL, "az_forced_prune: null argument or a negative count");
    AZ_REQUIRE(k >= 0.0 && k <= 64.0, AZ_EINVAL, "az_forced_prune: k must be finite and in [0, 64], got %g", k);
    int cstar = 0;
    for (int i = 1; i < n_children; ++i) if (N[i] > N[cstar]) cstar = i;
    if (n_children == 0) return AZ_OK;
    const double sq = sqrt((double)root_n);
    const double star = Q[cstar] + (P[cstar] * sq) / (double)(1 + N[cstar]);
    for (int i = 0; i < n_children; ++i)
        out_N[i] = (!(k > 0.0) || i == cstar) ? N[i] : forced_pruned(N[i], Q[i], P[i], root_n, sq, star, k);
    return AZ_OK;
}
