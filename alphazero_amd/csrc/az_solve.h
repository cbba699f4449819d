// az_solve.h -- exact endgames: the game-theoretic outcome of a late position, by a 16-lane group (gfx950 only).
//
// Othello, Connect4 and TicTacToe are finite: with few empty cells left the outcome under optimal play by both sides is a short
// alpha-beta over the bitboard rules of az_device.h away.  az_solve_grp answers it for one position per 16-lane group (the engine's
// lanes-per-game): the k <= 16 legal moves of the position are dealt one per lane, every lane solves the successor of its move alone
// with the window [-1, +1], and the group combines the lanes' answers by ballot.
//
//  * Iterative, on an explicit stack of MAXE frames per lane -- a frame per empty cell: frame i holds a position with (empties - i)
//    empty cells, so the depth is bounded at compile time.  A frame is three u64 in LDS (the two bitboards, the moves not yet tried);
//    the side to move and the best value so far of every frame are bit fields of two registers.  No recursion, no scratch arrays.
//  * An Othello pass costs no frame: a position whose mover has no move but whose opponent has one is entered as the opponent's.
//  * A node stops at the first move that wins for its mover.  A lane stops when a lane below it (with the action wanted) or any
//    lane (without) has finished with a win for the position's mover.
//  * The outcome is the minimax value, which no order, split or stop can change.  The action reported is the lowest action index
//    whose successor has that outcome: every lane searches its successor with the full window, so a lane's value is exact, and
//    only lanes ABOVE a finished win are stopped.
//  * It cannot spin: an iteration of a running lane consumes a move of its top frame or pops that frame, and a lane stops at
//    az_solve_ceiling(MAXE) iterations (AZ_SOLVE_CEILING: the caller reports it).  A lane that is not running only waits for the
//    group's ballot, which the running lanes bound.
//  * No workgroup barrier in here.  The loop's condition is uniform over the group, so the 16 lanes leave it together.
#pragma once
#include "az_device.h"

#define AZ_SOLVE_LPG 16         // lanes per position: one DPP row, the engine's lanes-per-game
#define AZ_SOLVE_FRAME_WORDS 3  // u64 per frame and lane: p1, m1, moves left

#define AZ_SOLVE_OK 0       // *winner (and *action) hold the answer
#define AZ_SOLVE_BUDGET 1   // a lane the answer needs ran out of its node budget
#define AZ_SOLVE_CEILING 2  // a lane the answer needs reached the iteration ceiling, or the position broke a precondition

// Iterations a lane may take.  Below its root move the lane sees a position of m = MAXE - 1 empty cells; a line of play fills
// distinct empty cells (a pass fills none and enters no node), so the lane enters at most sum_k m! / (m - k)! < e * m! < 3 * m!
// positions.  Every iteration but the pops enters one, and there is at most one pop per position entered: 2 * 3 * m! iterations.
// Beyond 2^24 the proven bound gives way to a bound on the kernel's running time (seconds on a shared device); alpha-beta on the
// window [-1, +1] stays orders of magnitude under either (DESIGN: measured node counts).
constexpr long long az_solve_ceiling(int max_empties) {
    long long f = 1;
    for (int i = 2; i < max_empties; ++i) f *= i;
    return 6 * f < (1LL << 24) ? 6 * f : (1LL << 24);
}

AZ_D u32 az_solve_ballot(bool p) { return (u32)(__ballot(p) >> (threadIdx.x & 48)) & 0xFFFFu; }

// az_play on an action BIT (az_legal_bits' space) instead of an action index: no integer division on the solver's path
AZ_D void az_solve_play(const GameDesc &gd, BB &b, int bit) {
    u64 own = b.player > 0 ? b.p1 : b.m1, opp = b.player > 0 ? b.m1 : b.p1;
    if (gd.game == AZ_OTHELLO) {
        const u64 mv = 1ULL << bit;
        const u64 f = oth_flips(own, opp, mv);
        own |= mv | f;
        opp &= ~f;
    } else if (gd.game == AZ_CONNECT4) {  // bit = column: lowest free row, as az_play
        const int filled = __popcll((own | opp) & c4_colmask(gd, bit));
        own |= 1ULL << ((gd.H - 1 - filled) * 8 + bit);
    } else {
        own |= 1ULL << bit;
    }
    if (b.player > 0) { b.p1 = own; b.m1 = opp; } else { b.m1 = own; b.p1 = opp; }
    b.player = -b.player;
}

// The outcome of `root` under optimal play, by the 16 lanes of a group (all must call it together; all get the same answer).
// Preconditions: the game is not over at `root` (az_status false) and root has at most MAXE empty cells.
//   stk        this lane's column of the block's frame store: u64 [MAXE * AZ_SOLVE_FRAME_WORDS][TPB] in LDS, stk = base + threadIdx.x
//   want_action  also report the lowest action that keeps the outcome (the Othello pass action `cells` where the mover must pass)
//   budget     0: none; otherwise a lane gives up before it enters more than `budget` positions
//   *nodes     positions entered by the group (informational: it depends on where the lanes were stopped)
// Returns AZ_SOLVE_OK with *winner in {-1, 0, +1} (an absolute player id, as az_status reports it), or why there is no answer.
template <int MAXE, int TPB>
AZ_D int az_solve_grp(const GameDesc &gd, BB root, int sub, u64 *stk, bool want_action, long long budget, int *winner, int *action,
                      unsigned long long *nodes) {
    static_assert(MAXE >= 1 && MAXE <= 12, "a frame's best value takes two bits of a 32-bit register; a move per lane needs moves <= empties < 16");
    enum { RUN = 0, FIN, IDLE, STOPPED, OUT_OF_BUDGET, AT_CEILING };
#define AZ_FRAME(f, q) stk[((f) * AZ_SOLVE_FRAME_WORDS + (q)) * TPB]
    u64 bits = az_legal_bits_grp(gd, root, root.player, sub);
    const bool pass = gd.game == AZ_OTHELLO && bits == 0;
    if (pass) {  // the game is not over, so the other side has a move: the same board with that side to move
        root.player = -root.player;
        bits = az_legal_bits_grp(gd, root, root.player, sub);
    }
    const int k = __popcll(bits);
    const bool broken = k < 1 || k > AZ_SOLVE_LPG || __popcll(gd.valid & ~(root.p1 | root.m1)) > MAXE;  // uniform over the group
    u64 mine = bits;  // this lane's move: the sub-th legal one in ascending action order
    for (int i = 0; i < sub; ++i) mine &= mine - 1;
    mine &= ~mine + 1;
    int state = (!broken && sub < k) ? RUN : IDLE;
    // frame 0 is the position itself with the lane's one move to try; the value the lane finishes with is that move's
    int sp = 0;
    u32 movers = root.player > 0 ? 1u : 0u;  // bit f: player +1 moves at frame f
    u32 bests = 0;                           // two bits per frame: 1 + the best value so far in the mover's frame (0: none yet = a loss)
    if (state == RUN) { AZ_FRAME(0, 0) = root.p1; AZ_FRAME(0, 1) = root.m1; AZ_FRAME(0, 2) = mine; }
    int rel = -1;  // the finished lane's value for the position's mover
    long long iters = 0;
    unsigned long long cnt = 0;
    const u32 stop_by = want_action ? ((1u << sub) - 1u) : 0xFFFFu;
    for (;;) {
        const u32 won = az_solve_ballot(state == FIN && rel > 0);
        if (state == RUN && (won & stop_by)) state = STOPPED;
        if (az_solve_ballot(state == RUN) == 0) break;
        if (state == RUN) {
            if (++iters > az_solve_ceiling(MAXE)) {
                state = AT_CEILING;
            } else {
                const int p = ((movers >> sp) & 1u) ? 1 : -1;
                const int best = (int)((bests >> (2 * sp)) & 3u) - 1;
                const u64 mv = AZ_FRAME(sp, 2);
                int w = 0;         // a value to fold into the top frame, as an absolute winner
                bool fold = false;
                if (mv == 0 || best > 0) {  // pop: every move tried, or a win for the mover
                    w = p * best;
                    --sp;
                    if (sp < 0) { state = FIN; rel = best; } else fold = true;
                } else if (budget > 0 && (long long)cnt >= budget) {
                    state = OUT_OF_BUDGET;
                } else {  // consume the lowest move left
                    AZ_FRAME(sp, 2) = mv & (mv - 1);
                    ++cnt;
                    BB c = {AZ_FRAME(sp, 0), AZ_FRAME(sp, 1), p};
                    az_solve_play(gd, c, __ffsll((long long)mv) - 1);
                    bool over;
                    u64 cm;
                    if (gd.game == AZ_OTHELLO) {  // az_status and az_legal_bits in one: the mover's flood is both
                        const u64 own = c.player > 0 ? c.p1 : c.m1, opp = c.player > 0 ? c.m1 : c.p1;
                        cm = oth_legal(own, opp, gd.valid);
                        over = false;
                        if (cm == 0) {
                            cm = oth_legal(opp, own, gd.valid);
                            if (cm == 0) {
                                over = true;
                                const int d = __popcll(c.p1) - __popcll(c.m1);
                                w = d > 0 ? 1 : (d < 0 ? -1 : 0);
                            } else {
                                c.player = -c.player;  // a pass: the same frame-to-be, the other side to move
                            }
                        }
                    } else {
                        over = az_status(gd, c, &w);
                        cm = over ? 0 : az_legal_bits(gd, c, c.player);
                    }
                    if (over) {
                        fold = true;
                    } else if (sp + 1 >= MAXE) {  // more empty cells than frames: the precondition was broken (never an LDS overrun)
                        state = AT_CEILING;
                    } else {
                        ++sp;
                        AZ_FRAME(sp, 0) = c.p1; AZ_FRAME(sp, 1) = c.m1; AZ_FRAME(sp, 2) = cm;
                        movers = (movers & ~(1u << sp)) | (c.player > 0 ? 1u << sp : 0u);
                        bests &= ~(3u << (2 * sp));
                    }
                }
                if (fold) {
                    const int r = (((movers >> sp) & 1u) ? 1 : -1) * w;
                    const int b0 = (int)((bests >> (2 * sp)) & 3u) - 1;
                    if (r > b0) bests = (bests & ~(3u << (2 * sp))) | ((u32)(r + 1) << (2 * sp));
                }
            }
        }
    }
#undef AZ_FRAME
    const u32 winm = az_solve_ballot(state == FIN && rel > 0), drawm = az_solve_ballot(state == FIN && rel == 0);
    const u32 budm = az_solve_ballot(state == OUT_OF_BUDGET), ceilm = az_solve_ballot(state == AT_CEILING);
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) cnt += (unsigned long long)__shfl_xor((long long)cnt, m, AZ_SOLVE_LPG);
    *nodes = cnt + 1;
    if (broken) return AZ_SOLVE_CEILING;
    int lane, best;
    if (winm) {
        best = 1; lane = __ffs((int)winm) - 1;
        // the win stands whatever the lanes that gave up would have found; the LOWEST winning action needs the lanes below it
        const u32 below = (budm | ceilm) & ((1u << lane) - 1u);
        if (want_action && below) return (ceilm & below) ? AZ_SOLVE_CEILING : AZ_SOLVE_BUDGET;
    } else {
        if (budm | ceilm) return ceilm ? AZ_SOLVE_CEILING : AZ_SOLVE_BUDGET;
        best = drawm ? 0 : -1;
        lane = drawm ? __ffs((int)drawm) - 1 : 0;  // every move loses: the lowest legal one
    }
    *winner = root.player * best;
    if (want_action) {
        u64 m = bits;
        for (int i = 0; i < lane; ++i) m &= m - 1;
        *action = pass ? gd.cells : az_bit_to_action(gd, __ffsll((long long)m) - 1);
    }
    return AZ_SOLVE_OK;
}
