/*
 * az_amd.h -- C ABI of the MI355X-native AlphaZero self-play engine (libaz_amd.so).
 *
 * The reference (t0m1ab/alphazero) is pure Python and has no FFI; its extension surface is the
 * Board / PolicyValueNetwork / MCT / AlphaZeroTrainer.self_play classes.  Each entry point below
 * names the reference interface it stands in for (paths relative to /root/reference/alphazero/).
 * The Python host layer (alphazero_amd/) binds these with ctypes; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  `stream` is a hipStream_t passed as
 *     void* (NULL = default stream).  Pointers prefixed d_ are DEVICE pointers, h_ are HOST pointers.
 *   - every function returns 0 on success or a negative AZ_E* code and never throws;
 *     az_last_error() returns the message of the calling thread's last failure.
 *   - encodings (identical to the reference's numpy objects):
 *       grid    int8 [H*W] row-major, values {-1,0,+1}      (Board.grid, base.py:112)
 *       player  int8 in {+1,-1}                              (Board.player)
 *       action  othello r*n+c, pass = n*n; tictactoe 3r+c; connect4 column
 *               (PolicyValueNetwork.to_neural_output, othello.py:404-412, connect4.py:430-435)
 *   - an engine handle is not re-entrant; different handles may be driven from different threads.
 */
#ifndef AZ_AMD_H
#define AZ_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_GAME_OTHELLO 0
#define AZ_GAME_CONNECT4 1
#define AZ_GAME_TICTACTOE 2

#define AZ_OK 0
#define AZ_EINVAL (-1)   /* bad argument (reference: ValueError in constructors) */
#define AZ_EHIP (-2)     /* HIP runtime failure */
#define AZ_ESTATE (-3)   /* call order / missing weights */
#define AZ_ECAPACITY (-4)/* node pool or sample buffer exhausted */
#define AZ_EILLEGAL (-5) /* illegal move (reference: ValueError, othello.py:199-200) */
#define AZ_EEVAL (-6)    /* the external evaluator (az_engine_set_evaluator) reported a failure */

#define AZ_TIE_MODE_LOWEST 0  /* fair_max ties -> lowest action index (deterministic, tests) */
#define AZ_TIE_MODE_RANDOM 1  /* fair_max ties -> uniform (utils.py:28-34), Philox stream */
#define AZ_NOISE_MODE_OFF 0
#define AZ_NOISE_MODE_PHILOX 1 /* root Dirichlet noise (mcts.py:235-240) from the Philox stream */
#define AZ_NOISE_MODE_HASH 2   /* closed-form noise from the root board hash (tests) */
#define AZ_EVAL_NET 0          /* PolicyValueNetwork.evaluate (base.py:357-367) on the HIP network */
#define AZ_EVAL_FAKE 1         /* closed-form fake network (tests; tools/closed_form.py) */
#define AZ_EVAL_ROLLOUT 2      /* TreeEval.ROLLOUT: plain UCT with random playouts, no network (mcts.py:38-42, 173-180) */
#define AZ_EVAL_EXTERNAL 3     /* the caller's evaluator (az_engine_set_evaluator): PolicyValueNetwork.evaluate, base.py:357-367 */

const char *az_last_error(void);
int az_version(void);

/* ---- batched board rules (K1/K2) -------------------------------------------------------------
 * replaces Board.get_moves / is_legal_move / play_move / is_game_over / get_winner / get_score
 * (othello.py:133-229, connect4.py:143-258, tictactoe.py:139-184) for n positions at once. */

/* d_legal[n][A] uint8: 1 where the action is legal for `d_for_player[i]` (0 = side to move,
 * base.py:163-171 `player` argument).  d_for_player may be NULL. */
int az_board_legal_batch(int game, int H, int W, const int8_t *d_grids, const int8_t *d_players,
                         const int8_t *d_for_player, int64_t n, uint8_t *d_legal, void *stream);
/* plays d_actions[i]; d_status[i] = 0 ok / AZ_EILLEGAL (board then copied unchanged). */
int az_board_play_batch(int game, int H, int W, const int8_t *d_grids, const int8_t *d_players,
                        const int32_t *d_actions, int64_t n, int8_t *d_out_grids, int8_t *d_out_players,
                        int32_t *d_status, void *stream);
/* d_over[i] uint8, d_winner[i] int8 (valid where over; 2 otherwise), d_score[i] int32 =
 * sum(player*grid) (Board.get_score of othello/connect4). */
int az_board_status_batch(int game, int H, int W, const int8_t *d_grids, const int8_t *d_players, int64_t n,
                          uint8_t *d_over, int8_t *d_winner, int32_t *d_score, void *stream);

/* ---- exact endgames ---------------------------------------------------------------------------
 * The outcome of n positions under optimal play by both sides (the reference has no counterpart: its players ask the network on
 * every position).  A position is a candidate when empties = popcount(valid cells & ~(p1 | m1)) <= max_empties.
 *   a finished game          d_winner = the winner as az_board_status_batch reports it, d_action = -1
 *   a solved position        d_winner = the outcome, an absolute player id in {-1, 0, +1}; d_action = the LOWEST action index whose
 *                            successor has that outcome -- a property of the position, not of the search order -- and Othello's pass
 *                            action H*W where the side to move must pass
 *   anything else            d_winner = AZ_UNSOLVED, d_action = -1: a position above the limit, or one for which a lane of the
 *                            solver entered node_budget positions (0: no budget; what counts is implementation-defined) or reached
 *                            the solver's iteration ceiling.  Never an error.
 * d_nodes (int64 [n], may be NULL) = positions the solver entered, informational.  One 16-lane group per position: the legal moves
 * are dealt over the lanes, each solved by an iterative alpha-beta on the window [-1, +1] with its stack in LDS (az_solve.h), the
 * device function a search with exact endgames sends its late leaves through.
 * AZ_EINVAL: max_empties outside [1, AZ_SOLVE_MAX_EMPTIES], a negative node_budget or n, a null d_grids / d_players / d_winner /
 * d_action with n > 0, a game or board az_board_status_batch refuses. */
#define AZ_SOLVE_MAX_EMPTIES 12
#define AZ_UNSOLVED 2
int az_solve_batch(int game, int H, int W, const int8_t *d_grids, const int8_t *d_players, int64_t n,
                   int32_t max_empties, int64_t node_budget,
                   int8_t *d_winner, int32_t *d_action, int64_t *d_nodes, void *stream);

/* ---- policy-value network (K5/K6) ------------------------------------------------------------
 * replaces OthelloNet / Connect4Net / TicTacToeNet .forward + PolicyValueNetwork.predict
 * (othello.py:341-382, connect4.py:370-412, tictactoe.py:289-316, base.py:350-355), eval mode. */
typedef struct az_net az_net;
int az_net_create(int game, int H, int W, int max_batch, az_net **out);
void az_net_destroy(az_net *net);
/* h_data: HOST float32 tensor of the torch state_dict entry `name` ("conv1.weight",
 * "bn1.running_var", "fc_probs.bias", ...).  Unknown keys (num_batches_tracked) return AZ_OK. */
int az_net_set_tensor(az_net *net, const char *name, const float *h_data, int64_t numel);
/* folds eval-mode BatchNorm into the preceding layer (float64), re-tiles the weights into MFMA
 * fragment order and uploads them.  Must be called after all tensors are set / updated. */
int az_net_commit(az_net *net, void *stream);
/* The same hand-off without a host round trip (update_network, trainer.py:383-387, when the trained module lives on the
 * GPU): d_data is a DEVICE float32 tensor, copied on `stream`; az_net_commit_device folds BatchNorm and re-tiles with
 * device kernels on `stream` (same float64 operation order as az_net_commit: identical bits).  A commit uses the
 * tensors of ITS kind only: set every tensor through the same path. */
int az_net_set_tensor_device(az_net *net, const char *name, const float *d_data, int64_t numel, void *stream);
int az_net_commit_device(az_net *net, void *stream);
/* d_input[B][H*W] float32 canonical boards (player*grid, base.py:363);
 * d_probs[B][A] = exp(log_softmax) policy, d_value[B] = tanh value. */
int az_net_forward(az_net *net, const float *d_input, int B, float *d_probs, float *d_value, void *stream);
/* same, but only the first min(*d_count, max_B) rows are evaluated: d_count is a DEVICE int written by an
 * earlier kernel on `stream` (the engine compacts the leaves that need an evaluation into the front rows). */
int az_net_forward_dyn(az_net *net, const float *d_input, const int32_t *d_count, int max_B, float *d_probs,
                       float *d_value, void *stream);
/* Lanes: a net has ONE set of activation rows (conv features, fc1 and fc2 outputs), so two forwards in flight on two streams
 * would overwrite each other.  az_net_set_lanes(net, n, rows) gives lanes 1 .. n - 1 activation rows of their own, `rows` each
 * (lane 0 is the net's own set, max_batch rows); it only grows, and waits for the device before it returns.  n in [1, 4];
 * AZ_EINVAL: n outside that, rows outside (0, max_batch], n > 1 on a net under AZ_DENSE_I8 (its digit planes are one set).
 * The TicTacToe MLP keeps no activation in memory: its lanes are names, only their count is recorded.
 * az_net_forward_lane is az_net_forward_dyn on the activation rows of `lane` (lane 0: exactly az_net_forward_dyn); forwards of
 * different lanes may be in flight together on different streams, issued from one host thread.  beside != 0 says that the
 * forward runs next to another one: the size thresholds that pick a layer's kernel were measured with the chip to itself, and
 * a forward that shares it picks by the thresholds measured for that regime.  Every kernel of a layer gives the same bits, so
 * the flag never changes a result; az_net_stage_kernel keeps answering for a lone launch. */
int az_net_set_lanes(az_net *net, int n_lanes, int rows);
int az_net_forward_lane(az_net *net, int lane, int beside, const float *d_input, const int32_t *d_count, int max_B,
                        float *d_probs, float *d_value, void *stream);
/* Evaluation averaged over the board's symmetries (ensemble inference: AlphaGo Zero evaluates each leaf in one of the eight
 * orientations, Silver et al. 2017 "Mastering the game of Go without human knowledge", Methods; KataGo's analysis mode averages
 * over all of them).  The reference has no counterpart: it uses the symmetries for training samples only (trainer.py:275-284).
 * A mask is a set of transform codes, bit t = code t: the codes of az_augment below (t & 1 horizontal reflection first, t >> 1
 * quarter turns of np.rot90) plus 0 for the identity.  Any subset on a square Othello / TicTacToe board, a subset of {0, 1} for
 * Connect4 (gravity rules rotations out on any board); AZ_SYM_ALL = every valid code; 0 = off.  The n = popcount(mask) members
 * are visited in ascending code order: each row is expanded into its n twins, the ordinary forward runs on the n * B rows, and
 *   d_probs[r][a] = (sum_j p[r n + j][cell of twin j that holds original action a]) / (float)n,   d_value[r] = (sum_j v[r n + j]) / (float)n
 * with float32 sums taken sequentially in member order (Othello's pass entry stays in place, Connect4 flips its columns).
 * Needs n * B <= max_batch (AZ_EINVAL otherwise); the scratch rows belong to the net and are allocated at the first call. */
#define AZ_SYM_ALL (-1)
int az_net_forward_sym(az_net *net, const float *d_input, int B, int32_t mask, float *d_probs, float *d_value, void *stream);
/* One symmetry per row instead of the average: row r is evaluated in the single orientation d_codes[r] (a transform code as above,
 * one byte per row, DEVICE memory).  The row's input plane is replaced by its twin under that code, the ordinary forward runs on the
 * B rows, d_probs[r][a] is the twin's entry for the cell that holds original action a (Othello's pass entry stays in place, Connect4
 * flips its columns) and d_value[r] the twin's value: copies only, no sum and no division.  Every code 0 is az_net_forward bit for
 * bit, every code c is az_net_forward_sym with mask 1 << c bit for bit.  The codes are not copied to the host and so are trusted:
 * a code the board does not have is read as the identity (the Python wrapper validates them).  AZ_EINVAL: a null argument,
 * B <= 0, B > max_batch.  This is the evaluation of az_engine_set_symmetry_random below with the codes given, not drawn. */
int az_net_forward_sym_codes(az_net *net, const float *d_input, int B, const uint8_t *d_codes, float *d_probs, float *d_value, void *stream);
int az_net_action_size(const az_net *net);
/* algorithmic FLOPs of one forward per board (2*MAC) */
int64_t az_net_flops_per_board(const az_net *net);
/* times `iters` back-to-back launches of one forward stage with HIP events on `stream`;
 * stage: 0 conv trunk, 1 fc1, 2 fc2, 3 heads, -1 whole forward.  *ms_per_launch out. */
int az_net_time_stage(az_net *net, int stage, int B, int iters, void *stream, float *ms_per_launch);
/* name of the kernel family of the plan for stage (0..3) of a lone launch of B boards, as rocprofv3 lists it (template arguments abbreviated) */
int az_net_stage_kernel(const az_net *net, int stage, int B, char *buf, int cap);
/* 1 where the trunk of a launch of B boards (beside as in az_net_forward_lane) runs the prefetching form of k_trunk_quad, else 0
 * (AZ_TRUNK_QUAD_PREFETCH: unset = by regime, 0 = never, 1 = wherever the form is built); the forms give the same bits */
int az_net_trunk_prefetch(const az_net *net, int B, int beside);
/* 1 where the trunk of that launch runs the prefetching form with vector stores (conv3's planes as paired LDS writes, conv4's features
 * as 16-byte stores), else 0 (AZ_TRUNK_QUAD_STORES: unset = by regime, 0 = never, 1 = wherever the prefetching form runs); the same bits */
int az_net_trunk_stores(const az_net *net, int B, int beside);
/* The plan of stage 0..3 of a launch of B boards (beside as in az_net_forward_lane) as text: the kernel by its own name and the
 * plan's fields for it, e.g. "k_trunk_quad form=2 lds_blocks=0 prefetch=1 stores=1", "k_gemm 64x64 form=1 rows=count" (rows=count: the
 * rows of a block follow the device row count, see az_net_gemm_rows; rows=64: they do not).  For tools' output. */
int az_net_stage_plan(const az_net *net, int stage, int B, int beside, char *buf, int cap);
/* Rows per block of fc1 (stage 1) / fc2 (stage 2) of a launch of B boards of which the device count fills `count`: 16, 32 or 64 on
 * k_gemm's 64 x 64 tile -- the narrowest form whose ceil(B / 64) row bands cover the count, where the plan lets the rows follow it
 * (AZ_GEMM_ROWS: unset = by regime, 0 = 64 everywhere, 1 = wherever the narrow forms exist) -- the tile's height on k_gemm's other
 * tiles, 0 where the stage runs another kernel.  Every form gives the same bits.  (ABI 115) */
int az_net_gemm_rows(const az_net *net, int stage, int B, int beside, int count);
/* One stage (0 trunk, 1 fc1, 2 fc2, 3 heads) of az_net_forward_lane with the same arguments: exactly the launch the forward makes for
 * that stage, reading the lane's activation rows as they stand.  For tools that time one stage beside another on two streams.
 * Only stage 3 writes d_probs / d_value (the fused tails: stage 1); they are required for every stage so that the call is the
 * forward's.  The launch carries no events: under az_net_profile(net, 1) it is NOT booked in any slot.
 * AZ_EINVAL: a null argument, a stage outside 0..3, the TicTacToe MLP (one stage), a lane or row count az_net_forward_lane refuses. */
int az_net_stage_lane(az_net *net, int lane, int beside, int stage, const float *d_input, const int32_t *d_count, int max_B,
                      float *d_probs, float *d_value, void *stream);
/* For a consumer that computes the policy / value heads itself from a lane's fc2 rows (the search step kernel k_step_heads).  (ABI 117)
 * az_net_forward_lane_fc2: az_net_forward_lane without its last stage -- trunk, fc1, fc2 on the lane's rows; rows [0, *d_count) of the
 * lane's fc2 activations are the result.
 * az_net_heads_view: what the consumer reads, each where the pointer is not null -- the lane's fc2 rows (F2 floats each), the head
 * matrix in k_heads2's MFMA fragment order [F2/16][NH/16][64 lanes][4], the padded bias [NH], NH (the padded logits: A priors, the
 * value logit at A) and F2.  The rows' pointer changes with az_net_set_lanes; the weights' pointers live as long as the net and their
 * contents change with az_net_commit / az_net_commit_device, so a holder by value sees every later commit.
 * Both: AZ_EINVAL for a net whose heads k_heads2 has no instantiation for (served: F2 = 512 with 80 or 48 padded logits, OthelloNet, on
 * float dense layers) and for a lane that does not exist. */
int az_net_forward_lane_fc2(az_net *net, int lane, int beside, const float *d_input, const int32_t *d_count, int max_B, void *stream);
int az_net_heads_view(az_net *net, int lane, const float **d_h2, const float **d_hwq, const float **d_hb, int32_t *NH, int32_t *F2);
/* Live measurement (the idiom of timers.py:53-76 applied per kernel): while enabled, every forward brackets its stage
 * launches with a start and a stop event each (hipExtLaunchKernelGGL).  ms_total[8] / launches[8], one slot per kernel family so that a slot's mean is the
 * figure rocprofv3 lists for that kernel: k_trunk2, fc1 and fc2 on the tiled GEMMs (k_gemm / k_gemm_solo; Connect4Net's fused tail
 * in the fc1 slot), k_heads, k_trunk (one board per wave) | fc1, fc2 on the small-batch kernels (k_dense_frag / k_dense_small),
 * k_trunk_q. */
int az_net_profile(az_net *net, int enable);
int az_net_profiling(const az_net *net); /* 1 while enabled (the engine then launches kernel by kernel instead of replaying graphs) */
int az_net_profile_read(az_net *net, double *ms_total, int64_t *launches);
/* correction to subtract per launch from ms_total before comparing with rocprofv3's kernel durations: 0 -- every profiled launch
 * carries its own start / stop events (the dispatch's begin / end timestamps); kept for callers written against rounds 1-3, which
 * recorded events BETWEEN the launches and calibrated the cost of an empty interval */
int az_net_profile_overhead(az_net *net, double *ms_per_interval);

/* ---- self-play engine (K3/K4/K7/K8/K9) -------------------------------------------------------
 * replaces AlphaZeroTrainer.self_play (trainer.py:215-273) driving AlphaZeroPlayer.get_move
 * (players.py:158-191) / MCT.search (mcts.py:226-269) for n_slots concurrent games in lock-step. */
typedef struct az_engine az_engine;
typedef struct {
    int32_t game, H, W;
    int32_t n_slots;           /* concurrent games resident in HBM */
    int32_t n_sim;             /* Config.simulations */
    double dirichlet_alpha;    /* < 0 : None */
    double dirichlet_epsilon;  /* < 0 : None */
    int32_t temp_max_step, temp_min_step; /* LinearTemperatureScheduler (schedulers.py:20-40) */
    int32_t tie_mode, noise_mode, evaluator;
    uint32_t seed;             /* Philox key word 0; word 1 is the game id */
    int32_t node_capacity;     /* nodes per tree pool (two pools per slot; the kept subtree is compacted at every move) */
    int32_t max_plies;         /* per game, sample staging */
    int64_t sample_capacity;   /* samples the output buffers can hold */
} az_engine_cfg;

typedef struct {
    int64_t games_done, samples, net_evals, lockstep_iters, plies;
    int32_t max_nodes_used, error_flags;
    int64_t graph_replays;  /* searches issued as one HIP graph launch since the engine was created */
    int32_t max_path_len;   /* longest root..leaf path (nodes) of a simulation since the last run/set_roots; only paths
                               longer than 16 nodes are recorded (they take the parent-chasing back-propagation), else 0 */
    int32_t reserved;
    int64_t cache_hits;     /* az_engine_set_eval_cache: the leaves answered from a slot group's table since the last az_engine_run began;
                               they count in net_evals too (ABI 113) */
} az_engine_stats;

/* `stream` (hipStream_t, may be the default stream): the stream the caller's own work is queued on.  The engine runs on a
 * stream of its own: every call first orders that stream behind `stream` and returns only when the engine's work is done.
 * One search (1 + 5 n_sim launches) is captured as a HIP graph the second time it is issued with the same shape and
 * replayed from then on (AZ_ENGINE_GRAPHS=0 in the environment switches that off). */
int az_engine_create(const az_engine_cfg *cfg, az_net *net, void *stream, az_engine **out);
void az_engine_destroy(az_engine *e);
/* plays games first_game_id .. first_game_id+n_games-1 to completion (slots are refilled as games
 * end) and blocks until done.  Samples accumulate in the output buffers from index 0. */
int az_engine_run(az_engine *e, uint32_t first_game_id, int32_t n_games);
int az_engine_get_stats(az_engine *e, az_engine_stats *out);
/* device views of the normalised samples (trainer.py:262-265, Sample.normalize):
 *   states int8 [S][H*W] = grid*player, pis float32 [S][A], zs int8 [S] = winner*player,
 *   meta int32 [S][4] = {game_id, move_idx, player, action}, visits int32 [S][A]. */
int az_engine_samples(az_engine *e, int64_t *n_samples, const int8_t **d_states, const float **d_pis,
                      const int8_t **d_zs, const int32_t **d_meta, const int32_t **d_visits);

/* finer-grained control (tests, arena-style use): */
/* puts n_roots positions into slots 0..n-1 (fresh trees); h_* are HOST arrays. */
int az_engine_set_roots(az_engine *e, const int8_t *h_grids, const int8_t *h_players, const uint32_t *h_game_ids,
                        const int32_t *h_plies, int32_t n_roots);
int az_engine_search(az_engine *e, int32_t n_sim);     /* MCT.search on every active slot */
/* MCT.get_action_probs + sampled move + Board.play_move + MCT.change_root (+ sample record) */
int az_engine_advance(az_engine *e);
/* Board.play_move + MCT.change_root (mcts.py:118-125) with externally chosen moves for slots 0..n-1 (arena
 * opponent / human): re-roots at the child when the tree holds it, else starts a fresh root.  AZ_EILLEGAL and
 * h_status[i] = AZ_EILLEGAL for an illegal move (reference: ValueError), boards untouched for those slots. */
int az_engine_play(az_engine *e, const int32_t *h_actions, int32_t n, int32_t *h_status);
/* root statistics of one slot to HOST arrays (capacity AZ_MAX 65): actions, N, Q, P */
int az_engine_root_children(az_engine *e, int32_t slot, int32_t *h_actions, int32_t *h_N, double *h_Q,
                            double *h_P, int32_t *count, int32_t *root_N);
/* Root readout of slots 0..n-1 in ONE kernel launch, with no per-slot host copy: everything Player.get_move returns -- (move,
 * action_probs, visit_counts, prior_probs), players.py:158-191 -- and what MCT.get_action_probs / get_prior_probs read
 * (mcts.py:95-116), for many positions at once.  az_engine_root_children is the one-slot form.  Rows are dense, indexed by action:
 *   d_visits int32 [n][A] child N;  d_Q, d_P float64 [n][A] the child's Q and (noised) prior, bit for bit;
 *   d_child uint8 [n][A] 1 where the root holds a child for the action (0 visits does not tell a legal unvisited move from an
 *   illegal one);  d_root_N int32 [n] the root's N;
 *   d_pi float32 [n][A], d_action int32 [n]: exactly the policy az_engine_advance would record and the move it would play now, at
 *   the slot's temperature: h_temps[g] (0 = fair_max over N under the engine's tie_mode, else N^(1/t) / sum and the sampled move),
 *   or the engine's LinearTemperatureScheduler at the slot's ply when h_temps is NULL;
 *   d_pv int32 [n][pv_len], 0 <= pv_len <= 16: the principal line -- from the root, step to the child with the greatest N (lowest
 *   action among equals) until a node is not expanded, has no children or its best child has N = 0; unused entries are -1.
 *   d_pv[g][0] is the deterministic most-visited move and may differ from d_action[g], which draws among equals under
 *   AZ_TIE_MODE_RANDOM and samples at a temperature above 0.
 * A slot is served when the engine searches it (active; in arena mode its colour to move) and its root is expanded with children;
 * any other slot gets action -1, root_N 0, zero rows and a line of -1.  Rows beyond n are not touched.  The call changes nothing:
 * trees, boards, counters, samples and random streams are as if it had not run.  Blocks until the outputs are written.
 * AZ_EINVAL: null e / out, n outside [1, n_slots], pv_len outside [0, 16], d_pv with pv_len 0, a temperature that is negative or
 * not finite (the message names the lowest such slot). */
typedef struct {            /* DEVICE pointers; any may be NULL = not wanted */
    int32_t *d_visits; float *d_pi; double *d_Q, *d_P; uint8_t *d_child;
    int32_t *d_action, *d_root_N, *d_pv; int32_t pv_len;
} az_root_readout;
/* h_temps: HOST double[n] or NULL (the engine's scheduler at each slot's ply) */
int az_engine_root_readout(az_engine *e, const double *h_temps, int32_t n, const az_root_readout *out);
/* The reference's tree (mcts.py:8-47 Node objects) grows without bound while MCT.search is called again and again on one root;
 * the engine's pools have a fixed size: nodes the slot's live pool holds, and re-allocation of all pools with a larger capacity
 * (trees kept).  The single-game MCT mirror grows its pools before a search could exhaust them. */
int az_engine_nodes_used(az_engine *e, int32_t slot, int32_t *n_nodes);
int az_engine_grow_pools(az_engine *e, int32_t node_capacity);

/* ---- arena support: Arena.play_game(s) (arena.py:36-185) for all slots at once -----------
 * h_sides[g] = +1/-1: the colour this engine searches for in slot g (0 = both colours, self-play).  az_engine_search
 * then only touches slots where that colour is to move.  az_engine_best_moves = MCT.get_action_probs(temp = 0) for
 * those slots (-1 elsewhere); az_engine_baseline_moves = RandomPlayer (kind 0) / GreedyPlayer (kind 1)
 * (players.py:76-123) for the slots where the OTHER colour is to move; az_engine_play applies a move vector
 * (-1 = none) to the boards and trees; az_engine_root_status reads every slot's position back (h_score = Board.get_score of
 * the side to move: sum(player*grid) for Othello / Connect4; TicTacToe 32767 for the reference's +inf, tictactoe.py:119-126, else 0). */
int az_engine_set_sides(az_engine *e, const int8_t *h_sides, int32_t n);
/* az_engine_best_moves is visit-based in every search mode: on an engine in the Gumbel mode it is NOT the move az_engine_advance
 * plays.  The move a player plays now is az_engine_player_moves. */
int az_engine_best_moves(az_engine *e, int32_t *h_actions);
/* The move every slot's player plays now, one launch, one thread per slot.  h_actions: HOST int32 [n_slots].  h_actions[g] equals
 * d_action[g] of az_engine_root_readout called with every temperature equal to `temp`: it is what az_engine_advance would play at
 * that temperature.  -1 unless the engine searches the slot now (active and, with sides set, its colour to move) and the root is
 * expanded with at least one child.  In the Gumbel mode (az_engine_set_gumbel) it is the Gumbel move over the slot's current
 * candidate set, whatever `temp` is.  With the mode off and temp == 0 it equals az_engine_best_moves element for element, with the
 * same AZ_P_TIE_MOVE draw; with temp > 0 the move is sampled on the AZ_P_MOVE_SAMPLE draw of (seed, game id, ply).  Reads only:
 * trees, boards, counters, samples and streams stay as they are.  AZ_EINVAL: a null argument, a `temp` that is negative or not
 * finite; AZ_ESTATE while a search is open. */
int az_engine_player_moves(az_engine *e, double temp, int32_t *h_actions);
int az_engine_baseline_moves(az_engine *e, int32_t kind, uint32_t seed, int32_t *h_actions);
/* az_engine_search in two halves, so that the arena's two players (arena.py:135-140: player1.get_move / player2.get_move, each on
 * the games where it is to move) think at the same time: _begin queues the search on the engine's own stream and returns, _end
 * waits for it and reports what az_engine_search would have.  Only calls on OTHER engines may come between the two. */
int az_engine_search_begin(az_engine *e, int32_t n_sim);
/* puts b's stream on a hardware queue that a's does not share (a stream of another priority), so that the two searches really
 * run side by side; before b's first search */
int az_engine_pair(az_engine *a, az_engine *b);
/* Slot groups of az_engine_run: the engine's slots are split into n contiguous groups (boundaries at multiples of the 16 games
 * a search block holds), and every group plays its plies as a launch chain of its own -- its own stream (the later groups' from
 * the other priority pool, as az_engine_pair), its own leaf-row counters and rows of the network batch, its own lane of the net,
 * its own linear search graph -- so that one group's tree kernels run while another group's network kernels hold the matrix
 * pipe.  The host keeps one ply queued per group.  Games depend on (seed, game id) only: the samples are the same rows bit for
 * bit, appended in another order.  n in {1, 2, 4}; 0 = auto (the default: the measured rule on game and slot count, DESIGN
 * section 20; 1 wherever groups are not served).  Served: az_engine_run of AZ_EVAL_NET / AZ_EVAL_FAKE engines in the plain
 * search.  Not served (auto: 1; an explicit n > 1: AZ_EINVAL naming the mode): AZ_EVAL_EXTERNAL, AZ_EVAL_ROLLOUT, either
 * symmetry mode, leaf_batch > 1, the Gumbel search, an engine of one block (16 slots) or less.  az_engine_search / _search_begin / _advance
 * never group.  Under az_net_profile a run plays as one group (today's launch sequence, so the profiled step describes
 * full-width kernels).  AZ_ENGINE_GROUPS=n in the environment overrides the setting at az_engine_create (ignored, as auto is,
 * by engines that do not serve groups).  Drops the captured graphs; AZ_ESTATE while a search is open.
 * az_engine_groups: the groups the next az_engine_run would play with. */
int az_engine_set_groups(az_engine *e, int32_t n);
int az_engine_groups(az_engine *e, int32_t *n);
int az_engine_search_end(az_engine *e);
int az_engine_root_status(az_engine *e, int8_t *h_players, uint8_t *h_over, int8_t *h_winner, int32_t *h_score);

/* Every leaf evaluation of this engine -- the root-prior pass and every lock-step -- averaged over the symmetries in `mask`
 * (az_net_forward_sym above: same codes, same arithmetic, on the pending rows only).  Off (mask 0) by default and after
 * az_engine_set_symmetry(e, 0), when the launch sequence is exactly the plain one.  Costs two small launches per lock-step and n
 * times the network rows.  The engine's cached search graphs are dropped.  AZ_EINVAL: a code the game or board does not have,
 * an engine whose evaluator is not AZ_EVAL_NET, a net with max_batch < n * n_slots; AZ_ESTATE while a search is open. */
int az_engine_set_symmetry(az_engine *e, int32_t mask);

/* Every leaf evaluation of this engine in ONE randomly drawn member of `mask` (the form AlphaGo Zero used in self-play and in match
 * play): the orientation bias of the network averages out over a search at the row count of the plain search.  The mask, its codes
 * and their validity are those of az_engine_set_symmetry; AZ_SYM_ALL = every valid code; 0 = off (the default), when the launch
 * sequence and every bit are the plain ones.  Contract -- members = the mask's codes in ascending order, n of them; every pending
 * network row (the fresh root of the root-prior pass or a leaf selected for evaluation) is evaluated in exactly one member:
 *   r = Philox4x32-10 keyed (seed, game_id[slot]) at counter (ply[slot], s, AZ_P_SYMMETRY = 8, 0)
 *   m = (uint32)(((uint64)r.x * n) >> 32),   code = members[m]
 * with s = (uint32)(sim + the simulations already run on this root) for the leaf of simulation sim (leaf_batch K: walker j of
 * lock-step t has sim = t * K + j) and s = 0xFFFFFFFF for the root-prior pass; ply is the root's ply.  The draw is a function of
 * the game alone, never of the slot, the row, the batch shape or the GPU.  The row is then evaluated as az_net_forward_sym_codes
 * evaluates a row with that code; the renormalisation over the legal moves that follows is untouched.  A mask that holds the
 * identity alone reproduces the plain search bit for bit.  Costs two small launches per lock-step and no extra network rows: it
 * needs max_batch >= leaf_batch * n_slots only, and composes with az_engine_set_leaf_batch in either order of the two calls.
 * Mutually exclusive with a non-zero ensemble mask: each of the two setters refuses while the other mode is in force.  The engine's
 * cached search graphs are dropped.  AZ_EINVAL: a code the game or board does not have, an engine whose evaluator is not
 * AZ_EVAL_NET, an ensemble mask in force, a net with max_batch < leaf_batch * n_slots; AZ_ESTATE while a search is open. */
int az_engine_set_symmetry_random(az_engine *e, int32_t mask);

/* Several leaves per slot and lock-step, kept apart by virtual loss.  The reference searches strictly one simulation after the
 * other (mcts.py:127-171 select_node, 197-223 back_propagate, 254-262 the loop of MCT.search); with leaf_batch = K > 1 a search of
 * n_sim simulations is ceil(n_sim / K) lock-steps, each walking up to K simulations ("walkers") per slot before ONE network call
 * on up to K * n_slots rows.  Walker j scores a child c of parent p as if every walker i < j of the same lock-step had already
 * lost through the nodes of its path: with v(x) = the number of those walkers whose path holds x,
 *   Q term  v(c) == 0 ? c.Q : (c.N * c.Q - v(c)) / (c.N + v(c)),     U term  c.P * sqrt(p.N + v(p)) / (1 + c.N + v(c))
 * in float64, one operation at a time.  Nothing virtual is stored: after the search the trees hold real statistics only and every
 * root has grown by exactly n_sim visits.  A walker that lands on the still unevaluated leaf of an earlier walker of its lock-step
 * (a collision) takes no network row and backs up that walker's value; az_engine_collisions counts them since the engine was
 * created.  This is a different search from the reference's: opt-in, default 1, and at 1 the launch sequence and every bit are
 * the plain ones.  For K > 1 the result depends on how simulations are split over search calls (search(3); search(5) walks
 * [3] [4,1], search(8) walks [4,4]); it still depends on nothing but (seed, game id, K) otherwise.  net_evals counts rows.
 * AZ_EINVAL: k outside [1, AZ_MAX_LEAF_BATCH], an AZ_EVAL_EXTERNAL or AZ_EVAL_ROLLOUT engine, k * n_slots beyond the network's
 * max_batch, a symmetry mask in force (and az_engine_set_symmetry refuses a mask while k > 1); AZ_ESTATE while a search is open
 * or from inside an evaluator.  The engine's cached search graphs are dropped. */
#define AZ_MAX_LEAF_BATCH 16
#define AZ_MAX_GROUPS 4  /* slot groups of az_engine_run (az_engine_set_groups) */
int az_engine_set_leaf_batch(az_engine *e, int32_t k);
int az_engine_collisions(az_engine *e, int64_t *n);

/* Gumbel root search ("Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022): the root samples m actions
 * without replacement with Gumbel noise, spends the simulations of a search on them by Sequential Halving, and is read out as the
 * policy improved by the completed Q-values instead of the visit counts -- the form that still improves the policy at 8 to 32
 * simulations.  A different search from the reference's: opt-in, m = 0 (the default) is off, when every launch and every bit are
 * the plain ones; 1 <= m <= AZ_MAX_GUMBEL switches it on.  Python's defaults: m 16, c_visit 50, c_scale 0.5 (Q is in [-1, 1] here:
 * the paper's c_scale 1 on values in [0, 1]), gumbel_scale 1; gumbel_scale 0 is a deterministic search for evaluation play.
 * While it is on no root noise is applied (F_NOISED stays clear), the move ignores the temperature schedule, and the walk below
 * the root is the plain PUCT walk.  Contract -- the root's children 0 .. nch - 1 in child-index order, float64, one operation at
 * a time:
 *   logit(a) = az_det_log of P(a)                   (the engine's deterministic log; -inf for P = 0)
 *   g(a)     = 0.0 when gumbel_scale == 0 (no draw); else gumbel_scale * (-L(-L(u))) with L = az_det_log,
 *              r = Philox4x32-10 keyed (seed, game_id) at counter (ply, 0xFFFF, AZ_P_GUMBEL = 9, action(a)),
 *              u = the 53-bit uniform az_u53 of (r.x, r.y), replaced by 2^-53 when 0: one draw per (game, ply, action), the same in every phase and
 *              every search call on that root, never a function of slot, row or batch shape
 *   vmix     = (sum over N(b) > 0 of P(b) Q(b)) / (sum over N(b) > 0 of P(b)), both in child-index order; 0.0 when no child is
 *              visited (or the divisor is 0).  The root's own network value is discarded, as the reference discards it: this is
 *              the visited-children term of the paper's v_mix alone (az_engine_set_gumbel_full below keeps the value and mixes it in)
 *   cq(a)    = N(a) > 0 ? Q(a) : vmix               (Q is in the root mover's frame)
 *   maxN     = max N(b), the real counts, visits kept by a re-rooting included
 *   sigma(a) = ((c_visit + (double)maxN) * c_scale) * cq(a)
 *   score(a) = (g(a) + logit(a)) + sigma(a)
 * Schedule, a pure function of (n, m0) with n the n_sim of the search call and m0 = min(m, nch); every search call runs a whole
 * schedule over the root's statistics as they stand.  m0 = 1: all simulations to child 0.  Otherwise L = ceil(log2 m0); phase p
 * considers m_p candidates, m_0 = m0, m_{p+1} = max(2, m_p / 2), for v_p = max(1, n / (L m_p)) rounds (integer divisions) of one
 * visit per candidate; phases follow each other until n simulations are dealt: the phase of two repeats, the last phase is cut.
 * At the first simulation of a phase the candidates become the m_p best by score of the previous set (phase 0: of all children),
 * ties -- among -inf too -- to the lowest child index whatever the tie mode; simulation i of a phase goes to candidate i mod m_p in
 * ascending child index.  The root is expanded as ever (first visit, then the walk stops at the child).
 * Move (az_engine_advance, az_engine_root_readout): the candidate of the slot's current set with the highest score on the final
 * statistics, lowest index among equals; an empty set (after this setter, after a move) means all children.  Policy target:
 * pi'(a) = E(x(a) - max x) / sum with E = az_det_exp, x(a) = logit(a) + sigma(a) (no g), the sum in child-index order, stored as float32 where
 * the visit-count policy is stored (the samples' pi, d_pi of the readout); the visits stay the visit counts.  A NaN score is
 * reported like a NaN PUCT score.  az_engine_best_moves stays visit-based; az_engine_player_moves reads this move.
 * AZ_EINVAL: m outside [0, AZ_MAX_GUMBEL]; with m > 0 a constant that is negative or not finite, an AZ_EVAL_ROLLOUT or
 * AZ_EVAL_EXTERNAL engine, leaf_batch > 1 in force (az_engine_set_leaf_batch(k > 1) in turn refuses while this mode is on);
 * AZ_ESTATE while a search is open.  The cached search graphs are dropped and the slots' candidate sets cleared; the symmetry
 * modes act on network rows and combine.  az_engine_gumbel_considered reads a slot's candidate set (bit i = child i). */
#define AZ_MAX_GUMBEL 16
int az_engine_set_gumbel(az_engine *e, int32_t m, double c_visit, double c_scale, double gumbel_scale);
int az_engine_gumbel_considered(az_engine *e, int32_t slot, uint64_t *mask);

/* Several Sequential Halving leaves per network call: gumbel_batch = K walkers per slot and lock-step for the Gumbel mode only
 * (az_engine_set_leaf_batch and az_engine_set_gumbel keep refusing each other).  Opt-in, default 1; accepted with the mode on or off
 * and in force only while m > 0: with the mode off, or at K = 1, every launch and every bit are unchanged.  Everything not named
 * here is the contract of az_engine_set_gumbel.  Sequential Halving fixes the root child of every simulation of a phase before the
 * phase starts, so the walks of a round run in disjoint subtrees.  The schedule depends on m0 = min(m, nch), which differs from
 * slot to slot, so each searching slot keeps a cursor s = the simulations of this search call already dealt:
 *   the search's first launch sets s = 0; a lock-step of the slot runs kt = min(K, end of the current phase - s, n - s) walkers
 *   j = 0 .. kt - 1; walker j is simulation s + j (plus the simulations already run on this root in every Philox counter, the
 *   symmetry draw of az_engine_set_symmetry_random included); then s += kt.  No lock-step crosses a phase boundary: a re-ranking
 *   can only fall on walker 0 and sees real statistics only, every earlier walker being backed up.  A root without children, and
 *   m0 = 1, take the one phase of n: all simulations to child 0, ceil(n / K) lock-steps.
 *   The host enqueues Lmax(n, m, K) = max over m0 in 1 .. m of the length of that plan (az_gumbel_locksteps; -1 for arguments out
 *   of range) lock-steps and the final backup-only launch -- a pure function, so the sequence captures as a graph; a slot whose
 *   plan is shorter idles in the rest (no walker, no row).  lockstep_iters grows by Lmax + 1 per search.
 *   The walkers of a lock-step run in ascending j, strictly one after the other.  Walker j takes the root step of the Gumbel mode
 *   -- the expansion on the first visit, child = candidate (i mod m_p), stop when the root was fresh or the child's real N is 0 --
 *   with no virtual count (the pick is forced), then descends from depth 1 with az_engine_set_leaf_batch's virtual-count scores over
 *   the earlier walkers' recorded paths (the root's child is node 1 of a path).  Leaf status, collisions (az_engine_collisions:
 *   with K > m_p several walkers share a root child and, while its N is 0, its pending leaf), backup order and node allocation
 *   order are az_engine_set_leaf_batch's.
 * Every root grows by exactly n visits per search call; the result is a function of (seed, game id, m, constants, K, n), never of
 * the slot, the slot count or the block.  AZ_EINVAL: k outside [1, AZ_MAX_LEAF_BATCH]; k > 1 while an ensemble mask is in force
 * (and az_engine_set_symmetry refuses a mask while k > 1); k * n_slots beyond the network's max_batch while the mode is on (with it
 * off az_engine_set_gumbel refuses then); AZ_ESTATE while a search is open.  A change of the walkers in force drops the cached
 * search graphs. */
int az_engine_set_gumbel_batch(az_engine *e, int32_t k);
int az_gumbel_locksteps(int32_t n_sim, int32_t m, int32_t k);

/* Full Gumbel search: the paper's v_mix with the node's own network value, and its deterministic selection below the root.  A switch
 * on top of the Gumbel mode: opt-in, default 0; accepted with the mode on or off and in force only while m > 0 (as gumbel_batch);
 * with it off nothing is allocated, no kernel touches the values and every launch and every bit are unchanged.  It works at
 * gumbel_batch 1 and above and with both symmetry modes the Gumbel mode combines with.  Everything not named here is the contract of
 * az_engine_set_gumbel and az_engine_set_gumbel_batch.  While it is in force:
 *   1. Every evaluated node keeps vhat = the raw float32 value row of the network call that evaluated it, in the frame of the player
 *      to move at the node (a fresh root's value is still not backed up, but it is kept).  A re-rooting copies the values with the
 *      nodes; az_engine_grow_pools moves them with the pools.
 *   2. For a node p with children b, in float64, one operation at a time, sums in child-index order:
 *        sumN = sum of N(b) (the real counts);  num, den = the sums over N(b) > 0 of P(b) Q(b) and of P(b)
 *        vmix(p) = vhat(p) when sumN == 0 or not den > 0; else (vhat(p) + (double)sumN * (num / den)) / (double)(1 + sumN)
 *      and this vmix replaces az_engine_set_gumbel's wherever that is used: the scores of Sequential Halving, the move, the policy
 *      target (samples' pi, d_pi of the readout; layouts unchanged).
 *   3. Below the root (depth >= 1) walker j at parent p takes, instead of the PUCT child, the maximum of
 *        key(b) = pi'(b) - (double)(N(b) + v(b)) / (double)(1 + sumN + vsum)
 *      with v(b) = the virtual count of az_engine_set_leaf_batch (the walkers i < j of this lock-step whose recorded path holds b;
 *      all 0 at gumbel_batch 1), vsum their sum over p's children, and pi' the policy target's formula at p:
 *        maxN = max N(b);  k = (c_visit + (double)maxN) * c_scale;  cq(b) = N(b) > 0 ? Q(b) : vmix(p)
 *        x(b) = L(P(b)) + k * cq(b);  e(b) = E(x(b) - max x);  pi'(b) = e(b) / sum e      (L = az_det_log, E = az_det_exp)
 *      Only real counts enter vmix, maxN and pi'.  Ties go to the lowest child index whatever the tie mode: no Philox draw is made
 *      below the root.  A NaN key is reported like a NaN PUCT score.  Break tests, first-visit expansion, leaf status, collisions,
 *      backup and allocation order are unchanged; the root step stays the scheduled pick.
 * A value that was never stored is never read: the call that brings the switch into force (this setter with on = 1 while m > 0, or
 * az_engine_set_gumbel(m > 0) with the switch on) returns AZ_ESTATE while an active slot's root is already evaluated -- start the
 * trees afresh first (az_engine_set_roots, az_engine_run; Python: set_roots, reset).  AZ_EINVAL: on outside {0, 1}; AZ_ESTATE while
 * a search is open.  A change of the value drops the cached search graphs.
 * az_engine_root_value reads vhat of a slot's root (inspection, as az_engine_gumbel_considered); AZ_ESTATE when the switch is not
 * in force, the slot holds no game or its root is not evaluated. */
int az_engine_set_gumbel_full(az_engine *e, int32_t on);
int az_engine_root_value(az_engine *e, int32_t slot, float *v);

/* Playout cap randomization (KataGo: Wu 2019, "Accelerating Self-Play Learning in Go", section 3.1): most plies of a self-play game are
 * searched with a few simulations and only played, a share p_full of them is searched in full and recorded, so that games -- and
 * with them independent value targets -- get cheaper while every recorded policy target comes from a full search.  The reference has
 * no counterpart: it spends config.simulations on every ply (trainer.py:215-273).  Opt-in: n_fast = 0 (the default) is off, when no
 * launch, kernel, allocation or output bit differs from an engine that never had it on; p_full is then not looked at.  On:
 * n_fast in [1, cfg.n_sim), p_full in (0, 1].  Contract:
 *   the coin of a ply   r = Philox4x32-10 keyed (seed, game_id) at counter (ply, 0xFFFF, AZ_P_PLAYOUT_CAP = 10, 0),
 *                       u = the 53-bit uniform az_u53 of (r.x, r.y); the ply is FULL iff u < p_full (p_full = 1.0: every ply).
 *                       One draw per (game id, ply): never a function of the slot, the slot group, the batch or the games resident.
 *   full ply            exactly the search with the mode off: every simulation of the search call, root noise under the engine's
 *                       noise mode, the sample recorded.
 *   fast ply            in a search call of n simulations the slot takes part in the lock-steps of the local simulation indices
 *                       s < min(n, n_fast) only (every search call on the root walks that budget again); after them it neither
 *                       walks nor takes a network row, and the backup that follows does nothing for it.  No root noise is applied
 *                       and the root is not marked as noised.  A fresh root is still evaluated in the root-prior pass.  The move is
 *                       chosen and played as ever -- temperature schedule, the AZ_P_MOVE_SAMPLE / AZ_P_TIE_MOVE draws, re-rooting --
 *                       but NO sample is recorded: `samples` does not grow, no pi / visits / state / meta row is written, and the
 *                       end-of-game z patch skips the ply.  The tree under the played move is kept as on any ply: a full ply that
 *                       follows inherits it (and applies its root noise on top).
 *   counters            az_engine_stats.plies counts every ply; az_engine_playout_cap_stats reads the plies played after a full and
 *                       after a fast search since the last az_engine_run / az_engine_set_roots, counted while the mode is on (both 0
 *                       with it off).  After a run with the mode on: samples == full_plies, plies == full_plies + fast_plies.
 * meta's move_idx stays the ply, so a game's samples have gaps.  A game still depends on (seed, game id, n_fast, p_full) only.
 * Served: the plain search of AZ_EVAL_NET / AZ_EVAL_FAKE engines through az_engine_run (1, 2 or 4 slot groups), az_engine_search,
 * _search_begin / _end and az_engine_advance.  Not served (AZ_EINVAL naming the mode; and while the cap is on the setters of those
 * modes refuse, naming the cap): leaf_batch > 1, the Gumbel search, either symmetry mode, AZ_EVAL_ROLLOUT, AZ_EVAL_EXTERNAL.
 * AZ_EINVAL also: n_fast outside [0, n_sim), p_full outside (0, 1] or not a number; AZ_ESTATE while a search is open.  A change of
 * either value drops the cached search graphs.
 * az_playout_cap_full: the coin as pure host code, 1 = full, 0 = fast; the arithmetic of the kernels (no engine, no GPU). */
int az_engine_set_playout_cap(az_engine *e, int32_t n_fast, double p_full);
int az_engine_playout_cap_stats(az_engine *e, int64_t *full_plies, int64_t *fast_plies);
int az_playout_cap_full(uint32_t seed, uint32_t game_id, int32_t ply, double p_full);

/* Forced playouts and policy target pruning (KataGo: Wu 2019, "Accelerating Self-Play Learning in Go", section 3.2): on a fully
 * searched ply every root child that has been visited at all receives at least sqrt(k P(c) N_root) playouts, so that a move the
 * noise proposed is explored far enough to be refuted or confirmed; when the ply's policy is read, the forced playouts PUCT would
 * not have spent are subtracted again and a child left with a single playout is removed, so that the recorded target -- and the move
 * drawn from it -- describe what the search believes.  The reference has no counterpart.  Opt-in: k = 0 (the default) is off, when
 * no launch, kernel, allocation or output bit differs from an engine that never had it on.  Every operation below is one IEEE double
 * operation in the order written (the library is built with -ffp-contract=off); sqrt is the correctly rounded one.  Contract:
 *   switch      k > 0 on (KataGo: k = 2), k = 0 off; k finite and in [0, 64], anything else AZ_EINVAL.
 *   forced ply  a ply of a slot this engine searches, the mode on, that is full in the playout cap's sense: every ply with the cap
 *               off, with it on the plies whose coin az_playout_cap_full(seed, game id, ply, p_full) says full.  Fast plies take
 *               no forced playouts and no pruning.
 *   selection   at depth 0 of a simulation's walk on a forced ply only.  R.N = the root's visit count as PUCT's square root takes
 *               it at that selection.  Child c is FORCED iff c.N > 0 && (double)c.N * (double)c.N < (k * c.P) * (double)R.N, with
 *               c.P the stored prior, root noise included (no square root is taken).  A forced child's key is +inf, every other
 *               child keeps its PUCT key, and the maximum is chosen as ever: several forced children are an ordinary tie
 *               (AZ_TIE_RANDOM: the AZ_P_TIE_SELECT draw of that (ply, simulation, depth 0); AZ_TIE_LOWEST: the lowest index).
 *               A fresh root has R.N = 0, so nothing is forced; a root inherited from the ply before applies the rule to the counts
 *               it inherited.  Below the root nothing changes.
 *   pruning     wherever the root's policy is read on a forced ply at a temperature other than 0 (az_engine_run / _advance,
 *               az_engine_root_readout, az_engine_player_moves).  c* = the child with the greatest N (lowest child index among
 *               equals, no draw); sq = sqrt((double)R.N); star = c*.Q + (c*.P * sq) / (double)(1 + c*.N).  The pruned count N'
 *               equals N for c* and for children with N = 0.  For every other child:
 *                 nf = (int)sqrt((k * c.P) * (double)R.N);  gap = star - c.Q;
 *                 need = c.N if gap <= 0.0; otherwise want = (c.P * sq) / gap - 1.0, and need = c.N if want >= (double)c.N,
 *                 else (int)floor(want) + 1;
 *                 N' = min(c.N, max(c.N - nf, need, 0));  if N' < c.N && N' <= 1 then N' = 0.
 *               The temperature formula (n at temperature 1, az_det_pow otherwise) takes N' in place of N for the recorded pi and
 *               for the move drawn from it, with the same AZ_P_MOVE_SAMPLE draw.  At temperature 0 nothing changes (the most
 *               visited child by the raw counts, pi one-hot).  The visits rows stay the raw counts.
 *   counters    az_engine_forced_playouts_stats: forced_picks = the root selections in which at least one child was forced, folded
 *               in once per ply when the move is played; pruned_playouts = the sum of N - N' over the recorded plies.  Since the
 *               last az_engine_run / az_engine_set_roots; both 0 with the mode off.  az_engine_stats is unchanged.
 * A readout's pi and action stay bit-equal to what az_engine_advance records and plays under the mode.
 * Served: the plain PUCT search of AZ_EVAL_NET / AZ_EVAL_FAKE engines through az_engine_run (1, 2 or 4 slot groups), az_engine_search,
 * _search_begin / _end, az_engine_advance and az_engine_root_readout, with the playout cap on or off.  Not served (AZ_EINVAL naming
 * the mode; and while the mode is on the setters of those modes refuse, naming forced playouts): leaf_batch > 1, the Gumbel search,
 * either symmetry mode, AZ_EVAL_ROLLOUT, AZ_EVAL_EXTERNAL.  AZ_ESTATE while a search is open.  A change of k drops the cached
 * search graphs.
 * az_forced_playout: the forced test as pure host code, 1 = forced (0 also for k <= 0); az_forced_prune: the pruned counts of a
 * root's n_children children (N, Q, P in child order) into out_N, AZ_OK or AZ_EINVAL; k = 0 copies N.  The kernels' arithmetic. */
int az_engine_set_forced_playouts(az_engine *e, double k);
int az_engine_forced_playouts_stats(az_engine *e, int64_t *forced_picks, int64_t *pruned_playouts);
int az_forced_playout(int32_t n, double p, int32_t root_n, double k);
int az_forced_prune(int32_t n_children, const int32_t *N, const double *Q, const double *P, int32_t root_n, double k, int32_t *out_N);

/* ---- resignation in self-play: a value threshold, a holdout and a game log ---------------------------------------
 * AlphaGo Zero / AlphaZero (Silver et al. 2017, "Mastering the game of Go without human knowledge", Methods: self-play): a game whose
 * search value has fallen below v_resign is given up; a share of the games is played out anyway so that the threshold's
 * false-positive rate is known, and v_resign is set from that share.  The reference has no counterpart: it plays every game to the
 * end (trainer.py:215-273).  Opt-in, default off: with the mode off no launch, kernel, allocation or output bit differs from an
 * engine that never had it on, and the four counters read 0.  Every operation below is one IEEE double operation in the order written.
 *   settings      v_resign in [-1, 0); consecutive = k in [1, 4]; min_ply >= 0; p_holdout in [0, 1].  OFF is spelled v_resign = NaN
 *                 (the other three are then not looked at).  AZ_EINVAL outside the ranges, AZ_ESTATE while a search is open.  The
 *                 settings are arguments of k_move alone, which is launched and never captured: no cached search graph holds them,
 *                 so a change drops none.
 *   value of a ply  from the root's children after the ply's search, in pool order i = 0 .. nc - 1:  S_N = sum N_i;
 *                 S_Q = sum over N_i > 0 of (double)N_i * Q_i, accumulated in that order in float64;  v_mean = S_Q / (double)S_N;
 *                 v_best = Q of the child with the greatest N (the lowest child index among equals);
 *                 v = v_best > v_mean ? v_best : v_mean.  A child's Q is the value for the root's mover.  The rule reads the raw N
 *                 and Q only: forced playouts are not pruned, proofs and the Gumbel search's completed Q are not consulted.
 *                 S_N == 0: the ply is untested.  az_resign_value is this arithmetic as pure host code, the function the kernels
 *                 call: *v = the value, NaN when S_N == 0; AZ_EINVAL for a null argument or a negative count.
 *   tested plies  the test runs when the ply's move is played (k_move), after the ply was recorded, counted and played exactly as
 *                 with the mode off, and only if the rules have not ended the game.  A ply p < min_ply is untested, and so is a fast
 *                 ply of the playout cap.  A tested ply pushes v into the mover's window of its last k tested values (one window per
 *                 side and game).  m = the maximum of a full window; low[side] = the minimum of m over the game, 2.0 while the
 *                 window has never been full.  The side TRIGGERS at the first ply where m < v_resign -- so it triggers at a
 *                 threshold t exactly when low < t, the statistic calibration needs.
 *   holdout       per game: r = Philox4x32-10 keyed (seed, game_id) at counter (0, 0xFFFF, AZ_P_RESIGN = 11, 0), u = az_u53 of (r.x, r.y);
 *                 the game is a holdout iff u < p_holdout.  Never a function of the slot, the slot group or the batch.
 *                 az_resign_holdout: the coin as pure host code, 1 = holdout.
 *   on a trigger  in a game that is not a holdout the mover resigns: the game ends at that ply with winner -mover, z is written with
 *                 that winner, games_done moves and the slot is refilled, on the path a finished game takes.  The ply just played
 *                 stays recorded and counted (under the playout cap samples == full_plies and plies == full + fast still hold).
 *                 In a holdout game only the first trigger is noted (ply, player); the game goes on and low keeps updating.
 *   counters      az_engine_resign_stats, since the last az_engine_run / az_engine_set_roots, counted as games end: resigned;
 *                 holdout_games; holdout_triggered = holdout games with a trigger; holdout_false_positives = those of them with
 *                 winner * trigger_player >= 0 (the side that would have resigned did not lose).
 *   game log      kept while the mode is on: one row per game of the last az_engine_run at index game_id - first_game_id, whatever
 *                 order the games finish in.  Row = int32[8]: game_id, plies, winner, ended (0 the rules / 1 resignation), holdout,
 *                 trigger_ply (-1 none), trigger_player (0 none), 0.  Beside it low = double[2] per game: [0] player +1, [1] player
 *                 -1.  az_engine_game_log returns n and DEVICE views valid until the next az_engine_run or az_engine_destroy; n = 0
 *                 and null views when the last run had the mode off.  p_holdout = 1.0 is the record-only form: every game is logged,
 *                 none is resigned, and the samples are bit-equal to the mode off.
 *   served        az_engine_run with 1, 2 or 4 slot groups, in every search mode and with every evaluator the run serves: the rule
 *                 reads the root's children and nothing else.  az_engine_advance and the arena never resign, whatever the setting.
 *                 A game still depends on (seed, game id, the settings) only.
 *   readout       az_engine_resign_values: d_v[slot] (device, double [n_slots]) = v of the slot's root as it stands, NaN where
 *                 S_N == 0, the root is not expanded or the slot holds no game.  One launch (k_resign_value), with the mode on or
 *                 off: a caller of the batched players or the arena applies its own rule with it. */
int az_engine_set_resign(az_engine *e, double v_resign, int32_t consecutive, int32_t min_ply, double p_holdout);
int az_engine_resign_stats(az_engine *e, int64_t *resigned, int64_t *holdout_games, int64_t *holdout_triggered,
                           int64_t *holdout_false_positives);
int az_engine_game_log(az_engine *e, int64_t *n, const int32_t **d_rows, const double **d_low);
int az_engine_resign_values(az_engine *e, double *d_v);
int az_resign_value(int32_t n_children, const int32_t *N, const double *Q, double *v);
int az_resign_holdout(uint32_t seed, uint32_t game_id, double p_holdout);

/* ---- leaf evaluation cache -------------------------------------------------------------------------------
 * Every game of an az_engine_run wave starts from the same position under one set of weights, and the network is a pure function
 * of (board, side to move): each slot group keeps a table of the network's outputs by exact position, filled and read on the device
 * by the plain search's step kernels.  A leaf found there takes no row of the lock-step's network batch and is backed up from the
 * stored 65 + 1 floats -- the bits the forward would have written, so the samples of a run do not change by a bit.  The table is
 * cleared at the start of every az_engine_run; nothing in it outlives a run or a set of weights.
 *   mode        AZ_EVAL_CACHE_AUTO: the measured rule (on for the shapes where it was measured to pay, az_search_plan.h:
 *               eval_cache_auto); AZ_EVAL_CACHE_OFF; AZ_EVAL_CACHE_ON: wherever it is served.  AZ_ENGINE_EVAL_CACHE in the
 *               environment, read when the engine is created, makes the request where this setter has not been called: unset = auto,
 *               0 = off, 1 = on (engines that do not serve the cache ignore it).
 *   capacity    entries per slot group, a power of two up to 2^22; 0 = the default, 2^18.  A full table, or four occupied entries
 *               behind a position's bucket, is a miss without an insert, never an error.
 *   stone_limit only positions with at most this many stones are looked up or inserted, 1 .. 64; 0 = the default, 12.
 *   counters    az_engine_eval_cache_stats: in_force = whether the next az_engine_run would cache; hits = the leaves answered from
 *               the table since the last az_engine_run began, folded in by every ply's last backup (also az_engine_stats.cache_hits).  az_engine_stats'
 *               net_evals keeps counting every evaluation the search consumed: net_evals - hits rows went through the network.
 * Served: az_engine_run (1, 2 or 4 slot groups) of an AZ_EVAL_NET engine in the plain PUCT search, with the playout cap and forced
 * playouts on or off.  Not served -- AZ_EVAL_CACHE_ON then answers AZ_EINVAL naming the mode, here or from az_engine_run if the mode
 * came later; the rule and the environment switch answer off: AZ_EVAL_FAKE / _ROLLOUT / _EXTERNAL, either symmetry mode, leaf_batch
 * > 1, the Gumbel search.  Never used, whatever the request: az_engine_search / _search_begin / az_engine_advance (the arena), and
 * a run whose net is under az_net_profile.  AZ_ESTATE while a search is open.  A change drops the cached search graphs. */
#define AZ_EVAL_CACHE_AUTO (-1)
#define AZ_EVAL_CACHE_OFF 0
#define AZ_EVAL_CACHE_ON 1
int az_engine_set_eval_cache(az_engine *e, int32_t mode, int32_t capacity, int32_t stone_limit);
int az_engine_eval_cache_stats(az_engine *e, int32_t *in_force, int64_t *hits);

/* The heads inside the search step kernel (ABI 117).  Where the form is in force az_engine_run's lock-step forwards
 * stop behind fc2 and the step kernels that hold a backup (k_step_heads) compute the policy / value heads of their own slots' rows
 * themselves, with k_heads2's arithmetic: four launches per lock-step for five, the same samples bit for bit.
 *   switch   AZ_ENGINE_STEP_HEADS in the environment, read when the engine is created: unset = the measured rule (az_search_plan.h:
 *            step_heads_auto), 0 = never, 1 = wherever served.
 *   served   az_engine_run (any slot groups, the evaluation cache on or off) of an AZ_EVAL_NET engine in the plain PUCT search whose
 *            net az_net_heads_view serves.  Not served, whatever the switch says: the playout cap, forced playouts, exact endgames,
 *            proof backup, PUCT settings, the Gumbel search, leaf_batch > 1, either symmetry mode, the external, fake and rollout
 *            evaluators; az_engine_search / _search_begin / az_engine_advance (the arena); a run whose net is under az_net_profile.
 * az_engine_step_heads: in_force = whether the next az_engine_run would run the form, used = whether the last one did. */
int az_engine_step_heads(az_engine *e, int32_t *in_force, int32_t *used);

/* ---- exact endgames in the search -------------------------------------------------------------------------
 * Near the end of a game the outcome of a position is a short alpha-beta away (az_solve_batch above): with the mode on the search
 * backs a late leaf up with that outcome instead of the network's guess, and the leaf takes no row of the network batch.  The
 * reference has no counterpart.  Opt-in: max_empties = 0 (the default) is off, when no launch, kernel, allocation or output bit
 * differs from an engine that never had it on; 1 .. AZ_EXACT_MAX_EMPTIES switches it on.  Contract:
 *   solved leaf   the leaf a simulation's walk ends on (depth >= 1) whose game is not over (az_status is tested first: a finished
 *                 game is never marked solved) and which has empties = popcount(valid cells & ~(p1 | m1)) <= max_empties.  Its
 *                 outcome w under optimal play by both sides is computed on the spot by az_solve.h's solver, without a budget:
 *                 every such leaf is solved.  The node is marked as a terminal node with winner w plus the flag bit F_SOLVED,
 *                 and from then on it IS a terminal node: no batch row, no input written, never children, backed up with
 *                 outcome = w now and on every later visit, not counted in net_evals.  (A solve that reached the solver's
 *                 iteration ceiling raises the engine's internal-error flag and leaves the leaf to the network.)
 *   solved root   a solved node that becomes a root -- the played move leads to it (az_engine_run, az_engine_advance), or
 *                 az_engine_play keeps it -- loses the terminal and the solved flag and keeps its N and Q: an unevaluated,
 *                 unexpanded root.  The root-prior pass evaluates it (the value discarded as ever), and its children are solved in
 *                 turn as the search reaches them.  The clearing is keyed on F_SOLVED: trees of an engine with the mode off never
 *                 take the branch.
 *   nothing else  PUCT, root noise, temperature, the move draw, the samples and z stay as they are.  A game depends on (seed, game
 *                 id, max_empties) only, never on the slot, the slot group or the batch.
 *   counters      az_engine_exact_endgame_stats: solved_leaves = the leaves solved (each node once: first-time solves;
 *                 deterministic), solver_nodes = the positions the solver entered for them (informational: it depends on where
 *                 the lanes of a group were stopped).  Since the last az_engine_run / az_engine_set_roots; both 0 with the mode
 *                 off.  az_engine_stats is unchanged.
 * Served: the plain PUCT search of AZ_EVAL_NET / AZ_EVAL_FAKE engines through az_engine_run (1, 2 or 4 slot groups),
 * az_engine_search, _search_begin / _end, az_engine_advance and az_engine_root_readout, with the leaf evaluation cache in force or
 * not (a leaf is tested for solving before the cache is consulted; a solved leaf is neither looked up nor inserted).  Not served
 * (AZ_EINVAL naming the mode; and while exact endgames are on the setters of those modes refuse, naming exact endgames):
 * leaf_batch > 1, the Gumbel search, either symmetry mode, the playout cap, forced playouts, AZ_EVAL_ROLLOUT, AZ_EVAL_EXTERNAL.
 * AZ_EINVAL also: max_empties outside [0, AZ_EXACT_MAX_EMPTIES].  AZ_ESTATE while a search is open, and for a change of the value
 * while an active slot holds a searched tree (its leaves were classified under the old value): start the trees afresh first
 * (az_engine_set_roots, az_engine_run).  A change drops the cached search graphs. */
#define AZ_EXACT_MAX_EMPTIES 10
int az_engine_set_exact_endgame(az_engine *e, int32_t max_empties);
int az_engine_exact_endgame_stats(az_engine *e, int64_t *solved_leaves, int64_t *solver_nodes);

/* ---- proof backup: MCTS-Solver (Winands, Bjornsson, Saito 2008) ---------------------------------------------
 * A finished game, or under exact endgames a solved leaf, is a terminal node whose winner is the truth.  With the mode on that
 * truth is backed up the tree as a proof, not only averaged into Q: a node is proven as soon as its children decide it, proven
 * nodes are not searched again, and the move and the policy target respect the proofs.  The reference has no counterpart.
 * Opt-in: on = 0 (the default) is off, when no launch, kernel, allocation or output bit differs from an engine that never had it
 * on.  Outcomes are absolute player ids in {-1, 0, +1}, as az_status and the solver report them; the mover of the node at path
 * position i (the root is 0) is root_player * (-1)^i -- an Othello pass is an action, the side to move alternates strictly.
 *   proven node   a node that has been backed up (N > 0; an unvisited child is never proven) and is either terminal (a finished
 *                 game, or a solved leaf of exact endgames), proven with its winner, or an expanded node p of mover m that
 *                 carries the flag bit F_PROVEN = 64 with the outcome in its winner byte.  p is proven when some child is proven
 *                 with outcome m -- then its outcome is m -- or when every one of its children is proven -- then 0 if some
 *                 child's outcome is 0, else -m.
 *   propagation   in the backup of a simulation whose leaf was terminal or proven (and of no other), after the unchanged N / Q
 *                 update: from the leaf's parent upward the rule is applied to each path node; a node it proves is marked and
 *                 the walk up goes on, the first node it does not prove ends it.  So between any two kernels an expanded node
 *                 carries F_PROVEN exactly when the rule holds for its children.  N and Q arithmetic does not change: a proven
 *                 node returns its exact outcome as the backup's reward, Q is never set to an infinity.  Re-rooting copies the
 *                 flag and the outcome; a proven root stays proven (a solved root is cleared as under exact endgames alone).
 *   walk          below the root a walk stops on an F_PROVEN node as on a terminal one: outcome = the node's, no network row,
 *                 no solver call, no cache lookup.  The root never stops a walk: every root grows by exactly n_sim visits.
 *   selection     at every depth a child proven as a loss for the parent's mover is no candidate, unless every child is one
 *                 (a root only).  At the root a child proven as a win for the root's mover takes the key +inf.  Ties among equal
 *                 keys are drawn as ever, among the candidates.
 *   move, target  wherever the move and the policy target are read (az_engine_run, az_engine_advance, az_engine_root_readout,
 *                 az_engine_player_moves): if some root child is a proven win for the root's mover only such children keep their
 *                 visit counts; otherwise children proven as the mover's loss count 0, unless all children are such -- or no
 *                 other child has been visited, when the counts stay as they are.  The temperature arithmetic then runs on those
 *                 counts, at temperature 0 included.  The visits rows, az_engine_best_moves, z and the samples' states are
 *                 untouched.
 *   nothing else  A game depends on (seed, game id, the mode, exact endgames' max_empties) only, never on the slot, the slot
 *                 group, the batch or the cache.
 *   counters      az_engine_proof_backup_stats: proven_nodes = interior nodes marked, each at its marking; proof_stops = walks
 *                 that ended on an F_PROVEN node; pruned_plies = plies played whose counts the rule changed.  Since the last
 *                 az_engine_run / az_engine_set_roots; all 0 with the mode off.  az_engine_stats is unchanged.
 *   root proofs   az_engine_root_proofs: d_out[slot] (device, int8 [n_slots]) = the proven outcome of the slot's root, or
 *                 AZ_UNSOLVED for a root that is not decided and for a slot without a game.  One launch; served with the mode
 *                 on or off (off: no interior node is ever marked).
 * Served where exact endgames are, and together with them, the leaf evaluation cache and slot groups.  Not served (AZ_EINVAL
 * naming the mode; and while proof backup is on the setters of those modes refuse, naming proof backup): leaf_batch > 1, the
 * Gumbel search, either symmetry mode, the playout cap, forced playouts, AZ_EVAL_ROLLOUT, AZ_EVAL_EXTERNAL.  AZ_ESTATE while a
 * search is open, and for a change while an active slot holds a searched tree.  A change drops the cached search graphs. */
int az_engine_set_proof_backup(az_engine *e, int32_t on);
int az_engine_proof_backup_stats(az_engine *e, int64_t *proven_nodes, int64_t *proof_stops, int64_t *pruned_plies);
int az_engine_root_proofs(az_engine *e, int8_t *d_out);

/* ---- PUCT exploration settings: c_init, c_base and first-play urgency ----------------------------------------
 * The search scores a child as Q + P sqrt(N_parent) / (1 + N): PUCT with the exploration constant fixed at 1 and an unvisited
 * child's Q fixed at 0, as the reference has it (Node.PUCT(c_puct=1.0), Q = 0 at construction).  These settings free both: the
 * constant, its growth with the parent's visits as the AlphaZero pseudocode writes it (Silver et al. 2018:
 * c(s) = log((1 + N(s) + c_base) / c_base) + c_init), and first-play urgency, the value an unvisited child is assumed to have
 * (Leela Chess Zero, KataGo: the parent's value minus a reduction that grows with the prior mass already visited).
 *   c_init   finite, in (0, 64].
 *   c_base   0: no growth.  Otherwise finite, in [1, 1e9].
 *   fpu      any negative value: off, an unvisited child's Q is 0 as in the reference (canonical: -1, what az_engine_puct then
 *            reports).  Otherwise finite, in [0, 4].
 * The triple (1.0, 0, off) is the mode off, the default: no launch, kernel or output bit differs from an engine that never had
 * another triple.  Every operation below is one IEEE double operation in the order written, no contraction; sqrt is the correctly
 * rounded one, LOG is the library's az_det_log, which det_log of alphazero_amd/gumbel.py follows bit for bit on the host.
 * For a parent p with children c_0 .. c_{k-1} (k <= 64), at every depth, the root included:
 *   sq    = sqrt((double)p.N)
 *   c     = c_base > 0 ? c_init + LOG(((1.0 + (double)p.N) + c_base) / c_base) : c_init
 *   vis   only when fpu >= 0.  Lane s of the game's 16 holds the children r * 16 + s, r = 0 .. 3:
 *           part_s = (((0.0 + t_0) + t_1) + t_2) + t_3,  t_r = c.P if that child exists and has c.N > 0, else 0.0;
 *         then a pairwise tree over the lanes with strides 1, 2, 4, 8 in that order: part_s = part_s + part_{s ^ stride}
 *         (addition commutes: every lane ends with the same bits); vis = part_0.
 *   q     of a child: c.Q if c.N > 0 or fpu < 0, else (-p.Q) - fpu * sqrt(vis).  p.Q is the parent's stored Q: a node's Q is kept
 *         in the frame of the player who moved into it, so -p.Q is the mover's own estimate; the root's stored Q likewise.
 *   key   = q + ((c * c.P) * sq) / (double)(1 + c.N)
 * The walk's break rules (a fresh node, N == 0), the tie rule (the AZ_P_TIE_SELECT draw of that (ply, sim, depth) under
 * AZ_TIE_RANDOM, the lowest index under AZ_TIE_LOWEST), root noise, the backup, the move, the policy target, visits, the readouts
 * and the temperature do not change.  A game depends on (seed, game id, the triple) only, never on the slot, the slot group, the
 * batch or the cache.
 * Served in the plain PUCT search of AZ_EVAL_NET and AZ_EVAL_FAKE engines (k_step_puct, k_step_puct_cached), in az_engine_run and
 * on the az_engine_set_roots / _search / _advance / _root_readout / _player_moves route, with slot groups and the leaf evaluation
 * cache.  Not served (AZ_EINVAL naming the mode; and while the settings are on the setters of those modes refuse, naming these):
 * AZ_EVAL_EXTERNAL, AZ_EVAL_ROLLOUT, either symmetry mode, leaf_batch > 1, the Gumbel search, the playout cap, forced playouts,
 * exact endgames, proof backup.  AZ_ESTATE while a search is open.  The settings may change between two searches of one tree (no
 * node depends on them); a change drops the cached search graphs.
 * az_puct_c and az_puct_key are c and key above as host arithmetic, the very functions the kernels call (az_puct_key computes sq
 * and c from parent_n; vis is read only where n_child == 0 and fpu >= 0). */
int az_engine_set_puct(az_engine *e, double c_init, double c_base, double fpu);
int az_engine_puct(az_engine *e, double *c_init, double *c_base, double *fpu);
double az_puct_c(int32_t parent_n, double c_init, double c_base);
double az_puct_key(double q_child, double p_child, int32_t n_child, int32_t parent_n, double parent_q, double vis,
                   double c_init, double c_base, double fpu);

/* ---- external evaluator: any PolicyValueNetwork / any object with evaluate() -----------------------------
 * The reference's MCT calls nn.evaluate(board) for every non-terminal leaf and for a fresh root (mcts.py:182-195, 231-233;
 * base.py:350-367).  An engine created with evaluator = AZ_EVAL_EXTERNAL (net may be NULL) hands each batch of pending leaves
 * to the caller instead of its HIP network: where AZ_EVAL_NET launches the network -- the root-prior pass and every lock-step
 * of az_engine_search, az_engine_run and az_engine_search_begin -- it calls `fn` on the calling thread.  `stream` is the
 * engine's own stream: what the callback queues there runs before the next step kernel.  Such a search is never captured as
 * a HIP graph (a host callback cannot be replayed).
 *   - the callback fills d_probs / d_value for rows [0, *d_count): probs as PolicyValueNetwork.predict returns them
 *     (exp(log_softmax), not yet renormalised: the engine applies the shipped get_normalized_probs rule), value in the
 *     side-to-move frame (evaluate()'s v times Board.player).  A prior that is negative or not finite, or a value that
 *     is not finite, fails the call with AZ_EINVAL naming the lowest such slot; nothing is rescaled or clamped.
 *   - a non-zero return fails the call with AZ_EEVAL: nothing more is queued for that search (az_engine_search_begin then
 *     leaves no search open).  After that, or after rejected outputs, the trees hold leaves that were never evaluated:
 *     every call except az_engine_destroy, az_engine_set_roots and az_engine_run returns AZ_ESTATE until one of those two
 *     has reset the slots.  A call into the same engine from inside the callback returns AZ_ESTATE.
 *   - az_engine_set_evaluator returns AZ_EINVAL on an engine that is not AZ_EVAL_EXTERNAL or while a search is open; a
 *     search with no evaluator set returns AZ_ESTATE. */
typedef struct {
    int32_t cap, H, W, A;       /* cap: host-side upper bound on the rows present (the network's batch cap) */
    const int32_t *d_count;     /* DEVICE: rows [0, *d_count) are pending leaves; rows beyond are scratch */
    const float *d_input;       /* [cap][H*W] player*grid, float32 (base.py:363) */
    const int8_t *d_grids;      /* [cap][H*W] Board.grid of the row's position */
    const int8_t *d_players;    /* [cap] Board.player */
    const int32_t *d_slots;     /* [cap] engine slot the row belongs to */
    float *d_probs;             /* out [cap][A] */
    float *d_value;             /* out [cap] */
} az_eval_batch;
typedef int (*az_eval_fn)(void *user, const az_eval_batch *batch, void *stream);
int az_engine_set_evaluator(az_engine *e, az_eval_fn fn, void *user);

/* ---- symmetry augmentation on the device ------------------------------------
 * replaces the loop of AlphaZeroTrainer.self_play (trainer.py:275-284) over Sample.create_reflection_twin /
 * create_rotation_twin: every sample with move_idx >= 2 gets its 7 twins (Connect4: 1) in the reference's
 * order; out meta[.][3] holds the transformation code 1..7 (1 reflection_horizontal, 2 rotation_90,
 * 3 reflection_horizontal+rotation_90, 4 rotation_180, ...).  az_augment_count returns the number of twins. */
int az_augment_count(int game, const int32_t *d_meta, int64_t S, int64_t *n_out, void *stream);
int az_augment(int game, int H, int W, const int8_t *d_state, const float *d_pi, const int8_t *d_z, const int32_t *d_meta,
               int64_t S, int8_t *d_out_state, float *d_out_pi, int8_t *d_out_z, int32_t *d_out_meta, int64_t out_capacity,
               void *stream);

/* ---- training step --------------------------------------------------------------------------
 * replaces the body of AlphaZeroTrainer.optimize_network's batch loop (trainer.py:346-366: zero_grad, forward in train
 * mode, loss_pi + loss_v, backward, optimizer.step) and torch.optim.SGD(lr, momentum, weight_decay) (trainer.py:326) for
 * OthelloNet / Connect4Net on device-resident samples.  Tensors travel under the reference's state-dict names and in
 * torch's layouts (othello.py:341-368, connect4.py:370-389); DEVICE pointers throughout. */
typedef struct az_trainer az_trainer;
/* game AZ othello (0, H = W in {6, 8}) or connect4 (1, H x W board); max_batch: multiple of 16, <= 512 */
int az_trainer_create(int game, int H, int W, int max_batch, az_trainer **out);
void az_trainer_destroy(az_trainer *t);
/* parameters and BatchNorm running statistics in (load) and out (store): name = state-dict key, numel must match */
int az_trainer_load(az_trainer *t, const char *name, const float *d_src, int64_t numel, void *stream);
int az_trainer_store(az_trainer *t, const char *name, float *d_dst, int64_t numel, void *stream);
/* a fresh optimizer (momentum buffers zeroed, step counter 0): what optimize_network creates per iteration (trainer.py:326) */
int az_trainer_begin(az_trainer *t, float lr, float momentum, float weight_decay, float dropout_p, uint32_t seed, void *stream);
int az_trainer_set_lr(az_trainer *t, float lr, void *stream); /* ExponentialLR between epochs (trainer.py:327, 381) */
/* n_steps steps: step s trains on rows d_perm[s*B .. s*B+B) of the sample arrays (d_state int8 [S][H*W] = grid * player,
 * d_pi float [S][A], d_z int8 [S], S = n_samples = len(memory) of trainer.py:288-318, whose indices d_perm holds) and writes its
 * losses to d_loss_pi[s], d_loss_v[s] (trainer.py:352-353).  Asynchronous.  A permutation entry outside [0, n_samples) is never
 * used as an address: the kernels train that batch slot on row 0 and raise a sticky flag, reported as AZ_EINVAL by az_trainer_check
 * (which waits for the enqueued steps) or by the next az_trainer_steps / az_trainer_begin call -- which checks the flag FIRST and, when
 * it reports it, has changed nothing and enqueued nothing of its own (the flag is cleared by the report: repeat the call). */
int az_trainer_steps(az_trainer *t, const int8_t *d_state, const float *d_pi, const int8_t *d_z, int64_t n_samples, const int64_t *d_perm,
                     int32_t n_steps, int32_t B, float *d_loss_pi, float *d_loss_v, void *stream);
int az_trainer_check(az_trainer *t);
/* test access: device pointer and element count of a workspace buffer of the last step ("c1".."c4", "y1", "h1", "dz1", ...) */
int az_trainer_debug(az_trainer *t, const char *name, void **d_ptr, int64_t *numel);
/* test access: EVERY device allocation of the trainer, by index in allocation order: its name, its class, its device pointer and its
 * size in bytes (*name stays valid until az_trainer_destroy).  AZ_EINVAL past the last index.  What a class means for a step:
 * parameters, momenta, running statistics and the Hyper block persist from step to step (az_trainer_load / az_trainer_begin set
 * them); a workspace buffer carries nothing from one step to the next: a step writes every element of it before reading it.
 * TicTacToeNet's single-kernel step has no workspace buffers (LDS only). */
#define AZ_TBUF_PARAMETER 0
#define AZ_TBUF_MOMENTUM 1
#define AZ_TBUF_RUNNING_STAT 2
#define AZ_TBUF_HYPER 3
#define AZ_TBUF_WORKSPACE 4
int az_trainer_buffer(az_trainer *t, int32_t index, const char **name, int32_t *cls, void **d_ptr, int64_t *n_bytes);

#ifdef __cplusplus
}
#endif
#endif
