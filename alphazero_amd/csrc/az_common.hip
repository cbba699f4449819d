// az_common.hip -- error reporting shared by every entry point of libaz_amd.so
#include "az_host.h"

static thread_local char g_err[512] = "";

void az_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char *az_last_error(void) { return g_err; }
extern "C" int az_version(void) { return 118; }  // 118: az_engine_set_resign, az_engine_resign_stats, az_engine_game_log, az_engine_resign_values, az_resign_value, az_resign_holdout; 117: az_net_forward_lane_fc2, az_net_heads_view, az_engine_step_heads; 116: az_engine_set_puct, az_engine_puct, az_puct_c, az_puct_key; 115: az_net_gemm_rows; 114: az_engine_set_proof_backup, az_engine_proof_backup_stats, az_engine_root_proofs; 113: az_engine_set_eval_cache, az_engine_eval_cache_stats; 112: az_net_stage_lane, az_net_stage_plan, az_net_trunk_stores; 111: az_net_trunk_prefetch; 110: az_engine_set_forced_playouts, az_engine_forced_playouts_stats, az_forced_playout, az_forced_prune; 109: az_engine_set_playout_cap, az_engine_playout_cap_stats, az_playout_cap_full; 108: az_engine_player_moves; 107: az_engine_set_gumbel_batch, az_gumbel_locksteps; 106: az_engine_root_readout; 105: AZ_EVAL_EXTERNAL, az_engine_set_evaluator, AZ_EEVAL; 104: az_trainer_steps takes n_samples, az_trainer_check, az_net_profile_read has eight slots; 103: az_engine_search_begin / _end / _pair; 102: az_trainer_*, az_engine_nodes_used / grow_pools, az_net_stage_kernel
