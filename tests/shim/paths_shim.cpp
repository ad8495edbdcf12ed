// tests/shim/paths_shim.cpp — TEST ONLY.  Compiles the product's launch-path resolver (camlasercalibratool_amd/csrc/abi_paths.hpp:
// what clc_set_launch's flags, the uploaded layouts and the sizes make every launcher pick) for the host with g++, and fills whole
// tables — one row per flag value — in one call, so tests/test_launch_paths.py can compare them with the rules restated in
// tests/launch_paths_ref.py across all flag values without a GPU.
#include "../../camlasercalibratool_amd/csrc/abi_paths.hpp"

using namespace clc_abi;

extern "C" {

// one row of 8 per flag: layout (0 tiles, 1 compact, 2 rows, 3 rows_z), threads, grid, prefetch, nt, deep, eval_equal, step_equal
void shim_plan_stream(const int* flags, long n, int grid_override, unsigned long long n_obs, long long n_rows, int rows_ok, int rows_z,
                      int compact_ok, int num_cus, int* out) {
  for (long i = 0; i < n; ++i, out += 8) {
    const StreamPlan p = plan_stream(decode_launch(grid_override, flags[i]), n_obs, n_rows, rows_ok, rows_z, compact_ok, num_cus);
    const int row[8] = {(int)p.layout, p.threads, p.grid, p.prefetch, p.nt, p.deep, p.eval_equal, p.step_equal};
    for (int k = 0; k < 8; ++k) out[k] = row[k];
  }
}

// one row of 3 per flag: single, coop, step_chain
void shim_plan_solve(const int* flags, long n, int grid_override, unsigned long long n_obs, long long n_rows, int rows_ok, int rows_z,
                     int compact_ok, int num_cus, int single_layout, int coop_layout, int small_on_coop, int auto_disable,
                     int profile_events, int* out) {
  for (long i = 0; i < n; ++i, out += 3) {
    const Steering s = decode_launch(grid_override, flags[i]);
    const StreamPlan sp = plan_stream(s, n_obs, n_rows, rows_ok, rows_z, compact_ok, num_cus);
    const SolvePlan r = plan_solve(s, sp, n_obs, single_layout, coop_layout, small_on_coop, auto_disable, profile_events);
    out[0] = r.single; out[1] = r.coop; out[2] = r.step_chain;
  }
}

// shape[12]: problems, total_tiles, max_tiles, n_rows, max_rows, compact_ok, rows_ok, rows_z, res_ok, res_z, res_rows, res_lanes.
// One row of 14 per flag: bpp, n_blocks, lm_threads, lm_blocks, compact, deep, nt, rows, rows_nt, rows_wave, one_wave, whole_solve,
// resident, res_nt
void shim_plan_batched(const int* flags, long n, int grid_override, int num_cus, const long long* shape, long long* out) {
  const BatchShape b = {(size_t)shape[0], (size_t)shape[1], shape[2], shape[3], shape[4], shape[5] != 0, shape[6] != 0, shape[7] != 0,
                        shape[8] != 0, shape[9] != 0, shape[10], (int)shape[11]};
  for (long i = 0; i < n; ++i, out += 14) {
    const BatchedLaunch l = plan_batched(decode_launch(grid_override, flags[i]), b, num_cus);
    const long long row[14] = {l.bpp, (long long)l.n_blocks, l.lm_threads, l.lm_blocks, l.compact, l.deep, l.nt, l.rows, l.rows_nt,
                               l.rows_wave, l.one_wave, l.whole_solve, l.resident, l.res_nt};
    for (int k = 0; k < 14; ++k) out[k] = row[k];
  }
}

// one row of 3 per flag: resident, first_lanes, one_hop
void shim_plan_upload(const int* flags, long n, int auto_disable, int batch, int* out) {
  for (long i = 0; i < n; ++i, out += 3) {
    const UploadPlan u = plan_upload(decode_launch(0, flags[i]), auto_disable, batch != 0);
    out[0] = u.resident; out[1] = u.first_lanes; out[2] = u.one_hop;
  }
}

}  // extern "C"
