// clc_abi_internal.hpp — what the translation units of the C-ABI (abi_*.hip) share: the handle, the per-call device
// pool, error reporting and the helpers that cross unit boundaries.  Not installed; include/clc.h is the interface.
//   abi_core.hip      handle lifecycle, options, launch configuration, small shared helpers
//   abi_layouts.hip   upload paths: re-encoding of the records into the compact / row / lane layouts, stored scans
//   abi_solve.hip     clc_eval, clc_solve and its launch sequences (step chain, single-workgroup resident, cooperative)
//   abi_frontend.hip  factor evaluation, manifold plus, information matrix, closed form, line fitting, scan conversion
//   abi_batched.hip   clc_solve_batched, clc_solve_multistart, clc_solve_subsets
//   abi_comm.hip      RCCL gather of the sharded batch's result records
//   abi_debug.hip     clc_debug_* / clc_time_* (test and profiling hooks; only with -DCLC_TEST_HOOKS)
// Built for gfx950 only (camlasercalibratool_amd/_build.py): every unit with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -mllvm -amdgpu-kernarg-preload-count=8 -c, linked with hipcc -shared.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <thread>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/clc.h"
#pragma GCC visibility pop
#include "clc_host.hpp"
#include "clc_kernels.hpp"
#include "clc_resident.hpp"
#include "clc_coop.hpp"
#include "abi_memory.hpp"
#include "abi_paths.hpp"

namespace clc_abi {

extern thread_local std::string g_last_error;
int fail(int code, const char* what, hipError_t e = hipSuccess);  // abi_core.hip

#define CLC_HIP(expr)                                                 \
  do {                                                                \
    hipError_t e_ = (expr);                                           \
    if (e_ != hipSuccess) return fail(CLC_ERR_HIP, #expr, e_);        \
  } while (0)

inline bool all_finite(const double* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

constexpr int kDefaultLookahead = 2;
int default_lookahead();  // abi_core.hip
constexpr int kSmallDoubles = 512;  // device + pinned scratch for small transfers


// Lane layout of clc_resident.hpp: j-major point rows, lane descriptors, row offsets per problem.
struct ResLayout {
  DeviceArray<double> d_xy;
  DeviceArray<clc::ResLane> d_desc;  // [P * lanes]
  DeviceArray<unsigned int> d_row;   // [P + 1]
  DeviceArray<double> d_z;   // with_z: the slots' z, j-major like d_xy, 8 bytes per slot
  bool with_z = false;       // some record has p.z != 0: 24-byte slots (cooperative layout; batched layout: the 512-lane z form)
  int wgs = 0;               // cooperative layout only: the workgroups the problem is dealt to (COOP_WGS, or COOP_SMALL_WGS: one-hop form)
  int lanes = 0;             // lanes per problem of the built layout (256 / 512)
  int max_ppl = 0;           // largest points-per-lane over the problems
  int uni_ppl = -1;          // >= 0: every problem has this many points per lane
  long long rows = 0;        // j-rows in all
  bool ok = false;
};

// The streaming layouts of one observation array (the single problem's, the batch's): 64-byte tiles; their compact copy (28 B/obs:
// tiles + group table), built at upload when the records compress; the row layout (clc_rows.hpp: xy rows + row descriptors).
struct StreamLayout {
  DeviceArray<double> d_tiles;
  DeviceArray<double> d_ctiles;
  DeviceArray<double> d_groups;
  DeviceArray<double> d_rxy;
  DeviceArray<char> rdesc_bytes;  // the row descriptors [n_rows + 1], then the wave split table behind them (clc::wave_split)
  long long n_groups = 0;
  long long n_rows = 0;
  bool compact_ok = false;
  bool rows_ok = false;
  bool rows_z = false;  // the rows carry z (some record has p.z != 0): ROW_DOUBLES_Z doubles per row
  void invalidate() { compact_ok = rows_ok = false; }
  clc::RowDesc* d_rdesc() const { return reinterpret_cast<clc::RowDesc*>(static_cast<char*>(rdesc_bytes)); }
};

constexpr long long kCoopBackoff0 = 16;  // solves the cooperative path rests after its first abort (doubles with every further one)

}  // namespace clc_abi

// Every owning member releases itself; the own stream is declared first, so it is destroyed after everything allocated on the device.
struct clc_handle {
  clc_abi::Stream own_stream;
  clc_abi::DevPool pool;  // temporaries of the entry points (DevBuf)
  int device = 0;
  int num_cus = 0;
  hipStream_t stream = nullptr;
  // single problem
  clc_abi::StreamLayout obs;
  size_t n_obs = 0;
  int split_grid = -1;  // grid the wave split table behind obs.d_rdesc was built for (-1: none)
  // resident pose-major scans (clc_store_observations): device copies + the host-side CSR offsets
  clc_abi::DeviceArray<double> d_sq;             // tag_q (w,x,y,z) [P*4]
  clc_abi::DeviceArray<double> d_st;             // tag_t [P*3]
  clc_abi::DeviceArray<double> d_spts;           // points [M*3]
  clc_abi::DeviceArray<double> d_sptl;           // points_on_line [ML*3]
  clc_abi::DeviceArray<long long> d_soff;        // pts_off [P+1], ptl_off [P+1], rec_off [P+1]
  std::vector<long long> s_pts_off, s_ptl_off;
  int store_poses = -1;                          // -1: nothing stored
  int64_t store_generation = 0;                  // bumped by every successful clc_store_observations (clc_store_generation)
  // host-side knowledge of reference-size stored scans (<= 16 384 points, <= 4 096 poses): what lets clc_select_observations plan the
  // layouts of the selection on the host and enqueue their construction without a single read-back (abi_layouts.hip, small_fast_upload)
  bool store_small = false;
  std::vector<double> s_tag_q, s_tag_t;          // tag poses (w, x, y, z) / t of the stored scans
  bool s_any_z_pts = false, s_any_z_ptl = false, s_any_z_ends = false;  // some p.z != 0 in points / points_on_line / the first + last point of a scan
  // staging of the small-problem upload path: ONE pinned block + its device twin per handle; `ev_stage` marks the last copy out of it
  clc_abi::PinnedArray<char> h_stage;
  clc_abi::DeviceArray<char> d_stage;
  clc_abi::Event ev_stage; bool stage_busy = false;
  clc_abi::DeviceArray<double> d_small_aos;      // the records of a small problem (never a pool block: kernels may still read it after the call returned)
  bool fast_small = true;                        // (hooks build: clc_debug_fast_small switches the path off for the A/B tests)
  long long fast_small_uploads = 0;
  bool store_lines_equal_points = false;         // points_on_line is bit for bit points (reference-size inputs only: see clc_store_observations)
  long long selection_key = -1;                  // the (stored scans, selection) the observation array was built from by clc_select_observations; -1: none
  long long selection_cfg = -1;                  // ... under these upload-time settings (launch flags, auto paths)
  // launch geometry (clc_set_launch): decoded into `steer`; the raw flags are the kernels' reduce_mode and part of selection_cfg
  clc_abi::Steering steer = clc_abi::decode_launch(0, -1);
  int launch_flags = clc_abi::kDefaultLaunchFlags;
  int auto_disable = 0;     // clc_set_auto_paths: 1 no cooperative solve, 2 no single-workgroup resident solve, 8 (at upload) no one-hop form
  bool small_on_coop = false;    // clc_set_small_on_coop (at upload): problems one workgroup holds also get the cooperative layout
  bool single_uni_ctrl = false;  // hooks build (clc_debug_single_controller): the single-workgroup kernel runs the cooperative kernel's controller
  clc_abi::DeviceArray<double> d_partials;  // two buffers of partial rows (ensure_partials): the step kernel alternates between them
  // LM state
  clc_abi::DeviceArray<clc::SolveBlock> d_block;  // {per-solve constants of the step-kernel chain, LM state x 2}: one allocation
  clc_abi::DeviceArray<clc_iteration> d_trace;
  // scratch
  clc_abi::DeviceArray<double> d_small;
  clc_abi::PinnedArray<double> h_small;
  clc_abi::PinnedArray<clc::HostMailbox, hipHostMallocCoherent | hipHostMallocMapped> h_mailbox;  // device address: h_mailbox.dev()
  std::vector<clc_abi::Event> ev;
  // batched problems
  clc_abi::StreamLayout batch;
  clc_abi::DeviceArray<long long> d_prob_row;  // [P+1] first row of every problem
  // resident ("lane") layouts (clc_resident.hpp): of the batched problems, and of a single problem small enough for one workgroup
  clc_abi::ResLayout bres, sres;
  // cooperative whole-GPU solve of one problem (clc_coop.hpp): the problem's lane layout in 256 chunks, the exchange boards, the
  // next free pass tag; disabled on the handle after a launch that timed out (the step chain takes over)
  clc_abi::ResLayout cres;
  clc_abi::DeviceArray<clc::CoopBoard> d_board;
  unsigned int coop_tag = 1;
  int coop_checked = 0;  // 0: co-residency not checked yet, 1: 256 workgroups fit the device, -1: they do not
  // after a launch that aborted the path rests for `coop_backoff` eligible solves (16, doubling with every further abort up to 2^20:
  // a GPU shared with long-running kernels of somebody else settles on the step chain; a one-off collision costs the first-pass
  // census timeout, 0.2 ms, once)
  long long coop_eligible = 0, coop_retry_at = 0, coop_backoff = clc_abi::kCoopBackoff0;
  int coop_aborts = 0;
  int coop_gate_waits_expired = 0;  // solves that took the step chain because another handle's cooperative launch held the device for > 5 ms
  long long coop_solves = 0;
  int coop_test_drop = 0;  // test hook: launch the next cooperative solve this many workgroups short (its exchange must time out)
  // single-problem resident solve: start pose in / result out through page-locked, device-mapped host memory
  // (one allocation: 8 doubles of pose, then the summary)
  clc_abi::PinnedArray<double, hipHostMallocCoherent | hipHostMallocMapped> h_spose;
  clc_abi::DeviceArray<long long> d_tile_off;  // [P+1]
  clc_abi::DeviceArray<long long> d_nobs;      // [P]
  // batched poses / summaries live in pinned, device-mapped host memory: the init kernel reads the start poses and the
  // finish kernel writes the results straight over PCIe (57 + 64 KB at C3) — three staged hipMemcpy calls through
  // pageable memory cost ~35 us each, a fifth of a C3 batch
  clc_abi::MappedArray<double> h_poses;           // [P*7]
  clc_abi::MappedArray<clc_summary> h_summaries;  // [P]
  clc_abi::DeviceArray<double> d_results;   // clc_result_record per problem of the last clc_solve_batched (clc_gather_results)
  size_t results_valid = 0;                 // number of valid records in d_results
  clc_abi::DeviceArray<unsigned int> d_queue;   // small device counter (active problems)
  clc_abi::DeviceArray<unsigned int> d_ticket;  // arrival counter of the fused evaluation+controller launch
  clc_abi::DeviceArray<clc::LmState> d_states;
  clc_abi::DeviceArray<double> d_bpartials;
  long long batch_max_tiles = 0;
  long long batch_max_rows = 0;  // most rows of the row layout any one problem owns (exact, from prob_row)
  size_t batch_total_tiles = 0;
  size_t n_problems = 0;
  // clc_solve_multistart: start poses / summaries (pinned, device-mapped) and result records of the starts
  clc_abi::MappedArray<double> h_ms_poses;
  clc_abi::MappedArray<clc_summary> h_ms_summaries;
  clc_abi::DeviceArray<double> d_ms_results;
  // clc_solve_subsets (staged like multi-start, in the three arrays above): the weight rows (pinned, device-mapped), and the lane -> block
  // map of problem 0's lane layout with the block offsets it was built for (empty: no map; dropped by every batched upload)
  clc_abi::MappedArray<uint8_t> h_sub_weights;
  clc_abi::DeviceArray<unsigned int> d_sub_lane_block;
  std::vector<int64_t> sub_offsets;
  size_t batch_records = 0;  // records of the uploaded batch
  // clc_closed_form_batched / clc_information_batched: the per-problem outputs of the finishing kernels, written straight over PCIe
  // (pinned, device-mapped), then the staged poses of clc_information_batched
  clc_abi::MappedArray<double> h_flow;

  clc::LmState* d_state() const { return &d_block->st[0]; }
  double* d_partials_b() const { return d_partials + d_partials.size() / 2; }  // the step kernel's second row buffer
  clc_summary* h_ssummary() const { return reinterpret_cast<clc_summary*>(h_spose + 8); }
  clc_summary* d_ssummary() const { return reinterpret_cast<clc_summary*>(h_spose.dev() + 8); }
};

namespace clc_abi {

// ---- abi_core.hip ----
int ensure_partials(clc_handle* h, int blocks);
int ensure_trace(clc_handle* h, int cap);
int ensure_events(clc_handle* h, size_t n);
void ensure_wave_split(clc_handle* h, int grid);

// Every unit with kernels: load its code object on the current device now (hipFuncGetAttributes on a kernel of the unit), so that
// the first call after clc_create does not pay the lazy module load (~2-8 ms per unit).
void warm_layouts();
void warm_solve();
void warm_frontend();
void warm_batched();
inline void warm_kernel(const void* f) {
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, f) != hipSuccess) (void)hipGetLastError();  // (never fatal: the launch itself reports a real problem)
}

// ---- abi_layouts.hip ----
// Resident layout limits: what the instantiations of resident_solve_kernel hold per lane (registers + LDS).
// 256-lane form: 256-thread workgroups, two problems per CU; 512-lane form: one 512-thread workgroup per CU (problems with more
// than 256 scans, or flag 8192).  Both hold 512 x 22 = 256 x 44 - 512 points at most.
constexpr int kResPR256 = 23, kResPL256 = 19, kResPR512 = 4, kResPL512 = 18;
// batches whose points carry z (p.z != 0 in some record): the 512-lane form with 24-byte slots — 10 points per lane in registers
// (60 VGPRs) + 12 in LDS (512 x 12 x 24 B = 147.5 KB): 512 x 22 points, the same capacity as the (x, y) form
constexpr int kResPRz = 10, kResPLz = 12;
// controller of the batched launches (clc_resident.hpp CTRL): 4-wave form / 8-wave form
constexpr int kResCtrl4 = 0, kResCtrl8 = 0;

// Re-encodes the staged records into L's compact and row layouts (d_prob_row: the batch's first row of every problem), and the lane
// layouts res / coop where given (coop: a single problem's lane layout in cooperative chunks, clc_coop.hpp).  L.d_tiles is not touched.
int build_layouts(clc_handle* h, const double* d_aos, size_t n_total, const std::vector<long long>& rec_off,
                  const std::vector<long long>& tile_off, StreamLayout& L, long long* d_prob_row, ResLayout* res, ResLayout* coop);
// builds the records of the stored scans' selection on the device into *aos (allocated here)
int flatten_on_device(clc_handle* h, bool linefit, bool boundary, DevBuf<double>* aos, long long* n_out);

// ---- abi_solve.hip ----
// the single problem's streaming launches under the handle's flags and layouts
inline StreamPlan stream_plan(const clc_handle* h) {
  return plan_stream(h->steer, h->n_obs, h->obs.n_rows, h->obs.rows_ok, h->obs.rows_z, h->obs.compact_ok, h->num_cus);
}
// one launch of the evaluation kernel the plan selects (K1), partial rows into h->d_partials
void launch_eval(clc_handle* h, const StreamPlan& sp, bool with_jac, bool with_loss, const double* d_pose, const int32_t* d_status, double lf,
                 const clc::Pose7* pose_arg = nullptr);
int solve_stepped(clc_handle* h, const clc_options& opt, const StreamPlan& sp, double pose[7], clc_summary* summary, clc_iteration* trace,
                  int trace_cap, std::chrono::steady_clock::time_point t0, int ev_first = -1, int ev_last = -1, float* ev_ms = nullptr);

// ---- abi_batched.hip ----
int batched_launch_setup(clc_handle* h, const clc_options& opt, BatchedLaunch* bl);
void launch_batched_eval(clc_handle* h, const clc_options& opt, const BatchedLaunch& bl);
// ONE launch of resident_solve_kernel over the handle's batch (bl.resident) on the handle's stream; start poses from the handle's pinned
// buffer.  d_summaries != nullptr: outcomes into d_poses / d_summaries / d_results (clc_solve_batched).  d_summaries == nullptr: the
// records-only form (clc_solve_batched_gather) — d_results / rec_host = the communicator's gather buffer and its pinned host twin
// ([totals record][gathered array]), this rank's segment seg_off doubles into the array, global index rec_base + k, `goal` = the
// totals' arrival count at the end of this launch (batched_write_record, clc_kernels.hpp).
// multistart != nullptr (clc_solve_multistart): `n_starts` workgroups, all on problem 0's layout, start poses / outcomes in the given buffers.
struct MultiStartLaunch {
  size_t n_starts = 0;
  double* d_poses = nullptr;
};
void launch_resident_batch(clc_handle* h, const clc_options& opt, const BatchedLaunch& bl, clc_summary* d_summaries, double* d_results,
                           double rec_base, double* rec_host, long long seg_off, unsigned long long goal, const MultiStartLaunch* multistart = nullptr);
// the checks clc_solve_batched makes on its options and start poses (shared with clc_solve_batched_gather); CLC_OK or the error set
int batched_check_inputs(const char* who, const clc_options& opt, const double* poses, size_t n_problems);

}  // namespace clc_abi
