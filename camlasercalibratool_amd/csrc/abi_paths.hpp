// abi_paths.hpp — which kernels a call launches: the flags of clc_set_launch decoded once (Steering), the Infinity Cache rules and the
// plans the launchers dispatch on — plan_stream (one problem's streaming launches: clc_eval, clc_information, the step chain, clc_closed_form,
// the timing hooks), plan_solve (clc_solve's route), plan_batched (clc_solve_batched), plan_upload (the lane layouts an upload builds).
// Pure functions of plain values, computed per call; host code only, no HIP (g++ builds it for tests/test_launch_paths.py).
#pragma once
#include <algorithm>
#include <cstddef>

#include "clc_rows.hpp"  // layout sizes: TILE, CTILE_DOUBLES, BLOCK, ROW_DOUBLES[_Z], RowDesc

namespace clc_abi {

// launch flags (clc_set_launch); the kernels get the raw int only as their reduce_mode argument (bit 0)
constexpr int FLAG_REDUCE_SHUFFLE = 1;  // reference wave reduction instead of the butterfly
constexpr int FLAG_PREFETCH = 2;        // software-pipelined tile loads (next tile in flight while computing)
constexpr int FLAG_NONTEMPORAL = 4;     // nt loads for the streamed tiles
constexpr int FLAG_COMPACT = 16;      // stream the compact layout (clc_stream.hpp) when it is available
constexpr int FLAG_DEEP = 64;            // compact layout: two tiles of points in flight per wave (HBM-resident arrays)
constexpr int FLAG_WG512 = 32;          // 512-thread workgroups with the 3:2 old/young wave tile weighting
constexpr int FLAG_STEP = 128;          // clc_solve: one step_kernel launch per LM iteration (compact or row layout)
constexpr int FLAG_ROWS = 256;          // row layout (clc_rows.hpp): 16 B/observation + 64 B/row, per-scan moments
constexpr int FLAG_EQUAL_WAVES = 512;        // row layout, 512-thread workgroups: equal shares per wave, cut at scan starts, instead of the 3:2 old/young weighting
constexpr int FLAG_BATCHED_WG256 = 1024;     // batched row kernel: 256-thread workgroups + block reduction instead of one wave per workgroup
constexpr int FLAG_BATCHED_LOCKSTEP = 2048;  // one-workgroup-per-problem batches: lockstep launches instead of batched_solve_kernel
constexpr int FLAG_NO_RESIDENT = 4096;       // batched solver: not the on-chip resident kernel (clc_resident.hpp) even where the problems fit
constexpr int FLAG_RESIDENT_WG512 = 8192;    // resident layout over 512 lanes per problem (one workgroup per CU) even where 256 lanes hold it
constexpr int kDefaultLaunchFlags = 2 | 16 | 32 | 128 | 256 | 512;  // prefetch + compact layout + 512-thread weighted workgroups + step kernel, tuned on MI355X (scripts/tune_eval.py, scripts/step_check.py)
constexpr int kDefaultBlocksPerCU = 1;   // 4 waves per CU with 2 tiles in flight each

struct Steering {  // clc_set_launch(grid_blocks, flags), decoded
  int grid_override = 0;  // > 0: the streaming grids, and no whole-solve kernel of clc_solve
  bool automatic = true;  // flags = -1: the defaults, with the size-dependent choices made per launch
  bool prefetch, nontemporal, compact, wg512, deep, step, rows, equal_waves, batched_wg256, lockstep, no_resident, resident_wg512;
};
inline Steering decode_launch(int grid_blocks, int flags) {
  const int f = flags < 0 ? kDefaultLaunchFlags : flags;
  const auto on = [f](int bit) { return (f & bit) != 0; };
  return {grid_blocks, flags < 0, on(FLAG_PREFETCH), on(FLAG_NONTEMPORAL), on(FLAG_COMPACT), on(FLAG_WG512), on(FLAG_DEEP), on(FLAG_STEP),
          on(FLAG_ROWS), on(FLAG_EQUAL_WAVES), on(FLAG_BATCHED_WG256), on(FLAG_BATCHED_LOCKSTEP), on(FLAG_NO_RESIDENT), on(FLAG_RESIDENT_WG512)};
}

// The MI355X memory-side cache (MI355X_MICROARCH.md).  With the default flags, an array beyond it streams from HBM: the deep pipeline (two
// tiles of points in flight per wave) pays there only (scripts/size_sweep.py: +10 % at 9e8 B, -8 % at 1e8 B).  Well beyond it (> 1.5x)
// streamed loads are also non-temporal (+5-8 % at 4.5e8-9e8 B; plain loads win while the array is cache-resident; at 2.9e8 B — C3 — a tie).
constexpr size_t kInfinityCacheBytes = 256u << 20;
inline bool beyond_cache(const Steering& s, size_t bytes) { return s.automatic && bytes > kInfinityCacheBytes; }
inline bool from_hbm(const Steering& s, size_t bytes) { return s.automatic && bytes > kInfinityCacheBytes + kInfinityCacheBytes / 2; }
inline bool nontemporal(const Steering& s, size_t bytes) { return s.nontemporal || from_hbm(s, bytes); }
inline size_t row_bytes(long long n_rows, bool z) { return (size_t)n_rows * ((z ? clc::ROW_DOUBLES_Z : clc::ROW_DOUBLES) * 8 + sizeof(clc::RowDesc)); }

enum class Layout { tiles, compact, rows, rows_z };

// One problem's streaming launches, as the kernels' template arguments.  threads: K1's (the step kernel runs 512, the closed form BLOCK);
// prefetch: the tile kernels' PF (compact: the deep pipeline); nt: K1's and the closed form's, and the step chain's on rows; deep: the step
// chain's on compact tiles; *_equal: equal, scan-aligned wave shares on rows instead of the 3:2 old/young weighting.
struct StreamPlan {
  Layout layout;
  int threads, grid;
  bool prefetch, nt, deep, eval_equal, step_equal;
  bool rows() const { return layout == Layout::rows || layout == Layout::rows_z; }
};

inline StreamPlan plan_stream(const Steering& s, size_t n_obs, long long n_rows, bool rows_ok, bool rows_z, bool compact_ok, int num_cus) {
  StreamPlan p;
  // With the default flags, arrays below ~2x10^5 observations keep the per-point compact layout: a launch is pure fixed cost there and the
  // row kernel's 16 prologue loads + per-scan expansion make it 0.4-0.5 us longer per LM iteration (8.5 vs 9.0 us at 5.5x10^3
  // observations, 8.8 vs 9.2 at 10^5; 13.2 vs 11.1 at 10^6 — scripts/r02_ab.py).
  if (s.rows && rows_ok && (!s.automatic || !compact_ok || n_obs >= 200000)) p.layout = rows_z ? Layout::rows_z : Layout::rows;
  else p.layout = s.compact && compact_ok ? Layout::compact : Layout::tiles;
  p.threads = s.wg512 ? 512 : 256;
  // Every CU takes a share (the tile map is proportional, a wave may own zero tiles): up to one workgroup per CU keeps lm_kernel's partial-row
  // reduction short; with 256-thread workgroups, arrays that give every wave >= 16 tiles get 2 per CU.  Never more workgroups than tiles.
  const long long tiles = (long long)((n_obs + clc::TILE - 1) / clc::TILE);
  const int per_cu = (!s.wg512 && tiles >= 16LL * (clc::BLOCK / 64) * 2 * num_cus) ? 2 * kDefaultBlocksPerCU : kDefaultBlocksPerCU;
  const long long cap = s.grid_override > 0 ? s.grid_override : (long long)per_cu * num_cus;
  const long long want = tiles < 1 ? 1 : tiles;
  p.grid = (int)(want < cap ? want : cap);
  p.deep = s.deep || beyond_cache(s, n_obs * 28);  // (28 B per observation: the compact tiles' bytes)
  p.prefetch = p.layout == Layout::compact ? p.deep : s.prefetch || s.wg512;
  if (p.rows()) p.nt = nontemporal(s, row_bytes(n_rows, rows_z));
  else p.nt = p.layout == Layout::compact ? nontemporal(s, n_obs * 28) : s.nontemporal;
  // Equal shares (flag 512) pay where a wave's share is a scan or two; the evaluation kernel ALONE with tens of rows per wave and more is
  // 3-7 % faster with the 3:2 shares (scripts/r02_ab.py: 6.2 vs 6.8 us at 1e6 observations, but 15.4 vs 14.7 at 4e6 and 45.1 vs 42.1 at
  // 1.6e7) — the step kernel is not (its wave 0 starts late anyway): it keeps them at every size.  Rows that carry z: 3:2 shares.
  p.step_equal = p.layout == Layout::rows && s.equal_waves;
  p.eval_equal = p.step_equal && s.wg512 && !(s.automatic && n_rows > 16LL * 8 * p.grid);
  return p;
}

// clc_solve's route.  single: the single-workgroup resident kernel (first, or where the cooperative one is not tried or times out); coop:
// the cooperative kernel first (subject to the caller's back-off count); else step_chain, or the [eval, lm] launch pair.  The whole-solve
// kernels run with the default flags only (the explicit flag sets select the step chain / launch pair the bit-identity tests compare;
// profile_events = 1 asks for per-pass events); auto_disable: clc_set_auto_paths' mask.
struct SolvePlan { bool single, coop, step_chain; };
inline SolvePlan plan_solve(const Steering& s, const StreamPlan& sp, size_t n_obs, bool single_layout, bool coop_layout,
                            bool small_on_coop, int auto_disable, int profile_events) {
  const bool whole = s.automatic && s.grid_override == 0 && profile_events != 1;
  SolvePlan r;
  r.single = single_layout && whole && (auto_disable & 2) == 0;
  // (clc_set_small_on_coop: a problem one workgroup holds ALSO has the cooperative layout and runs on 32 workgroups first)
  r.coop = coop_layout && whole && (auto_disable & 1) == 0 && (!r.single || small_on_coop);
  r.step_chain = s.step && sp.layout != Layout::tiles && s.wg512 && n_obs < 0x7FFFFFFFull && profile_events != 1;
  return r;
}

// Launch geometry of the batched solver (clc_solve_batched and the timing hook).  bpp: workgroups per problem; one_wave: rows_wave with
// exactly one wave per problem; whole_solve: batched_solve_kernel, one workgroup per problem, the whole solve in one launch; resident:
// resident_solve_kernel, the same with the problem read from HBM once and kept on chip.
struct BatchedLaunch {
  int bpp = 1;
  size_t n_blocks = 0;
  int lm_threads = 64;
  unsigned lm_blocks = 0;
  bool compact = false, deep = false, nt = false, rows = false, rows_nt = false, rows_wave = false, one_wave = false;
  bool whole_solve = false, resident = false, res_nt = false;
};
struct BatchShape {  // the uploaded batch: its streaming layouts (max_*: the largest problem) and its lane layout (res_*)
  size_t problems, total_tiles;
  long long max_tiles, n_rows, max_rows;
  bool compact_ok, rows_ok, rows_z, res_ok, res_z;
  long long res_rows;
  int res_lanes;
};

inline BatchedLaunch plan_batched(const Steering& s, const BatchShape& b, int num_cus) {
  BatchedLaunch bl;
  const size_t P = b.problems;
  bl.rows = s.rows && b.rows_ok;
  // one wave per workgroup once the batch is many times wider than the chip (C4 shard: 8 192 problems, -5...7 % per batch); for batches of
  // about a thousand problems the 256-thread form is 3-4 % ahead (scripts/r02_shard_step_timing.py)
  bl.rows_wave = bl.rows && !s.batched_wg256 && (!s.automatic || P >= 8 * (size_t)num_cus);
  // enough workgroups to fill the chip: >= 2 per CU in total, never more than one per 4 tiles
  const size_t target_blocks = s.grid_override > 0 ? (size_t)s.grid_override : 4 * (size_t)num_cus;
  int bpp = (int)((target_blocks + P - 1) / P);
  bpp = std::max(1, std::min(bpp, (int)std::max<long long>(1, b.max_tiles / 4)));
  // batched_lm_kernel sums a problem's partial rows in ONE thread: with hundreds of rows per problem (a handful of long problems) that sum
  // took longer than the evaluation (393 us per pass at 4 problems x 9.6e4 observations, 256 rows each)
  bpp = std::min(bpp, 16);
  // single-wave workgroups: as many waves as the 256-thread form would have — except for batches at least four times wider than the chip's
  // resident waves (C4 shard), where ONE wave per problem is faster still (224-235 vs 239-245 us per launch, 1.52 vs 1.60 ms per batch):
  // no partial rows to combine, scans never cut
  bl.one_wave = bl.rows_wave && bpp == 1 && P >= 32 * (size_t)num_cus;
  if (bl.rows_wave && !bl.one_wave) bpp *= clc::BLOCK / 64;
  bl.bpp = bpp;
  bl.n_blocks = P * (size_t)bpp;
  bl.lm_blocks = (unsigned)((P + bl.lm_threads - 1) / bl.lm_threads);
  bl.compact = s.compact && b.compact_ok;
  const size_t ctile_bytes = b.total_tiles * clc::CTILE_DOUBLES * sizeof(double);
  bl.nt = s.nontemporal || (bl.compact && from_hbm(s, ctile_bytes));
  bl.deep = s.deep || beyond_cache(s, ctile_bytes);
  bl.rows_nt = bl.rows && nontemporal(s, row_bytes(b.n_rows, b.rows_z));
  // One workgroup per problem running the problem's WHOLE solve in one launch (batched_solve_kernel) beats the lockstep launches wherever a
  // pass over the batch is not bandwidth-bound anyway — per evaluation pass, 10^4-observation problems: 17 vs 69 us at 24 problems, 28 vs
  // 52 at 512, 49 vs 65 at 1 024 (C3), 96 vs 115 at 2 048, a tie at 4 096 (0.7 GB), 390 vs 370 at 8 192 (1.4 GB); 10^5-observation
  // problems (1 500 rows each): 78 vs 54 us at 4 problems, 91 vs 70 at 24, a tie at 256 (scripts/probes/c3_exp.py).  So: unless the rows
  // exceed 1 GiB (a C4 shard: lockstep, one wave per problem) or one problem is so long (> 1 024 rows, ~6.5e4 observations) that four
  // waves are too few.  Problems that fit a workgroup's registers + LDS are read from HBM once and solved on chip (clc_resident.hpp).
  bl.whole_solve = bl.rows && !b.rows_z && !s.lockstep && row_bytes(b.n_rows, b.rows_z) <= (1ull << 30) && b.max_rows <= 1024;
  bl.resident = b.res_ok && !s.no_resident && !s.lockstep;
  bl.res_nt = nontemporal(s, (size_t)b.res_rows * (size_t)b.res_lanes * (b.res_z ? 3 : 2) * sizeof(double));
  return bl;
}

// What an upload builds: lane layouts at all (flag 4096: none); the cooperative layout's one-hop form (auto-path mask bit 8: not); the lanes
// per problem of the first try (a batch: 256 — two problems per CU — unless flag 8192; a single problem: 512, it has its CU to itself).
struct UploadPlan { bool resident, one_hop; int first_lanes; };
inline UploadPlan plan_upload(const Steering& s, int auto_disable, bool batch) {
  return {!s.no_resident, (auto_disable & 8) == 0, batch && !s.resident_wg512 ? 256 : 512};
}

}  // namespace clc_abi
