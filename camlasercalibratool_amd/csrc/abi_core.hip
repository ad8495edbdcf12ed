// abi_core.hip — handle lifecycle, options, launch configuration and the small helpers every unit uses.
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "clc_abi_internal.hpp"

using namespace clc_abi;

namespace clc_abi {

thread_local std::string g_last_error;

int fail(int code, const char* what, hipError_t e) {
  char buf[512];
  if (e != hipSuccess)
    std::snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  else
    std::snprintf(buf, sizeof(buf), "%s", what);
  g_last_error = buf;
  return code;
}

// experiments: CLC_LAUNCH_AHEAD overrides the default launch-ahead depth (options with launch_ahead = 0)
int default_lookahead() {
  static const int v = [] {
    const char* e = std::getenv("CLC_LAUNCH_AHEAD");
    const int n = e ? std::atoi(e) : 0;
    return n > 0 ? n : kDefaultLookahead;
  }();
  return v;
}

// Partial rows.  The capacity is a whole number of 256-row rounds: the controller reads rows in rounds of 256 from
// unclamped addresses and masks the ones beyond the grid afterwards (clc::lm_tail), so every round must be mapped.
// Two buffers: the step kernel alternates between them by launch parity (d_partials_b).
int ensure_partials(clc_handle* h, int blocks) {
  if (2 * (size_t)blocks * clc::NACC9 <= h->d_partials.size()) return CLC_OK;
  const size_t doubles = 2 * (size_t)((blocks + clc::BLOCK - 1) / clc::BLOCK * clc::BLOCK) * clc::NACC9;
  CLC_HIP(h->d_partials.grow(doubles));
  // on the handle's stream: a null-stream memset is not ordered against kernels on a non-blocking stream
  CLC_HIP(hipMemsetAsync(h->d_partials, 0, sizeof(double) * doubles, h->stream));
  return CLC_OK;
}

int ensure_trace(clc_handle* h, int cap) {
  if (cap > 0) CLC_HIP(h->d_trace.grow((size_t)cap));
  return CLC_OK;
}

int ensure_events(clc_handle* h, size_t n) {
  while (h->ev.size() < n) {
    Event e;
    CLC_HIP(hipEventCreate(e.out()));
    h->ev.push_back(std::move(e));
  }
  return CLC_OK;
}

// The wave split table of the row layout's equal-shares mode (clc_kernels.hpp wave_split_kernel): rebuilt, on the
// handle's stream in front of the launches that read it, when the grid changed since the last upload.
void ensure_wave_split(clc_handle* h, int grid) {
  if (h->split_grid == grid) return;
  const clc::RowDesc* desc = h->obs.d_rdesc();
  int* table = reinterpret_cast<int*>(h->obs.d_rdesc() + h->obs.n_rows + 1);
  const int total = grid * 8 + 1;
  hipLaunchKernelGGL(clc::wave_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, desc, (int)h->obs.n_rows,
                     grid, table);
  h->split_grid = grid;
}

}  // namespace clc_abi

namespace {
__global__ void first_launch_kernel(unsigned int* p) {
  if (p == nullptr) return;
  p[0] = 0u;
}
}  // namespace

extern "C" {

int clc_version(void) { return CLC_VERSION; }

const char* clc_last_error(void) { return g_last_error.c_str(); }

void clc_options_default(clc_options* o) {
  if (!o) return;
  o->max_num_iterations = 100;  // src/LaseCamCalCeres.cpp:304
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->use_loss = 1;              // #define LOSSFUNCTION, :212
  o->loss_scale_factor = 0.05;  // CauchyLoss(0.05 * scale), :249
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->launch_ahead = 0;
  o->profile_events = 0;
}

static int create_init(clc_handle* h);

int clc_create(clc_handle** out, int device) {
  if (!out) return fail(CLC_ERR_INVALID_ARG, "clc_create: out is NULL");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(CLC_ERR_NO_DEVICE, "clc_create: no HIP device available (this library has no CPU fallback)", e);
  if (device < 0 || device >= count) return fail(CLC_ERR_INVALID_ARG, "clc_create: bad device index");
  CLC_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  CLC_HIP(hipGetDeviceProperties(&prop, device));
  clc_handle* h = new clc_handle();
  h->device = device;
  h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // (everything below can fail half-way — a busy or full device: the handle and what it already owns are released then)
  const int rc = create_init(h);
  if (rc != CLC_OK) { clc_destroy(h); return rc; }
  *out = h;
  return CLC_OK;
}

// The allocations, the stream and the warm-up of a new handle; on any error the caller (clc_create) destroys the handle.
static int create_init(clc_handle* h) {
  if (const char* e = std::getenv("CLC_AUTO_PATHS_DISABLE")) {
    const int m = std::atoi(e);
    if (m >= 0 && m <= 11 && (m & 4) == 0) h->auto_disable = m;
  }
  if (const char* e = std::getenv("CLC_SMALL_ON_COOP")) h->small_on_coop = std::atoi(e) != 0;
  CLC_HIP(hipStreamCreateWithFlags(h->own_stream.out(), hipStreamNonBlocking));
  h->stream = h->own_stream;
  CLC_HIP(h->d_block.grow(1));
  CLC_HIP(h->d_small.grow(kSmallDoubles));
  CLC_HIP(h->h_small.grow(kSmallDoubles));
  CLC_HIP(h->d_queue.grow(1));
  CLC_HIP(h->d_ticket.grow(1));
  CLC_HIP(hipMemsetAsync(h->d_ticket, 0, sizeof(unsigned int), h->own_stream));
  CLC_HIP(hipMemsetAsync(h->d_queue, 0, sizeof(unsigned int), h->own_stream));  // (counters are zero between launches)
  CLC_HIP(hipStreamSynchronize(h->own_stream));  // the caller may switch streams (clc_set_stream) before the first launch
  CLC_HIP(h->h_mailbox.grow(1));
  std::memset(h->h_mailbox, 0, sizeof(clc::HostMailbox));
  // start pose / outcome of the single-workgroup resident solve (one allocation: 8 doubles of pose, then the summary)
  static_assert(sizeof(clc_summary) % sizeof(double) == 0, "the summary follows the pose in whole doubles");
  CLC_HIP(h->h_spose.grow(8 + sizeof(clc_summary) / sizeof(double)));
  // The code objects of the units that hold kernels are loaded here, not by the first call that launches one of their kernels: the
  // reference's programs call the path once per process, and that one call then took 20 ms instead of 1 (CLC_LAZY_MODULES=1: leave
  // it to the first launches — a process that creates handles it may never use).
  if (!std::getenv("CLC_LAZY_MODULES")) {
    warm_layouts();
    warm_solve();
    warm_frontend();
    // (the batched unit's code object — the twelve resident instantiations, a quarter of the library — is loaded by the first
    // clc_upload_batched instead: the reference's one calibration per process never launches a batched kernel)
    // ... and what else only the FIRST launch / copy / allocation of a process pays: the stream's hardware queue (first launch), the
    // runtime's staging buffers for pageable copies (first hipMemcpy each way), the buffers every solve uses
    hipLaunchKernelGGL(first_launch_kernel, dim3(1), dim3(64), 0, h->stream, h->d_queue);
    double tmp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    CLC_HIP(hipMemcpyAsync(h->d_small, tmp, sizeof(tmp), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(tmp, h->d_small, sizeof(tmp), hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipStreamSynchronize(h->stream));
    CLC_HIP(hipMemcpy(h->d_small, tmp, sizeof(tmp), hipMemcpyHostToDevice));
    CLC_HIP(hipMemcpy(tmp, h->d_small, sizeof(tmp), hipMemcpyDeviceToHost));
    {  // (copies of hundreds of kilobytes from pageable memory take another path than tiny ones: 7 ms the first time)
      std::vector<double> big((size_t)1 << 17, 0.0);
      DevBuf<double> dbig(&h->pool);
      CLC_HIP(dbig.alloc(big.size()));
      CLC_HIP(hipMemcpy(dbig.p, big.data(), big.size() * sizeof(double), hipMemcpyHostToDevice));
      CLC_HIP(hipMemcpy(big.data(), dbig.p, big.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    int rc = ensure_partials(h, h->num_cus);
    if (rc == CLC_OK) rc = ensure_trace(h, 128);
    if (rc == CLC_OK) rc = ensure_events(h, 2);
    if (rc != CLC_OK) return rc;
    CLC_HIP(hipStreamSynchronize(h->stream));
  }
  return CLC_OK;
}

void clc_destroy(clc_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}

int clc_set_stream(clc_handle* h, void* hip_stream) {
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_set_stream: NULL handle");
  hipStream_t next = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : h->own_stream;
  if (next == h->stream) return CLC_OK;
  // A finished solve may still have up to launch_ahead + 1 no-op launches queued on the old stream; they forward the
  // terminated LM state into the buffers the next solve initialises.  Drain them before anything runs elsewhere.
  CLC_HIP(hipSetDevice(h->device));
  CLC_HIP(hipStreamSynchronize(h->stream));
  h->stream = next;
  return CLC_OK;
}

int clc_set_auto_paths(clc_handle* h, int disable_mask) {
  if (!h || disable_mask < 0 || (disable_mask & ~(1 | 2 | 8)) != 0) return fail(CLC_ERR_INVALID_ARG, "clc_set_auto_paths: the mask is a sum of 1, 2, 8");
  h->auto_disable = disable_mask;
  return CLC_OK;
}

int clc_set_small_on_coop(clc_handle* h, int enable) {
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_set_small_on_coop: NULL handle");
  h->small_on_coop = enable != 0;
  return CLC_OK;
}

int clc_get_path_info(const clc_handle* h, clc_path_info* out) {
  if (!h || !out) return fail(CLC_ERR_INVALID_ARG, "clc_get_path_info: bad argument");
  std::memset(out, 0, sizeof(*out));
  out->single_resident = h->sres.ok ? 1 : 0;
  out->single_lanes = h->sres.ok ? h->sres.lanes : 0;
  out->single_points_per_lane = h->sres.ok ? h->sres.max_ppl : 0;
  out->coop_resident = h->cres.ok ? 1 : 0;
  out->coop_points_per_lane = h->cres.ok ? h->cres.max_ppl : 0;
  out->coop_points_carry_z = h->cres.ok && h->cres.with_z ? 1 : 0;
  out->coop_workgroups = h->cres.ok ? h->cres.wgs : 0;
  out->coop_resting = h->coop_eligible < h->coop_retry_at ? 1 : 0;
  out->coop_timeouts = h->coop_aborts;
  out->batched_resident = h->bres.ok ? 1 : 0;
  out->batched_lanes = h->bres.ok ? h->bres.lanes : 0;
  out->batched_points_per_lane = h->bres.ok ? h->bres.max_ppl : 0;
  out->batched_points_carry_z = h->bres.ok && h->bres.with_z ? 1 : 0;
  out->rows_layout = h->obs.rows_ok ? (h->obs.rows_z ? 2 : 1) : 0;
  out->batched_rows_layout = h->batch.rows_ok ? (h->batch.rows_z ? 2 : 1) : 0;
  out->coop_solves = h->coop_solves;
  out->batched_lane_rows = h->bres.ok ? h->bres.rows : 0;
  out->n_rows = h->obs.n_rows;
  out->batched_n_rows = h->batch.n_rows;
  out->coop_gate_waits_expired = h->coop_gate_waits_expired;
  return CLC_OK;
}

int clc_set_launch(clc_handle* h, int grid_blocks, int flags) {
  if (!h || grid_blocks < 0 || flags < -1 || flags > 16383)
    return fail(CLC_ERR_INVALID_ARG, "clc_set_launch: bad argument");
  h->launch_flags = flags < 0 ? kDefaultLaunchFlags : flags;
  h->steer = decode_launch(grid_blocks, flags);
  return CLC_OK;
}

int clc_device_info(clc_handle* h, char* name, int name_cap, int* num_cus) {
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_device_info: NULL handle");
  hipDeviceProp_t prop;
  CLC_HIP(hipGetDeviceProperties(&prop, h->device));
  if (name && name_cap > 0) std::snprintf(name, (size_t)name_cap, "%s (%s)", prop.name, prop.gcnArchName);
  if (num_cus) *num_cus = h->num_cus;
  return CLC_OK;
}

void* clc_pinned_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, std::max<size_t>(bytes, 8), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

void clc_pinned_free(void* p) {
  if (p) (void)hipHostFree(p);
}


}  // extern "C"
