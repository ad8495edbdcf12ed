// abi_joint.hip — clc_joint_options_default, clc_joint_refine(_device): the joint refinement of the board poses and the camera-laser
// extrinsic (K18 in clc_joint.hpp).  A unit of its own: the kernels of abi_campose.hip are held to their register figures, and this
// one is held to its own (tests/test_joint_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "clc_joint.hpp"

using namespace clc_abi;

namespace {

namespace jt = clc::jt;

// The joint call's options: the caller's or the defaults; checked.
int joint_options(const clc_joint_options* in, const clc_camera* cam, clc_joint_options* o, const char* who) {
  if (in) *o = *in; else clc_joint_options_default(o, cam);
  const std::string w(who);
  if (!(std::isfinite(o->sigma_corner) && o->sigma_corner > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": sigma_corner must be finite and > 0").c_str());
  if (!(std::isfinite(o->sigma_laser) && o->sigma_laser > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": sigma_laser must be finite and > 0").c_str());
  if (o->hold_board_poses && o->hold_extrinsic) return fail(CLC_ERR_INVALID_ARG, (w + ": both hold flags set").c_str());
  return CLC_OK;
}

// lift (rounded) into a.lifted, then one workgroup per problem, on the handle's stream.
hipError_t launch_joint(clc_handle* h, const clc_camera& cam, const float* corners_dev, float* lifted_dev, const jt::JointArgs& a,
                        size_t n_problems) {
  if (a.n_corners > 0) {
    const unsigned blocks = (unsigned)(((size_t)a.n_corners + clc::cp::LIFT_THREADS - 1) / clc::cp::LIFT_THREADS);
    hipLaunchKernelGGL((clc::cp::campose_lift_kernel<true>), dim3(blocks), dim3(clc::cp::LIFT_THREADS), 0, h->stream, cam,
                       corners_dev + 2 * a.first_corner, a.n_corners, nullptr, lifted_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(jt::joint_refine_kernel, dim3((unsigned)n_problems), dim3(jt::JOINT_THREADS), 0, h->stream, a);
  return hipGetLastError();
}

jt::JointArgs base_args(const clc_options& opt, const clc_joint_options& jo) {
  jt::JointArgs a{};
  a.opt = opt;
  a.sigma_corner = jo.sigma_corner;
  a.sigma_laser = jo.sigma_laser;
  a.hold_board_poses = jo.hold_board_poses ? 1 : 0;
  a.hold_extrinsic = jo.hold_extrinsic ? 1 : 0;
  return a;
}

}  // namespace

extern "C" {

void clc_joint_options_default(clc_joint_options* o, const clc_camera* cam) {
  if (!o) return;
  // 0.3 px and 0.01 m: the noise levels of the project's simulations (simdata, tests/robustpose_cases.py)
  const double f = cam ? std::sqrt(std::fabs(cam->proj[0] * cam->proj[1])) : 0.0;
  o->sigma_corner = f > 0.0 ? 0.3 / f : 0.0;
  o->sigma_laser = 0.01;
  o->hold_board_poses = 0;
  o->hold_extrinsic = 0;
}

int clc_joint_refine(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in,
                     const float* corners_px, const float* board_xy, const int64_t* corner_offsets, const double* pts,
                     const int64_t* pts_offsets, const uint8_t* keep, size_t n_images, const int64_t* problem_offsets, size_t n_problems,
                     double* q_ca_wxyz, double* t_ca, double* poses_cl, clc_summary* summaries, double* H_cl, double* cost_parts,
                     int32_t* image_status) {
  const char* who = "clc_joint_refine";
  // everything that can be refused without the device first
  CLC_TRY(camera_check(cam, who));
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  clc_joint_options jo;
  CLC_TRY(joint_options(jopt_in, cam, &jo, who));
  if ((n_images > 0 && (!corner_offsets || !pts_offsets || !q_ca_wxyz || !t_ca || !image_status)) ||
      (n_problems > 0 && (!poses_cl || !summaries)))
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine: bad argument");
  if (n_images > 0x7FFFFFFFull || n_problems > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine: too many images");
  if (!problem_offsets && n_problems > 1) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine: bad argument");
  std::vector<long long> crel, prel, orel;
  size_t M = 0, N = 0, span = 0;
  CLC_TRY(host_offsets(who, corner_offsets, n_images, true, nullptr, &crel, &M));
  CLC_TRY(host_offsets(who, pts_offsets, n_images, true, nullptr, &prel, &N));
  if (problem_offsets) {
    CLC_TRY(host_offsets(who, problem_offsets, n_problems, true, nullptr, &orel, &span));
    if (n_problems > 0 && (size_t)problem_offsets[n_problems] > n_images)
      return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine: problem_offsets beyond n_images");
  }
  if (!h || (M > 0 && (!corners_px || !board_xy)) || (N > 0 && !pts)) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  const size_t n = n_images, np = n_problems;
  DevBuf<float> bc(&h->pool), bb(&h->pool), bl(&h->pool);
  DevBuf<long long> bco(&h->pool), bpo(&h->pool), bpr(&h->pool);
  DevBuf<double> bp(&h->pool), bq(&h->pool), bt(&h->pool), bcl(&h->pool), bH(&h->pool), bcp(&h->pool);
  DevBuf<unsigned char> bk(&h->pool);
  DevBuf<int32_t> bs(&h->pool);
  DevBuf<clc_summary> bsum(&h->pool);
  DevBuf<jt::JointImage> bws(&h->pool);
  CLC_HIP(bc.alloc(2 * M)); CLC_HIP(bb.alloc(2 * M)); CLC_HIP(bl.alloc(2 * M)); CLC_HIP(bp.alloc(3 * N));
  CLC_HIP(bco.alloc(n + 1)); CLC_HIP(bpo.alloc(n + 1)); CLC_HIP(bq.alloc(4 * n)); CLC_HIP(bt.alloc(3 * n)); CLC_HIP(bs.alloc(n));
  CLC_HIP(bcl.alloc(7 * np)); CLC_HIP(bsum.alloc(np)); CLC_HIP(bws.alloc(n));
  if (keep) CLC_HIP(bk.alloc(n));
  if (problem_offsets) CLC_HIP(bpr.alloc(np + 1));
  if (H_cl) CLC_HIP(bH.alloc(36 * np));
  if (cost_parts) CLC_HIP(bcp.alloc(2 * np));
  if (M > 0) {
    CLC_HIP(hipMemcpyAsync(bc.p, corners_px + 2 * corner_offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bb.p, board_xy + 2 * corner_offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  if (N > 0) CLC_HIP(hipMemcpyAsync(bp.p, pts + 3 * pts_offsets[0], 3 * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
  std::vector<int32_t> st0(n, CLC_JOINT_NOT_KEPT);  // images outside every problem
  if (n > 0) {
    CLC_HIP(hipMemcpyAsync(bco.p, crel.data(), (n + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bpo.p, prel.data(), (n + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bq.p, q_ca_wxyz, 4 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bt.p, t_ca, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bs.p, st0.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (keep) CLC_HIP(hipMemcpyAsync(bk.p, keep, n, hipMemcpyHostToDevice, h->stream));
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  if (problem_offsets)
    CLC_HIP(hipMemcpyAsync(bpr.p, problem_offsets, (np + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bcl.p, poses_cl, 7 * np * sizeof(double), hipMemcpyHostToDevice, h->stream));
  jt::JointArgs a = base_args(opt, jo);
  a.lifted = bl.p; a.board = bb.p; a.coff = bco.p; a.first_corner = 0; a.n_corners = (long long)M;
  a.pts = bp.p; a.poff = bpo.p; a.keep = keep ? bk.p : nullptr; a.prob_off = problem_offsets ? bpr.p : nullptr;
  a.first_image = 0; a.n_images = (long long)n;
  a.q = bq.p; a.t = bt.p; a.poses_cl = bcl.p; a.summaries = bsum.p; a.H_cl = H_cl ? bH.p : nullptr;
  a.cost_parts = cost_parts ? bcp.p : nullptr; a.status = bs.p; a.ws = bws.p;
  CLC_HIP(launch_joint(h, *cam, bc.p, bl.p, a, np));
  if (n > 0) {
    CLC_HIP(hipMemcpyAsync(q_ca_wxyz, bq.p, 4 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipMemcpyAsync(t_ca, bt.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipMemcpyAsync(image_status, bs.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  }
  CLC_HIP(hipMemcpyAsync(poses_cl, bcl.p, 7 * np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(summaries, bsum.p, np * sizeof(clc_summary), hipMemcpyDeviceToHost, h->stream));
  if (H_cl) CLC_HIP(hipMemcpyAsync(H_cl, bH.p, 36 * np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (cost_parts) CLC_HIP(hipMemcpyAsync(cost_parts, bcp.p, 2 * np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (size_t k = 0; k < np; ++k) summaries[k].solve_ms = ms;
  return CLC_OK;
}

int clc_joint_refine_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in,
                            const float* corners_px_dev, const float* board_xy_dev, const int64_t* corner_offsets_dev,
                            const double* pts_dev, const int64_t* pts_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                            const int64_t* problem_offsets_dev, size_t n_problems, double* q_ca_wxyz_dev, double* t_ca_dev,
                            double* poses_cl_dev, clc_summary* summaries_dev, double* H_cl_dev, double* cost_parts_dev,
                            int32_t* image_status_dev) {
  const char* who = "clc_joint_refine_device";
  CLC_TRY(camera_check(cam, who));
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  clc_joint_options jo;
  CLC_TRY(joint_options(jopt_in, cam, &jo, who));
  if (!h || (n_images > 0 && (!corner_offsets_dev || !pts_offsets_dev || !q_ca_wxyz_dev || !t_ca_dev || !image_status_dev)) ||
      (n_problems > 0 && (!poses_cl_dev || !summaries_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_device: bad argument");
  if (n_images > 0x7FFFFFFFull || n_problems > 0x7FFFFFFFull)
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_device: too many images");
  if (!problem_offsets_dev && n_problems > 1) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_device: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  // the image and corner ranges, to size the lifted corners and the workspace: one small read ahead of the enqueue (as
  // clc_board_poses_device reads the ends of its offsets)
  long long ends[3] = {0, 0, 0};
  if (n_images > 0) {
    DevBuf<long long> be(&h->pool);
    CLC_HIP(be.alloc(3));
    hipLaunchKernelGGL(jt::joint_ends_kernel, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<const long long*>(problem_offsets_dev),
                       reinterpret_cast<const long long*>(corner_offsets_dev), (long long)n_images, be.p);
    CLC_HIP(hipGetLastError());
    CLC_HIP(hipMemcpyAsync(ends, be.p, sizeof ends, hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipStreamSynchronize(h->stream));
  }
  if (ends[0] < 0 || ends[1] < 0 || ends[2] < ends[1]) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_device: offsets not monotone");
  const size_t M = (size_t)(ends[2] - ends[1]);
  if (M > 0 && (!corners_px_dev || !board_xy_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_device: bad argument");
  DevBuf<float> bl(&h->pool);
  DevBuf<jt::JointImage> bws(&h->pool);
  CLC_HIP(bl.alloc(2 * M));
  CLC_HIP(bws.alloc(n_images));
  jt::JointArgs a = base_args(opt, jo);
  a.lifted = bl.p; a.board = board_xy_dev; a.coff = reinterpret_cast<const long long*>(corner_offsets_dev);
  a.first_corner = ends[1]; a.n_corners = (long long)M;
  a.pts = pts_dev; a.poff = reinterpret_cast<const long long*>(pts_offsets_dev); a.keep = keep_dev;
  a.prob_off = reinterpret_cast<const long long*>(problem_offsets_dev);
  a.first_image = ends[0]; a.n_images = (long long)n_images;
  a.q = q_ca_wxyz_dev; a.t = t_ca_dev; a.poses_cl = poses_cl_dev; a.summaries = summaries_dev; a.H_cl = H_cl_dev;
  a.cost_parts = cost_parts_dev; a.status = image_status_dev; a.ws = bws.p;
  CLC_HIP(launch_joint(h, *cam, corners_px_dev, bl.p, a, n_problems));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

}  // extern "C"
