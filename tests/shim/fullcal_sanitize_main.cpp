// tests/shim/fullcal_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the per-problem host functions of K23 (fullcal_shim.cpp:
// the solve and the weights) on the edge shapes, every array allocated at its exact size, meant to be built with
// -fsanitize=address,undefined and run as an ordinary process (tests/test_fullcal_host.py): an index past an image's corners, its
// points, its weights, the workspace or a problem's images stops it.  The synthetic boards stand at one place and one depth: with the
// intrinsics and the range scale free these problems are not well posed and their answers mean nothing (kappa runs to -1); what
// is checked is every memory access and every undefined operation on the way.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fullcal_shim.cpp"

namespace {

struct Batch {
  std::vector<float> corners, board;
  std::vector<double> pts, q, t, cl, rg;
  std::vector<long long> coff{0}, poff{0}, prob{0};
  std::vector<unsigned char> keep;
};

const double FX = 400.0, CX = 320.0, CY = 240.0;
const double TCL[3] = {0.05, -0.02, 0.1};  // the true T_cl: no rotation
const double B_TRUE = 0.02, K_TRUE = 0.005;

// image `k` of a batch: a 6x6 tag board turned 0.25 + 0.07 (k % 5) rad about its y axis and 0.1 (k % 3) about x, 1 m away, nc
// corners (tag by tag) with a small deterministic wobble, np laser points on a line across the board plane as a scanner with
// (B_TRUE, K_TRUE) measures them; every 11th point is pulled 0.2 m towards the scanner, every 23rd corner moved 6 px
void add_image(Batch* b, long long k, long long nc, long long np) {
  const double ay = 0.25 + 0.07 * (double)(k % 5), ax = 0.1 * (double)(k % 3) - 0.1;
  const double cy_ = std::cos(ay), sy = std::sin(ay), cx_ = std::cos(ax), sx = std::sin(ax);
  const double R[9] = {cy_, 0, sy, sx * sy, cx_, -sx * cy_, -cx_ * sy, sx, cx_ * cy_};  // Rx(ax) Ry(ay)
  const double t[3] = {-0.2, -0.2, 1.0 + 0.05 * (double)(k % 4)};
  const double tag = 0.055, pitch = 0.055 * 1.3;
  const double ox[4] = {0, tag, tag, 0}, oy[4] = {0, 0, tag, tag};
  for (long long i = 0; i < nc; ++i) {
    const long long g = i / 4, c = i % 4;
    const double X = pitch * (double)(g % 6) + ox[c], Y = pitch * (double)((g / 6) % 6) + oy[c];
    const double P[3] = {R[0] * X + R[1] * Y + t[0], R[3] * X + R[4] * Y + t[1], R[6] * X + R[7] * Y + t[2]};
    b->board.push_back((float)X);
    b->board.push_back((float)Y);
    b->corners.push_back((float)(FX * P[0] / P[2] + CX + 0.2 * (double)((i * 7 + k) % 5 - 2) + (i % 23 == 22 ? 6.0 : 0.0)));
    b->corners.push_back((float)(FX * P[1] / P[2] + CY + 0.2 * (double)((i * 3 + k) % 5 - 2)));
  }
  for (long long i = 0; i < np; ++i) {
    const double s = -0.5 + (double)i / (double)(np > 1 ? np - 1 : 1), X = 0.2 + s, Y = 0.2 + (0.3 + 0.2 * (double)(k % 4)) * s;
    const double w = 0.004 * (double)((i * 5 + k) % 7 - 3);  // off the plane
    double p[3];
    for (int r = 0; r < 3; ++r) p[r] = R[3 * r] * X + R[3 * r + 1] * Y + R[3 * r + 2] * w + t[r] - TCL[r];
    const double rho = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const double f = ((rho - B_TRUE) / (1.0 + K_TRUE) - (i % 11 == 10 ? 0.2 : 0.0)) / rho;
    for (int r = 0; r < 3; ++r) b->pts.push_back(p[r] * f);
  }
  b->coff.push_back(b->coff.back() + nc);
  b->poff.push_back(b->poff.back() + np);
  b->keep.push_back(1);
}

void end_problem(Batch* b) {
  b->prob.push_back((long long)b->keep.size());
  const double cl0[7] = {TCL[0] + 0.01, TCL[1] - 0.01, TCL[2] + 0.02, 0.005, -0.004, 0.003, 1.0};
  const double nn = std::sqrt(cl0[3] * cl0[3] + cl0[4] * cl0[4] + cl0[5] * cl0[5] + 1.0);
  for (int i = 0; i < 7; ++i) b->cl.push_back(i < 3 ? cl0[i] : cl0[i] / nn);
  b->rg.push_back(0.0);
  b->rg.push_back(0.0);
}

int run(const char* name, Batch* b, unsigned intr_mask, int range_mask, int hold_board, int hold_ext, bool null_corners,
        const std::vector<int>& want_term_failure, long long nonfinite_image = -1) {
  const long long n = (long long)b->keep.size(), np = (long long)b->prob.size() - 1;
  clc_camera cam{};
  cam.model = CLC_CAMERA_PINHOLE;
  cam.proj[0] = FX; cam.proj[1] = FX; cam.proj[2] = CX; cam.proj[3] = CY;
  clc_options opt;
  shim_pose_options_default(&opt);
  clc_full_options fo;
  shim_full_options_default(&fo, cam.model);
  fo.hold_intrinsics_mask = intr_mask;
  fo.hold_range_mask = range_mask;
  fo.hold_board_poses = hold_board;
  fo.hold_extrinsic = hold_ext;
  const bool use_corners = !(hold_board && intr_mask == 0xFFu);
  // the start poses: K10 on every image; the start camera a little off
  b->q.assign((size_t)(4 * n), 0.0);
  b->t.assign((size_t)(3 * n), 0.0);
  std::vector<double> rms10((size_t)n);
  std::vector<int> st10((size_t)n), st((size_t)n, -99);
  shim_board_poses(&cam, &opt, b->corners.data(), b->board.data(), b->coff.data(), n, b->q.data(), b->t.data(), rms10.data(), st10.data(), nullptr);
  clc_camera cam0 = cam;
  cam0.proj[0] *= 1.005; cam0.proj[1] *= 0.995; cam0.proj[2] += 1.0; cam0.dist[0] = 0.01;
  std::vector<clc_camera> cams((size_t)np, cam0);
  std::vector<clc_summary> sm((size_t)np);
  std::vector<double> H((size_t)(256 * np)), parts((size_t)(2 * np)), rms((size_t)np), cl = b->cl, rg = b->rg;
  std::vector<double> wc(b->corners.size() / 2, -7.0), wl(b->pts.size() / 3, -7.0);
  shim_calibrate_full(&opt, &fo, null_corners ? nullptr : b->corners.data(), null_corners ? nullptr : b->board.data(),
                      null_corners ? nullptr : b->coff.data(), b->pts.data(), b->poff.data(), b->keep.data(), n, b->prob.data(), np,
                      cams.data(), b->q.data(), b->t.data(), cl.data(), rg.data(), sm.data(), H.data(), parts.data(), rms.data(), st.data(),
                      null_corners ? nullptr : wc.data(), wl.data());
  int bad = 0;
  for (long long k = 0; k < np; ++k) {
    const bool failed = sm[(size_t)k].termination == CLC_FAILURE;
    std::printf("%-14s problem %lld: images %4lld termination %d iterations %2d cost %.4e -> %.4e  b %.5f kappa %.6f fx %.3f\n", name, k,
                b->prob[(size_t)k + 1] - b->prob[(size_t)k], sm[(size_t)k].termination, sm[(size_t)k].num_iterations,
                sm[(size_t)k].initial_cost, sm[(size_t)k].final_cost, rg[(size_t)(2 * k)], rg[(size_t)(2 * k + 1)], cams[(size_t)k].proj[0]);
    if (failed != (want_term_failure[(size_t)k] != 0) || sm[(size_t)k].termination == CLC_RUNNING) ++bad;
    if (!failed && !(sm[(size_t)k].final_cost <= sm[(size_t)k].initial_cost)) ++bad;
    for (int i = 0; i < 7; ++i)
      if (!std::isfinite(cl[(size_t)(7 * k + i)])) ++bad;
    for (int i = 0; i < 2; ++i)
      if (!std::isfinite(rg[(size_t)(2 * k + i)])) ++bad;
    for (int i = 0; i < 4; ++i)
      if (!std::isfinite(cams[(size_t)k].proj[i]) || !std::isfinite(cams[(size_t)k].dist[i])) ++bad;
  }
  for (long long i = 0; i < n; ++i) {
    const long long nc = b->coff[(size_t)i + 1] - b->coff[(size_t)i];
    const int want = !b->keep[(size_t)i] ? CLC_JOINT_NOT_KEPT : (use_corners && nc < 4) ? CLC_JOINT_TOO_FEW
                     : i == nonfinite_image ? CLC_JOINT_NONFINITE : CLC_JOINT_OK;
    if (st[(size_t)i] != want) { std::printf("  image %lld: status %d, expected %d\n", i, st[(size_t)i], want); ++bad; }
  }
  for (double w : wl)
    if (w == -7.0) { ++bad; break; }  // every point of every image belongs to a problem here: a weight or NaN
  // the nullable outputs left out, one problem without problem offsets
  std::vector<double> q2 = b->q, t2 = b->t, cl2 = b->cl, rg2 = b->rg;
  std::vector<clc_camera> cams2((size_t)np, cam0);
  shim_calibrate_full(&opt, &fo, b->corners.data(), b->board.data(), b->coff.data(), b->pts.data(), b->poff.data(), nullptr, n,
                      np == 1 ? nullptr : b->prob.data(), np, cams2.data(), q2.data(), t2.data(), cl2.data(), rg2.data(), sm.data(), nullptr,
                      nullptr, nullptr, st.data(), nullptr, nullptr);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  {  // images per problem: 1, 2, W - 1, W, W + 1 and T + 1 (4 corners, 2 points per image)
    Batch b;
    const long long counts[] = {1, 2, 3, 4, 5};
    long long k = 0;
    for (long long c : counts) {
      for (long long i = 0; i < c; ++i) add_image(&b, k++, 144, 100);
      end_problem(&b);
    }
    for (long long i = 0; i < 257; ++i) add_image(&b, k++, 4, 2);
    end_problem(&b);
    bad += run("images", &b, 0xF0u, 0, 0, 0, false, {0, 0, 0, 0, 0, 0});  // (one and two images: the distortion held)
  }
  {  // corners per image 3 (dropped), 4, 63, 64, 65, 144; points per image 0, 1, 63, 64, 65, 1081
    Batch b;
    const long long nc[] = {3, 4, 63, 64, 65, 144}, np[] = {0, 1, 63, 64, 65, 1081};
    for (int i = 0; i < 6; ++i) add_image(&b, i, nc[i], 100);
    end_problem(&b);
    for (int i = 0; i < 6; ++i) add_image(&b, 6 + i, 144, np[i]);
    end_problem(&b);
    bad += run("shapes", &b, 0u, 0, 0, 0, false, {0, 0});
    bad += run("hold board", &b, 0u, 0, 1, 0, false, {0, 0});
    bad += run("no corners", &b, 0xFFu, 0, 1, 0, true, {0, 0});
    bad += run("hold cl", &b, 0u, 0, 0, 1, false, {0, 0});
    bad += run("hold range", &b, 0u, 3, 0, 0, false, {0, 0});
    bad += run("hold camera", &b, 0xFFu, 0, 0, 0, false, {0, 0});
    // everything held but one parameter: kappa, then the focal length fx
    bad += run("only kappa", &b, 0xFFu, 1, 1, 1, false, {0, 0});
    bad += run("only fx", &b, 0xFEu, 3, 1, 1, false, {0, 0});
  }
  {  // one image; keep with holes, a problem with every image dropped, an empty problem, no laser point at all, a zero-range point
    Batch b;
    for (int i = 0; i < 7; ++i) add_image(&b, i, 144, 50);
    b.keep[1] = b.keep[4] = 0;
    end_problem(&b);
    for (int i = 0; i < 3; ++i) add_image(&b, 7 + i, i == 1 ? 2 : 144, 20);
    b.keep[7] = b.keep[9] = 0;
    end_problem(&b);
    end_problem(&b);
    for (int i = 0; i < 4; ++i) add_image(&b, 10 + i, 144, 0);
    end_problem(&b);
    for (int i = 0; i < 5; ++i) add_image(&b, 14 + i, 144, 60);
    for (int r = 0; r < 3; ++r) b.pts[(size_t)(3 * (b.poff[16] + 17) + r)] = 0.0;
    end_problem(&b);
    bad += run("holes", &b, 0u, 0, 0, 0, false, {0, 1, 1, 0, 0}, 16);
  }
  if (bad) return 1;
  std::printf("shapes ok\n");
  return 0;
}
