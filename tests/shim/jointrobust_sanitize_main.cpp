// tests/shim/jointrobust_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the per-problem host functions of K22
// (jointrobust_shim.cpp: the robust solve and the weights) on the edge shapes, with planted outliers, every array allocated at its
// exact size, meant to be built with -fsanitize=address,undefined and run as an ordinary process (tests/test_jointrobust_host.py):
// an index past an image's corners, its points, its weights, the workspace or a problem's images stops it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jointrobust_shim.cpp"

namespace {

struct Batch {
  std::vector<float> corners, board;
  std::vector<double> pts, q, t, cl;
  std::vector<long long> coff{0}, poff{0}, prob{0};
  std::vector<unsigned char> keep;
};

const double FX = 400.0, CX = 320.0, CY = 240.0;
const double TCL[3] = {0.05, -0.02, 0.1};  // the true T_cl: no rotation

// image `k` of a batch: a 6x6 tag board turned 0.25 + 0.07 (k % 5) rad about its y axis and 0.1 (k % 3) about x, 1 m away, nc
// corners (tag by tag) with a small deterministic wobble (every 19th moved by 6 px), np laser points on a line across the board
// plane (every 9th pulled 0.12 m off it)
void add_image(Batch* b, long long k, long long nc, long long np) {
  const double ay = 0.25 + 0.07 * (double)(k % 5), ax = 0.1 * (double)(k % 3) - 0.1;
  const double cy_ = std::cos(ay), sy = std::sin(ay), cx_ = std::cos(ax), sx = std::sin(ax);
  // R = Rx(ax) Ry(ay)
  const double R[9] = {cy_, 0, sy, sx * sy, cx_, -sx * cy_, -cx_ * sy, sx, cx_ * cy_};
  const double t[3] = {-0.2, -0.2, 1.0 + 0.05 * (double)(k % 4)};
  const double tag = 0.055, pitch = 0.055 * 1.3;
  const double ox[4] = {0, tag, tag, 0}, oy[4] = {0, 0, tag, tag};
  for (long long i = 0; i < nc; ++i) {
    const long long g = i / 4, c = i % 4;
    const double X = pitch * (double)(g % 6) + ox[c], Y = pitch * (double)((g / 6) % 6) + oy[c];
    const double P[3] = {R[0] * X + R[1] * Y + t[0], R[3] * X + R[4] * Y + t[1], R[6] * X + R[7] * Y + t[2]};
    b->board.push_back((float)X);
    b->board.push_back((float)Y);
    b->corners.push_back((float)(FX * P[0] / P[2] + CX + 0.2 * (double)((i * 7 + k) % 5 - 2) + (i % 19 == 7 ? 6.0 : 0.0)));
    b->corners.push_back((float)(FX * P[1] / P[2] + CY + 0.2 * (double)((i * 3 + k) % 5 - 2)));
  }
  for (long long i = 0; i < np; ++i) {
    const double s = -0.5 + (double)i / (double)(np > 1 ? np - 1 : 1), X = 0.2 + s, Y = 0.2 + (0.3 + 0.2 * (double)(k % 4)) * s;
    const double w = 0.004 * (double)((i * 5 + k) % 7 - 3) + (i % 9 == 4 ? 0.12 : 0.0);  // off the plane
    for (int r = 0; r < 3; ++r) b->pts.push_back(R[3 * r] * X + R[3 * r + 1] * Y + R[3 * r + 2] * w + t[r] - TCL[r]);
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
}

int run(const char* name, Batch* b, int hold_board, int hold_ext, const std::vector<int>& want_term_failure, double loss_corner = 3.0,
        double loss_laser = 5.0) {
  const long long n = (long long)b->keep.size(), np = (long long)b->prob.size() - 1;
  clc_camera cam{};
  cam.model = CLC_CAMERA_PINHOLE;
  cam.proj[0] = FX; cam.proj[1] = FX; cam.proj[2] = CX; cam.proj[3] = CY;
  clc_options opt;
  shim_pose_options_default(&opt);
  clc_joint_options jo;
  shim_joint_options_default(&jo, &cam);
  jo.hold_board_poses = hold_board;
  jo.hold_extrinsic = hold_ext;
  clc_joint_loss_options lo;
  shim_joint_loss_options_default(&lo, &jo);
  lo.loss_corner = loss_corner;
  lo.loss_laser = loss_laser;
  // the start poses: K10 on every image
  b->q.assign((size_t)(4 * n), 0.0);
  b->t.assign((size_t)(3 * n), 0.0);
  std::vector<double> rms((size_t)n);
  std::vector<int> st10((size_t)n), st((size_t)n, -99);
  shim_board_poses(&cam, &opt, b->corners.data(), b->board.data(), b->coff.data(), n, b->q.data(), b->t.data(), rms.data(), st10.data(), nullptr);
  std::vector<clc_summary> sm((size_t)np);
  std::vector<double> H((size_t)(36 * np)), parts((size_t)(2 * np)), cl = b->cl;
  std::vector<double> wc((size_t)b->coff.back(), -7.0), wl((size_t)b->poff.back(), -7.0);  // every image lies in a problem: all written
  shim_joint_refine_robust(&cam, &opt, &jo, &lo, b->corners.data(), b->board.data(), b->coff.data(), b->pts.data(), b->poff.data(),
                           b->keep.data(), n, b->prob.data(), np, b->q.data(), b->t.data(), cl.data(), sm.data(), H.data(), parts.data(),
                           st.data(), wc.data(), wl.data());
  int bad = 0;
  for (long long k = 0; k < np; ++k) {
    const bool failed = sm[(size_t)k].termination == CLC_FAILURE;
    std::printf("%-12s problem %lld: images %4lld termination %d iterations %2d cost %.4e -> %.4e\n", name, k, b->prob[(size_t)k + 1] - b->prob[(size_t)k],
                sm[(size_t)k].termination, sm[(size_t)k].num_iterations, sm[(size_t)k].initial_cost, sm[(size_t)k].final_cost);
    if (failed != (want_term_failure[(size_t)k] != 0) || sm[(size_t)k].termination == CLC_RUNNING) ++bad;
    if (!failed && !(sm[(size_t)k].final_cost <= sm[(size_t)k].initial_cost)) ++bad;
    for (int i = 0; i < 7; ++i)
      if (!std::isfinite(cl[(size_t)(7 * k + i)])) ++bad;
  }
  for (long long i = 0; i < n; ++i) {
    const long long nc = b->coff[(size_t)i + 1] - b->coff[(size_t)i];
    const int want = !b->keep[(size_t)i] ? CLC_JOINT_NOT_KEPT : nc < 4 ? CLC_JOINT_TOO_FEW : CLC_JOINT_OK;
    if (st[(size_t)i] != want) { std::printf("  image %lld: status %d, expected %d\n", i, st[(size_t)i], want); ++bad; }
    // the weights: in (0, 1] (exactly 1 without a loss) where the image takes part in a problem that did not fail, NaN elsewhere
    long long pb = 0;
    while (b->prob[(size_t)pb + 1] <= i) ++pb;
    const bool part = want == CLC_JOINT_OK && sm[(size_t)pb].termination != CLC_FAILURE;
    for (long long j = b->coff[(size_t)i]; j < b->coff[(size_t)i + 1]; ++j) {
      const double w = wc[(size_t)j];
      if (part ? !(w > 0.0 && w <= 1.0 && (loss_corner != 0.0 || w == 1.0)) : w == w) { std::printf("  image %lld corner %lld: weight %g\n", i, j, w); ++bad; }
    }
    for (long long j = b->poff[(size_t)i]; j < b->poff[(size_t)i + 1]; ++j) {
      const double w = wl[(size_t)j];
      if (part ? !(w > 0.0 && w <= 1.0 && (loss_laser != 0.0 || w == 1.0)) : w == w) { std::printf("  image %lld point %lld: weight %g\n", i, j, w); ++bad; }
    }
  }
  // the nullable outputs left out
  std::vector<double> q2 = b->q, t2 = b->t, cl2 = b->cl;
  shim_joint_refine_robust(&cam, &opt, &jo, &lo, b->corners.data(), b->board.data(), b->coff.data(), b->pts.data(), b->poff.data(), nullptr,
                           n, np == 1 ? nullptr : b->prob.data(), np, q2.data(), t2.data(), cl2.data(), sm.data(), nullptr, nullptr, st.data(),
                           nullptr, nullptr);
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
    bad += run("images", &b, 0, 0, {0, 0, 0, 0, 0, 0});
  }
  {  // corners per image 3 (dropped), 4, 63, 64, 65, 144; points per image 0, 1, 63, 64, 65, 1081
    Batch b;
    const long long nc[] = {3, 4, 63, 64, 65, 144}, np[] = {0, 1, 63, 64, 65, 1081};
    for (int i = 0; i < 6; ++i) add_image(&b, i, nc[i], 100);
    end_problem(&b);
    for (int i = 0; i < 6; ++i) add_image(&b, 6 + i, 144, np[i]);
    end_problem(&b);
    bad += run("shapes", &b, 0, 0, {0, 0});
    bad += run("hold board", &b, 1, 0, {0, 0});
    bad += run("hold cl", &b, 0, 1, {0, 0});
    bad += run("no loss", &b, 0, 0, {0, 0}, 0.0, 0.0);
    bad += run("laser loss", &b, 0, 0, {0, 0}, 0.0, 5.0);
    bad += run("corner loss", &b, 0, 0, {0, 0}, 3.0, 0.0);
  }
  {  // keep with holes, a problem with every image dropped, an empty problem, no laser point at all
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
    bad += run("holes", &b, 0, 0, {0, 1, 1, 0});
  }
  if (bad) return 1;
  std::printf("shapes ok\n");
  return 0;
}
