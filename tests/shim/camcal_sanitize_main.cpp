// tests/shim/camcal_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the per-problem host function of K19 and the
// closed-form start (camcal_shim.cpp) on the edge shapes, every array allocated at its exact size, meant to be built with
// -fsanitize=address,undefined and run as an ordinary process (tests/test_camcal_host.py): an index past an image's corners, the
// workspace or a problem's images stops it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "camcal_shim.cpp"

namespace {

struct Batch {
  std::vector<float> corners, board;
  std::vector<double> q, t;
  std::vector<long long> coff{0}, prob{0};
  std::vector<unsigned char> keep;
  std::vector<clc_camera> cams;
};

clc_camera true_camera(int model) {
  clc_camera c{};
  c.model = model;
  c.proj[0] = 400.0; c.proj[1] = 398.0; c.proj[2] = 322.0; c.proj[3] = 238.0;
  if (model == CLC_CAMERA_PINHOLE) { c.dist[0] = -0.2; c.dist[1] = 0.05; c.dist[2] = 1e-4; c.dist[3] = -2e-4; }
  else { c.dist[0] = -0.02; c.dist[1] = -5e-4; c.dist[2] = 0.0; c.dist[3] = 0.0; }
  return c;
}

// image `k` of a batch: a 6x6 tag board turned 0.25 + 0.07 (k % 5) rad about its y axis and 0.15 (k % 3) - 0.15 about x, about 0.8 m
// away and off the axis, nc corners (tag by tag; `spread`: the board's four corner tags first) with a small deterministic wobble;
// the start pose is the true one moved by a centimetre
void add_image(Batch* b, const clc_camera& cam, long long k, long long nc, bool spread = false) {
  const double ay = 0.25 + 0.07 * (double)(k % 5), ax = 0.15 * (double)(k % 3) - 0.15;
  const double cy_ = std::cos(ay), sy = std::sin(ay), cx_ = std::cos(ax), sx = std::sin(ax);
  const double R[9] = {cy_, 0, sy, sx * sy, cx_, -sx * cy_, -cx_ * sy, sx, cx_ * cy_};  // Rx(ax) Ry(ay)
  const double t[3] = {-0.25 + 0.04 * (double)(k % 4), -0.2 + 0.03 * (double)(k % 5), 0.8 + 0.05 * (double)(k % 4)};
  const double tag = 0.055, pitch = 0.055 * 1.3;
  const double ox[4] = {0, tag, tag, 0}, oy[4] = {0, 0, tag, tag};
  const long long corner_tags[4] = {0, 5, 30, 35};
  for (long long i = 0; i < nc; ++i) {
    const long long g = spread && i < 16 ? corner_tags[i / 4] : i / 4, c = i % 4;
    const double X = pitch * (double)(g % 6) + ox[c], Y = pitch * (double)((g / 6) % 6) + oy[c];
    const double P[3] = {R[0] * X + R[1] * Y + t[0], R[3] * X + R[4] * Y + t[1], R[6] * X + R[7] * Y + t[2]};
    double px[2];
    clc::cp::cam_project(cam, P, px);
    b->board.push_back((float)X);
    b->board.push_back((float)Y);
    b->corners.push_back((float)(px[0] + 0.2 * (double)((i * 7 + k) % 5 - 2)));
    b->corners.push_back((float)(px[1] + 0.2 * (double)((i * 3 + k) % 5 - 2)));
  }
  double qx[4];
  clc::bf::rot_to_quat_xyzw(R, qx);
  b->q.push_back(qx[3]); b->q.push_back(qx[0]); b->q.push_back(qx[1]); b->q.push_back(qx[2]);
  b->t.push_back(t[0] + 0.01); b->t.push_back(t[1] - 0.01); b->t.push_back(t[2] + 0.01);
  b->coff.push_back(b->coff.back() + nc);
  b->keep.push_back(1);
}

void end_problem(Batch* b, clc_camera cam) {
  b->prob.push_back((long long)b->keep.size());
  cam.proj[0] *= 1.01; cam.proj[1] *= 0.99; cam.proj[2] += 2.0; cam.proj[3] -= 1.5;  // the start: off the truth
  b->cams.push_back(cam);
}

int run(const char* name, Batch* b, unsigned mask, int hold_board, const std::vector<int>& want_failure, bool with_prob_off = true) {
  const long long n = (long long)b->keep.size(), np = (long long)b->prob.size() - 1;
  clc_options o;
  shim_pose_options_default(&o);
  clc_camcal_options co;
  shim_camcal_options_default(&co, b->cams[0].model);
  co.hold_mask |= mask;
  co.hold_board_poses = hold_board;
  std::vector<clc_summary> sm((size_t)np);
  std::vector<double> H((size_t)(64 * np)), rms((size_t)np);
  std::vector<int> st((size_t)n, -99);
  const std::vector<double> q0 = b->q, t0 = b->t;
  shim_camera_calibrate(&o, &co, b->corners.data(), b->board.data(), b->coff.data(), b->keep.data(), n, with_prob_off ? b->prob.data() : nullptr,
                        np, b->cams.data(), b->q.data(), b->t.data(), sm.data(), H.data(), rms.data(), st.data());
  int bad = 0;
  for (long long k = 0; k < np; ++k) {
    const bool failure = sm[(size_t)k].termination == CLC_FAILURE;
    if (failure != (want_failure[(size_t)k] != 0)) {
      std::printf("%s: problem %lld ends %d\n", name, k, sm[(size_t)k].termination);
      ++bad;
    }
    if (!failure && !(rms[(size_t)k] < 1.0)) { std::printf("%s: problem %lld rms %g\n", name, k, rms[(size_t)k]); ++bad; }
  }
  for (long long i = 0; i < n; ++i)
    if (st[(size_t)i] != CLC_CAMCAL_OK || hold_board)
      for (int c = 0; c < 4; ++c)
        if (b->q[(size_t)(4 * i + c)] != q0[(size_t)(4 * i + c)] || (c < 3 && b->t[(size_t)(3 * i + c)] != t0[(size_t)(3 * i + c)])) {
          std::printf("%s: image %lld moved\n", name, i);
          ++bad;
          break;
        }
  std::printf("%s: %lld problems, %lld images%s\n", name, np, n, bad ? " FAILED" : "");
  return bad;
}

int guess(const char* name, const Batch& b, int want_used) {
  const long long n = (long long)b.keep.size();
  std::vector<double> H((size_t)(9 * n));
  std::vector<int> st((size_t)n);
  int used = -1;
  const double f = shim_camera_guess(640, 480, b.corners.data(), b.board.data(), b.coff.data(), n, H.data(), st.data(), &used);
  const bool ok = used == want_used && (want_used < 2 ? f != f : (f > 300.0 && f < 520.0));
  std::printf("%s: guess f = %g from %d images%s\n", name, f, used, ok ? "" : " FAILED");
  return ok ? 0 : 1;
}

}  // namespace

int main() {
  int bad = 0;
  for (int model : {CLC_CAMERA_PINHOLE, CLC_CAMERA_KANNALA_BRANDT}) {
    const clc_camera cam = true_camera(model);
    const unsigned dist_held = 0xF0u;
    {  // images per problem: 1, 2, waves - 1, waves, waves + 1 — too few for 8 intrinsics: the distortion held
      Batch b;
      long long k = 0;
      for (long long P : {1LL, 2LL, 3LL, 4LL, 5LL}) {
        for (long long i = 0; i < P; ++i) add_image(&b, cam, k++, 144);
        end_problem(&b, cam);
      }
      bad += run("images per problem", &b, dist_held, 0, {0, 0, 0, 0, 0});
    }
    {  // threads + 1 images of 4 x 4 corners from the board's corner tags
      Batch b;
      for (long long i = 0; i < 257; ++i) add_image(&b, cam, i, 16, true);
      end_problem(&b, cam);
      bad += run("257 images", &b, 0, 0, {0});
      bad += guess("257 images", b, 257);
    }
    {  // corners per image: 3 (dropped), 4, 63, 64, 65, 144 (+ full images so that the intrinsics are fixed); keep with holes; a fully
       // dropped problem between live ones; one problem without problem offsets
      Batch b;
      long long k = 0;
      for (long long nc : {3LL, 4LL, 63LL, 64LL, 65LL, 144LL, 144LL, 144LL, 144LL, 144LL}) add_image(&b, cam, k++, nc);
      b.keep[7] = 0;
      end_problem(&b, cam);
      add_image(&b, cam, k++, 3);
      add_image(&b, cam, k++, 144);
      b.keep.back() = 0;
      end_problem(&b, cam);
      for (int i = 0; i < 6; ++i) add_image(&b, cam, k++, 144);
      end_problem(&b, cam);
      end_problem(&b, cam);  // no images at all
      bad += run("corner counts, keep, dropped problem", &b, 0, 0, {0, 1, 0, 1});
      bad += run("the same, board poses held", &b, 0, 1, {0, 1, 0, 1});
      bad += run("the same, everything but the poses held", &b, 0xFFu, 0, {0, 1, 0, 1});
      bad += guess("corner counts", b, 16);
      Batch one;
      for (int i = 0; i < 6; ++i) add_image(&one, cam, i, 144);
      end_problem(&one, cam);
      bad += run("no problem offsets", &one, 1u << 2, 0, {0}, false);
    }
    {  // the closed-form start with nothing usable
      Batch b;
      add_image(&b, cam, 0, 3);
      add_image(&b, cam, 1, 144);
      bad += guess("one usable image", b, 1);
    }
  }
  if (bad) return 1;
  std::printf("shapes ok\n");
  return 0;
}
