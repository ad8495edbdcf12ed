// tests/shim/robustpose_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the per-image host functions of K16
// (robustpose_shim.cpp) on the edge shapes, every array allocated at its exact size, meant to be built with
// -fsanitize=address,undefined and run as an ordinary process (tests/test_robustpose_host.py): an index past an image's corners, its
// groups or its slot of the compacted arrays stops it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "robustpose_shim.cpp"

namespace {

// a fronto-parallel 6x6 tag board seen by the identity camera (f = 1) from z = 1, `n` corners of it, tag by tag
void make(long long n, std::vector<float>* L, std::vector<float>* B) {
  const double tag = 0.055, pitch = 0.055 * 1.3;
  const double cx[4] = {0, tag, tag, 0}, cy[4] = {0, 0, tag, tag};
  L->resize(2 * n);
  B->resize(2 * n);
  for (long long k = 0; k < n; ++k) {
    const long long g = k / 4, c = k % 4;
    const double X = pitch * (double)(g % 6) + cx[c], Y = pitch * (double)((g / 6) % 6) + cy[c] + 0.5 * (double)(g / 36);
    (*B)[2 * k] = (float)X;
    (*B)[2 * k + 1] = (float)Y;
    // a small deterministic wobble, well inside the 2 px / 367 gate
    (*L)[2 * k] = (float)(X - 0.2 + 1e-4 * (double)((k * 7) % 5 - 2));
    (*L)[2 * k + 1] = (float)(Y - 0.2 + 1e-4 * (double)((k * 3) % 5 - 2));
  }
}

int run(const char* name, std::vector<float>& L, std::vector<float>& B, const clc_robust_pose_options& ro, int want_status,
        int want_inliers) {
  const long long n = (long long)L.size() / 2;
  clc_options opt;
  shim_pose_options_default(&opt);
  std::vector<unsigned char> mask((size_t)n), first((size_t)n);
  std::vector<float> sub_l((size_t)(2 * n)), sub_b((size_t)(2 * n));
  std::vector<int> counts((size_t)(n / 4));
  std::vector<double> costs((size_t)(n / 4));
  double q[4], t[3], rms;
  int status, ni, bg, nf;
  clc_summary sm;
  shim_robust_image(&opt, &ro, L.data(), B.data(), n, 0, q, t, &rms, &status, &sm, mask.data(), sub_l.data(), sub_b.data(), &ni, &bg, &nf,
                    first.data(), counts.data(), costs.data());
  std::printf("%-18s n %4lld status %2d inliers %4d best_group %3d fits %d\n", name, n, status, ni, bg, nf);
  if (status != want_status || ni != want_inliers) {
    std::printf("  expected status %d, inliers %d\n", want_status, want_inliers);
    return 1;
  }
  return 0;
}

}  // namespace

int main() {
  clc_robust_pose_options ro{8.0 / 367.0, 2.0 / 367.0, 4, 4};
  int bad = 0;
  std::vector<float> L, B;
  const long long sizes[] = {0, 3, 4, 5, 7, 8, 144, 252, 256, 260};
  for (long long n : sizes) {
    make(n, &L, &B);
    char name[32];
    std::snprintf(name, sizeof name, "clean %lld", n);
    bad += run(name, L, B, ro, n >= 4 ? CLC_POSE_OK : CLC_POSE_NO_CONSENSUS, n >= 4 ? (int)n : 0);
  }
  make(144, &L, &B);
  L[2 * 45] = std::nanf("");
  bad += run("nan corner", L, B, ro, CLC_POSE_OK, 143);
  make(144, &L, &B);
  L[2 * 30] = L[2 * 29];  // three collinear corners in group 7 (corner 2 on corner 1): den == 0, an invalid group
  L[2 * 30 + 1] = L[2 * 29 + 1];
  bad += run("collinear group", L, B, ro, CLC_POSE_OK, 143);
  make(144, &L, &B);
  for (long long k = 0; k < 144; ++k) { L[2 * k] = (float)((k * 37) % 101) * 0.01f; L[2 * k + 1] = (float)((k * 53) % 89) * 0.01f; }
  bad += run("all outliers", L, B, ro, CLC_POSE_NO_CONSENSUS, 0);
  make(144, &L, &B);
  for (int c = 0; c < 8; ++c) std::swap(L[2 * 8 + c], L[2 * 40 + c]);  // tags 2 and 10 swapped
  bad += run("swapped tags", L, B, ro, CLC_POSE_OK, 136);
  make(8, &L, &B);  // collinear quads only: a chessboard row
  for (long long k = 0; k < 8; ++k) { B[2 * k] = 0.03f * (float)k; B[2 * k + 1] = 0.f; L[2 * k] = B[2 * k]; L[2 * k + 1] = 0.f; }
  bad += run("collinear quads", L, B, ro, CLC_POSE_NO_CONSENSUS, 0);
  make(144, &L, &B);
  ro.max_fits = 1;
  bad += run("max_fits 1", L, B, ro, CLC_POSE_OK, 144);
  if (bad) return 1;
  std::printf("shapes ok\n");
  return 0;
}
