// tests/shim/altpose_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the per-image host function of K17
// (altpose_shim.cpp) on the edge shapes, every array allocated at its exact size, meant to be built with
// -fsanitize=address,undefined and run as an ordinary process (tests/test_altpose_host.py): an index past an image's corners, its
// mask or its slot of the compacted arrays stops it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "altpose_shim.cpp"

namespace {

// a 6x6 tag board tilted 0.25 rad about its y axis, seen by the identity camera (f = 1) from z = `dist`: `n` corners, tag by tag
void make(long long n, double dist, std::vector<float>* L, std::vector<float>* B) {
  const double tag = 0.055, pitch = 0.055 * 1.3, ca = std::cos(0.25), sa = std::sin(0.25);
  const double cx[4] = {0, tag, tag, 0}, cy[4] = {0, 0, tag, tag};
  L->resize(2 * n);
  B->resize(2 * n);
  for (long long k = 0; k < n; ++k) {
    const long long g = k / 4, c = k % 4;
    const double X = pitch * (double)(g % 6) + cx[c], Y = pitch * (double)((g / 6) % 6) + cy[c];
    (*B)[2 * k] = (float)X;
    (*B)[2 * k + 1] = (float)Y;
    const double x = ca * (X - 0.2), y = Y - 0.2, z = dist - sa * (X - 0.2);
    // a small deterministic wobble
    (*L)[2 * k] = (float)(x / z + 2e-4 * (double)((k * 7) % 5 - 2));
    (*L)[2 * k + 1] = (float)(y / z + 2e-4 * (double)((k * 3) % 5 - 2));
  }
}

int run(const char* name, const std::vector<float>& L, const std::vector<float>& B, const std::vector<unsigned char>* mask, int status_in,
        bool want_none) {
  const long long n = (long long)L.size() / 2;
  clc_options opt;
  shim_pose_options_default(&opt);
  clc_alt_pose_options ao;
  shim_alt_options_default(&ao);
  // the input pose: K10 on the set itself (every array of its exact size)
  std::vector<float> sl, sb;
  for (long long k = 0; k < n; ++k)
    if (!mask || (*mask)[k]) { sl.push_back(L[2 * k]); sl.push_back(L[2 * k + 1]); sb.push_back(B[2 * k]); sb.push_back(B[2 * k + 1]); }
  double q_in[4] = {1, 0, 0, 0}, t_in[3] = {0, 0, 1}, rms_in = 0.0;
  int st_in = CLC_POSE_TOO_FEW;
  {
    clc::cp::PoseShared* sh = new clc::cp::PoseShared;
    double pose7[7], r = 0.0;
    const int st = clc::cp::board_pose_image(opt, sl.data(), sb.data(), (long long)sl.size() / 2, *sh, pose7, &r);
    clc::cp::board_pose_store(st, pose7, r, 0, q_in, t_in, &rms_in, &st_in);
    delete sh;
  }
  if (status_in != 0) st_in = status_in;
  std::vector<float> sub_l((size_t)(2 * n)), sub_b((size_t)(2 * n));
  double q[4], t[3], rms, cin, calt, ratio, ra, na;
  int kind = -1;
  unsigned char amb = 9, bet = 9;
  clc_summary sm;
  shim_alt_image(&opt, &ao, L.data(), B.data(), n, mask ? mask->data() : nullptr, q_in, t_in, &st_in, 0, sub_l.data(), sub_b.data(), q, t,
                 &rms, &cin, &calt, &ratio, &ra, &na, &kind, &amb, &bet, &sm);
  std::printf("%-16s n %4lld set %4zu kind %d ratio %9.4f rot_angle %.3e ambiguous %d better %d\n", name, n, sl.size() / 2, kind, ratio, ra,
              (int)amb, (int)bet);
  // the nullable outputs left out
  int kind2 = -1;
  shim_alt_image(&opt, &ao, L.data(), B.data(), n, mask ? mask->data() : nullptr, q_in, t_in, &st_in, 0, sub_l.data(), sub_b.data(), nullptr,
                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &kind2, nullptr, nullptr, nullptr);
  if ((kind == CLC_ALT_NONE) != want_none || kind2 != kind || amb > 1 || bet > 1) {
    std::printf("  expected %s\n", want_none ? "CLC_ALT_NONE" : "a fit");
    return 1;
  }
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  std::vector<float> L, B;
  const long long sizes[] = {0, 3, 4, 5, 63, 64, 65, 144};
  for (long long n : sizes) {
    make(n, 1.0, &L, &B);
    char name[32];
    std::snprintf(name, sizeof name, "near %lld", n);
    bad += run(name, L, B, nullptr, 0, n < 4);
  }
  make(144, 4.0, &L, &B);
  bad += run("far 144", L, B, nullptr, 0, false);
  make(144, 1.0, &L, &B);
  std::vector<unsigned char> m(144, 0);
  m[3] = m[64] = m[70] = m[143] = 1;
  bad += run("mask 4", L, B, &m, 0, false);
  m[70] = 0;
  bad += run("mask 3", L, B, &m, CLC_POSE_OK, true);
  std::fill(m.begin(), m.end(), 1);
  bad += run("status_in", L, B, &m, CLC_POSE_DEGENERATE, true);
  for (int k = 76; k < 80; ++k) m[k] = 0;
  std::vector<float> Ln = L;
  Ln[2 * 77] = std::nanf("");
  bad += run("nan outside", Ln, B, &m, 0, false);
  Ln = L;
  Ln[2 * 10 + 1] = std::nanf("");
  {
    // the input pose from the clean corners, the call on the spoilt ones: by hand, as run() fits its input on what it is given
    clc_options opt;
    shim_pose_options_default(&opt);
    clc_alt_pose_options ao;
    shim_alt_options_default(&ao);
    clc::cp::PoseShared* sh = new clc::cp::PoseShared;
    double pose7[7], r = 0.0, q_in[4], t_in[3], rms_in;
    int st_in;
    const int st = clc::cp::board_pose_image(opt, L.data(), B.data(), 144, *sh, pose7, &r);
    clc::cp::board_pose_store(st, pose7, r, 0, q_in, t_in, &rms_in, &st_in);
    delete sh;
    std::vector<float> sub_l(288), sub_b(288);
    int kind = -1;
    double ratio = 0.0;
    shim_alt_image(&opt, &ao, Ln.data(), B.data(), 144, nullptr, q_in, t_in, &st_in, 0, sub_l.data(), sub_b.data(), nullptr, nullptr, nullptr,
                   nullptr, nullptr, &ratio, nullptr, nullptr, &kind, nullptr, nullptr, nullptr);
    std::printf("%-16s kind %d\n", "nan inside", kind);
    if (st_in != CLC_POSE_OK || kind != CLC_ALT_NONE || ratio == ratio) bad += 1;
  }
  if (bad) return 1;
  std::printf("shapes ok\n");
  return 0;
}
