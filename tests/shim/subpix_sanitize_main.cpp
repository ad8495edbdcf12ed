// tests/shim/subpix_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the edge shapes of K24's host functions
// (subpix_shim.cpp), every array of its exact size (the image without a byte after its last row, the mask tables at 2 w + 1): built
// with -fsanitize=address,undefined and run as an ordinary process by tests/test_subpix_host.py.  Not loaded into Python, not run on
// a GPU.
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "subpix_shim.cpp"

namespace {

int check(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
  return 0;
}

// An X-junction at (cx, cy), turned by `angle`, with a soft edge; a little deterministic noise.
void saddle(std::vector<uint8_t>& img, int width, int height, long long pitch, double cx, double cy, double angle) {
  unsigned s = 12345u;
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) {
      const double u = std::cos(angle) * (x - cx) + std::sin(angle) * (y - cy), v = -std::sin(angle) * (x - cx) + std::cos(angle) * (y - cy);
      const double g = std::tanh(u) * std::tanh(v);  // -1 .. 1
      s = s * 1664525u + 1013904223u;
      img[(size_t)(y * pitch + x)] = (uint8_t)(125.0 + 95.0 * g + (double)((s >> 24) & 3));
    }
}

}  // namespace

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const int sizes[][3] = {{1, 1, 1}, {2, 3, 2}, {33, 21, 40}, {61, 47, 61}, {7, 64, 9}};  // width, height, pitch
  const int wins[][4] = {{1, 1, -1, -1}, {3, 3, -1, -1}, {5, 3, -1, -1}, {11, 11, -1, -1}, {15, 15, -1, -1}, {5, 5, 1, 1}, {1, 15, 0, 0}, {3, 3, 3, 3}};
  long long total = 0, by_status[6] = {0, 0, 0, 0, 0, 0};
  for (const auto& sz : sizes)
    for (const auto& wn : wins)
      for (int first = 0; first < 2; ++first) {
        const int width = sz[0], height = sz[1];
        const long long pitch = sz[2];
        const long long n_images = 3;
        std::vector<uint8_t> img((size_t)(n_images * height * pitch), (uint8_t)128);  // image 0 is flat
        for (int k = 1; k < n_images; ++k) {
          std::vector<uint8_t> one((size_t)(height * pitch));
          saddle(one, width, height, pitch, 0.47 * width + k, 0.52 * height, 0.3 * k);
          for (size_t i = 0; i < one.size(); ++i) img[(size_t)(k * height * pitch) + i] = one[i];
        }
        // image 0: 2 corners, image 1: none, image 2: 67; the starts cover the image, its borders and its corners, and the refusals
        const long long o0 = first ? 3 : 0;
        const long long offsets[4] = {o0, o0 + 2, o0 + 2, o0 + 69};
        const size_t M = (size_t)offsets[3];
        std::vector<float> cin(2 * M, -5.0f), cout(2 * M, -9.0f);
        std::vector<int32_t> st(M, -99), it(M, -99);
        std::vector<double> lam(M, -1.0);
        for (long long c = o0; c < offsets[3]; ++c) {
          const long long k = c - o0;
          cin[(size_t)(2 * c)] = (float)((double)((k * 37) % 101) / 101.0 * width);
          cin[(size_t)(2 * c + 1)] = (float)((double)((k * 53) % 103) / 103.0 * height);
        }
        const size_t e = (size_t)(2 * (o0 + 2));
        cin[e + 0] = 0.0f; cin[e + 1] = 0.0f;                                        // the image's corners
        cin[e + 2] = (float)width - 0.25f; cin[e + 3] = (float)height - 0.25f;
        cin[e + 4] = nan; cin[e + 5] = 1.0f;                                         // refused starts
        cin[e + 6] = 0.5f; cin[e + 7] = inf;
        cin[e + 8] = -1.0f; cin[e + 9] = 0.0f;
        cin[e + 10] = (float)width; cin[e + 11] = 0.0f;
        cin[e + 12] = 3.0e9f; cin[e + 13] = -3.0e9f;
        clc_subpix_options o;
        shim_subpix_options_default(&o, 0);
        o.win_x = wn[0]; o.win_y = wn[1]; o.zero_x = wn[2]; o.zero_y = wn[3];
        o.max_iter = first ? 100 : 5;
        o.eps = first ? 0.0 : 0.1;
        shim_corner_subpix(&o, img.data(), width, height, pitch, n_images, cin.data(), offsets, cout.data(), st.data(), it.data(), lam.data());
        for (long long c = 0; c < (long long)M; ++c) {
          if (c < o0) { check(st[(size_t)c] == -99 && cout[(size_t)(2 * c)] == -9.0f, "rows ahead of offsets[0] untouched"); continue; }
          const int s = st[(size_t)c];
          check(s >= CLC_SUBPIX_NONFINITE && s <= CLC_SUBPIX_CONVERGED, "a status");
          check(it[(size_t)c] >= 0 && it[(size_t)c] <= o.max_iter, "an iteration count");
          ++by_status[s - CLC_SUBPIX_NONFINITE];
          ++total;
        }
        check(st[(size_t)o0] == CLC_SUBPIX_SINGULAR && cout[(size_t)(2 * o0)] == cin[(size_t)(2 * o0)], "a flat image is singular");
        check(st[e / 2 + 2] == CLC_SUBPIX_NONFINITE && st[e / 2 + 3] == CLC_SUBPIX_NONFINITE, "non-finite starts");
        check(st[e / 2 + 4] == CLC_SUBPIX_LEFT_IMAGE && st[e / 2 + 5] == CLC_SUBPIX_LEFT_IMAGE && st[e / 2 + 6] == CLC_SUBPIX_LEFT_IMAGE, "outside starts");
        check(cout[e + 12] == 3.0e9f && it[e / 2 + 6] == 0, "an outside start comes back");
        // in place, and without the optional outputs
        std::vector<float> inplace(cin);
        shim_corner_subpix(&o, img.data(), width, height, pitch, n_images, inplace.data(), offsets, inplace.data(), nullptr, nullptr, nullptr);
        for (long long c = o0; c < (long long)M; ++c) {
          const float a = inplace[(size_t)(2 * c)], b = cout[(size_t)(2 * c)];
          check((a == b) || (a != a && b != b), "in place: the same result");
        }
      }
  // no image, and images without a corner
  {
    clc_subpix_options o;
    shim_subpix_options_default(&o, 11);
    const long long none[3] = {4, 4, 4};
    std::vector<uint8_t> img(2 * 4 * 4, (uint8_t)1);
    shim_corner_subpix(&o, img.data(), 4, 4, 4, 2, nullptr, none, nullptr, nullptr, nullptr, nullptr);
    shim_corner_subpix(&o, nullptr, 4, 4, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  }
  std::printf("corners %lld: nonfinite %lld reverted %lld left %lld singular %lld max_iter %lld converged %lld\nshapes ok\n", total, by_status[0],
              by_status[1], by_status[2], by_status[3], by_status[4], by_status[5]);
  return 0;
}
