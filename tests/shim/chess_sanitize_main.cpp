// tests/shim/chess_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the edge shapes of K25's detection (chess_shim.cpp):
// images down to 1 x 1, widths and pitches that leave no row aligned, a base address at every offset from a word boundary, every
// suppression radius, every array of its exact size (the images without a byte ahead of the first row or after the last one): built
// with -fsanitize=address,undefined and run as an ordinary process by tests/test_chess_host.py.  Not loaded into Python, not run on a
// GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "chess_shim.cpp"

namespace {

int check(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
  return 0;
}

}  // namespace

int main() {
  const int sizes[][3] = {{1, 1, 1}, {11, 11, 11}, {10, 30, 13}, {33, 21, 40}, {61, 47, 61}, {64, 16, 64}, {65, 17, 67}, {130, 35, 131}};  // width, height, pitch
  long long total = 0, overflowed = 0;
  for (const auto& sz : sizes)
    for (int r = 1; r <= 7; ++r)
      for (int shift = 0; shift < 4; ++shift)
        for (long long n_images = 1; n_images <= 3; n_images += 2) {
          const int width = sz[0], height = sz[1];
          const long long pitch = sz[2];
          const size_t bytes = (size_t)(n_images * height * pitch);
          // the allocation is exactly the images; `shift` moves its first byte off the word boundary malloc gives
          uint8_t* block = (uint8_t*)std::malloc(bytes + (size_t)shift);
          uint8_t* img = block + shift;
          unsigned s = 977u + (unsigned)(r * 31 + shift);
          for (size_t i = 0; i < bytes; ++i) {
            s = s * 1664525u + 1013904223u;
            const long long x = (long long)(i % (size_t)pitch), y = (long long)(i / (size_t)pitch) % height;
            img[i] = (uint8_t)((((x / 9) + (y / 7)) & 1 ? 40 : 200) + ((s >> 24) & 7));  // a chessboard of 9 x 7 pixel squares
          }
          clc_chess_options o{r == 1 ? 1 : 200, r, r == 2 ? 0 : 250, r == 3 ? 1 : (r == 4 ? 1024 : 64), 0};
          const size_t stride = (size_t)o.max_per_image;
          std::vector<float> xy(2 * (size_t)n_images * stride, -7.0f);
          std::vector<int32_t> r5((size_t)n_images * stride, -7), count((size_t)n_images, -7), raw((size_t)n_images, -7), status((size_t)n_images, -7);
          shim_chess_corners(&o, img, width, height, pitch, n_images, 2, xy.data(), r5.data(), count.data(), raw.data(), status.data());
          for (long long k = 0; k < n_images; ++k) {
            check(status[(size_t)k] == CLC_CHESS_OK || status[(size_t)k] == CLC_CHESS_OVERFLOW, "a status");
            check(count[(size_t)k] >= 0 && count[(size_t)k] <= o.max_per_image && raw[(size_t)k] >= count[(size_t)k], "the counts");
            if (status[(size_t)k] == CLC_CHESS_OVERFLOW) { check(count[(size_t)k] == 0, "overflow: no candidate"); ++overflowed; }
            if (width < 11 || height < 11) check(raw[(size_t)k] == 0, "an empty domain");
            for (int c = 0; c < o.max_per_image; ++c) {
              const float x = xy[2 * ((size_t)k * stride + (size_t)c)], y = xy[2 * ((size_t)k * stride + (size_t)c) + 1];
              if (c < count[(size_t)k]) check(x >= 5 && x < width - 5 && y >= 5 && y < height - 5 && r5[(size_t)k * stride + (size_t)c] >= o.threshold, "a candidate of the domain");
              else check(x != x && y != y && r5[(size_t)k * stride + (size_t)c] == 0, "the padding");
            }
            total += count[(size_t)k];
          }
          // without the optional outputs: the same candidates
          std::vector<float> xy2(xy.size(), -7.0f);
          std::vector<int32_t> count2((size_t)n_images, -7), status2((size_t)n_images, -7);
          shim_chess_corners(&o, img, width, height, pitch, n_images, 170, xy2.data(), nullptr, count2.data(), nullptr, status2.data());
          check(std::memcmp(xy.data(), xy2.data(), xy.size() * sizeof(float)) == 0 && count == count2 && status == status2, "the optional outputs left out");
          std::free(block);
        }
  std::printf("candidates %lld, images overflowed %lld\nshapes ok\n", total, overflowed);
  return 0;
}
