// tests/shim/tags_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the edge shapes of K27 (tags_shim.cpp) behind K25's
// detection (chess_shim.cpp): images from 1 x 1 to 130 x 35, widths and pitches that leave no row aligned, a base address at every
// offset from a word boundary, every array of its exact size (the images without a byte ahead of the first row or after the last one):
// built with -fsanitize=address,undefined and run as an ordinary process by tests/test_tags_host.py.  Not loaded into Python, not run
// on a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "chess_shim.cpp"
#include "tags_shim.cpp"

namespace {

int check(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
  return 0;
}

}  // namespace

int main() {
  const int sizes[][3] = {{1, 1, 1}, {11, 11, 11}, {10, 30, 13}, {33, 21, 40}, {61, 47, 61}, {64, 16, 64}, {65, 17, 67}, {130, 35, 131}};  // width, height, pitch
  long long images = 0, edges_kept = 0, quads = 0, tags = 0;
  for (const auto& sz : sizes)
    for (int variant = 0; variant < 4; ++variant)
      for (int shift = 0; shift < 4; ++shift)
        for (long long n_images = 1; n_images <= 3; n_images += 2) {
          const int width = sz[0], height = sz[1];
          const long long pitch = sz[2];
          const size_t bytes = (size_t)(n_images * height * pitch);
          uint8_t* block = (uint8_t*)std::malloc(bytes + (size_t)shift);
          uint8_t* img = block + shift;
          unsigned s = 2701u + (unsigned)(variant * 31 + shift);
          const int sq = 9 + 4 * variant;  // a chessboard of squares of 9 .. 21 pixels: every inner corner a candidate, every side an edge
          for (size_t i = 0; i < bytes; ++i) {
            s = s * 1664525u + 1013904223u;
            const long long x = (long long)(i % (size_t)pitch), y = (long long)(i / (size_t)pitch) % height;
            img[i] = (uint8_t)((((x / sq) + (y / sq)) & 1 ? 40 : 200) + ((s >> 24) & 7));
          }
          clc_chess_options co{200, 3, 250, variant == 0 ? 7 : 1024, 0};
          const size_t stride = (size_t)co.max_per_image, T = (size_t)(variant + 1);
          std::vector<float> xy(2 * (size_t)n_images * stride, -7.0f);
          std::vector<int32_t> count((size_t)n_images, -7), status((size_t)n_images, -7);
          shim_chess_corners(&co, img, width, height, pitch, n_images, 2, xy.data(), nullptr, count.data(), nullptr, status.data());
          const uint64_t codes[3] = {0x1A5u, 0x0F3u, 0x111u};
          clc_tag_family f{3, 1 + (variant & 1), 3, 4, codes};
          clc_tag_options o{8, variant == 3 ? 200 : 0, 40, variant == 2 ? 8 : 0, variant == 1 ? 1 : 256, 0};
          std::vector<int32_t> edges((size_t)n_images * stride * (size_t)shim_tag_edge_ints(), -7);
          std::vector<float> corners((size_t)n_images * T * 8, -7.0f);
          std::vector<int32_t> hamming((size_t)n_images * T, -7), cnt((size_t)n_images, -7), st((size_t)n_images, -7), nq((size_t)n_images, -7),
              nf((size_t)n_images, -7), nd((size_t)n_images, -7);
          std::vector<double> strength((size_t)n_images * T * 4, -7.0);
          shim_tag_grid(&f, &o, img, width, height, pitch, n_images, xy.data(), count.data(), status.data(), (int32_t)stride, (int32_t)T, 1,
                        edges.data(), corners.data(), hamming.data(), cnt.data(), st.data(), nq.data(), nf.data(), nd.data(), strength.data());
          for (long long k = 0; k < n_images; ++k) {
            check(st[(size_t)k] == CLC_TAG_OK, "a status");
            check(cnt[(size_t)k] >= 0 && cnt[(size_t)k] <= (int32_t)T && nq[(size_t)k] >= 0 && nf[(size_t)k] >= 0 && nd[(size_t)k] >= 0, "the counts");
            int seen = 0;
            for (size_t id = 0; id < T; ++id) {
              const int hm = hamming[(size_t)k * T + id];
              check(hm >= -1 && hm <= f.max_hamming, "a distance");
              for (int j = 0; j < 8; ++j) {
                const float v = corners[((size_t)k * T + id) * 8 + (size_t)j];
                check(hm < 0 ? v != v : (v >= 0 && v < (j & 1 ? height : width)), "a corner");
              }
              for (int j = 0; j < 4; ++j) check(strength[((size_t)k * T + id) * 4 + (size_t)j] != strength[((size_t)k * T + id) * 4 + (size_t)j], "a strength");
              seen += hm >= 0;
            }
            check(seen == cnt[(size_t)k], "count");
            for (int p = 0; p < count[(size_t)k]; ++p) edges_kept += edges[((size_t)k * stride + (size_t)p) * (size_t)shim_tag_edge_ints()];
            quads += nq[(size_t)k]; tags += cnt[(size_t)k]; ++images;
          }
          // without the optional outputs: the same tags; then the compaction into arrays of exactly the tags seen
          std::vector<float> corners2(corners.size(), -7.0f);
          std::vector<int32_t> hamming2(hamming.size(), -7), cnt2((size_t)n_images, -7), st2((size_t)n_images, -7);
          shim_tag_grid(&f, &o, img, width, height, pitch, n_images, xy.data(), count.data(), status.data(), (int32_t)stride, (int32_t)T, 1,
                        edges.data(), corners2.data(), hamming2.data(), cnt2.data(), st2.data(), nullptr, nullptr, nullptr, nullptr);
          check(std::memcmp(corners.data(), corners2.data(), corners.size() * sizeof(float)) == 0 && hamming == hamming2 && cnt == cnt2, "the optional outputs left out");
          long long M = 0;
          for (long long k = 0; k < n_images; ++k) M += 4 * cnt[(size_t)k];
          std::vector<float> px((size_t)(2 * M)), bd((size_t)(2 * M));
          std::vector<long long> off((size_t)n_images + 1, -7);
          shim_tag_points(corners.data(), hamming.data(), n_images, (int32_t)T, 1, 0.05, 0.3, px.data(), bd.data(), off.data());
          check(off[0] == 0 && off[(size_t)n_images] == M, "the offsets");
          std::free(block);
        }
  std::printf("images %lld, edges kept %lld, quads %lld, tags %lld\nshapes ok\n", images, edges_kept, quads, tags);
  check(edges_kept > 0 && quads > 0, "the shapes exercise edges and quads");
  return 0;
}
