// tests/shim/tags_quads_main.cpp — TEST ONLY.  A stand-alone program over what K25's detection never hands to K27 (tags_shim.cpp) but
// a caller's arrays could: candidates outside the image, so that edge samples and decode samples leave it; a full candidate list with
// every edge list full, so that the quad list and max_quads reach their ends; coincident and collinear quads, which have no
// homography.  Built with -fsanitize=address,undefined and run as an ordinary process by tests/test_tags_host.py.  Not loaded into
// Python, not run on a GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tags_shim.cpp"

namespace {

int check(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
  return 0;
}

}  // namespace

int main() {
  namespace tg = clc::tags;
  const int width = 40, height = 30, stride = 1024, T = 5;
  const long long pitch = 41;
  uint8_t* img = (uint8_t*)std::malloc((size_t)(height * pitch));  // exactly the image
  unsigned s = 2702u;
  for (long long i = 0; i < height * pitch; ++i) {
    s = s * 1664525u + 1013904223u;
    img[i] = (uint8_t)(s >> 24);
  }
  const uint64_t codes[2] = {0x0u, 0xFFFFu};
  long long quads = 0, rejected_runs = 0;
  for (int layout = 0; layout < 4; ++layout)
    for (int max_quads = 1; max_quads <= 1024; max_quads = max_quads == 1 ? 3 : (max_quads == 3 ? 1024 : 1025)) {
      std::vector<float> xy(2 * (size_t)stride);
      for (int c = 0; c < stride; ++c) {
        float x, y;
        if (layout == 0) { x = (float)((c * 7) % 60 - 10); y = (float)((c * 13) % 50 - 10); }       // many outside the image
        else if (layout == 1) { x = 20.0f; y = 15.0f; }                                               // coincident
        else if (layout == 2) { x = (float)(c % 40); y = 15.0f; }                                     // collinear
        else { x = (float)(c % 40); y = (float)((c / 40) % 30); }                                     // all inside
        xy[2 * (size_t)c] = x; xy[2 * (size_t)c + 1] = y;
      }
      const int32_t count = stride, status = CLC_CHESS_OK;
      clc_tag_family f{4, 2, 2, 8, codes};
      clc_tag_options o{8, 0, 40, 8, max_quads, 0};
      std::vector<int32_t> edges((size_t)stride * tg::EDGE_INTS);
      std::vector<float> corners((size_t)T * 8, -7.0f);
      std::vector<int32_t> hamming((size_t)T, -7);
      int32_t cnt = -7, st = -7, nq = -7, nf = -7, nd = -7;
      // the edges of the image itself between these candidates (noise: few or none pass), through both stages
      shim_tag_grid(&f, &o, img, width, height, pitch, 1, xy.data(), &count, &status, stride, T, 1, edges.data(), corners.data(), hamming.data(), &cnt,
                    &st, &nq, &nf, &nd, nullptr);
      check(st == CLC_TAG_OK && cnt >= 0 && cnt <= T && nq >= 0 && nd >= 0, "the image's own edges");
      // every edge list full: p -> p + 1, p + 255, p + 256, p + 512 (mod 1024, in increasing q), so that 4-cycles exist
      const int steps[4] = {1, 255, 256, 512};
      for (int p = 0; p < stride; ++p) {
        int q[4];
        for (int j = 0; j < 4; ++j) q[j] = (p + steps[j]) % stride;
        for (int i = 0; i < 4; ++i)
          for (int j = i + 1; j < 4; ++j)
            if (q[j] < q[i]) { const int t = q[i]; q[i] = q[j]; q[j] = t; }
        int32_t* e = edges.data() + (size_t)p * tg::EDGE_INTS;
        e[0] = 4;
        for (int j = 0; j < 4; ++j) { e[1 + 3 * j] = q[j]; e[2 + 3 * j] = 300; e[3 + 3 * j] = 1200; }
      }
      tg::TagArgs a{};
      a.width = width; a.height = height; a.stride = stride; a.d = f.side; a.b = f.border; a.n_codes = f.n_codes; a.max_hamming = f.max_hamming;
      a.min_side = 8; a.max_side = 30; a.contrast = 40; a.max_border_errors = 8; a.max_quads = max_quads; a.n_tags = T; a.pitch = pitch;
      a.images = img; a.cand_xy = xy.data(); a.cand_count = &count; a.cand_status = &status; a.codes = codes; a.edges = edges.data();
      a.corners = corners.data(); a.hamming = hamming.data(); a.count = &cnt; a.status = &st; a.n_quads = &nq; a.n_foreign = &nf;
      static tg::DecodeLds D;
      tg::decode_image(a, 0, D);
      check(st == CLC_TAG_OK && nq > 1024 && cnt >= 0 && cnt <= T && nf >= 0, "full edge lists");
      if (layout == 1 || layout == 2) { check(cnt == 0 && nf == 0, "no homography: no tag"); ++rejected_runs; }
      for (int id = 0; id < T; ++id)
        for (int j = 0; j < 8; ++j) {
          const float v = corners[(size_t)id * 8 + (size_t)j];
          check(hamming[(size_t)id] < 0 ? v != v : v == v, "a corner");
        }
      quads += nq;
    }
  std::free(img);
  std::printf("quads %lld, runs without a homography %lld\nshapes ok\n", quads, rejected_runs);
  return 0;
}
