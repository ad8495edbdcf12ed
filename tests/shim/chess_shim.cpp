// tests/shim/chess_shim.cpp — TEST ONLY.  Compiles K25 (camlasercalibratool_amd/csrc/clc_chess.hpp: the tile's load, response and
// suppression, the image's selection) for the host with g++.  The threads of a workgroup are a loop, the barrier between two passes is
// the end of the loop, the append to an image's raw list a plain increment; the tiles and the images of a launch are loops.  The tests
// compare it with the numpy restatement tests/chess_ref.py, and the GPU tests compare the device against it bit for bit.
#include <vector>

#include "../../camlasercalibratool_amd/csrc/clc_chess.hpp"

extern "C" {

int shim_chess_options_size() { return (int)sizeof(clc_chess_options); }
int shim_chess_tile_w() { return clc::chess::TILE_W; }
int shim_chess_tile_h() { return clc::chess::TILE_H; }

// clc_chess_corners on the host (valid options); cand_r5 and count_raw nullable.  `chunk`: images per launch (the device form's 170).
void shim_chess_corners(const clc_chess_options* o, const uint8_t* images, int32_t width, int32_t height, long long pitch, long long n_images,
                        long long chunk, float* cand_xy, int32_t* cand_r5, int32_t* count, int32_t* count_raw, int32_t* status) {
  namespace ch = clc::chess;
  if (n_images <= 0) return;
  if (chunk > n_images) chunk = n_images;
  ch::ChessArgs a{};
  a.width = width; a.height = height; a.threshold = o->threshold; a.nms_radius = o->nms_radius; a.rel_permille = o->rel_permille;
  a.max_per_image = o->max_per_image; a.pitch = pitch; a.n_images = n_images; a.images = images;
  a.tiles_x = ((long long)width + ch::TILE_W - 1) / ch::TILE_W;
  const long long tiles_y = ((long long)height + ch::TILE_H - 1) / ch::TILE_H;
  std::vector<unsigned int> raw_count((size_t)chunk);
  std::vector<int32_t> raw((size_t)chunk * ch::RAW_CAP * 3);  // exactly the launch's lists
  a.raw_count = raw_count.data(); a.raw = raw.data();
  a.cand_xy = cand_xy; a.cand_r5 = cand_r5; a.count = count; a.count_raw = count_raw; a.status = status;
  static thread_local ch::Tile L;
  for (long long first = 0; first < n_images; first += chunk) {
    const long long n = n_images - first < chunk ? n_images - first : chunk;
    a.first = first;
    for (long long k = 0; k < n; ++k) raw_count[(size_t)k] = 0;
    if (width >= 2 * ch::RING + 1 && height >= 2 * ch::RING + 1)
      for (long long k = 0; k < n; ++k)
        for (long long ty = 0; ty < tiles_y; ++ty)
          for (long long tx = 0; tx < a.tiles_x; ++tx) ch::process_tile(a, k, tx, ty, L);
    for (long long k = 0; k < n; ++k) ch::select_image(a, k);
  }
}

}  // extern "C"
