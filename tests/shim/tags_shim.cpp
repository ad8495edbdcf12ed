// tests/shim/tags_shim.cpp — TEST ONLY.  Compiles K27 (camlasercalibratool_amd/csrc/clc_tags.hpp: the directed edges, the quads and the
// decode of an image, the compaction) for the host with g++.  The threads of a workgroup and the lanes of a wave are loops, the barrier
// between two passes is the end of the loop; the images of a launch are a loop.  The candidates come from K25's shim
// (tests/shim/chess_shim.cpp).  The tests compare it with the numpy restatement tests/tags_ref.py, and the GPU tests compare the device
// against it bit for bit.
#include "../../camlasercalibratool_amd/csrc/clc_tags.hpp"

extern "C" {

int shim_tag_options_size() { return (int)sizeof(clc_tag_options); }
int shim_tag_family_size() { return (int)sizeof(clc_tag_family); }
int shim_tag_edge_ints() { return clc::tags::EDGE_INTS; }

// The stages of clc_tag_grid after the detection, on the host (valid options; sopt NULL).  cand_*: [n_images][stride] as
// clc_chess_corners wrote them; edges: scratch of n_images stride EDGE_INTS ints; n_quads, n_foreign, n_edges_dropped, strength nullable.
void shim_tag_grid(const clc_tag_family* f, const clc_tag_options* o, const uint8_t* images, int32_t width, int32_t height, long long pitch,
                   long long n_images, const float* cand_xy, const int32_t* cand_count, const int32_t* cand_status, int32_t stride, int32_t cols,
                   int32_t rows, int32_t* edges, float* corners, int32_t* hamming, int32_t* count, int32_t* status, int32_t* n_quads,
                   int32_t* n_foreign, int32_t* n_edges_dropped, double* strength) {
  namespace tg = clc::tags;
  tg::TagArgs a{};
  a.width = width; a.height = height; a.stride = stride; a.d = f->side; a.b = f->border; a.n_codes = f->n_codes; a.max_hamming = f->max_hamming;
  a.min_side = o->min_side_px; a.max_side = o->max_side_px ? o->max_side_px : (width < height ? width : height);
  a.contrast = o->contrast; a.max_border_errors = o->max_border_errors; a.max_quads = o->max_quads; a.n_tags = cols * rows;
  a.pitch = pitch; a.images = images; a.cand_xy = cand_xy; a.cand_count = cand_count; a.cand_status = cand_status; a.codes = f->codes;
  a.edges = edges; a.corners = corners; a.hamming = hamming; a.count = count; a.status = status; a.n_quads = n_quads; a.n_foreign = n_foreign;
  a.n_edges_dropped = n_edges_dropped; a.strength = strength;
  static thread_local tg::EdgeLds E;
  static thread_local tg::DecodeLds D;
  for (long long k = 0; k < n_images; ++k) tg::edges_image(a, k, E);
  for (long long k = 0; k < n_images; ++k) tg::decode_image(a, k, D);
}

// clc_tag_grid_points_device on the host.
void shim_tag_points(const float* corners, const int32_t* hamming, long long n_images, int32_t cols, int32_t rows, double tag_size,
                     double tag_spacing, float* corners_px, float* board_xy, long long* offsets) {
  namespace tg = clc::tags;
  tg::PointArgs g{};
  g.corners = corners; g.hamming = hamming; g.n_images = n_images; g.cols = cols; g.n_tags = cols * rows; g.tag_size = tag_size;
  g.tag_spacing = tag_spacing; g.corners_px = corners_px; g.board_xy = board_xy; g.offsets = offsets;
  static thread_local tg::ScanLds S;
  tg::scan_counts(g, S);
  int32_t flag[tg::LANES];
  for (long long i = 0; i < n_images; ++i) tg::points_image(g, i, flag);
}

}  // extern "C"
