// clc_tags.hpp — K27: the corners of a Kalibr-style tag grid from K25's candidates.  Every tag corner of such a board
// touches a black spacer square diagonally, so it is an X-junction and K25 finds it; this header turns the candidates of an image into
// tag quads, reads and decodes their payload against the caller's code table and writes the corners by tag id.  Every step before the
// homography is exact integer arithmetic; the homography is K26's 4-point solve (clc_boardorder.hpp: the same rows, the same
// elimination, every operation rounded on its own), and its only use is to choose the pixel nearest each cell's centre.
//
//   tag_edges_kernel    one 256-thread workgroup per image.  The candidates go into LDS; a thread owns the slot p and walks q in
//                       increasing order: the pair passes where its twelve samples (six inside, six outside, half a border width off
//                       the edge) lie in the image and min(outside) - max(inside) >= contrast.  The first CLC_TAG_MAX_OUT passing
//                       edges of p are kept with their two sums, further ones counted.  No atomics: nothing depends on timing.
//   tag_decode_kernel   one wave per image.  The quads of p0 are the 4 x 4 x 4 paths over the kept edges, one per lane, in
//                       lexicographic order of (p1, p2, p3) by the lane number; per quad the threshold, the homography, the cells
//                       over the lanes, the four rotations of the word, the codes x rotations over the lanes and a wave minimum
//                       under (Hamming, id, rotation); per id the smallest (Hamming, quad rank); then the corners by id.
//   tag_scan_kernel, tag_points_kernel   the compaction for clc_board_poses_device: a scan over the images' counts, then one wave per
//                       image that writes the seen tags' corners and board points in id order.
//
// tests/shim/tags_shim.cpp compiles this header for the host with g++ and runs the same code with the threads as loops; the device is
// compared with it bit for bit.  (The unit that launches these kernels names K25's and K26's types through the aliases below.)
#pragma once
#include "../../include/clc.h"
#include "clc_math.hpp"
#include "clc_boardorder.hpp"

namespace clc {
namespace tags {

namespace bo = clc::boardorder;

typedef clc_chess_options DetectOptions;  // K25's options
constexpr int DETECT_OVERFLOW = CLC_CHESS_OVERFLOW;
inline void detect_options_default(DetectOptions* o) { clc_chess_options_default(o); }
constexpr int MAX_CAND = CLC_CHESS_MAX_CANDIDATES;
constexpr int MAX_OUT = CLC_TAG_MAX_OUT, MAX_QUADS = CLC_TAG_MAX_QUADS, MAX_TAGS = CLC_TAG_MAX_TAGS;
constexpr int S = 8;                       // an edge is sampled at the fractions (2 i + 1) / (2 S), i = 1 .. S - 2
constexpr int EDGE_THREADS = 256, LANES = 64, SCAN_THREADS = 256;
constexpr int EDGE_INTS = 1 + 3 * MAX_OUT;  // per slot: the kept edges' number, then (q, sum inside, sum outside) of each
constexpr int NOT_SEEN = 0x7FFFFFFF;
static_assert(MAX_OUT == 4 && LANES == 64, "a lane per path of three kept edges");
static_assert(MAX_QUADS <= 1024 && MAX_TAGS <= 1024 && CLC_TAG_MAX_CODES <= 4096, "the packed keys");

// Everything of one launch; every array begins at the launch's first image.
struct TagArgs {
  int32_t width, height, stride;  // stride: the candidates' slots per image
  int32_t d, b, n_codes, max_hamming;
  int32_t min_side, max_side, contrast, max_border_errors, max_quads, n_tags;
  long long pitch;
  const uint8_t* images;
  const float* cand_xy;         // [k][stride][2]
  const int32_t* cand_count;    // [k]
  const int32_t* cand_status;   // [k]
  const uint64_t* codes;        // [n_codes]
  int32_t* edges;               // [k][stride][EDGE_INTS]
  float* corners;               // [k][n_tags][4][2]
  int32_t* hamming;             // [k][n_tags]
  int32_t* count;               // [k]
  int32_t* status;              // [k]
  int32_t* n_quads;             // [k], nullable, as the two below
  int32_t* n_foreign;
  int32_t* n_edges_dropped;
  double* strength;             // [k][n_tags][4], nullable: NaN (no refinement follows)
};

struct PointArgs {
  const float* corners;     // [n][n_tags][4][2]
  const int32_t* hamming;   // [n][n_tags]
  long long n_images;
  int32_t cols, n_tags;
  double tag_size, tag_spacing;
  float* corners_px;        // [M][2]
  float* board_xy;          // [M][2]
  long long* offsets;       // [n + 1]
};

// f(t) on every thread of the workgroup of n threads (host: a loop), and the barrier between two such passes.
template <class F>
CLC_HD void threads(int n, F f) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)n;
  f((int)threadIdx.x);
#else
  for (int t = 0; t < n; ++t) f(t);
#endif
}
CLC_HD void barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

// v[0] = the sum (op 0) or the smallest (op 1) of v[0 .. n - 1], n a power of two, by halves across the threads.
CLC_HD void fold(int32_t* v, int n, int op) {
  for (int w = n / 2; w >= 1; w >>= 1) {
    threads(n, [&](int t) {
      if (t >= w) return;
      const int32_t x = v[t], y = v[t + w];
      v[t] = op ? (y < x ? y : x) : x + y;
    });
    barrier();
  }
}

CLC_HD long long floor_div(long long a, long long m) {  // m > 0
  const long long q = a / m;
  return (a % m != 0 && a < 0) ? q - 1 : q;
}

// round(a / den) = floor((2 a + den) / (2 den))
CLC_HD long long round_div(long long a, long long den) { return floor_div(2 * a + den, 2 * den); }

// ---------------------------------------------------------------------------------------------------------------------------------
// Directed edges
// ---------------------------------------------------------------------------------------------------------------------------------
struct EdgeLds {
  int32_t cx[MAX_CAND], cy[MAX_CAND];
  int32_t red[EDGE_THREADS];
};

// The candidates of the launch's image k as integers into LDS (every thread of the workgroup of n_threads calls it) -> their number.
CLC_HD int load_candidates(const TagArgs& a, long long k, int n_threads, int32_t* cx, int32_t* cy) {
  int n = a.cand_status[k] == DETECT_OVERFLOW ? 0 : a.cand_count[k];
  n = n < 0 ? 0 : (n > a.stride ? a.stride : (n > MAX_CAND ? MAX_CAND : n));
  const float* xy = a.cand_xy + k * (long long)a.stride * 2;
  threads(n_threads, [&](int t) {
    for (int s = t; s < n; s += n_threads) {
      cx[s] = (int32_t)xy[2 * s];
      cy[s] = (int32_t)xy[2 * s + 1];
    }
  });
  barrier();
  return n;
}

// The edge p -> q of an image (img: its first byte): true where it passes, with the sums of its inside and outside samples.
CLC_HD bool edge_test(const TagArgs& a, const uint8_t* img, int px, int py, int qx, int qy, int32_t* sum_in, int32_t* sum_out) {
  const long long vx = (long long)qx - px, vy = (long long)qy - py;
  const long long v2 = vx * vx + vy * vy;
  if (v2 < (long long)a.min_side * a.min_side || v2 > (long long)a.max_side * a.max_side) return false;
  const long long dd = a.d + 2 * a.b, den = 4 * S * dd;
  const long long ox = -vy * a.b * 2 * S, oy = vx * a.b * 2 * S;  // n b 2 S with n = (-vy, vx)
  int lo_out = 255, hi_in = 0, si = 0, so = 0;
  for (int i = 1; i <= S - 2; ++i) {
    const long long bx = (long long)px * den + vx * (2 * i + 1) * 2 * dd, by = (long long)py * den + vy * (2 * i + 1) * 2 * dd;
    const long long ix = round_div(bx + ox, den), iy = round_div(by + oy, den), ux = round_div(bx - ox, den), uy = round_div(by - oy, den);
    if (ix < 0 || ix >= a.width || iy < 0 || iy >= a.height || ux < 0 || ux >= a.width || uy < 0 || uy >= a.height) return false;
    const int vi = img[iy * a.pitch + ix], vo = img[uy * a.pitch + ux];
    hi_in = vi > hi_in ? vi : hi_in;
    lo_out = vo < lo_out ? vo : lo_out;
    si += vi; so += vo;
  }
  if (lo_out - hi_in < a.contrast) return false;
  *sum_in = si; *sum_out = so;
  return true;
}

// The launch's image k: every thread of its workgroup calls it (host: once).
CLC_HD void edges_image(const TagArgs& a, long long k, EdgeLds& L) {
  const int n = load_candidates(a, k, EDGE_THREADS, L.cx, L.cy);
  const uint8_t* img = a.images + k * (long long)a.height * a.pitch;
  threads(EDGE_THREADS, [&](int t) {
    int dropped = 0;
    for (int p = t; p < n; p += EDGE_THREADS) {
      int32_t* e = a.edges + (k * (long long)a.stride + p) * EDGE_INTS;
      int kept = 0;
      for (int q = 0; q < n; ++q) {
        int32_t si, so;
        if (q == p || !edge_test(a, img, L.cx[p], L.cy[p], L.cx[q], L.cy[q], &si, &so)) continue;
        if (kept < MAX_OUT) {
          e[1 + 3 * kept] = q; e[2 + 3 * kept] = si; e[3 + 3 * kept] = so;
          ++kept;
        } else {
          ++dropped;
        }
      }
      e[0] = kept;
    }
    L.red[t] = dropped;
  });
  barrier();
  fold(L.red, EDGE_THREADS, 0);
  threads(EDGE_THREADS, [&](int t) {
    if (t == 0 && a.n_edges_dropped) a.n_edges_dropped[k] = L.red[0];
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Quads and decode
// ---------------------------------------------------------------------------------------------------------------------------------
struct DecodeLds {
  double system[bo::FIXED_DOUBLES + 4];  // K26's 8 x 8 system, its copy, h and its flags (bo::carve with n = 0)
  int32_t cx[MAX_CAND], cy[MAX_CAND];
  int16_t quad[MAX_QUADS * 4];
  int32_t tagkey[MAX_TAGS];   // per id: Hamming << 20 | quad rank << 2 | rotation, NOT_SEEN
  int32_t red[LANES];
  int32_t path[LANES * 4];    // a lane's path: valid, p1, p2, p3
  unsigned long long word[4];
  uint8_t cell[128];          // dd dd <= 121: 1 white
  int32_t misc[4];            // [0] quads so far, [1] a sample left the image, [2] white border cells, [3] foreign decodes
  // the image's outputs, parked here from the first pass to the last so that they hold no scalar registers across the decode loop
  float* corners;
  double* strength;
  int32_t *hamming, *count, *status, *n_quads, *n_foreign;
  int32_t overflow;
};
static_assert(sizeof(double) * (bo::FIXED_DOUBLES + 4) >= (size_t)bo::FIXED_BYTES, "K26's fixed LDS");

// The source cell of cell (r, c) of the word read from the corner p_k instead of p_0.
CLC_HD void rotated_cell(int k, int d, int r, int c, int* r0, int* c0) {
  if (k == 0) { *r0 = r; *c0 = c; }
  else if (k == 1) { *r0 = c; *c0 = d - 1 - r; }
  else if (k == 2) { *r0 = d - 1 - r; *c0 = d - 1 - c; }
  else { *r0 = d - 1 - c; *c0 = r; }
}

// The kept edge p -> q: its sum of samples, or -1.  (Branch-free: the entries past the kept ones are read and not used.)
CLC_HD int edge_sum(const int32_t* edges_k, int p, int q) {
  const int32_t* e = edges_k + (long long)p * EDGE_INTS;
  const int kept = e[0];
  int sum = -1;
  for (int j = MAX_OUT - 1; j >= 0; --j) sum = (j < kept && e[1 + 3 * j] == q) ? e[2 + 3 * j] + e[3 + 3 * j] : sum;
  return sum;
}

// The launch's image k: every lane of its wave calls it (host: once).
CLC_HD void decode_image(const TagArgs& a, long long k, DecodeLds& L) {
  const int n = load_candidates(a, k, LANES, L.cx, L.cy);
  const int32_t* E = a.edges + k * (long long)a.stride * EDGE_INTS;
  const uint8_t* img = a.images + k * (long long)a.height * a.pitch;
  const int d = a.d, dd = a.d + 2 * a.b;
  threads(LANES, [&](int lane) {
    for (int id = lane; id < a.n_tags; id += LANES) L.tagkey[id] = NOT_SEEN;
    if (lane < 4) L.misc[lane] = 0;
    if (lane == 0) {
      L.corners = a.corners + k * (long long)a.n_tags * 8;
      L.strength = a.strength ? a.strength + k * (long long)a.n_tags * 4 : nullptr;
      L.hamming = a.hamming + k * (long long)a.n_tags;
      L.count = a.count + k; L.status = a.status + k;
      L.n_quads = a.n_quads ? a.n_quads + k : nullptr;
      L.n_foreign = a.n_foreign ? a.n_foreign + k : nullptr;
      L.overflow = a.cand_status[k] == DETECT_OVERFLOW ? 1 : 0;
    }
  });
  barrier();
  // the quads in lexicographic order: p0 ascending, its paths by the lane number
  for (int p0 = 0; p0 < n; ++p0) {
    const int n0 = E[(long long)p0 * EDGE_INTS];
    if (n0 == 0) continue;
    threads(LANES, [&](int lane) {
      const int e1 = lane >> 4, e2 = (lane >> 2) & 3, e3 = lane & 3;
      // (branch-free: a lane whose path has ended goes on from slot p0, whose lists exist, and stays refused)
      const int32_t* e0 = E + (long long)p0 * EDGE_INTS;
      bool ok = e1 < n0;
      int p1 = e0[1 + 3 * e1];
      ok = ok && p1 > p0;
      p1 = ok ? p1 : p0;
      const int32_t* l1 = E + (long long)p1 * EDGE_INTS;
      ok = ok && e2 < l1[0];
      int p2 = l1[1 + 3 * e2];
      ok = ok && p2 > p0;
      p2 = ok ? p2 : p0;
      const int32_t* l2 = E + (long long)p2 * EDGE_INTS;
      ok = ok && e3 < l2[0];
      int p3 = l2[1 + 3 * e3];
      ok = ok && p3 > p0 && p3 != p1;
      p3 = ok ? p3 : p0;
      ok = ok && edge_sum(E, p3, p0) >= 0;
      L.path[4 * lane] = ok ? 1 : 0; L.path[4 * lane + 1] = p1; L.path[4 * lane + 2] = p2; L.path[4 * lane + 3] = p3;
    });
    barrier();
    threads(LANES, [&](int lane) {
      if (lane != 0) return;
      int nq = L.misc[0];
      for (int l = 0; l < LANES; ++l) {
        if (!L.path[4 * l]) continue;
        if (nq < a.max_quads) {
          L.quad[4 * nq] = (int16_t)p0;
          for (int j = 1; j < 4; ++j) L.quad[4 * nq + j] = (int16_t)L.path[4 * l + j];
        }
        ++nq;
      }
      L.misc[0] = nq;
    });
    barrier();
  }
  const int n_all = L.misc[0], n_dec = n_all < a.max_quads ? n_all : a.max_quads;
  const bo::Lds B = bo::carve(L.system, 0);
  for (int rank = 0; rank < n_dec; ++rank) {
    barrier();  // the quad before this one has been read to its end
    int p[4];
    for (int j = 0; j < 4; ++j) p[j] = L.quad[4 * rank + j];
    int thr = 0;
    for (int j = 0; j < 4; ++j) thr += edge_sum(E, p[j], p[(j + 1) & 3]);
    const bool solved = bo::fit(B, 4, [&](int m, double* X, double* Y, double* u, double* v) {
      *X = (m == 1 || m == 2) ? 1.0 : 0.0;
      *Y = m >= 2 ? 1.0 : 0.0;
      const int s = L.quad[4 * rank + m];
      *u = (double)L.cx[s];
      *v = (double)L.cy[s];
    });
    if (!solved) continue;
    threads(LANES, [&](int lane) {
      if (lane == 0) L.misc[1] = 0;
    });
    barrier();
    threads(LANES, [&](int lane) {
      CLC_BO_NO_CONTRACT
      const double* h = B.h();
      for (int cell = lane; cell < dd * dd; cell += LANES) {
        const int r = cell / dd, c = cell - r * dd;
        const double X = ((double)c + 0.5) / (double)dd, Y = ((double)r + 0.5) / (double)dd;
        const double w0 = h[6] * X, w1 = h[7] * Y, ws = w0 + w1, w = ws + 1.0;
        const double u0 = h[0] * X, u1 = h[1] * Y, us = u0 + u1, un = us + h[2];
        const double v0 = h[3] * X, v1 = h[4] * Y, vs = v0 + v1, vn = vs + h[5];
        const double xr = rint(un / w), yr = rint(vn / w);
        if (!(xr >= 0.0 && xr <= (double)(a.width - 1) && yr >= 0.0 && yr <= (double)(a.height - 1))) {  // (a NaN as well)
          L.misc[1] = 1;
          L.cell[cell] = 0;
          continue;
        }
        const int I = img[(long long)yr * a.pitch + (long long)xr];
        L.cell[cell] = 48 * I > thr ? 1 : 0;
      }
    });
    barrier();
    if (L.misc[1]) continue;
    threads(LANES, [&](int lane) {
      if (lane < 4) {
        unsigned long long w = 0;
        for (int r = 0; r < d; ++r)
          for (int c = 0; c < d; ++c) {
            int r0, c0;
            rotated_cell(lane, d, r, c, &r0, &c0);
            w = (w << 1) | (unsigned long long)L.cell[(r0 + a.b) * dd + (c0 + a.b)];
          }
        L.word[lane] = w;
      } else if (lane == 4) {
        int white = 0;
        for (int r = 0; r < dd; ++r)
          for (int c = 0; c < dd; ++c)
            if (r < a.b || r >= dd - a.b || c < a.b || c >= dd - a.b) white += L.cell[r * dd + c];
        L.misc[2] = white;
      }
    });
    barrier();
    if (L.misc[2] > a.max_border_errors) continue;
    threads(LANES, [&](int lane) {
      int best = NOT_SEEN;
      for (int item = lane; item < 4 * a.n_codes; item += LANES) {
        const int id = item >> 2, rot = item & 3;
        const int ham = __builtin_popcountll(L.word[rot] ^ a.codes[id]);
        const int key = (ham << 14) | (id << 2) | rot;
        best = key < best ? key : best;
      }
      L.red[lane] = best;
    });
    barrier();
    fold(L.red, LANES, 1);
    threads(LANES, [&](int lane) {
      if (lane != 0) return;
      const int key = L.red[0], ham = key >> 14, id = (key >> 2) & 4095, rot = key & 3;
      if (ham > a.max_hamming) return;
      if (id >= a.n_tags) { ++L.misc[3]; return; }
      const int mine = (ham << 20) | (rank << 2) | rot;
      if (mine < L.tagkey[id]) L.tagkey[id] = mine;
    });
  }
  barrier();
  threads(LANES, [&](int lane) {
    int seen = 0;
    float* corners = L.corners;
    double* strength = L.strength;
    int32_t* hamming = L.hamming;
    for (int id = lane; id < a.n_tags; id += LANES) {
      const int key = L.tagkey[id];
      float* out = corners + (long long)id * 8;
      if (strength)
        for (int j = 0; j < 4; ++j) strength[(long long)id * 4 + j] = __builtin_nan("");
      if (key == NOT_SEEN) {
        for (int j = 0; j < 8; ++j) out[j] = __builtin_nanf("");
        hamming[id] = -1;
        continue;
      }
      const int rank = (key >> 2) & 1023, rot = key & 3;
      for (int j = 0; j < 4; ++j) {  // corner j of the tag: the quad's corner rot + 3 - j
        const int s = L.quad[4 * rank + ((rot + 3 - j) & 3)];
        out[2 * j] = (float)L.cx[s];
        out[2 * j + 1] = (float)L.cy[s];
      }
      hamming[id] = key >> 20;
      ++seen;
    }
    L.red[lane] = seen;
  });
  barrier();
  fold(L.red, LANES, 0);
  threads(LANES, [&](int lane) {
    if (lane != 0) return;
    *L.count = L.red[0];
    *L.status = L.overflow ? CLC_TAG_OVERFLOW : CLC_TAG_OK;
    if (L.n_quads) *L.n_quads = L.misc[0];
    if (L.n_foreign) *L.n_foreign = L.misc[3];
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The compaction
// ---------------------------------------------------------------------------------------------------------------------------------
struct ScanLds {
  long long v[SCAN_THREADS];
  long long carry;
};

// offsets[i + 1] = 4 x the tags seen in the images 0 .. i: every thread of the one workgroup calls it (host: once).
CLC_HD void scan_counts(const PointArgs& g, ScanLds& L) {
  threads(SCAN_THREADS, [&](int t) {
    if (t == 0) { L.carry = 0; g.offsets[0] = 0; }
  });
  barrier();
  for (long long first = 0; first < g.n_images; first += SCAN_THREADS) {
    threads(SCAN_THREADS, [&](int t) {
      long long c = 0;
      if (first + t < g.n_images) {
        const int32_t* ham = g.hamming + (first + t) * (long long)g.n_tags;
        for (int id = 0; id < g.n_tags; ++id) c += ham[id] >= 0 ? 1 : 0;
      }
      L.v[t] = c;
    });
    barrier();
    threads(SCAN_THREADS, [&](int t) {
      if (t != 0) return;  // (256 additions per 256 images: the counting above is the work)
      long long run = L.carry;
      for (int i = 0; i < SCAN_THREADS; ++i) { run += L.v[i]; L.v[i] = run; }
      L.carry = run;
    });
    barrier();
    threads(SCAN_THREADS, [&](int t) {
      if (first + t < g.n_images) g.offsets[first + t + 1] = 4 * L.v[t];
    });
    barrier();
  }
}

// Image img: every lane of its wave calls it (host: once).  flag: 64 ints of LDS.
CLC_HD void points_image(const PointArgs& g, long long img, int32_t* flag) {
  CLC_BO_NO_CONTRACT
  const int32_t* ham = g.hamming + img * (long long)g.n_tags;
  const float* in = g.corners + img * (long long)g.n_tags * 8;
  const double period = g.tag_size * (1.0 + g.tag_spacing);
  long long run = g.offsets[img];
  for (int id0 = 0; id0 < g.n_tags; id0 += LANES) {
    threads(LANES, [&](int lane) { flag[lane] = (id0 + lane < g.n_tags && ham[id0 + lane] >= 0) ? 1 : 0; });
    barrier();
    int total = 0;
    for (int l = 0; l < LANES; ++l) total += flag[l];
    threads(LANES, [&](int lane) {
      CLC_BO_NO_CONTRACT
      if (!flag[lane]) return;
      int before = 0;
      for (int l = 0; l < lane; ++l) before += flag[l];
      const int id = id0 + lane, row = id / g.cols, col = id - row * g.cols;
      const double X0 = (double)col * period, Y0 = (double)row * period, X1 = X0 + g.tag_size, Y1 = Y0 + g.tag_size;
      float* px = g.corners_px + (run + 4 * (long long)before) * 2;
      float* bd = g.board_xy + (run + 4 * (long long)before) * 2;
      for (int j = 0; j < 8; ++j) px[j] = in[(long long)id * 8 + j];
      bd[0] = (float)X0; bd[1] = (float)Y0; bd[2] = (float)X1; bd[3] = (float)Y0;
      bd[4] = (float)X1; bd[5] = (float)Y1; bd[6] = (float)X0; bd[7] = (float)Y1;
    });
    barrier();
    run += 4 * (long long)total;
  }
}

#if defined(__HIPCC__)

// K27, first kernel: blockIdx.x = the image of the launch.
static __global__ __launch_bounds__(EDGE_THREADS) void tag_edges_kernel(const TagArgs a) {
  __shared__ EdgeLds L;
  edges_image(a, (long long)blockIdx.x, L);
}

// K27, second kernel: one wave per image of the launch.
static __global__ __launch_bounds__(LANES) void tag_decode_kernel(const TagArgs a) {
  __shared__ DecodeLds L;
  decode_image(a, (long long)blockIdx.x, L);
}

// The compaction: one workgroup scans the counts, then one wave per image.
static __global__ __launch_bounds__(SCAN_THREADS) void tag_scan_kernel(const PointArgs g) {
  __shared__ ScanLds L;
  scan_counts(g, L);
}
static __global__ __launch_bounds__(LANES) void tag_points_kernel(const PointArgs g, long long first) {
  __shared__ int32_t flag[LANES];
  points_image(g, first + (long long)blockIdx.x, flag);
}

#endif  // __HIPCC__

}  // namespace tags
}  // namespace clc
