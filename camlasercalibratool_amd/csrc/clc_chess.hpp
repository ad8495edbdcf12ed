// clc_chess.hpp — K25: chessboard-corner candidates of many uint8 images at once.  The response is ChESS (Bennett &
// Lasenby) scaled by 5, so that every step is exact int32 arithmetic on the image; what follows it is a non-maximum suppression with
// a total order on ties and a selection under a total order: the result holds the same bits however the work was scheduled.
//
//   per pixel (x, y) of the domain 5 <= x < width - 5, 5 <= y < height - 5, with s_n the 16 ring samples and the 5 cross samples:
//     SR = sum_{n<4} |(s_n + s_{n+8}) - (s_{n+4} + s_{n+12})|,  DR = sum_{n<8} |s_n - s_{n+8}|,  ring = sum s_n,  loc = sum cross,
//     R5 = 5 SR - 5 DR - |5 ring - 16 loc|                                  (|R5| <= 30 600: an int16 holds it)
//
//   chess_response_nms_kernel   one 256-thread workgroup per tile of 64 x 16 pixels.  The tile and a halo of 5 + r go into LDS as bytes,
//                               by aligned 4-byte loads where the word lies inside the image allocation (two words and a funnel shift
//                               where the row is not aligned) and by predicated byte loads at the allocation's two ends: nothing
//                               outside [images, images + n_images height pitch) is read.  R5 on the tile + r goes into LDS as int16
//                               (NO_RESPONSE outside the domain); the suppression reads LDS only.  A survivor is appended to its
//                               image's raw list by atomicAdd on the image's counter; a slot past RAW_CAP is counted, not written.
//   chess_select_kernel         one wave per image: the largest R5, the relative gate, the rank of every kept candidate by counting
//                               those ahead of it under (-R5, y, x), the first max_per_image in rank order, NaN / 0 in the padding.
//                               A counter past RAW_CAP: CLC_CHESS_OVERFLOW and no candidate (never a subset that depends on timing).
//
// tests/shim/chess_shim.cpp compiles this header for the host with g++ and runs the same per-tile and per-image code with the threads
// as loops; the device is compared with it bit for bit.
#pragma once
#include "../../include/clc.h"
#include "clc_math.hpp"

#include <string.h>

namespace clc {
namespace chess {

constexpr int TILE_W = 64, TILE_H = 16, THREADS = 256;
constexpr int RING = 5;                                     // the ring's radius: the margin of the domain
constexpr int MAX_R = 7;                                    // nms_radius <= 7
constexpr int IMG_STRIDE = TILE_W + 2 * (RING + MAX_R);     // bytes per LDS image row (88: a multiple of 4)
constexpr int IMG_ROWS = TILE_H + 2 * (RING + MAX_R);       // 40
constexpr int RESP_STRIDE = TILE_W + 2 * MAX_R;             // int16 per LDS response row (78)
constexpr int RESP_ROWS = TILE_H + 2 * MAX_R;               // 30
constexpr int RAW_CAP = CLC_CHESS_RAW_CAP;
constexpr int NO_RESPONSE = -32768;                         // below every R5: a pixel outside the domain never suppresses
static_assert(IMG_STRIDE % 4 == 0, "LDS image rows are whole words");

struct ChessArgs {
  int32_t width, height, threshold, nms_radius, rel_permille, max_per_image;
  long long pitch;       // bytes per image row
  long long n_images;    // of the whole allocation: the bound of every read
  long long first;       // the first image of this launch; the launch's image k is first + k
  long long tiles_x;
  const uint8_t* images;
  unsigned int* raw_count;  // [images of the launch]
  int32_t* raw;             // [images of the launch][RAW_CAP][3]: x, y, R5
  // outputs, indexed by the absolute image
  float* cand_xy;       // [n][max_per_image][2]
  int32_t* cand_r5;     // [n][max_per_image], nullable
  int32_t* count;       // [n]
  int32_t* count_raw;   // [n], nullable
  int32_t* status;      // [n]
};

// What one tile's workgroup keeps in LDS (host: an ordinary object): 3 520 + 4 680 bytes.
struct Tile {
  uint32_t img[IMG_ROWS * IMG_STRIDE / 4];
  int16_t resp[RESP_ROWS * RESP_STRIDE];
};

// f(t) on every thread of the workgroup (host: a loop), and the barrier between two such passes.
template <class F>
CLC_HD void each_thread(int n, F f) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)n;
  f((int)threadIdx.x);
#else
  for (int t = 0; t < n; ++t) f(t);
#endif
}
CLC_HD void group_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

// The 4 image bytes at byte offsets off .. off + 3 of the allocation [0, total), little end first; a byte outside it reads 0.
CLC_HD uint32_t load_bytes4(const uint8_t* base, long long off, long long total) {
  if (off >= 0 && off + 4 <= total) {
    const uint8_t* p = base + off;
    const long long sh = (long long)((uintptr_t)p & 3u);
    if (off - sh >= 0 && (sh == 0 || off - sh + 8 <= total)) {  // the aligned word(s) holding them lie inside the allocation
      uint32_t lo, hi = 0;
#if defined(__HIP_DEVICE_COMPILE__)
      lo = *reinterpret_cast<const uint32_t*>(p - sh);
      if (sh) hi = *reinterpret_cast<const uint32_t*>(p - sh + 4);
#else
      memcpy(&lo, p - sh, 4);
      if (sh) memcpy(&hi, p - sh + 4, 4);
#endif
      return sh ? (lo >> (8 * sh)) | (hi << (32 - 8 * sh)) : lo;
    }
  }
  uint32_t v = 0;
  for (int b = 0; b < 4; ++b) {
    const long long o = off + b;
    if (o >= 0 && o < total) v |= (uint32_t)base[o] << (8 * b);
  }
  return v;
}

// R5 at the LDS image position (row, col) (bytes, row stride IMG_STRIDE).
CLC_HD int response5(const uint8_t* im, int row, int col) {
  const uint8_t* c = im + row * IMG_STRIDE + col;
  auto I = [&](int dx, int dy) { return (int)c[dy * IMG_STRIDE + dx]; };
  const int s0 = I(0, -5), s1 = I(2, -5), s2 = I(3, -3), s3 = I(5, -2), s4 = I(5, 0), s5 = I(5, 2), s6 = I(3, 3), s7 = I(2, 5);
  const int s8 = I(0, 5), s9 = I(-2, 5), s10 = I(-3, 3), s11 = I(-5, 2), s12 = I(-5, 0), s13 = I(-5, -2), s14 = I(-3, -3), s15 = I(-2, -5);
  auto ab = [](int v) { return v < 0 ? -v : v; };
  const int sr = ab((s0 + s8) - (s4 + s12)) + ab((s1 + s9) - (s5 + s13)) + ab((s2 + s10) - (s6 + s14)) + ab((s3 + s11) - (s7 + s15));
  const int dr = ab(s0 - s8) + ab(s1 - s9) + ab(s2 - s10) + ab(s3 - s11) + ab(s4 - s12) + ab(s5 - s13) + ab(s6 - s14) + ab(s7 - s15);
  const int ring = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) + ((s8 + s9) + (s10 + s11)) + ((s12 + s13) + (s14 + s15));
  const int loc = I(0, 0) + I(1, 0) + I(-1, 0) + I(0, 1) + I(0, -1);
  return 5 * sr - 5 * dr - ab(5 * ring - 16 * loc);
}

// One more raw candidate of the launch's image k (host: the threads run one after another).
CLC_HD void append_raw(const ChessArgs& a, long long k, int x, int y, int r5) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned int slot = atomicAdd(a.raw_count + k, 1u);
#else
  const unsigned int slot = a.raw_count[k]++;
#endif
  if (slot >= (unsigned int)RAW_CAP) return;
  int32_t* e = a.raw + (k * RAW_CAP + (long long)slot) * 3;
  e[0] = x; e[1] = y; e[2] = r5;
}

// The tile (tx, ty) of the launch's image k: every thread of its workgroup calls it (host: once).
CLC_HD void process_tile(const ChessArgs& a, long long k, long long tx, long long ty, Tile& L) {
  const int r = a.nms_radius, halo = RING + r;
  const long long x0 = tx * TILE_W, y0 = ty * TILE_H;
  // (wave-uniform) a tile without a pixel of the domain
  if (x0 >= (long long)a.width - RING || y0 >= (long long)a.height - RING || x0 + TILE_W <= RING || y0 + TILE_H <= RING) return;
  const long long total = a.n_images * (long long)a.height * a.pitch;
  const long long origin = (a.first + k) * (long long)a.height * a.pitch + (y0 - halo) * a.pitch + (x0 - halo);  // of LDS byte (0, 0)
  const int lww = (TILE_W + 2 * halo + 3) / 4, lh = TILE_H + 2 * halo;  // words per row (at most IMG_STRIDE / 4) and rows of the LDS image
  each_thread(THREADS, [&](int t) {
    int row = t / lww, w = t - row * lww;
    const int drow = THREADS / lww, dw = THREADS - drow * lww;
    for (int i = t; i < lww * lh; i += THREADS) {
      L.img[row * (IMG_STRIDE / 4) + w] = load_bytes4(a.images, origin + (long long)row * a.pitch + 4 * w, total);
      row += drow; w += dw;
      if (w >= lww) { w -= lww; ++row; }
    }
  });
  group_barrier();
  const uint8_t* im = reinterpret_cast<const uint8_t*>(L.img);
  const int rw = TILE_W + 2 * r, rh = TILE_H + 2 * r;  // the responses: the tile + r
  each_thread(THREADS, [&](int t) {
    int i = t / rw, j = t - i * rw;
    const int di = THREADS / rw, dj = THREADS - di * rw;
    for (int q = t; q < rw * rh; q += THREADS) {
      const long long x = x0 - r + j, y = y0 - r + i;
      const bool in_domain = x >= RING && x < (long long)a.width - RING && y >= RING && y < (long long)a.height - RING;
      L.resp[i * RESP_STRIDE + j] = (int16_t)(in_domain ? response5(im, i + RING, j + RING) : NO_RESPONSE);
      i += di; j += dj;
      if (j >= rw) { j -= rw; ++i; }
    }
  });
  group_barrier();
  each_thread(THREADS, [&](int t) {
    for (int q = t; q < TILE_W * TILE_H; q += THREADS) {
      const int px = q & (TILE_W - 1), py = q / TILE_W;
      const int16_t* c = L.resp + (py + r) * RESP_STRIDE + (px + r);
      const int v = c[0];
      if (v < a.threshold) continue;  // (and every pixel outside the domain: threshold >= 1)
      bool keep = true;
      for (int dy = -r; dy <= r && keep; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
          const int u = c[dy * RESP_STRIDE + dx];
          const bool before = dy < 0 || (dy == 0 && dx < 0);  // q ahead of p in raster order
          if (u > v || (u == v && before)) { keep = false; break; }
        }
      if (keep) append_raw(a, k, (int)(x0 + px), (int)(y0 + py), v);
    }
  });
}

// a ahead of b under (-R5, y, x)
CLC_HD bool ahead(int ar, int ay, int ax, int br, int by, int bx) {
  if (ar != br) return ar > br;
  if (ay != by) return ay < by;
  return ax < bx;
}

// The reduction of f(lane) over the 64 lanes of the image's wave, the same on every lane (host: a loop).  op: 0 max, 1 sum.
template <class F>
CLC_HD int wave_reduce_i32(int op, F f) {
#if defined(__HIP_DEVICE_COMPILE__)
  int v = f((int)(threadIdx.x & 63));
  for (int m = 32; m >= 1; m >>= 1) {
    const int o = __shfl_xor(v, m, 64);
    v = op ? v + o : (o > v ? o : v);
  }
  return v;
#else
  int v = f(0);
  for (int l = 1; l < 64; ++l) {
    const int o = f(l);
    v = op ? v + o : (o > v ? o : v);
  }
  return v;
#endif
}

// The launch's image k: every lane of its wave calls it (host: once).
CLC_HD void select_image(const ChessArgs& a, long long k) {
  const long long n = a.first + k;
  const int cap = a.max_per_image;
  const unsigned int counted = a.raw_count[k];
  const bool overflow = counted > (unsigned int)RAW_CAP;
  const int c = overflow ? 0 : (int)counted;
  const int32_t* raw = a.raw + k * RAW_CAP * 3;
  const int best = wave_reduce_i32(0, [&](int lane) {
    int m = NO_RESPONSE;
    for (int i = lane; i < c; i += 64) m = raw[3 * i + 2] > m ? raw[3 * i + 2] : m;
    return m;
  });
  const long long gate = (long long)a.rel_permille * (long long)best;
  auto kept = [&](int r5) { return 1000ll * (long long)r5 >= gate; };
  const int n_kept = wave_reduce_i32(1, [&](int lane) {
    int m = 0;
    for (int i = lane; i < c; i += 64) m += kept(raw[3 * i + 2]) ? 1 : 0;
    return m;
  });
  const int n_out = n_kept < cap ? n_kept : cap;
  float* xy = a.cand_xy + n * (long long)cap * 2;
  int32_t* r5o = a.cand_r5 ? a.cand_r5 + n * (long long)cap : nullptr;
  each_thread(64, [&](int lane) {
    for (int s = n_out + lane; s < cap; s += 64) {
      xy[2 * s] = __builtin_nanf("");
      xy[2 * s + 1] = __builtin_nanf("");
      if (r5o) r5o[s] = 0;
    }
    for (int i = lane; i < c; i += 64) {
      const int x = raw[3 * i], y = raw[3 * i + 1], v = raw[3 * i + 2];
      if (!kept(v)) continue;
      int rank = 0;  // (a candidate ahead of a kept one is kept: its R5 is no smaller)
      for (int j = 0; j < c; ++j) rank += ahead(raw[3 * j + 2], raw[3 * j + 1], raw[3 * j], v, y, x) ? 1 : 0;
      if (rank >= cap) continue;
      xy[2 * rank] = (float)x;
      xy[2 * rank + 1] = (float)y;
      if (r5o) r5o[rank] = v;
    }
    if (lane == 0) {
      a.count[n] = n_out;
      if (a.count_raw) a.count_raw[n] = (int32_t)(counted > 0x7FFFFFFFu ? 0x7FFFFFFFu : counted);
      a.status[n] = overflow ? CLC_CHESS_OVERFLOW : CLC_CHESS_OK;
    }
  });
}

#if defined(__HIPCC__)

// K25, first kernel: blockIdx.x = the tile (row-major), blockIdx.y = the image of the launch.
static __global__ __launch_bounds__(THREADS) void chess_response_nms_kernel(const ChessArgs a) {
  __shared__ Tile L;
  const long long tile = (long long)blockIdx.x;
  const long long ty = tile / a.tiles_x;
  process_tile(a, (long long)blockIdx.y, tile - ty * a.tiles_x, ty, L);
}

// K25, second kernel: one wave per image of the launch.
static __global__ __launch_bounds__(64) void chess_select_kernel(const ChessArgs a) { select_image(a, (long long)blockIdx.x); }

#endif  // __HIPCC__

}  // namespace chess
}  // namespace clc
