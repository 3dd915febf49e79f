// ddpx — what the stride-2 convolution families share (conv_igemm_s2.hip in bf16, f32_conv_s2.hip in fp32): the
// problem shape, the tap shifts of the gathered operand, the data gradient's four parity classes.
#pragma once

#include "ddpx_pipe.h"

namespace ddpx {
namespace s2 {

using pipe::FastDiv;
using pipe::make_fastdiv;

struct ClassGeom {  // one parity class of the data gradient, in launch order
  int ph, pw;       // parity of the class's input rows / columns
  int Hc, Wc;       // its pixels per image column / row
  int rows;         // N*Hc*Wc
  int tile0;        // its first row tile in the launch
  FastDiv dWc, dHc;
};

// shift of the gathered pixel for tap index tl: forward / wgrad (ky - pad, kx - pad) in x; dgrad class
// (ph, pw) the dy pixel (i + da, j + db) and the weight's tap
__device__ __forceinline__ void fwd_shift(int ks, int tl, int& da, int& db) {
  const int ky = (tl * 11) >> 5, kx = tl - ky * 3;  // tl / 3 for tl < 9
  da = ks == 3 ? ky - 1 : 0;
  db = ks == 3 ? kx - 1 : 0;
}
__device__ __forceinline__ void dgrad_shift(int ks, int ph, int pw, int tl, int& da, int& db, int& tap) {
  const int a = pw ? tl >> 1 : tl, b = pw ? tl & 1 : 0;  // tl = a * (1 + pw) + b
  const int ky = ph ? 2 * a : 1, kx = pw ? 2 * b : 1;
  da = ph ? 1 - a : 0;
  db = pw ? 1 - b : 0;
  tap = ks == 3 ? ky * 3 + kx : 0;
}

struct Shape {
  int N, H, W, C, Co, ks, Ho, Wo, T;
  long long Po;
};

// rows (= columns) of tile 0 (128x128) and tile 1 (64x64)
static int tile_rows(int t) { return t == 0 ? 128 : 64; }

// the data gradient's classes in launch order (most taps first); returns the row tiles in all
static int make_classes(const Shape& s, int bm, ClassGeom* cls) {
  static const int order[4][2] = {{1, 1}, {1, 0}, {0, 1}, {0, 0}};
  int t0 = 0;
  for (int q = 0; q < 4; ++q) {
    ClassGeom& c = cls[q];
    c.ph = order[q][0]; c.pw = order[q][1];
    c.Hc = (s.H - c.ph + 1) / 2; c.Wc = (s.W - c.pw + 1) / 2;
    c.rows = s.N * c.Hc * c.Wc;
    c.tile0 = t0;
    c.dWc = make_fastdiv(c.Wc);
    c.dHc = make_fastdiv(c.Hc);
    t0 += (c.rows + bm - 1) / bm;
  }
  // an empty class (H or W of 1) has no tiles: its tile0 equals the next one's, and the kernel's scan
  // (last class with tile0 <= row tile) passes over it
  return t0;
}

}  // namespace s2
}  // namespace ddpx
