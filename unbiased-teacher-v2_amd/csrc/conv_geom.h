// Integer geometry shared by the convolution kernels (conv.hip, conv_bf16.hip, bottleneck.hip): the level table of multi-level
// activations, the XCD-aware tile order, the NHWC output-row decode, the tap-validity mask, the record of the per-row geometry
// table (rowinfo) and the accumulator zero fill.  Every formula is written once, here; every helper is forced inline and does the
// integer operations, in the widths, of the kernel text it stands for (the widths differ per kernel on purpose: see nhwc_row).
#pragma once
#include "common.h"

#define CONV_MAX_LEVELS 8
// Multi-level ("ragged") activations: rows [start[l], start[l+1]) hold N images of H[l] x W[l] pixels
// (level-first layout of DESIGN.md section 2), so ONE launch covers every FPN level of a shared head.
struct LevelTab {
  int n;                         // 0 = single dense NHWC tensor
  int start[CONV_MAX_LEVELS + 1];
  int H[CONV_MAX_LEVELS], W[CONV_MAX_LEVELS];
};

// host: fill the table for N images of nlev levels; returns the total row count
static inline int fill_levels(LevelTab& lt, int nlev, int N, const int* H, const int* W) {
  lt.n = nlev;
  int off = 0;
  for (int l = 0; l < CONV_MAX_LEVELS; ++l) {
    lt.start[l] = off;
    if (l < nlev) {
      lt.H[l] = H[l];
      lt.W[l] = W[l];
      off += N * H[l] * W[l];
    } else {
      lt.H[l] = lt.W[l] = 1;
    }
  }
  lt.start[CONV_MAX_LEVELS] = off;
  return off;
}

// row m of a level-first matrix -> its level's H, W, the pixel (oh, ow) and the index of its image's first pixel
__device__ __forceinline__ void ml_decode(const LevelTab& lt, int m, int& pixbase, int& H, int& W, int& oh, int& ow) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < CONV_MAX_LEVELS; ++i)
    if (i < lt.n && m >= lt.start[i]) l = i;
  H = lt.H[l];
  W = lt.W[l];
  const int r = m - lt.start[l], hw = H * W;
  const int n = r / hw, rem = r - n * hw;
  oh = rem / W;
  ow = rem - oh * W;
  pixbase = lt.start[l] + n * hw;
}

// XCD-aware tile order: workgroup bid of nwg runs on XCD bid % 8 (observed dispatch rule; speed only); each XCD walks a contiguous
// range of tiles, so neighbouring tiles (shared halo rows, same weights) hit one L2.  A bijection of [0, nwg) for any nwg.
__device__ __forceinline__ int xcd_tile(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Output pixel (n, oh, ow) of an [N, OH, OW] output over an [N, H, W] input: the input pixel index of its image's first pixel and
// the input row / column of tap (0, 0) (may lie outside the image).  PB is the width the caller keeps its pixel base in (the
// 128-tile kernels: long long; the v2 family, whose launch path bounds the operand below 2^31 elements: int).
template <typename PB>
__device__ __forceinline__ void nhwc_row_at(int n, int oh, int ow, int H, int W, int stride, int pad, PB& pixbase, int& ih0, int& iw0) {
  ih0 = oh * stride - pad;
  iw0 = ow * stride - pad;
  pixbase = (PB)n * H * W;
}
// the same from the output row m = (n * OH + oh) * OW + ow
template <typename PB>
__device__ __forceinline__ void nhwc_row(int m, int OH, int OW, int H, int W, int stride, int pad, PB& pixbase, int& ih0, int& iw0) {
  const int hw = OH * OW;
  const int n = m / hw, rem = m - n * hw;
  const int oh = rem / OW, ow = rem - oh * OW;
  nhwc_row_at(n, oh, ow, H, W, stride, pad, pixbase, ih0, iw0);
}

// bit kh * KW + kw is set iff tap (kh, kw) of the row whose tap (0, 0) is input pixel (ih0, iw0) lies inside the H x W image
// (row_valid false: a row past the end of the matrix, which has no taps - tested with every tap, as the tile prologues always did)
__device__ __forceinline__ unsigned tap_mask(int ih0, int iw0, int H, int W, int KH, int KW, bool row_valid = true) {
  unsigned mk = 0;
  for (int kh = 0; kh < KH; ++kh)
    for (int kw = 0; kw < KW; ++kw)
      if (row_valid && (unsigned)(ih0 + kh) < (unsigned)H && (unsigned)(iw0 + kw) < (unsigned)W) mk |= 1u << (kh * KW + kw);
  return mk;
}

// One record of the per-output-row geometry table (utv2_rowinfo_nhwc): {anchor, (W << 16) | mask} - anchor = the input pixel index of
// tap (0, 0) (may lie outside the image), W = the input row length, mask = tap_mask of the row.  Tap (kh, kw) of the row reads input
// pixel anchor + kh * W + kw iff its mask bit is set.  The mask has ROWINFO_MAX_TAPS bits; W stays below ROWINFO_MAX_W so the
// packed word is non-negative and the arithmetic shift returns W.
#define ROWINFO_W_SHIFT 16
#define ROWINFO_MAX_TAPS ROWINFO_W_SHIFT
#define ROWINFO_MAX_W (1 << (31 - ROWINFO_W_SHIFT))
struct RowGeom {
  int anchor, W;
  unsigned mask;
};
__device__ __forceinline__ int2 rowinfo_pack(int anchor, int W, int mask) { return make_int2(anchor, (W << ROWINFO_W_SHIFT) | mask); }
template <typename R>   // R: int2, or the two-int vector a kernel keeps the record in
__device__ __forceinline__ RowGeom rowinfo_unpack(const R& ri) {
  return RowGeom{ri.x, ri.y >> ROWINFO_W_SHIFT, (unsigned)(ri.y & ((1 << ROWINFO_W_SHIFT) - 1))};
}
// mask bit `tap` (< ROWINFO_MAX_TAPS) of a record
template <typename R>
__device__ __forceinline__ int rowinfo_tap(const R& ri, int tap) { return (ri.y >> tap) & 1; }

// accumulator tiles start at zero
template <int A>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[A]) {
#pragma unroll
  for (int i = 0; i < A; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
}
template <int A, int B>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[A][B]) {
#pragma unroll
  for (int i = 0; i < A; ++i) zero_acc(acc[i]);
}
