// One frozen 64-channel identity BasicBlock (D2 BasicBlock with FrozenBN folded to scale / shift: both 3x3 convs stride 1 pad 1, no
// shortcut conv; every res2 block of R-18 / R-34 under MODEL.BACKBONE.FREEZE_AT 2, student and teacher) as ONE kernel:
//
//     c1 = h16(relu(conv1(x) s1 + b1))            zero outside the image (conv2's zero padding applies to c1)
//     y  = h16(relu(conv2(c1) s2 + b2 + x))       x, y: [N, H, W, 64] 16-bit NHWC
//
// Unfused that is two launches of the 16-bit conv kernel which move x (read), c1 (write + read), x again (residual) and y; fused, c1
// lives in LDS and the block moves x once (plus its two-pixel halo, mostly L2 hits between neighbouring tiles of one XCD) and y.  The
// price: conv1 is computed on the tile's 10 x 18 halo, 180 / 128 of its pixels (padded to 192 for the 32-pixel MFMA blocks).  No backward
// exists for a frozen stage, so nothing has to be kept.
//
// Workgroup = 4 waves = one 8 x 16 output tile of one image, the geometry, GEMM orientation (TRANSPOSED: A = weights [co][k], B = pixels
// [px][k], C[co][px]; a lane holds 4 consecutive channels of one pixel per accumulator quad) and tap streaming of csrc/bottleneck.hip:
//   prologue x on the tile's 12 x 20 halo (240 pixels x 128 B) global -> registers -> LDS, ZERO outside the image.
//   phase 1  conv1 from x in LDS (implicit im2col = shifted row addresses) on the 192 halo pixels of c1: 12 MFMA blocks (6 pixel x 2
//            channel) = 3 per wave.  The 18 taps of w1 and w2 are ONE stream: 8 KB per tap, register ring three taps ahead, double-buffered
//            in LDS, so conv2's first taps arrive while conv1 still computes.
//   between  every lane takes the residual (its own output pixel of x, in the accumulator layout: 16 registers) out of LDS; then c1
//            [192 px][64] overwrites x.
//   phase 2  conv2 from c1 exactly as the bottleneck's phase 2: wave w owns pixel block w, both channel blocks.
//   epilogue acc * s2 + b2 + x, ReLU, rounding in the accumulator layout -> a wave-private 16-bit patch in the (dead) tap buffers -> y in
//            full 128-byte rows.
// LDS: 30 KB (x, then c1 in its first 24 KB) + 16 KB (tap buffers, then the output patches) + 1 KB (scale / shift) = 47 KB -> three
// workgroups per CU, which overlap each other's load and MFMA phases.  All LDS rows are 128 bytes, XOR-swizzled on their 16-byte slots
// (slot ^ (row & 7)) so the 32-row fragment reads are conflict-free.  blockIdx -> tile through xcd_tile (conv_geom.h).
#include "common.h"
#include "conv_geom.h"

#define BB_TH 8
#define BB_TW 16
#define BB_C 64
#define BB_CW 18                         // c1 halo: 10 x 18
#define BB_CHALO 180
#define BB_CP 192
#define BB_XW 20                         // x halo: 12 x 20
#define BB_XHALO 240
#define BB_XPIECES (BB_XHALO * 8)        // 16-byte pieces of the x halo
#define BB_X (BB_XHALO * 128)
#define BB_WBUF 8192
#define BB_TAPROW (9 * BB_C)             // elements of one output channel's row of a [64][3][3][64] weight
#define BB_LDS (BB_X + 2 * BB_WBUF + 256 * 4)

struct BbArgs {
  const h16_t* x;
  h16_t* y;
  const h16_t *w1, *w2;                  // [64][3*3*64] each (tap-major, channel-minor)
  const float *s1, *b1, *s2, *b2;        // folded FrozenBN scale / shift per output channel
  int N, H, W, tiles_x, tiles_y, ntiles;
};

__device__ __forceinline__ bf16x8_t bb_frag(const unsigned char* smem, int off) { return *(const bf16x8_t*)(smem + off); }

// 16-byte piece `slot` of row `row` of a swizzled [rows][128 B] LDS image
__device__ __forceinline__ int bb_at(int row, int slot) { return row * 128 + ((slot ^ (row & 7)) << 4); }

__global__ __launch_bounds__(256, 3) void basicblock_fused(BbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // LDS map: [0, 30K): x on the 12 x 20 halo, then (first 24 KB) c1 on the 10 x 18 halo; [30K, 46K): the two tap buffers, then the four
  // wave-private output patches (4 KB each); [46K, 47K): s1 b1 s2 b2
  unsigned char* xl = smem;
  unsigned char* c1 = smem;
  unsigned char* wl = smem + BB_X;
  float* prm = (float*)(smem + BB_X + 2 * BB_WBUF);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, fh = lane >> 5;

  const int t = xcd_tile(blockIdx.x, a.ntiles);
  const int per = a.tiles_x * a.tiles_y;
  const int n = t / per, rem = t - n * per, ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
  const int y0 = ty * BB_TH, x0 = tx * BB_TW;
  const h16_t* ximg = a.x + (size_t)n * a.H * a.W * BB_C;

  // ---------------- prologue: the x halo, the first three taps, the parameters ----------------
  const bf16x8_t zero8 = {};
  bf16x8_t xv[8];
  int xdst[8];                           // LDS offset of the piece, -1: none (1920 pieces over 8 x 256 threads)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int q = tid + 256 * i, hp = q >> 3, slot = q & 7;
    const int hy = hp / BB_XW, hx = hp - hy * BB_XW, gy = y0 - 2 + hy, gx = x0 - 2 + hx;
    const bool in = q < BB_XPIECES && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    xv[i] = in ? *(const bf16x8_t*)(ximg + ((size_t)gy * a.W + gx) * BB_C + slot * 8) : zero8;
    xdst[i] = q < BB_XPIECES ? bb_at(hp, slot) : -1;
  }
  // taps: two pieces per thread of a [64 co][64 ci] tap image (128-byte rows); tap g of the stream = tap g of w1 (g < 9), tap g - 9 of w2
  const int t2co[2] = {tid >> 3, (tid + 256) >> 3}, t2slot = tid & 7;
  bf16x8_t tr[3][2];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int i = 0; i < 2; ++i) tr[g][i] = *(const bf16x8_t*)(a.w1 + t2co[i] * BB_TAPROW + g * BB_C + t2slot * 8);
  {
    const float* srcs[4] = {a.s1, a.b1, a.s2, a.b2};
    prm[tid] = srcs[tid >> 6][tid & 63];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (xdst[i] >= 0) *(bf16x8_t*)(xl + xdst[i]) = xv[i];
#pragma unroll
  for (int i = 0; i < 2; ++i) *(bf16x8_t*)(wl + bb_at(t2co[i], t2slot)) = tr[0][i];
  __syncthreads();

  // ---------------- phase 1: c1 = relu(conv1(x) * s1 + b1) on the 10 x 18 halo ----------------
  f32x16 acc1[3];
  zero_acc(acc1);
  const int pbA = wave, pbB = 4 + (wave >> 1), cbB = wave & 1;   // blocks (pbA, 0), (pbA, 1), (pbB, cbB)
  const int pxA = pbA * 32 + l31, pxB = pbB * 32 + l31;
  // x-halo pixel under tap (0, 0) of the c1-halo pixel; the 12 padding pixels (>= 180) read pixel 0 (their c1 is forced to zero)
  const int hA = (pxA / BB_CW) * BB_XW + pxA % BB_CW;
  const int hB = pxB < BB_CHALO ? (pxB / BB_CW) * BB_XW + pxB % BB_CW : 0;
  const int w0row = l31, w1row = 32 + l31;
  const int p = wave * 32 + l31, pr = p >> 4, pc = p & 15;      // this lane's output pixel of the tile
  bf16x4_t res[2][4];                                            // its residual, channels cb * 32 + 8 q + 4 fh .. + 3
#pragma unroll
  for (int g = 0; g < 9; ++g) {
    const unsigned char* cur = wl + (g & 1) * BB_WBUF;
    unsigned char* nxt = wl + ((g + 1) & 1) * BB_WBUF;
    {                                   // ring slot g % 3 went to LDS one iteration ago
      const h16_t* wsrc = (g + 3 < 9) ? a.w1 + (g + 3) * BB_C : a.w2 + (g + 3 - 9) * BB_C;
#pragma unroll
      for (int i = 0; i < 2; ++i) tr[g % 3][i] = *(const bf16x8_t*)(wsrc + t2co[i] * BB_TAPROW + t2slot * 8);
    }
    const int dy = g / 3, dx = g - dy * 3;
    const int ra = hA + dy * BB_XW + dx, rb = hB + dy * BB_XW + dx;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int slot = ks * 2 + fh;
      const bf16x8_t xa = bb_frag(xl, bb_at(ra, slot));
      const bf16x8_t xb = bb_frag(xl, bb_at(rb, slot));
      const bf16x8_t wa = bb_frag(cur, bb_at(w0row, slot));
      const bf16x8_t wb = bb_frag(cur, bb_at(w1row, slot));
      acc1[0] = mfma_32x32x16(wa, xa, acc1[0]);
      acc1[1] = mfma_32x32x16(wb, xa, acc1[1]);
      acc1[2] = mfma_32x32x16(cbB ? wb : wa, xb, acc1[2]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *(bf16x8_t*)(nxt + bb_at(t2co[i], t2slot)) = tr[(g + 1) % 3][i];
    if (g == 8) {                       // x is overwritten after the barrier: the residual leaves LDS now
      const int xr = (pr + 2) * BB_XW + pc + 2;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) res[cb][q] = *(const bf16x4_t*)(xl + bb_at(xr, cb * 4 + q) + fh * 8);
    }
    __syncthreads();
  }

  // c1 epilogue: value = acc * s + b, ReLU, zero outside the image, round, 8-byte LDS stores over the (dead) x halo
  {
    const int pxs[3] = {pxA, pxA, pxB}, cbs[3] = {0, 1, cbB};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int px = pxs[i];
      const int hy = px / BB_CW, hx = px - hy * BB_CW, gy = y0 - 1 + hy, gx = x0 - 1 + hx;
      const bool ok = px < BB_CHALO && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ch = cbs[i] * 32 + 8 * q + 4 * fh;
        const f32x4 sc = *(const f32x4*)(prm + ch), bi = *(const f32x4*)(prm + 64 + ch);
        bf16x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = acc1[i][4 * q + j] * sc[j] + bi[j];
          v = ok ? fmaxf(v, 0.f) : 0.f;
          o[j] = (h16_t)v;
        }
        *(bf16x4_t*)(c1 + bb_at(px, cbs[i] * 4 + q) + fh * 8) = o;
      }
    }
  }
  __syncthreads();

  // ---------------- phase 2: y = relu(conv2(c1) * s2 + b2 + x) ----------------
  f32x16 acc2[2];
  zero_acc(acc2);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int g = 9 + tap;
    const unsigned char* cur = wl + (g & 1) * BB_WBUF;
    unsigned char* nxt = wl + ((g + 1) & 1) * BB_WBUF;
    if (g + 3 < 18) {
#pragma unroll
      for (int i = 0; i < 2; ++i) tr[g % 3][i] = *(const bf16x8_t*)(a.w2 + t2co[i] * BB_TAPROW + (g + 3 - 9) * BB_C + t2slot * 8);
    }
    const int dy = tap / 3, dx = tap - dy * 3;
    const int h = (pr + dy) * BB_CW + pc + dx;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int slot = ks * 2 + fh;
      const bf16x8_t xf = bb_frag(c1, bb_at(h, slot));
      const bf16x8_t wa = bb_frag(cur, bb_at(w0row, slot));
      const bf16x8_t wb = bb_frag(cur, bb_at(w1row, slot));
      acc2[0] = mfma_32x32x16(wa, xf, acc2[0]);
      acc2[1] = mfma_32x32x16(wb, xf, acc2[1]);
    }
    if (g + 1 < 18) {
#pragma unroll
      for (int i = 0; i < 2; ++i) *(bf16x8_t*)(nxt + bb_at(t2co[i], t2slot)) = tr[(g + 1) % 3][i];
    }
    __syncthreads();
  }

  // epilogue: the tap buffers are dead; wave w's 32 pixels x 128 B go through its own 4 KB patch so that y is written in full rows
  unsigned char* patch = wl + wave * 4096;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ch = cb * 32 + 8 * q + 4 * fh;
      const f32x4 sc = *(const f32x4*)(prm + 128 + ch), bi = *(const f32x4*)(prm + 192 + ch);
      bf16x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (h16_t)fmaxf(acc2[cb][4 * q + j] * sc[j] + bi[j] + (float)res[cb][q][j], 0.f);
      *(bf16x4_t*)(patch + bb_at(l31, cb * 4 + q) + fh * 8) = o;
    }
  __syncthreads();
  h16_t* yout = a.y + (size_t)n * a.H * a.W * BB_C;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int piece = i * 64 + lane, prow = piece >> 3, slot = piece & 7;
    const int pp = wave * 32 + prow, gy = y0 + (pp >> 4), gx = x0 + (pp & 15);
    const bf16x8_t o = bb_frag(patch, bb_at(prow, slot));
    if (gy < a.H && gx < a.W) *(bf16x8_t*)(yout + ((size_t)gy * a.W + gx) * BB_C + slot * 8) = o;
  }
}

extern "C" {

// One frozen identity BasicBlock of 64 channels (both convs 3x3 stride 1 pad 1), 16-bit NHWC (R-18 / R-34 res2).
// x, y: [N, H, W, 64] of this library's 16-bit type (y != x); w1, w2: [64][3][3][64] 16-bit; s* / b*: fp32 scale and shift of the folded
// FrozenBN per output channel.  y = h16(relu(conv2(h16(relu(conv1(x) s1 + b1))) s2 + b2 + x)).
int utv2_basicblock_fwd_bf16(const void* x, void* y, const void* w1, const void* w2, const float* s1, const float* b1, const float* s2,
                             const float* b2, int N, int H, int W, int C, hipStream_t stream) {
  if (!x || !y || x == y || !w1 || !w2 || !s1 || !b1 || !s2 || !b2 || N < 1 || H < 1 || W < 1) return UTV2_EARG;
  if (C != BB_C) return UTV2_EARG;
  if ((long long)H * W * BB_C > 0x7fffffffll) return UTV2_EARG;
  BbArgs a;
  a.x = (const h16_t*)x; a.y = (h16_t*)y; a.w1 = (const h16_t*)w1; a.w2 = (const h16_t*)w2;
  a.s1 = s1; a.b1 = b1; a.s2 = s2; a.b2 = b2;
  a.N = N; a.H = H; a.W = W;
  a.tiles_x = cdiv(W, BB_TW); a.tiles_y = cdiv(H, BB_TH);
  const long long nt = (long long)N * a.tiles_x * a.tiles_y;
  if (nt > 0x7fffffff) return UTV2_EARG;
  a.ntiles = (int)nt;
  hipLaunchKernelGGL(basicblock_fused, dim3((unsigned)a.ntiles), dim3(256), BB_LDS, stream, a);
  return utv2_launch_status();
}

// 1 when utv2_basicblock_fwd_bf16 takes this block shape (C channels in and out, conv1's stride, with / without a shortcut conv)
int utv2_basicblock_supported(int C, int stride, int has_shortcut) { return C == BB_C && stride == 1 && !has_shortcut; }

}  // extern "C"
