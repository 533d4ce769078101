// GroupNorm(G groups) + optional ReLU over ROIS: x is dense [R][HW][C] (the NHWC RoIAlign output and the box head's conv outputs on
// it, Detectron2 FastRCNNConvFCHead with NORM "GN"), statistics per (ROI, group).  A ROI is small - POOLER_RESOLUTION^2 = 49 rows of
// 256 channels, 25 KB in 16 bit - and there are thousands of them, the opposite of the tower segments utv2_groupnorm_relu_seg_* is
// built for (at most 160 segments of thousands of rows, three launches each way).  Here ONE workgroup owns a ROI at a time
// (grid-stride over R) and makes a single pass over the tensor in each direction.
//
// Tile mapping (256 threads): thread t owns channel quad c4 = t % (C / 4) and row lane rl = t / (C / 4) of RL = 256 / (C / 4) row
// lanes (threads past RL * C / 4 idle: C / 4 need not divide 256); it takes rows rl, rl + RL, ... of the ROI.  A wave's load is whole
// rows (C = 256: one 1 KB / 512 B row per wave instruction).  A thread's channel quad lies in one group (cpg % 4 == 0), so its gamma,
// beta, mean and rstd are loop constants.  With at most GN_ROI_NR rows per thread (49 x 256: 13) the ROI stays in registers between
// the statistics and the apply step; a larger ROI (up to 196 x 1024) is read again, from the L2 it has just been pulled through.
//
// Group sums: per-thread partials go through LDS and every thread of a group adds the group's partials in the same fixed order
// (row lane major) - the lanes of one group sit in several waves, so a wave shuffle alone cannot finish them, and the order is
// independent of the launch.  No atomics anywhere: dgamma / dbeta are bit-identical from run to run.
#include <stdint.h>
#include "common.h"

#define GN_ROI_NR 13        // rows a thread keeps in registers: ceil(49 / 4), the 7 x 7 ROI of 256 channels
#define GN_ROI_MAX_HW 196   // 14 x 14
#define GN_ROI_MAX_C 1024
#define GN_ROI_GRID 1024    // workgroups of the ROI kernels: four per CU; also the row count of the backward's partial sums

// f(i, row) for the thread's rows row = rl + i * RL < HW.  NR > 0: i is a compile-time index into the thread's register tile (at most NR
// rows: the launch site guarantees it); NR == 0: a plain loop
template <int NR, typename F>
__device__ __forceinline__ void gn_roi_rows(int rl, int RL, int HW, F f) {
  if constexpr (NR > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i)
      if (rl + i * RL < HW) f(i, rl + i * RL);
  } else {
    for (int i = 0, row = rl; row < HW; ++i, row += RL) f(i, row);
  }
}

// The forward's value before the ReLU; its sign is the mask the backward recomputes from x, so both use this one expression (the
// library is built with -ffp-contract=off: the same roundings wherever it is inlined).
__device__ __forceinline__ float gn_roi_affine(float x, float m, float r, float ga, float be) { return (x - m) * r * ga + be; }

// Compensated (Kahan) running sum.  Every in-kernel sum of values or products goes through it: one large element in a group (a ROI
// that is zero but for one pixel) otherwise swamps the small terms added after it - a plain fp32 chain lost 1.5e-6 of such a
// variance (relative), and with it the forward's error bound.  (No fast-math: the compiler keeps the compensation.)
struct GnRoiSum {
  float s = 0.f, c = 0.f;
  __device__ __forceinline__ void add(float v) {
    const float y = v - c, t = s + y;
    c = (t - s) - y;
    s = t;
  }
};

// Sum over the group of thread (c4, any row lane) of the per-thread partials in red[t] (t = rl * C4 + c4), row lane major, then quad
// order: the same order in every thread of the group.
__device__ __forceinline__ float gn_roi_group_sum(const float* red, int c4, int C4, int cpg4, int RL) {
  const int q0 = c4 / cpg4 * cpg4;
  GnRoiSum s;
  for (int k = 0; k < RL; ++k)
    for (int j = 0; j < cpg4; ++j) s.add(red[k * C4 + q0 + j]);
  return s.s;
}

// Statistics in two steps from the tile: the mean m0, then the sums of (x - m0) and (x - m0)^2 - the centred form (the sum x^2 form
// cancels on inputs far from zero: mean 100, std 1 loses four digits of the variance in fp32).  The first-moment residual corrects
// what the fp32 sum of m0 lost: mean = m0 + d, var = sum (x - m0)^2 / n - d^2 (biased), rstd = 1 / sqrt(var + eps).
template <typename T, int NR>
__global__ __launch_bounds__(256) void gn_roi_fwd(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                T* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int R, int HW, int C,
                                                int G, float eps, int relu) {
  __shared__ float red[3][256];
  const int C4 = C >> 2, cpg4 = (C / G) >> 2, RL = 256 / C4;
  const int t = threadIdx.x, c4 = t % C4, rl = t / C4;
  const bool on = rl < RL;
  const int g = c4 / cpg4;
  const float inv_n = 1.f / (float)(HW * (C / G));
  f32x4 ga = {0.f, 0.f, 0.f, 0.f}, be = {0.f, 0.f, 0.f, 0.f};
  if (on) { ga = ((const f32x4*)gamma)[c4]; be = ((const f32x4*)beta)[c4]; }
  for (int roi = blockIdx.x; roi < R; roi += gridDim.x) {
    const size_t base = (size_t)roi * HW * C4 + c4;
    f32x4 v[NR > 0 ? NR : 1];
    auto at = [&](int i, int row) -> f32x4 {   // row `row` = the thread's i-th: from the register tile, or from memory again
      if constexpr (NR > 0) return v[i];
      else return ld4(x, base + (size_t)row * C4);
    };
    GnRoiSum s;
    if (on) {
      if constexpr (NR > 0) gn_roi_rows<NR>(rl, RL, HW, [&](int i, int row) { v[i] = ld4(x, base + (size_t)row * C4); });
      gn_roi_rows<NR>(rl, RL, HW, [&](int i, int row) {
        const f32x4 a = at(i, row);
        s.add((a[0] + a[1]) + (a[2] + a[3]));
      });
    }
    red[0][t] = s.s;
    __syncthreads();
    float m = 0.f, r = 0.f;
    GnRoiSum d, q;
    if (on) {
      m = gn_roi_group_sum(red[0], c4, C4, cpg4, RL) * inv_n;
      gn_roi_rows<NR>(rl, RL, HW, [&](int i, int row) {
        const f32x4 a = at(i, row);
        const float e0 = a[0] - m, e1 = a[1] - m, e2 = a[2] - m, e3 = a[3] - m;
        d.add((e0 + e1) + (e2 + e3));
        q.add((e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3));
      });
    }
    red[1][t] = d.s;
    red[2][t] = q.s;
    __syncthreads();   // (the next ROI writes red[0] only after this barrier, red[1..2] only after its own first one)
    if (on) {
      const float dm = gn_roi_group_sum(red[1], c4, C4, cpg4, RL) * inv_n;
      float var = gn_roi_group_sum(red[2], c4, C4, cpg4, RL) * inv_n - dm * dm;
      if (var < 0.f) var = 0.f;
      m += dm;
      r = 1.f / sqrtf(var + eps);
      if (rl == 0 && c4 % cpg4 == 0) {
        mean[(size_t)roi * G + g] = m;
        rstd[(size_t)roi * G + g] = r;
      }
      gn_roi_rows<NR>(rl, RL, HW, [&](int i, int row) {
        const f32x4 a = at(i, row);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = gn_roi_affine(a[e], m, r, ga[e], be[e]);
          o[e] = relu ? fmaxf(p, 0.f) : p;
        }
        st4(y, base + (size_t)row * C4, o);
      });
    }
  }
}

// Backward.  g = dy where the forward's ReLU passed (the sign of gn_roi_affine, recomputed from x), xh = (x - mean) * rstd.  Per channel
// A = sum_rows g * xh, B = sum_rows g (this ROI's share of dgamma / dbeta); per group s1 = sum_c gamma * A, s2 = sum_c gamma * B;
// dx = rstd * (gamma * g - (xh * s1 + s2) / n).  The row lanes' A / B meet in LDS, row lane 0 adds them in lane order, keeps the
// running column sums of the workgroup's ROIs (taken in ascending order) and leaves them in part[blockIdx][2][C] at the end.
template <typename T, int NR>
__global__ __launch_bounds__(256) void gn_roi_bwd(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, T* __restrict__ dx, float* __restrict__ part, int R,
                                                int HW, int C, int G, int relu) {
  __shared__ float red[2][256 * 4];            // [A | B][thread][e]
  __shared__ float col[2][GN_ROI_MAX_C];       // gamma * {A, B} of the ROI per channel
  const int C4 = C >> 2, cpg = C / G, cpg4 = cpg >> 2, RL = 256 / C4;
  const int t = threadIdx.x, c4 = t % C4, rl = t / C4;
  const bool on = rl < RL;
  const int g = c4 / cpg4;
  const float inv_n = 1.f / (float)(HW * cpg);
  f32x4 ga = {0.f, 0.f, 0.f, 0.f}, be = {0.f, 0.f, 0.f, 0.f};
  if (on) { ga = ((const f32x4*)gamma)[c4]; be = ((const f32x4*)beta)[c4]; }
  f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = {0.f, 0.f, 0.f, 0.f};   // row lane 0: column sums over this workgroup's ROIs
  for (int roi = blockIdx.x; roi < R; roi += gridDim.x) {
    const size_t base = (size_t)roi * HW * C4 + c4;
    f32x4 vg[NR > 0 ? NR : 1], vh[NR > 0 ? NR : 1];   // g and xh of the thread's rows
    float m = 0.f, r = 0.f;
    // (g, xh) of one row from memory
    auto load = [&](int row, f32x4& gg, f32x4& xh) {
      gg = ld4(dy, base + (size_t)row * C4);
      const f32x4 xx = ld4(x, base + (size_t)row * C4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (relu) gg[e] = gn_roi_affine(xx[e], m, r, ga[e], be[e]) > 0.f ? gg[e] : 0.f;
        xh[e] = (xx[e] - m) * r;
      }
    };
    GnRoiSum A[4], B[4];
    if (on) {
      m = mean[(size_t)roi * G + g];
      r = rstd[(size_t)roi * G + g];
      gn_roi_rows<NR>(rl, RL, HW, [&](int i, int row) {
        f32x4 gg, xh;
        load(row, gg, xh);
        if constexpr (NR > 0) { vg[i] = gg; vh[i] = xh; }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          A[e].add(gg[e] * xh[e]);
          B[e].add(gg[e]);
        }
      });
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[0][t * 4 + e] = A[e].s;
      red[1][t * 4 + e] = B[e].s;
    }
    __syncthreads();
    if (on && rl == 0) {
      for (int k = 1; k < RL; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          A[e].add(red[0][(k * C4 + c4) * 4 + e]);
          B[e].add(red[1][(k * C4 + c4) * 4 + e]);
        }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        accA[e] += A[e].s;
        accB[e] += B[e].s;
        col[0][c4 * 4 + e] = ga[e] * A[e].s;
        col[1][c4 * 4 + e] = ga[e] * B[e].s;
      }
    }
    __syncthreads();   // (the next ROI writes red only after this barrier, col only after its own first one)
    if (on) {
      GnRoiSum t1, t2;
      for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        t1.add(col[0][c]);
        t2.add(col[1][c]);
      }
      const float s1 = t1.s * inv_n, s2 = t2.s * inv_n;
      gn_roi_rows<NR>(rl, RL, HW, [&](int i, int row) {
        f32x4 gg, xh;
        if constexpr (NR > 0) { gg = vg[i]; xh = vh[i]; }
        else load(row, gg, xh);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = r * (ga[e] * gg[e] - (xh[e] * s1 + s2));
        st4(dx, base + (size_t)row * C4, o);
      });
    }
  }
  if (on && rl == 0) {
    float* out = part + (size_t)blockIdx.x * 2 * C;
    ((f32x4*)out)[c4] = accA;
    ((f32x4*)(out + C))[c4] = accB;
  }
}

// dgamma[c] += sum_b part[b][0][c], dbeta[c] += sum_b part[b][1][c] over the nb workgroups of gn_roi_bwd.  One block per 32 channels:
// thread (q = t % 16, lane = t / 16) walks every 16th row of one quad of the A (q < 8) or the B plane with four loads in flight; the
// 16 lanes are added in lane order.
__global__ __launch_bounds__(256) void gn_roi_param_reduce(const float* __restrict__ part, float* __restrict__ dgamma,
                                                         float* __restrict__ dbeta, int nb, int C) {
  __shared__ f32x4 red[16][16];
  const int q = threadIdx.x & 15, ln = threadIdx.x >> 4;
  const int plane = q >> 3, c = blockIdx.x * 32 + (q & 7) * 4;
  f32x4 a[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    for (int b = ln; b < nb; b += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (b + 16 * u < nb) a[u] += *(const f32x4*)(part + ((size_t)(b + 16 * u) * 2 + plane) * C + c);
    }
  }
  red[ln][q] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (ln == 0 && c < C) {
    f32x4 s = red[0][q];
    for (int k = 1; k < 16; ++k) s += red[k][q];
    f32x4* dst = (f32x4*)((plane ? dbeta : dgamma) + c);
    *dst += s;
  }
}

static inline bool gn_roi_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// (the channel rules of gn_check without its divisibility of 256: idle threads cover a C / 4 that does not divide the workgroup)
static int gn_roi_check(int R, int HW, int C, int G, int dtype) {
  return !(R < 0 || HW < 1 || HW > GN_ROI_MAX_HW || G < 1 || C < 4 || (C & 3) || C > GN_ROI_MAX_C || (C % G) || ((C / G) & 3) ||
           (dtype != UTV2_F32 && dtype != UTV2_BF16));
}

static inline int gn_roi_grid(int R) { return R < GN_ROI_GRID ? R : GN_ROI_GRID; }

// the ROI stays in registers when every thread has at most GN_ROI_NR rows of it
static inline bool gn_roi_resident(int HW, int C) {
  const int RL = 256 / (C >> 2);
  return (HW + RL - 1) / RL <= GN_ROI_NR;
}

extern "C" {

int64_t utv2_groupnorm_roi_workspace_floats(int R, int C) { return (int64_t)(R < 1 ? 1 : gn_roi_grid(R)) * 2 * C; }

// x, y: [R][HW][C] of `dtype`; mean, rstd: fp32 [R][G] (saved for the backward).  Statistics and arithmetic are fp32.
int utv2_groupnorm_roi_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int R, int HW, int C,
                           int G, float eps, int relu, int dtype, hipStream_t stream) {
  if (!gn_roi_check(R, HW, C, G, dtype) || !gamma || !beta || !gn_roi_aligned(gamma) || !gn_roi_aligned(beta)) return UTV2_EARG;
  if (R == 0) return UTV2_OK;
  if (!x || !y || !mean || !rstd || !gn_roi_aligned(x) || !gn_roi_aligned(y)) return UTV2_EARG;
  with_type(dtype, [&](auto tag) {
    using T = TAG_T(tag);
    if (gn_roi_resident(HW, C))
      hipLaunchKernelGGL((gn_roi_fwd<T, GN_ROI_NR>), dim3(gn_roi_grid(R)), dim3(256), 0, stream, (const T*)x, gamma, beta, (T*)y, mean, rstd,
                         R, HW, C, G, eps, relu);
    else
      hipLaunchKernelGGL((gn_roi_fwd<T, 0>), dim3(gn_roi_grid(R)), dim3(256), 0, stream, (const T*)x, gamma, beta, (T*)y, mean, rstd, R, HW,
                         C, G, eps, relu);
  });
  return utv2_launch_status();
}

// dx written (`dtype`, like dy and x); dgamma / dbeta (fp32 [C]) accumulated (+=).  The ReLU mask is recomputed from x, mean, rstd,
// gamma and beta with the forward's expression.  ws: utv2_groupnorm_roi_workspace_floats(R, C) floats.
int utv2_groupnorm_roi_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           void* dx, float* dgamma, float* dbeta, float* ws, int R, int HW, int C, int G, int relu, int dtype,
                           hipStream_t stream) {
  if (!gn_roi_check(R, HW, C, G, dtype) || !gamma || !beta || !dgamma || !dbeta || !gn_roi_aligned(gamma) || !gn_roi_aligned(beta) ||
      !gn_roi_aligned(dgamma) || !gn_roi_aligned(dbeta))
    return UTV2_EARG;
  if (R == 0) return UTV2_OK;
  if (!dy || !x || !dx || !mean || !rstd || !ws || !gn_roi_aligned(dy) || !gn_roi_aligned(x) || !gn_roi_aligned(dx) || !gn_roi_aligned(ws))
    return UTV2_EARG;
  const int nb = gn_roi_grid(R);
  with_type(dtype, [&](auto tag) {
    using T = TAG_T(tag);
    if (gn_roi_resident(HW, C))
      hipLaunchKernelGGL((gn_roi_bwd<T, GN_ROI_NR>), dim3(nb), dim3(256), 0, stream, (const T*)dy, (const T*)x, mean, rstd, gamma, beta,
                         (T*)dx, ws, R, HW, C, G, relu);
    else
      hipLaunchKernelGGL((gn_roi_bwd<T, 0>), dim3(nb), dim3(256), 0, stream, (const T*)dy, (const T*)x, mean, rstd, gamma, beta, (T*)dx, ws,
                         R, HW, C, G, relu);
  });
  hipLaunchKernelGGL(gn_roi_param_reduce, dim3(cdiv(C, 32)), dim3(256), 0, stream, (const float*)ws, dgamma, dbeta, nb, C);
  return utv2_launch_status();
}

}  // extern "C"
