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
#include <initializer_list>
#include <type_traits>
#include "common.h"

#define GN_ROI_NR 13        // rows a thread keeps in registers: ceil(49 / 4), the 7 x 7 ROI of 256 channels
#define GN_ROI_MAX_HW 196   // 14 x 14
#define GN_ROI_MAX_C 1024
#define GN_ROI_GRID 1024    // workgroups of the ROI kernels: four per CU; also the row count of the backward's partial sums

// A thread in the tile mapping above: channel quad c4 (of C4), row lane rl (of RL; `on`: not an idle thread past RL * C4), the group g
// of its quad (cpg4 quads per group), 1 / (elements of a group), the quad's gamma and beta (zero in an idle thread).
struct GnRoiLane { int C4, cpg4, RL, t, c4, rl, g; bool on; float inv_n; f32x4 ga, be; };
__device__ __forceinline__ GnRoiLane gn_roi_lane(const float* __restrict__ gamma, const float* __restrict__ beta, int HW, int C, int G) {
  GnRoiLane L;
  L.C4 = C >> 2, L.cpg4 = (C / G) >> 2, L.RL = 256 / L.C4, L.t = threadIdx.x, L.c4 = L.t % L.C4, L.rl = L.t / L.C4;
  L.on = L.rl < L.RL, L.g = L.c4 / L.cpg4, L.inv_n = 1.f / (float)(HW * (C / G));
  L.ga = L.be = f32x4{0.f, 0.f, 0.f, 0.f};
  if (L.on) { L.ga = ((const f32x4*)gamma)[L.c4]; L.be = ((const f32x4*)beta)[L.c4]; }
  return L;
}

// f(i, row) for the thread's rows row = rl + i * RL < HW.  NR > 0: i is a compile-time index into the thread's register tile (at most NR
// rows: the launch site guarantees it); NR == 0: a plain loop
template <int NR, typename F>
__device__ __forceinline__ void gn_roi_rows(const GnRoiLane& L, int HW, F f) {
  if constexpr (NR > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i)
      if (L.rl + i * L.RL < HW) f(i, L.rl + i * L.RL);
  } else {
    for (int i = 0, row = L.rl; row < HW; ++i, row += L.RL) f(i, row);
  }
}

// The normalised value, and the forward's value before the ReLU; the sign of the latter is the mask the backward recomputes from x,
// so both kernels use these two expressions (the library is built with -ffp-contract=off: the same roundings wherever they are inlined).
__device__ __forceinline__ float gn_roi_xhat(float x, float m, float r) { return (x - m) * r; }
__device__ __forceinline__ float gn_roi_affine(float x, float m, float r, float ga, float be) { return gn_roi_xhat(x, m, r) * ga + be; }

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
__device__ __forceinline__ float gn_roi_group_sum(const float* red, const GnRoiLane& L) {
  const int q0 = L.c4 / L.cpg4 * L.cpg4;
  GnRoiSum s;
  for (int k = 0; k < L.RL; ++k)
    for (int j = 0; j < L.cpg4; ++j) s.add(red[k * L.C4 + q0 + j]);
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
  const GnRoiLane L = gn_roi_lane(gamma, beta, HW, C, G);
  for (int roi = blockIdx.x; roi < R; roi += gridDim.x) {
    const size_t base = (size_t)roi * HW * L.C4 + L.c4;
    f32x4 v[NR > 0 ? NR : 1];
    auto at = [&](int i, int row) -> f32x4 {   // row `row` = the thread's i-th: from the register tile, or from memory again
      if constexpr (NR > 0) return v[i];
      else return ld4(x, base + (size_t)row * L.C4);
    };
    GnRoiSum s;
    if (L.on) {
      if constexpr (NR > 0) gn_roi_rows<NR>(L, HW, [&](int i, int row) { v[i] = ld4(x, base + (size_t)row * L.C4); });
      gn_roi_rows<NR>(L, HW, [&](int i, int row) {
        const f32x4 a = at(i, row);
        s.add((a[0] + a[1]) + (a[2] + a[3]));
      });
    }
    red[0][L.t] = s.s;
    __syncthreads();
    float m = 0.f, r = 0.f;
    GnRoiSum d, q;
    if (L.on) {
      m = gn_roi_group_sum(red[0], L) * L.inv_n;
      gn_roi_rows<NR>(L, HW, [&](int i, int row) {
        const f32x4 a = at(i, row);
        const float e0 = a[0] - m, e1 = a[1] - m, e2 = a[2] - m, e3 = a[3] - m;
        d.add((e0 + e1) + (e2 + e3));
        q.add((e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3));
      });
    }
    red[1][L.t] = d.s;
    red[2][L.t] = q.s;
    __syncthreads();   // (the next ROI writes red[0] only after this barrier, red[1..2] only after its own first one)
    if (L.on) {
      const float dm = gn_roi_group_sum(red[1], L) * L.inv_n;
      float var = gn_roi_group_sum(red[2], L) * L.inv_n - dm * dm;
      if (var < 0.f) var = 0.f;
      m += dm;
      r = 1.f / sqrtf(var + eps);
      if (L.rl == 0 && L.c4 % L.cpg4 == 0) {
        mean[(size_t)roi * G + L.g] = m;
        rstd[(size_t)roi * G + L.g] = r;
      }
      gn_roi_rows<NR>(L, HW, [&](int i, int row) {
        const f32x4 a = at(i, row);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = gn_roi_affine(a[e], m, r, L.ga[e], L.be[e]);
          o[e] = relu ? fmaxf(p, 0.f) : p;
        }
        st4(y, base + (size_t)row * L.C4, o);
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
  const GnRoiLane L = gn_roi_lane(gamma, beta, HW, C, G);
  f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = {0.f, 0.f, 0.f, 0.f};   // row lane 0: column sums over this workgroup's ROIs
  for (int roi = blockIdx.x; roi < R; roi += gridDim.x) {
    const size_t base = (size_t)roi * HW * L.C4 + L.c4;
    f32x4 vg[NR > 0 ? NR : 1], vh[NR > 0 ? NR : 1];   // g and xh of the thread's rows
    float m = 0.f, r = 0.f;
    // (g, xh) of one row from memory
    auto load = [&](int row, f32x4& gg, f32x4& xh) {
      gg = ld4(dy, base + (size_t)row * L.C4);
      const f32x4 xx = ld4(x, base + (size_t)row * L.C4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (relu) gg[e] = gn_roi_affine(xx[e], m, r, L.ga[e], L.be[e]) > 0.f ? gg[e] : 0.f;
        xh[e] = gn_roi_xhat(xx[e], m, r);
      }
    };
    GnRoiSum A[4], B[4];
    if (L.on) {
      m = mean[(size_t)roi * G + L.g];
      r = rstd[(size_t)roi * G + L.g];
      gn_roi_rows<NR>(L, HW, [&](int i, int row) {
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
      red[0][L.t * 4 + e] = A[e].s;
      red[1][L.t * 4 + e] = B[e].s;
    }
    __syncthreads();
    if (L.on && L.rl == 0) {
      for (int k = 1; k < L.RL; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          A[e].add(red[0][(k * L.C4 + L.c4) * 4 + e]);
          B[e].add(red[1][(k * L.C4 + L.c4) * 4 + e]);
        }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        accA[e] += A[e].s;
        accB[e] += B[e].s;
        col[0][L.c4 * 4 + e] = L.ga[e] * A[e].s;
        col[1][L.c4 * 4 + e] = L.ga[e] * B[e].s;
      }
    }
    __syncthreads();   // (the next ROI writes red only after this barrier, col only after its own first one)
    if (L.on) {
      GnRoiSum t1, t2;
      for (int c = L.g * L.cpg4 * 4; c < (L.g + 1) * L.cpg4 * 4; ++c) {
        t1.add(col[0][c]);
        t2.add(col[1][c]);
      }
      const float s1 = t1.s * L.inv_n, s2 = t2.s * L.inv_n;
      gn_roi_rows<NR>(L, HW, [&](int i, int row) {
        f32x4 gg, xh;
        if constexpr (NR > 0) { gg = vg[i]; xh = vh[i]; }
        else load(row, gg, xh);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = r * (L.ga[e] * gg[e] - (xh[e] * s1 + s2));
        st4(dx, base + (size_t)row * L.C4, o);
      });
    }
  }
  if (L.on && L.rl == 0) {
    float* out = part + (size_t)blockIdx.x * 2 * C;
    ((f32x4*)out)[L.c4] = accA;
    ((f32x4*)(out + C))[L.c4] = accB;
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

// The argument test of both entries, in two stages around the empty batch: the shape rules (the channel rules of gn_check without its
// divisibility of 256: idle threads cover a C / 4 that does not divide the workgroup) and the parameter pointers; R == 0 is then OK
// whatever the tensor pointers are; else the tensors (quads) and the statistics (mean, rstd: non-null).  -> true: launch; false: return rc
static bool gn_roi_args(int& rc, int R, int HW, int C, int G, int dtype, std::initializer_list<const void*> params,
                        std::initializer_list<const void*> tensors, const float* mean, const float* rstd) {
  auto quads = [](std::initializer_list<const void*> ps) {   // every pointer non-null and 16-byte aligned (read or written as quads)
    for (const void* p : ps) if (!p || ((uintptr_t)p & 15)) return false;
    return true;
  };
  rc = UTV2_EARG;
  if (R < 0 || HW < 1 || HW > GN_ROI_MAX_HW || G < 1 || C < 4 || (C & 3) || C > GN_ROI_MAX_C || (C % G) || ((C / G) & 3) ||
      (dtype != UTV2_F32 && dtype != UTV2_BF16) || !quads(params))
    return false;
  if (R == 0) rc = UTV2_OK;
  return R > 0 && quads(tensors) && mean && rstd;
}

static inline int gn_roi_grid(int R) { return R < GN_ROI_GRID ? R : GN_ROI_GRID; }
// the ROI stays in registers when every thread has at most GN_ROI_NR rows of it
static inline bool gn_roi_resident(int HW, int C) {
  const int RL = 256 / (C >> 2);
  return (HW + RL - 1) / RL <= GN_ROI_NR;
}

// f(TypeTag<T>, integral_constant NR): T from `dtype`, NR = GN_ROI_NR for a resident ROI, 0 for a re-read one - the four instantiations
template <typename F>
static void gn_roi_launch(int dtype, int HW, int C, F&& f) {
  with_type(dtype, [&](auto tag) {
    if (gn_roi_resident(HW, C)) f(tag, std::integral_constant<int, GN_ROI_NR>{});
    else f(tag, std::integral_constant<int, 0>{});
  });
}

extern "C" {

int64_t utv2_groupnorm_roi_workspace_floats(int R, int C) { return (int64_t)(R < 1 ? 1 : gn_roi_grid(R)) * 2 * C; }

// x, y: [R][HW][C] of `dtype`; mean, rstd: fp32 [R][G] (saved for the backward).  Statistics and arithmetic are fp32.
int utv2_groupnorm_roi_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int R, int HW, int C,
                           int G, float eps, int relu, int dtype, hipStream_t stream) {
  int rc;
  if (!gn_roi_args(rc, R, HW, C, G, dtype, {gamma, beta}, {x, y}, mean, rstd)) return rc;
  gn_roi_launch(dtype, HW, C, [&](auto tag, auto nr) {
    using T = TAG_T(tag);
    hipLaunchKernelGGL((gn_roi_fwd<T, decltype(nr)::value>), dim3(gn_roi_grid(R)), dim3(256), 0, stream, (const T*)x, gamma, beta, (T*)y, mean,
                       rstd, R, HW, C, G, eps, relu);
  });
  return utv2_launch_status();
}

// dx written (`dtype`, like dy and x); dgamma / dbeta (fp32 [C]) accumulated (+=).  The ReLU mask is recomputed from x, mean, rstd,
// gamma and beta with the forward's expression.  ws: utv2_groupnorm_roi_workspace_floats(R, C) floats.
int utv2_groupnorm_roi_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           void* dx, float* dgamma, float* dbeta, float* ws, int R, int HW, int C, int G, int relu, int dtype,
                           hipStream_t stream) {
  int rc;
  if (!gn_roi_args(rc, R, HW, C, G, dtype, {gamma, beta, dgamma, dbeta}, {dy, x, dx, ws}, mean, rstd)) return rc;
  const int nb = gn_roi_grid(R);
  gn_roi_launch(dtype, HW, C, [&](auto tag, auto nr) {
    using T = TAG_T(tag);
    hipLaunchKernelGGL((gn_roi_bwd<T, decltype(nr)::value>), dim3(nb), dim3(256), 0, stream, (const T*)dy, (const T*)x, mean, rstd, gamma, beta,
                       (T*)dx, ws, R, HW, C, G, relu);
  });
  hipLaunchKernelGGL(gn_roi_param_reduce, dim3(cdiv(C, 32)), dim3(256), 0, stream, (const float*)ws, dgamma, dbeta, nb, C);
  return utv2_launch_status();
}

}  // extern "C"
