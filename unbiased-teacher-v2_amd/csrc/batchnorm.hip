// BatchNorm2d + ReLU of the FCOS towers (MODEL.FCOS.NORM "BN" / "SyncBN", reference fcos/fcos.py:262-281) on the level-first [P, C]
// activation.  A STATISTIC SET is a contiguous row range: the rows of one FPN level that belong to one forward call of the reference
// (its BatchNorm2d of that level sees exactly those rows).  Sets come from the canvas geometry only: the host lists them (at most
// UTV2_BN_MAX_SETS), they travel as a kernel argument, nothing here depends on device data.
//
// Every reduction is two-stage with a fixed order and no atomics (bit-reproducible):
//   stage 1  one block per CHUNK of 64 rows of one set x 256 channels: four row lanes per channel, each summing its rows in order,
//            combined in lane order -> partial[chunk][2][C], fp64
//   stage 2  one block per (set, 64 channels): eight slices walk the set's chunks with stride 8, combined in slice order -> [S][2][C]
// The two moments are carried in fp64 from the first add on (the square of a 24-bit value is exact in fp64), so var = E[x^2] - mean^2
// is taken in fp64: a channel of mean 300 and spread 0.05 keeps 8 significant digits of its variance.  No fp32 E[x^2] - mean^2.
#include <stdint.h>
#include <initializer_list>
#include "common.h"
#include "bn_sets.h"   // BnSets, bn_fill_sets, bn_gate, BN_CHUNK (rows per stage-1 block)

#define BN_COLS 256      // channels per stage-1 / apply block: 64 quads
#define BN_LANES 4       // row lanes of a 256-thread block
#define BN_SLICES 8      // stage-2 slices

// chunk -> (set, first row, rows of the chunk)
__device__ __forceinline__ void bn_chunk(const BnSets& st, int chunk, int& s, int& r0, int& nr) {
  s = 0;
  while (s + 1 < st.n && chunk >= st.chunk0[s + 1]) ++s;
  const int off = (chunk - st.chunk0[s]) * BN_CHUNK;
  r0 = st.row0[s] + off;
  nr = min(BN_CHUNK, st.rows[s] - off);
}

// A thread's tile in the five chunk x 256-channel kernels: channel quad q (channels c .. c + 3), row lane rl, which takes rows rl,
// rl + BN_LANES, ... < nr of the chunk that starts at row r0 of set s.  c may lie past C in the last column block.
struct BnTile {
  int q, rl, c, s, r0, nr;
  __device__ __forceinline__ size_t quad(int r, int C) const { return ((size_t)(r0 + r) * C + c) >> 2; }   // ld4 / st4 index of row r
};
__device__ __forceinline__ BnTile bn_tile(const BnSets& st) {
  BnTile t;
  t.q = threadIdx.x & 63, t.rl = threadIdx.x >> 6, t.c = blockIdx.y * BN_COLS + t.q * 4;
  bn_chunk(st, blockIdx.x, t.s, t.r0, t.nr);
  return t;
}

// the quad's four fp64 per-channel coefficients from row `row` of an [S][C] (row = s) or [S][2][C] (row = 2 s + k) table
__device__ __forceinline__ void bn_coef4(const double* __restrict__ tab, size_t row, int C, int c, double (&out)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) out[e] = tab[row * C + c + e];
}
// the backward's g = dy * [y > 0] and xhat = (x - mean) * rstd in fp64 (the mask in float, then widened: the value of y > 0 ? (double)dy : 0.0)
__device__ __forceinline__ void bn_gx(float dy, float y, float x, double mu, double rs, double& g, double& xh) {
  g = (double)(y > 0.f ? dy : 0.f), xh = ((double)x - mu) * rs;
}
// torch's ReLU: a NaN stays a NaN (fmax would make it 0)
__device__ __forceinline__ double bn_relu(double t) { return t > 0.0 ? t : (t != t ? t : 0.0); }

// lane-ordered sum of the four row lanes' fp64 pairs; result in lane 0 of each quad column.  red: [2][BN_LANES][BN_COLS] doubles
__device__ __forceinline__ void bn_combine_lanes(double (&a)[4], double (&b)[4], double* red, int q, int rl) {
#pragma unroll
  for (int e = 0; e < 4; ++e) red[(0 * BN_LANES + rl) * BN_COLS + q * 4 + e] = a[e], red[(1 * BN_LANES + rl) * BN_COLS + q * 4 + e] = b[e];
  __syncthreads();
  if (rl == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double sa = red[q * 4 + e], sb = red[(BN_LANES)*BN_COLS + q * 4 + e];
#pragma unroll
      for (int l = 1; l < BN_LANES; ++l) sa += red[(0 * BN_LANES + l) * BN_COLS + q * 4 + e], sb += red[(1 * BN_LANES + l) * BN_COLS + q * 4 + e];
      a[e] = sa, b[e] = sb;
    }
  }
}

// stage-1 epilogue: the row lanes combined, then partial[chunk][0][c .. c + 3] = a, [1][...] = b
__device__ __forceinline__ void bn_store_partial(double (&a)[4], double (&b)[4], double* red, const BnTile& t, int C, double* __restrict__ partial) {
  bn_combine_lanes(a, b, red, t.q, t.rl);
  if (t.rl == 0 && t.c < C) {
    double* p = partial + (size_t)blockIdx.x * 2 * C + t.c;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = a[e], p[C + e] = b[e];
  }
}

// Stage 1 of both directions: row(i4, a, b) adds row quad i4's terms into the lane's two fp64 sums, rows in order; then the epilogue.
template <typename Row>
__device__ __forceinline__ void bn_stage1(const BnTile& t, int C, double* __restrict__ partial, Row row) {
  __shared__ double red[2 * BN_LANES * BN_COLS];
  double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
  if (t.c < C)
    for (int r = t.rl; r < t.nr; r += BN_LANES) row(t.quad(r, C), a, b);
  bn_store_partial(a, b, red, t, C, partial);
}

// stage 1, forward: partial[chunk][0][c] = sum x, [1][c] = sum x^2 over the chunk's rows
template <typename T>
__global__ void __launch_bounds__(256) bn_stats_partial_kernel(const T* __restrict__ x, double* __restrict__ partial, BnSets st, int C) {
  bn_stage1(bn_tile(st), C, partial, [&](size_t i4, double (&a)[4], double (&b)[4]) {
    const f32x4 v = ld4(x, i4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (double)v[e];
      a[e] += d, b[e] += d * d;
    }
  });
}

// stage 2 (both directions): out[s][k][c] = (sum over the set's chunks of partial[chunk][k][c]) * (divide ? 1 / rows(s) : 1)
__global__ void __launch_bounds__(64 * BN_SLICES) bn_reduce_kernel(const double* __restrict__ partial, double* __restrict__ out, BnSets st, int C,
                                                                   int divide) {
  __shared__ double red[2 * BN_SLICES * 64];
  const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl, s = blockIdx.y;
  double a = 0, b = 0;
  if (c < C)
    for (int ch = st.chunk0[s] + sl; ch < st.chunk0[s + 1]; ch += BN_SLICES) {
      a += partial[(size_t)ch * 2 * C + c];
      b += partial[(size_t)ch * 2 * C + C + c];
    }
  red[sl * 64 + cl] = a;
  red[(BN_SLICES + sl) * 64 + cl] = b;
  __syncthreads();
  if (sl == 0 && c < C) {
    for (int l = 1; l < BN_SLICES; ++l) {
      a += red[l * 64 + cl];
      b += red[(BN_SLICES + l) * 64 + cl];
    }
    const double m = divide ? 1.0 / (double)st.rows[s] : 1.0;
    out[((size_t)s * 2 + 0) * C + c] = a * m;
    out[((size_t)s * 2 + 1) * C + c] = b * m;
  }
}

// finalize: one thread per channel walks the sets IN ORDER (two sets of one level update its running statistics one after the other, as
// the reference's two forward calls do).  mode 0 (training): from moments[s] = [mean, mean of squares]; mode 1 (eval): from the running
// statistics, which stay untouched.  count_mul: ranks whose equal-sized sets the moments average (SyncBN: the count is rows * count_mul);
// biased_running: the running variance takes the biased variance ([D2-recall] NaiveSyncBatchNorm) instead of var * n / (n - 1).
__global__ void bn_finalize_kernel(const double* __restrict__ moments, const float* __restrict__ gamma, float* __restrict__ running_mean,
                                   float* __restrict__ running_var, double* __restrict__ mean_out, double* __restrict__ rstd_out,
                                   double* __restrict__ scale_out, BnSets st, int C, double eps, double momentum, int mode, int count_mul,
                                   int biased_running) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  for (int s = 0; s < st.n; ++s) {
    const size_t pc = (size_t)st.level[s] * C + c, sc = (size_t)s * C + c;
    double mean, var;
    if (mode == 0) {
      const double m2 = moments[((size_t)s * 2 + 1) * C + c];
      mean = moments[((size_t)s * 2 + 0) * C + c];
      var = fmax(m2 - mean * mean, 0.0);
      const double n = (double)st.rows[s] * (double)count_mul;
      const double vrun = biased_running ? var : var * (n / (n - 1.0));
      const double rm = (double)running_mean[pc], rv = (double)running_var[pc];
      running_mean[pc] = (float)(rm + momentum * (mean - rm));     // one rounding into the fp32 arena
      running_var[pc] = (float)(rv + momentum * (vrun - rv));
    } else {
      mean = (double)running_mean[pc];
      var = (double)running_var[pc];
    }
    const double rstd = 1.0 / sqrt(var + eps);
    mean_out[sc] = mean;
    rstd_out[sc] = rstd;
    scale_out[sc] = (double)gamma[pc] * rstd;
  }
}

// y = relu(x * scale + shift) with shift = beta - mean * scale, evaluated as (x - mean) * scale + beta: the same value without the
// cancellation of two large products when |mean| is large against the spread.  The three operations run in fp64 from the fp64
// per-channel coefficients: y is the correctly rounded value of the exact expression up to the final rounding (fp32 output: one
// rounding; 16-bit output: through fp32, within 1 ulp).  fp32 arithmetic misses that bound where the value cancels to near zero; what
// the fp64 operations and conversions cost against the pass's HBM traffic is a measured figure, not assumed.
template <typename T>
__global__ void __launch_bounds__(256) bn_apply_relu_kernel(const T* __restrict__ x, T* __restrict__ y, const double* __restrict__ mean,
                                                            const double* __restrict__ scale, const float* __restrict__ beta, BnSets st, int C) {
  const BnTile t = bn_tile(st);
  if (t.c >= C) return;
  double mu[4], sc[4];
  bn_coef4(mean, t.s, C, t.c, mu), bn_coef4(scale, t.s, C, t.c, sc);
  const f32x4 be = ld4(beta, ((size_t)st.level[t.s] * C + t.c) >> 2);
  for (int r = t.rl; r < t.nr; r += BN_LANES) {
    const size_t i4 = t.quad(r, C);
    const f32x4 v = ld4(x, i4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)bn_relu(((double)v[e] - mu[e]) * sc[e] + (double)be[e]);
    st4(y, i4, o);
  }
}

// stage 1, backward: partial[chunk][0][c] = sum g, [1][c] = sum g * xhat; g = dy * [y > 0], xhat = (x - mean) * rstd
template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_partial_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x,
                                                             const double* __restrict__ mean, const double* __restrict__ rstd,
                                                             double* __restrict__ partial, BnSets st, int C) {
  const BnTile t = bn_tile(st);
  double mu[4], rs[4];
  if (t.c < C) bn_coef4(mean, t.s, C, t.c, mu), bn_coef4(rstd, t.s, C, t.c, rs);
  bn_stage1(t, C, partial, [&](size_t i4, double (&a)[4], double (&b)[4]) {
    const f32x4 g = ld4(dy, i4), yy = ld4(y, i4), xx = ld4(x, i4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double ge, xh;
      bn_gx(g[e], yy[e], xx[e], mu[e], rs[e], ge, xh);
      a[e] += ge, b[e] += ge * xh;
    }
  });
}

// parameter gradients: dgamma[level] += sum g * xhat, dbeta[level] += sum g, the sets of a level in order; sums of several ranks
// (count_mul > 1) enter as their mean, which the data-parallel gradient average leaves unchanged
__global__ void bn_bwd_param_kernel(const double* __restrict__ sums, float* __restrict__ dgamma, float* __restrict__ dbeta, BnSets st, int C,
                                    int count_mul) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double w = 1.0 / (double)count_mul;
  for (int s = 0; s < st.n; ++s) {
    const size_t pc = (size_t)st.level[s] * C + c;
    dbeta[pc] += (float)(sums[((size_t)s * 2 + 0) * C + c] * w);
    dgamma[pc] += (float)(sums[((size_t)s * 2 + 1) * C + c] * w);
  }
}

// stage 2, backward: dx = gamma * rstd * (g - sum g / n - xhat * sum g xhat / n), n = rows * count_mul
template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x,
                                                        const double* __restrict__ mean, const double* __restrict__ rstd,
                                                        const float* __restrict__ gamma, const double* __restrict__ sums, T* __restrict__ dx,
                                                        BnSets st, int C, int count_mul) {
  const BnTile t = bn_tile(st);
  if (t.c >= C) return;
  const f32x4 ga = ld4(gamma, ((size_t)st.level[t.s] * C + t.c) >> 2);
  const double n = (double)st.rows[t.s] * (double)count_mul;
  double mu[4], rs[4], mg[4], mgx[4], k[4];   // fp64 throughout, as in the apply pass
  bn_coef4(mean, t.s, C, t.c, mu), bn_coef4(rstd, t.s, C, t.c, rs);
  bn_coef4(sums, (size_t)t.s * 2 + 0, C, t.c, mg), bn_coef4(sums, (size_t)t.s * 2 + 1, C, t.c, mgx);
#pragma unroll
  for (int e = 0; e < 4; ++e) mg[e] = mg[e] / n, mgx[e] = mgx[e] / n, k[e] = (double)ga[e] * rs[e];
  for (int r = t.rl; r < t.nr; r += BN_LANES) {
    const size_t i4 = t.quad(r, C);
    const f32x4 g = ld4(dy, i4), yy = ld4(y, i4), xx = ld4(x, i4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double ge, xh;
      bn_gx(g[e], yy[e], xx[e], mu[e], rs[e], ge, xh);
      o[e] = (float)(k[e] * ((ge - mg[e]) - xh * mgx[e]));
    }
    st4(dx, i4, o);
  }
}

static inline dim3 bn_grid(const BnSets& st, int C) { return dim3(st.chunk0[st.n], cdiv(C, BN_COLS)); }

extern "C" {

int utv2_bn_chunks(int nsets, const int* set_rows_host) {
  if (nsets < 1 || nsets > UTV2_BN_MAX_SETS || !set_rows_host) return UTV2_EARG;
  int c = 0;
  for (int s = 0; s < nsets; ++s) c += bn_chunks_of(set_rows_host[s]);
  return c;
}

int utv2_bn_stats_partial(const void* x, int dtype, double* partial, int64_t P, int C, int nsets, const int* set_row0_host,
                          const int* set_rows_host, hipStream_t stream) {
  BnSets st;
  if (bn_gate(st, BN_ROW0, nsets, set_row0_host, set_rows_host, nullptr, 0, P, {{x, BN_ACTQ}, {partial, BN_ANY}}, dtype, C, true)) return UTV2_EARG;
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(bn_stats_partial_kernel<T>, bn_grid(st, C), dim3(256), 0, stream, (const T*)x, partial, st, C);
  });
  return utv2_launch_status();
}

int utv2_bn_reduce(const double* partial, double* out, int C, int nsets, const int* set_rows_host, int divide, hipStream_t stream) {
  BnSets st;
  if (bn_gate(st, BN_ROWS_ONLY, nsets, nullptr, set_rows_host, nullptr, 0, 0, {{partial, BN_ANY}, {out, BN_ANY}}, UTV2_F32, C, false)) return UTV2_EARG;
  hipLaunchKernelGGL(bn_reduce_kernel, dim3((C + 63) / 64, nsets), dim3(64 * BN_SLICES), 0, stream, partial, out, st, C, divide);
  return utv2_launch_status();
}

int utv2_bn_finalize(const double* moments, const float* gamma, float* running_mean, float* running_var, double* mean, double* rstd,
                     double* scale, int C, int nlevels, int nsets, const int* set_rows_host, const int* set_level_host, double eps,
                     double momentum, int mode, int count_mul, int biased_running, hipStream_t stream) {
  if (count_mul < 1 || (mode != 0 && mode != 1) || (mode == 0 && !moments)) return UTV2_EARG;
  BnSets st;
  if (bn_gate(st, BN_LEVEL, nsets, nullptr, set_rows_host, set_level_host, nlevels, 0,
              {{gamma, BN_ANY}, {running_mean, BN_ANY}, {running_var, BN_ANY}, {mean, BN_ANY}, {rstd, BN_ANY}, {scale, BN_ANY}}, UTV2_F32, C, false))
    return UTV2_EARG;
  for (int s = 0; s < nsets && mode == 0; ++s)
    if ((int64_t)set_rows_host[s] * count_mul < 2) return UTV2_EARG;   // "Expected more than 1 value per channel"
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, moments, gamma, running_mean, running_var, mean, rstd,
                     scale, st, C, eps, momentum, mode, count_mul, biased_running);
  return utv2_launch_status();
}

int utv2_bn_apply_relu(const void* x, void* y, int dtype, const double* mean, const double* scale, const float* beta, int64_t P, int C,
                       int nlevels, int nsets, const int* set_row0_host, const int* set_rows_host, const int* set_level_host,
                       hipStream_t stream) {
  BnSets st;
  if (bn_gate(st, BN_ROW0 | BN_LEVEL, nsets, set_row0_host, set_rows_host, set_level_host, nlevels, P,
              {{x, BN_ACTQ}, {y, BN_ACTQ}, {mean, BN_ANY}, {scale, BN_ANY}, {beta, BN_F32Q}}, dtype, C, true))
    return UTV2_EARG;
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(bn_apply_relu_kernel<T>, bn_grid(st, C), dim3(256), 0, stream, (const T*)x, (T*)y, mean, scale, beta, st, C);
  });
  return utv2_launch_status();
}

int utv2_bn_bwd_partial(const void* dy, const void* y, const void* x, int dtype, const double* mean, const double* rstd, double* partial,
                        int64_t P, int C, int nsets, const int* set_row0_host, const int* set_rows_host, hipStream_t stream) {
  BnSets st;
  if (bn_gate(st, BN_ROW0, nsets, set_row0_host, set_rows_host, nullptr, 0, P,
              {{dy, BN_ACTQ}, {y, BN_ACTQ}, {x, BN_ACTQ}, {mean, BN_ANY}, {rstd, BN_ANY}, {partial, BN_ANY}}, dtype, C, true))
    return UTV2_EARG;
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(bn_bwd_partial_kernel<T>, bn_grid(st, C), dim3(256), 0, stream, (const T*)dy, (const T*)y, (const T*)x, mean, rstd, partial, st, C);
  });
  return utv2_launch_status();
}

int utv2_bn_bwd_apply(const void* dy, const void* y, const void* x, void* dx, int dtype, const double* mean, const double* rstd,
                      const float* gamma, const double* sums, float* dgamma, float* dbeta, int64_t P, int C, int nlevels, int nsets,
                      const int* set_row0_host, const int* set_rows_host, const int* set_level_host, int count_mul, hipStream_t stream) {
  BnSets st;
  if (count_mul < 1 || bn_gate(st, BN_ROW0 | BN_LEVEL, nsets, set_row0_host, set_rows_host, set_level_host, nlevels, P,
                               {{dy, BN_ACTQ}, {y, BN_ACTQ}, {x, BN_ACTQ}, {dx, BN_ACTQ}, {mean, BN_ANY}, {rstd, BN_ANY}, {gamma, BN_F32Q},
                                {sums, BN_ANY}, {dgamma, BN_ANY}, {dbeta, BN_ANY}}, dtype, C, true))
    return UTV2_EARG;
  hipLaunchKernelGGL(bn_bwd_param_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, sums, dgamma, dbeta, st, C, count_mul);
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(bn_bwd_dx_kernel<T>, bn_grid(st, C), dim3(256), 0, stream, (const T*)dy, (const T*)y, (const T*)x, mean, rstd, gamma, sums,
                       (T*)dx, st, C, count_mul);
  });
  return utv2_launch_status();
}

}  // extern "C"
