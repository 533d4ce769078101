// TEST.PRECISE_BN for the BatchNorm FCOS towers: the population statistics of a BatchNorm layer estimated on the device from a number
// of training-mode forward calls, then written into its running buffers once ([D2-recall] hooks.PreciseBN, [fvcore-recall]
// update_bn_stats; restated in DESIGN.md).
//
// The estimator's state is fp64 per (level, channel): state[level][0][c] = pop_mean, [1][c] = pop_sq (mean of squares), [2][c] = num
// (images seen so far; carried per channel so that a channel's thread owns everything it reads and writes).  One STATISTIC SET (bn_sets.h)
// of batch size B, batch mean m and unbiased batch variance v adds
//     num += B;  q = m * m + v * (B - 1) / B;  pop_mean += (m - pop_mean) * (B / num);  pop_sq += (q - pop_sq) * (B / num)
// with v = var * n / (n - 1), n = rows * count_mul: the value utv2_bn_finalize mode 0 moves the running variance by (biased_running: var
// itself, as there).  The sets are applied IN ORDER by one thread per channel: no atomics, one fixed order, bit-reproducible.
// `update` also emits mean / rstd / scale of utv2_bn_finalize mode 0, operation for operation, so a statistics-only forward runs
// stats_partial, reduce, precise_update, apply_relu - one launch where training runs finalize - and touches no running buffer.
// `commit` writes running_mean = pop_mean and running_var = pop_sq - pop_mean^2, each rounded once to fp32, for every layer of a head.
#include <stdint.h>
#include "common.h"
#include "bn_sets.h"

#define BNP_MAX_LAYERS 32   // layers per commit launch (pointer tables by value)

struct BnpImages { int b[UTV2_BN_MAX_SETS]; };
struct BnpLayers {
  float* mean[BNP_MAX_LAYERS];
  float* var[BNP_MAX_LAYERS];
};

__global__ void bn_precise_update_kernel(const double* __restrict__ moments, const float* __restrict__ gamma, double* __restrict__ state,
                                         double* __restrict__ mean_out, double* __restrict__ rstd_out, double* __restrict__ scale_out,
                                         BnSets st, BnpImages im, int C, double eps, int count_mul, int biased_running) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  for (int s = 0; s < st.n; ++s) {
    const size_t pc = (size_t)st.level[s] * C + c, sc = (size_t)s * C + c;
    // mean, var, rstd, scale: the lines of bn_finalize_kernel mode 0
    const double m2 = moments[((size_t)s * 2 + 1) * C + c];
    const double mean = moments[((size_t)s * 2 + 0) * C + c];
    const double var = fmax(m2 - mean * mean, 0.0);
    const double n = (double)st.rows[s] * (double)count_mul;
    const double vrun = biased_running ? var : var * (n / (n - 1.0));
    const double rstd = 1.0 / sqrt(var + eps);
    mean_out[sc] = mean;
    rstd_out[sc] = rstd;
    scale_out[sc] = (double)gamma[pc] * rstd;
    // the estimator [fvcore-recall]
    double* ps = state + (size_t)st.level[s] * 3 * C + c;
    const double B = (double)im.b[s];
    const double num = ps[2 * C] + B;
    const double q = mean * mean + vrun * ((B - 1.0) / B);
    const double w = B / num;
    const double pm = ps[0], pq = ps[C];
    ps[0] = pm + (mean - pm) * w;
    ps[C] = pq + (q - pq) * w;
    ps[2 * C] = num;
  }
}

// one thread per (layer, level, channel); a level that no set has reached (num == 0) keeps its buffers
__global__ void bn_precise_commit_kernel(const double* __restrict__ state, BnpLayers ly, int nlayers, int nlevels, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t LC = (int64_t)nlevels * C;
  if (i >= nlayers * LC) return;
  const int k = (int)(i / LC), l = (int)((i - k * LC) / C), c = (int)(i - k * LC - (int64_t)l * C);
  const double* ps = state + ((size_t)k * nlevels + l) * 3 * C + c;
  if (!(ps[2 * C] > 0.0)) return;
  const double pm = ps[0], pq = ps[C];
  ly.mean[k][(size_t)l * C + c] = (float)pm;
  ly.var[k][(size_t)l * C + c] = (float)(pq - pm * pm);
}

extern "C" {

int utv2_bn_precise_update(const double* moments, const float* gamma, double* state, double* mean, double* rstd, double* scale, int C,
                           int nlevels, int nsets, const int* set_rows_host, const int* set_level_host, const int* set_images_host,
                           double eps, int count_mul, int biased_running, hipStream_t stream) {
  if (count_mul < 1 || !set_images_host) return UTV2_EARG;
  BnSets st;
  if (bn_gate(st, BN_LEVEL, nsets, nullptr, set_rows_host, set_level_host, nlevels, 0,
              {{moments, BN_ANY}, {gamma, BN_ANY}, {state, BN_ANY}, {mean, BN_ANY}, {rstd, BN_ANY}, {scale, BN_ANY}}, UTV2_F32, C, true))
    return UTV2_EARG;
  BnpImages im;
  for (int s = 0; s < UTV2_BN_MAX_SETS; ++s) im.b[s] = 0;
  for (int s = 0; s < nsets; ++s) {
    if ((int64_t)set_rows_host[s] * count_mul < 2 || set_images_host[s] < 1) return UTV2_EARG;   // n < 2 | B < 1
    im.b[s] = set_images_host[s];
  }
  hipLaunchKernelGGL(bn_precise_update_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, moments, gamma, state, mean, rstd, scale, st, im, C,
                     eps, count_mul, biased_running);
  return utv2_launch_status();
}

int utv2_bn_precise_commit(const double* state, float* const* running_mean_host, float* const* running_var_host, int nlayers, int nlevels,
                           int C, hipStream_t stream) {
  if (!state || !running_mean_host || !running_var_host || nlayers < 1 || nlevels < 1 || C < 4 || (C & 3)) return UTV2_EARG;
  if ((int64_t)nlayers * nlevels * C >= ((int64_t)1 << 31)) return UTV2_EARG;
  for (int k = 0; k < nlayers; ++k)
    if (!running_mean_host[k] || !running_var_host[k]) return UTV2_EARG;
  for (int k0 = 0; k0 < nlayers; k0 += BNP_MAX_LAYERS) {
    const int nk = nlayers - k0 < BNP_MAX_LAYERS ? nlayers - k0 : BNP_MAX_LAYERS;
    BnpLayers ly;
    for (int k = 0; k < BNP_MAX_LAYERS; ++k) ly.mean[k] = k < nk ? running_mean_host[k0 + k] : nullptr, ly.var[k] = k < nk ? running_var_host[k0 + k] : nullptr;
    const int64_t total = (int64_t)nk * nlevels * C;
    hipLaunchKernelGGL(bn_precise_commit_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       state + (size_t)k0 * nlevels * 3 * C, ly, nk, nlevels, C);
    const int rc = utv2_launch_status();
    if (rc) return rc;
  }
  return UTV2_OK;
}

}  // extern "C"
