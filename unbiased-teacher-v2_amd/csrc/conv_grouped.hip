// Grouped 3x3 convolution (ResNeXt conv2): NHWC, pad 1, stride 1 or 2, G groups of g = C / G channels (g % 4 == 0), C input and
// C output channels.  Forward (FrozenBN scale / shift + ReLU epilogue), dgrad (FrozenBN multiplier folded into the weights, ReLU mask
// of the producer and a residual in the epilogue) and a deterministic split-pixel wgrad.
//
// Operands are fp32 (the exact-fp32 mode) or h16_t (bf16, or fp16 in the -DUTV2_H16=_Float16 build); arithmetic is fp32 fmaf in
// a fixed order either way, so one source serves all three precision modes.  The weight is the arena matrix [C][3][3][g] as it
// stands (row k = output channel k, reading input channels [g * (k / g), g * (k / g) + g)): no im2col, no flipped weight image.
//
// Thread tiles: a forward / dgrad thread owns 4 consecutive channels (one group: g % 4 == 0) of GPX consecutive pixels of one row, so
// the 4 x 4 weight block of a (tap, channel quad) step is loaded once for GPX pixels, and the 9-tap halo is served by L1 / L2: threads
// next to each other in a wave hold neighbouring channel quads of the same pixels, so the activations are read as whole 16-byte runs
// and the quads of one group are broadcast.  The wgrad thread owns a 4 x 4 block (output-channel quad x input-channel quad) of one tap
// over a contiguous range of output pixels (one split); the splits' partial sums are reduced in split order by a second launch.
#include "common.h"

namespace {

constexpr int GPX = 4;      // pixels per forward / dgrad thread

__host__ __device__ inline int gcdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// one 4-element load as fp32 from an 8-byte (h16) / 16-byte (fp32) aligned address
template <typename T> __device__ __forceinline__ f32x4 q4(const T* p) { return ld4(p, 0); }

template <typename T, typename TO>
__global__ __launch_bounds__(256) void utv2_gconv3x3_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w, TO* __restrict__ y,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                int N, int H, int W, int C, int g, int stride, int OH, int OW, int OWT,
                                                                int relu) {
  const int CQ = C >> 2;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (int64_t)N * OH * OWT * CQ) return;
  const int cq = (int)(tid % CQ);
  int64_t r = tid / CQ;
  const int owt = (int)(r % OWT);
  r /= OWT;
  const int oh = (int)(r % OH);
  const int n = (int)(r / OH);
  const int co = cq * 4, cin0 = co - co % g, ow0 = owt * GPX;
  const int64_t wrow = (int64_t)9 * g;      // one weight row
  float acc[GPX][4];
#pragma unroll
  for (int p = 0; p < GPX; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[p][j] = 0.f;
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = oh * stride - 1 + kh;
    if (ih < 0 || ih >= H) continue;
    const T* xrow = x + ((int64_t)n * H + ih) * W * C + cin0;
    for (int kw = 0; kw < 3; ++kw) {
      int iw[GPX];
      bool ok[GPX];
#pragma unroll
      for (int p = 0; p < GPX; ++p) {
        iw[p] = (ow0 + p) * stride - 1 + kw;
        ok[p] = ow0 + p < OW && iw[p] >= 0 && iw[p] < W;
      }
      const T* wt = w + (int64_t)co * wrow + (kh * 3 + kw) * g;
      for (int c = 0; c < g; c += 4) {
        f32x4 wv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wv[j] = q4(wt + j * wrow + c);
#pragma unroll
        for (int p = 0; p < GPX; ++p) {
          if (!ok[p]) continue;
          const f32x4 xv = q4(xrow + (int64_t)iw[p] * C + c);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[p][j] = fmaf(xv[e], wv[j][e], acc[p][j]);
        }
      }
    }
  }
  f32x4 sc, sh;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sc[j] = scale ? scale[co + j] : 1.f;
    sh[j] = shift ? shift[co + j] : 0.f;
  }
#pragma unroll
  for (int p = 0; p < GPX; ++p) {
    if (ow0 + p >= OW) continue;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t = scale ? acc[p][j] * sc[j] : acc[p][j];
      t = t + sh[j];
      v[j] = relu ? fmaxf(t, 0.f) : t;
    }
    st4(y + (((int64_t)n * OH + oh) * OW + ow0 + p) * C + co, 0, v);
  }
}

// dx[n][ih][iw][c] = sum over taps (kh, kw) with ih = oh * stride - 1 + kh (likewise iw) and output channels k of c's group of
// dy[n][oh][ow][k] * scale[k] * w[k][kh][kw][c % g]; then the epilogue: mask (dx = mask > 0 ? dx : 0), + residual.
template <typename T, typename TO>
__global__ __launch_bounds__(256) void utv2_gconv3x3_dgrad_kernel(const T* __restrict__ dy, const T* __restrict__ w, TO* __restrict__ dx,
                                                                  const float* __restrict__ scale, const TO* __restrict__ mask,
                                                                  const TO* __restrict__ residual, int N, int H, int W, int C, int g,
                                                                  int stride, int OH, int OW, int IWT) {
  const int CQ = C >> 2;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (int64_t)N * H * IWT * CQ) return;
  const int cq = (int)(tid % CQ);
  int64_t r = tid / CQ;
  const int iwt = (int)(r % IWT);
  r /= IWT;
  const int ih = (int)(r % H);
  const int n = (int)(r / H);
  const int ci = cq * 4, k0 = ci - ci % g, cl = ci - k0, iw0 = iwt * GPX;
  const int64_t wrow = (int64_t)9 * g;
  float acc[GPX][4];
#pragma unroll
  for (int p = 0; p < GPX; ++p)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[p][e] = 0.f;
  for (int kh = 0; kh < 3; ++kh) {
    int oh = ih + 1 - kh;
    if (oh < 0 || oh % stride) continue;
    oh /= stride;
    if (oh >= OH) continue;
    const T* dyrow = dy + ((int64_t)n * OH + oh) * OW * C + k0;
    for (int kw = 0; kw < 3; ++kw) {
      int ow[GPX];
      bool ok[GPX];
#pragma unroll
      for (int p = 0; p < GPX; ++p) {
        const int t = iw0 + p + 1 - kw;
        ow[p] = t / stride;
        ok[p] = iw0 + p < W && t >= 0 && t % stride == 0 && ow[p] < OW;
      }
      const T* wt = w + (int64_t)k0 * wrow + (kh * 3 + kw) * g + cl;
      for (int k = 0; k < g; k += 4) {
        f32x4 wv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wv[j] = q4(wt + (int64_t)(k + j) * wrow);
          if (scale) wv[j] = wv[j] * scale[k0 + k + j];
        }
#pragma unroll
        for (int p = 0; p < GPX; ++p) {
          if (!ok[p]) continue;
          const f32x4 dv = q4(dyrow + (int64_t)ow[p] * C + k);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[p][e] = fmaf(dv[j], wv[j][e], acc[p][e]);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < GPX; ++p) {
    if (iw0 + p >= W) continue;
    const int64_t o = (((int64_t)n * H + ih) * W + iw0 + p) * C + ci;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = acc[p][e];
    if (mask) {
      const f32x4 m = q4(mask + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
    }
    if (residual) v = v + q4(residual + o);
    st4(dx + o, 0, v);
  }
}

// ws[split][k][kh][kw][c] = sum over the split's output pixels m of dy[m][k] * x[input pixel of m at tap (kh, kw)][group(k) * g + c].
// Thread (kq, tap, cq): output channels 4 kq .. 4 kq + 3, input channels 4 cq .. 4 cq + 3 of the group, one tap.
template <typename T>
__global__ __launch_bounds__(256) void utv2_gconv3x3_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ ws,
                                                                  int N, int H, int W, int C, int g, int stride, int OH, int OW,
                                                                  int per_split) {
  const int GQ = g >> 2;
  const int tpl = (C >> 2) * 9 * GQ;      // threads per split
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tpl) return;
  const int cq = t % GQ;
  const int tap = (t / GQ) % 9;
  const int kq = t / (GQ * 9);
  const int k = kq * 4, cin = k - k % g + cq * 4, kh = tap / 3, kw = tap % 3;
  const int64_t M = (int64_t)N * OH * OW;
  const int64_t m0 = (int64_t)blockIdx.y * per_split;
  const int64_t m1 = m0 + per_split < M ? m0 + per_split : M;
  float acc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[j][e] = 0.f;
  if (m0 < M) {
    int ow = (int)(m0 % OW), oh = (int)((m0 / OW) % OH), n = (int)(m0 / ((int64_t)OW * OH));
    for (int64_t m = m0; m < m1; ++m) {
      const int ih = oh * stride - 1 + kh, iw = ow * stride - 1 + kw;
      if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
        const f32x4 dv = q4(dy + m * C + k);
        const f32x4 xv = q4(x + (((int64_t)n * H + ih) * W + iw) * C + cin);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(dv[j], xv[e], acc[j][e]);
      }
      if (++ow == OW) {
        ow = 0;
        if (++oh == OH) {
          oh = 0;
          ++n;
        }
      }
    }
  }
  float* o = ws + (int64_t)blockIdx.y * C * 9 * g + (int64_t)k * 9 * g + tap * g + cq * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = acc[j][e];
    st4(o + (int64_t)j * 9 * g, 0, v);
  }
}

// dw[i] (+)= scale[row of i] * sum over splits s (in order) of ws[s][i]
__global__ __launch_bounds__(256) void utv2_gconv3x3_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                         const float* __restrict__ scale, int64_t n, int row, int splits,
                                                                         int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += ws[(int64_t)sp * n + i];
  if (scale) s = s * scale[i / row];
  dw[i] = accumulate ? dw[i] + s : s;
}

bool shape_ok(int N, int H, int W, int C, int G, int stride, int OH, int OW) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || G <= 0 || C % G) return false;
  const int g = C / G;
  if (g % 4 || (stride != 1 && stride != 2)) return false;
  return OH == (H - 1) / stride + 1 && OW == (W - 1) / stride + 1;
}

int wgrad_splits(int N, int OH, int OW, int C, int G) {
  const int g = C / G;
  const int64_t tpl = (int64_t)(C / 4) * 9 * (g / 4);
  const int64_t M = (int64_t)N * OH * OW;
  int64_t s = (262144 + tpl - 1) / tpl;           // about 1024 threads per CU over the chip
  const int64_t cap_ws = ((int64_t)1 << 25) / ((int64_t)C * 9 * g);   // <= 128 MB of partial sums
  if (s > cap_ws) s = cap_ws;
  if (s > 256) s = 256;
  if (s > (M + 31) / 32) s = (M + 31) / 32;       // >= 32 pixels per split
  return s < 1 ? 1 : (int)s;
}

}  // namespace

extern "C" {

int utv2_gconv3x3_supported(int C, int G) { return C > 0 && G > 0 && C % G == 0 && (C / G) % 4 == 0; }

int utv2_gconv3x3_fwd(const void* x, const void* w, int op_dtype, void* y, int y_dtype, const float* scale, const float* shift, int N,
                      int H, int W, int C, int G, int stride, int OH, int OW, int relu, hipStream_t stream) {
  if (!x || !w || !y || !shape_ok(N, H, W, C, G, stride, OH, OW)) return UTV2_EARG;
  const int OWT = gcdiv(OW, GPX);
  const int64_t n = (int64_t)N * OH * OWT * (C / 4);
  const dim3 grid(gcdiv(n, 256)), block(256);
  const int g = C / G;
#define GF_LAUNCH(T, TO)                                                                                                   \
  hipLaunchKernelGGL((utv2_gconv3x3_fwd_kernel<T, TO>), grid, block, 0, stream, (const T*)x, (const T*)w, (TO*)y, scale, shift, N, H, \
                     W, C, g, stride, OH, OW, OWT, relu)
  if (op_dtype == UTV2_F32 && y_dtype == UTV2_F32) GF_LAUNCH(float, float);
  else if (op_dtype == UTV2_BF16 && y_dtype == UTV2_BF16) GF_LAUNCH(h16_t, h16_t);
  else if (op_dtype == UTV2_BF16 && y_dtype == UTV2_F32) GF_LAUNCH(h16_t, float);
  else return UTV2_EARG;
#undef GF_LAUNCH
  return utv2_launch_status();
}

int utv2_gconv3x3_dgrad(const void* dy, const void* w, int op_dtype, void* dx, int dx_dtype, const float* scale, const void* mask,
                        const void* residual, int N, int H, int W, int C, int G, int stride, int OH, int OW, hipStream_t stream) {
  if (!dy || !w || !dx || !shape_ok(N, H, W, C, G, stride, OH, OW)) return UTV2_EARG;
  const int IWT = gcdiv(W, GPX);
  const int64_t n = (int64_t)N * H * IWT * (C / 4);
  const dim3 grid(gcdiv(n, 256)), block(256);
  const int g = C / G;
#define GD_LAUNCH(T, TO)                                                                                                        \
  hipLaunchKernelGGL((utv2_gconv3x3_dgrad_kernel<T, TO>), grid, block, 0, stream, (const T*)dy, (const T*)w, (TO*)dx, scale,       \
                     (const TO*)mask, (const TO*)residual, N, H, W, C, g, stride, OH, OW, IWT)
  if (op_dtype == UTV2_F32 && dx_dtype == UTV2_F32) GD_LAUNCH(float, float);
  else if (op_dtype == UTV2_BF16 && dx_dtype == UTV2_BF16) GD_LAUNCH(h16_t, h16_t);
  else if (op_dtype == UTV2_BF16 && dx_dtype == UTV2_F32) GD_LAUNCH(h16_t, float);
  else return UTV2_EARG;
#undef GD_LAUNCH
  return utv2_launch_status();
}

int utv2_gconv3x3_wgrad_splits(int N, int OH, int OW, int C, int G) {
  if (N <= 0 || OH <= 0 || OW <= 0 || C <= 0 || G <= 0 || C % G || (C / G) % 4) return 0;
  return wgrad_splits(N, OH, OW, C, G);
}

int64_t utv2_gconv3x3_wgrad_workspace_floats(int N, int OH, int OW, int C, int G) {
  const int s = utv2_gconv3x3_wgrad_splits(N, OH, OW, C, G);
  return s <= 0 ? 0 : (int64_t)s * C * 9 * (C / G);
}

int utv2_gconv3x3_wgrad(const void* x, const void* dy, int op_dtype, float* dw, float* ws, const float* scale, int N, int H, int W,
                        int C, int G, int stride, int OH, int OW, int accumulate, hipStream_t stream) {
  if (!x || !dy || !dw || !ws || !shape_ok(N, H, W, C, G, stride, OH, OW)) return UTV2_EARG;
  const int g = C / G;
  const int splits = wgrad_splits(N, OH, OW, C, G);
  const int64_t M = (int64_t)N * OH * OW;
  const int per_split = (int)((M + splits - 1) / splits);
  const int tpl = (C / 4) * 9 * (g / 4);
  const dim3 grid(gcdiv(tpl, 256), splits), block(256);
  if (op_dtype == UTV2_F32)
    hipLaunchKernelGGL((utv2_gconv3x3_wgrad_kernel<float>), grid, block, 0, stream, (const float*)x, (const float*)dy, ws, N, H, W, C, g,
                       stride, OH, OW, per_split);
  else if (op_dtype == UTV2_BF16)
    hipLaunchKernelGGL((utv2_gconv3x3_wgrad_kernel<h16_t>), grid, block, 0, stream, (const h16_t*)x, (const h16_t*)dy, ws, N, H, W, C,
                       g, stride, OH, OW, per_split);
  else
    return UTV2_EARG;
  int rc = utv2_launch_status();
  if (rc) return rc;
  const int64_t n = (int64_t)C * 9 * g;
  hipLaunchKernelGGL(utv2_gconv3x3_wgrad_reduce_kernel, dim3(gcdiv(n, 256)), dim3(256), 0, stream, ws, dw, scale, n, 9 * g, splits,
                     accumulate);
  return utv2_launch_status();
}

}  // extern "C"
