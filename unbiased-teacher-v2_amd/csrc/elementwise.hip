// HBM-bound elementwise / reduction kernels of the UTv2 step (gfx950).
// All arithmetic fp32, one rounding per written operation (the library is built with
// -ffp-contract=off) so results are comparable op-for-op with the reference's eager
// PyTorch expressions.
#include <stdlib.h>
#include "common.h"

// ---------------------------------------------------------------------------------------------
// Teacher EMA  (ubteacher/engine/trainer.py:468-486 == :950-968)
//   new_teacher = student * (1 - keep) + teacher * keep      evaluated exactly as written:
//   two rounded products and one rounded sum; a = (float)(1 - keep), b = (float)keep.
// One launch over the whole flat state arena: 12 B/element algorithmic traffic.
// mirror16 (optional): the 16-bit copy of the arena the mixed-precision convs read (RNE of the value just written) - saves the
// conversion pass that would re-read the arena at the start of the next forward.
__global__ __launch_bounds__(256) void ema_axpby_f32(float* __restrict__ teacher, const float* __restrict__ student,
                                                   size_t n4, size_t n, float a, float b, h16_t* __restrict__ mirror16) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  f32x4* t4 = (f32x4*)teacher;
  const f32x4* s4 = (const f32x4*)student;
  for (size_t j = i; j < n4; j += stride) {
    f32x4 t = t4[j], s = s4[j], r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = __fadd_rn(__fmul_rn(s[e], a), __fmul_rn(t[e], b));
    t4[j] = r;
    if (mirror16) st4(mirror16, j, r);
  }
  // tail
  for (size_t j = n4 * 4 + i; j < n; j += stride) {
    const float r = __fadd_rn(__fmul_rn(student[j], a), __fmul_rn(teacher[j], b));
    teacher[j] = r;
    if (mirror16) mirror16[j] = (h16_t)r;
  }
}

// ---------------------------------------------------------------------------------------------
// Dynamic loss scaling for the fp16 AMP mode, with torch.cuda.amp.GradScaler's semantics (the reference: engine/trainer.py:207,
// 424-426 `scaler.scale(losses).backward(); scaler.step(optimizer); scaler.update()`), entirely on the device - no host read of
// the inf flag.  state = fp32 {scale, found_inf, growth_tracker}:
//   backward runs on scale * loss;  amp_found_inf marks non-finite gradients;  the AMP forms of the SGD kernels unscale (g / scale) and
//   apply the update unless found_inf (GradScaler.step skips optimizer.step());  amp_update_scale: found_inf ? scale *= backoff,
//   tracker = 0 : (++tracker == interval ? scale *= growth, tracker = 0), then clears found_inf.
// x - x is 0 for finite x, NaN for +-inf and NaN
__device__ __forceinline__ bool is_finite_f(float x) { return x - x == 0.f; }

__global__ __launch_bounds__(256) void amp_found_inf_f32(const float* __restrict__ g, size_t n4, size_t n, float* __restrict__ state) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (; i < n4; i += stride) {
    const f32x4 v = ((const f32x4*)g)[i];
    bad |= !(is_finite_f(v[0]) & is_finite_f(v[1]) & is_finite_f(v[2]) & is_finite_f(v[3]));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (size_t k = n4 * 4; k < n; ++k) bad |= !is_finite_f(g[k]);
  if (__any(bad) && (threadIdx.x & 63) == 0) state[1] = 1.0f;   // every writer stores the same value: order-free
}

__global__ void amp_update_scale_f32(float* __restrict__ state, float growth, float backoff, int interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float scale = state[0], tracker = state[2];
  if (state[1] != 0.f) {
    scale *= backoff;
    tracker = 0.f;
  } else {
    tracker += 1.f;
    if (tracker >= (float)interval) {
      const float grown = scale * growth;
      if (is_finite_f(grown)) scale = grown;       // only while the grown scale is finite
      tracker = 0.f;
    }
  }
  state[0] = scale;
  state[1] = 0.f;
  state[2] = tracker;
}

// ---------------------------------------------------------------------------------------------
// SGD with momentum + weight decay on a flat arena (D2 build_optimizer: torch.optim.SGD, momentum 0.9).
//   g = grad * gscale (AMP: grad * (1 / loss scale) * gscale) ; clip ; g += wd*p ; buf = mom*buf + g ; p -= lr*(nesterov ? g + mom*buf : buf)
// sgd_elem is the ONE place the update is written: the flat kernel below calls it with no clip and no Nesterov as literals (those
// branches fold away), the segmented kernel (next section) with its runtime clip between the gradient multiplier and the weight decay.
enum { SEG_CLIP_NONE = 0, SEG_CLIP_VALUE = 1, SEG_CLIP_NORM = 2 };

template <bool AMP>
__device__ __forceinline__ float sgd_elem(float pv, float gr, float& mv, float inv, float gscale, int clip_mode, float cf, float cv,
                                          float wd, float mom, float lr, int nesterov) {
  float gv = AMP ? __fmul_rn(__fmul_rn(gr, inv), gscale) : __fmul_rn(gr, gscale);
  if (clip_mode == SEG_CLIP_NORM) gv = __fmul_rn(gv, cf);
  else if (clip_mode == SEG_CLIP_VALUE) gv = gv < -cv ? -cv : (gv > cv ? cv : gv);   // a NaN stays a NaN (clamp_)
  gv = __fadd_rn(gv, __fmul_rn(wd, pv));
  mv = __fadd_rn(__fmul_rn(mom, mv), gv);
  const float step = nesterov ? __fadd_rn(gv, __fmul_rn(mom, mv)) : mv;
  return __fsub_rn(pv, __fmul_rn(lr, step));
}

// The flat form: one element per lane.  `gscale` multiplies the gradient (1/world for DDP mean); AMP: `state` as above; otherwise grad is
// zeroed afterwards if zero_grad != 0 (saves the separate memset pass).
template <bool AMP>
__global__ __launch_bounds__(256) void sgd_momentum_f32(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, size_t n,
                                                      float lr, float mom, float wd, float gscale, int zero_grad,
                                                      const float* __restrict__ state, h16_t* __restrict__ mirror16) {
  float inv = 1.f;
  if (AMP) {
    if (state[1] != 0.f) return;                     // non-finite gradients: the step is skipped (a fresh mirror16 stays fresh)
    inv = 1.0f / state[0];                           // the scale is a power of two: exact
  }
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float mv = m[i];
    const float pn = sgd_elem<AMP>(p[i], g[i], mv, inv, gscale, SEG_CLIP_NONE, 1.f, 0.f, wd, mom, lr, 0);
    m[i] = mv;
    p[i] = pn;
    if (mirror16) mirror16[i] = (h16_t)pn;
    if (!AMP && zero_grad) g[i] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// Per-tensor gradient clipping and Nesterov momentum inside the SGD update (SOLVER.CLIP_GRADIENTS.*, SOLVER.NESTEROV).
// [D2-recall] maybe_add_gradient_clipping runs, inside optimizer.step(), one clipper PER PARAMETER TENSOR on the unscaled gradient:
//   "value": clip_grad_value_ - g = clamp(g, -v, v);   "norm": clip_grad_norm_ - g *= min(1, v / (||g||_p + 1e-6)), p in {2, 1, inf};
// then torch.optim.SGD: g += wd*p ; buf = mom*buf + g ; p -= lr*(nesterov ? g + mom*buf : buf).
// The arena knows nothing of tensors, so the host hands over a WORK LIST that tiles the updated range: chunk c is the elements
// [chunk_start[c], chunk_start[c+1]) with the weight decay chunk_wd[c], and belongs to reference tensor ("segment") chunk_seg[c], or to
// none (-1: alignment padding and unexported rows - coefficient 1).  A chunk never crosses a segment
// border; a long segment is many chunks, so no tensor is serialised onto one workgroup.  Workgroups walk the list grid-stride; inside a
// chunk the head up to the first 16-byte boundary and the tail are done by single lanes, the body with 16-byte accesses.
// The norm is two-stage and atomic-free (bit-reproducible): seg_norm_partial writes one fp64 partial per chunk (every product and sum in
// fp64: a square of an fp32 value is exact there), seg_clip_coef adds a segment's partials in a fixed order with one wave and rounds
// once, at the end: coef = (float)min(1, v / (mult * norm + 1e-6)), mult = grad_scale / loss scale - the multiplier the update applies
// to the raw gradient (norms are homogeneous, so the norm of the scaled gradient is mult * the norm of the raw one).
enum { SEG_NORM_L2 = 0, SEG_NORM_L1 = 1, SEG_NORM_INF = 2 };

template <int KIND>
__device__ __forceinline__ double seg_norm_term(float v) {
  const double d = (double)v;
  return KIND == SEG_NORM_L2 ? d * d : fabs(d);
}

// sum, or a maximum that keeps a NaN once it has seen one (torch's max does)
template <int KIND>
__device__ __forceinline__ double seg_norm_join(double a, double b) {
  if (KIND != SEG_NORM_INF) return a + b;
  return (b > a || b != b) ? b : a;
}

template <int KIND>
__device__ __forceinline__ double seg_norm_wave(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = seg_norm_join<KIND>(v, __shfl_down(v, off, WAVE));
  return v;
}

// How a workgroup of 256 lanes walks chunk [s, e): the body is n4 quads from a, the first 16-byte boundary (the arena's base is 16-byte
// aligned); lanes 0..2 take the head elements in front of it, lanes 4..6 the tail elements behind the body; i = lane t's head or tail
// element, or -1
struct ChunkSplit {
  int64_t a, n4, tail, i;
};
__device__ __forceinline__ ChunkSplit chunk_split(int64_t s, int64_t e, int t) {
  ChunkSplit k;
  k.a = (s + 3) & ~(int64_t)3;
  if (k.a > e) k.a = e;
  k.n4 = (e - k.a) >> 2;
  k.tail = k.a + 4 * k.n4;
  k.i = -1;
  if (t < k.a - s) k.i = s + t;
  else if (t >= 4 && t - 4 < e - k.tail) k.i = k.tail + t - 4;
  return k;
}

template <int KIND>
__global__ __launch_bounds__(256) void seg_norm_partial(const float* __restrict__ g, const int64_t* __restrict__ chunk_start,
                                                      const int32_t* __restrict__ chunk_seg, int nchunks,
                                                      double* __restrict__ partial) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    if (chunk_seg[c] < 0) continue;                  // the same for the whole workgroup; nobody reads a gap's partial
    const ChunkSplit k = chunk_split(chunk_start[c], chunk_start[c + 1], t);
    double acc = k.i >= 0 ? seg_norm_term<KIND>(g[k.i]) : 0.0;
    for (int64_t j = t; j < k.n4; j += 4 * 256) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {                  // four independent 16-byte loads in flight per lane
        const int64_t jj = j + 256 * u;
        v[u] = jj < k.n4 ? *(const f32x4*)(g + k.a + 4 * jj) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = seg_norm_join<KIND>(acc, seg_norm_term<KIND>(v[u][q]));
    }
    acc = seg_norm_wave<KIND>(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0)
      partial[c] = seg_norm_join<KIND>(seg_norm_join<KIND>(red[0], red[1]), seg_norm_join<KIND>(red[2], red[3]));
    __syncthreads();                                 // red is written again in the next round
  }
}

// one wave per segment; seg_chunks[s] = {first chunk, chunk count}; state (AMP): the loss scale is read here, on the device
template <int KIND>
__global__ __launch_bounds__(64) void seg_clip_coef(const double* __restrict__ partial, const int32_t* __restrict__ seg_chunks, int nseg,
                                                  double clip_value, float gscale, const float* __restrict__ state,
                                                  float* __restrict__ coef) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= nseg) return;
  const int first = seg_chunks[2 * s], cnt = seg_chunks[2 * s + 1];
  double acc = 0.0;
  for (int i = lane; i < cnt; i += 64) acc = seg_norm_join<KIND>(acc, partial[first + i]);
  acc = seg_norm_wave<KIND>(acc);
  if (lane == 0) {
    const double mult = state ? (double)gscale / (double)state[0] : (double)gscale;
    const double norm = (KIND == SEG_NORM_L2 ? sqrt(acc) : acc) * mult;
    const double c = clip_value / (norm + 1e-6);
    coef[s] = (float)(c > 1.0 ? 1.0 : c);            // a NaN norm gives a NaN coefficient, as clip_grad_norm_ does
  }
}

template <bool AMP>
__global__ __launch_bounds__(256) void sgd_seg_f32(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 h16_t* __restrict__ mirror16, const int64_t* __restrict__ chunk_start,
                                                 const int32_t* __restrict__ chunk_seg, const float* __restrict__ chunk_wd, int nchunks,
                                                 const float* __restrict__ coef, int clip_mode, float cv, float lr, float mom,
                                                 float gscale, int nesterov, const float* __restrict__ state) {
  float inv = 1.f;
  if (AMP) {
    if (state[1] != 0.f) return;                     // non-finite gradients: the step is skipped (a fresh mirror16 stays fresh)
    inv = 1.0f / state[0];                           // the scale is a power of two: exact
  }
  const int t = threadIdx.x;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const ChunkSplit k = chunk_split(chunk_start[c], chunk_start[c + 1], t);
    const int seg = chunk_seg[c];
    const float cf = (clip_mode == SEG_CLIP_NORM && seg >= 0) ? coef[seg] : 1.f;
    const float wd = chunk_wd[c];
    if (k.i >= 0) {
      float mv = m[k.i];
      const float pn = sgd_elem<AMP>(p[k.i], g[k.i], mv, inv, gscale, clip_mode, cf, cv, wd, mom, lr, nesterov);
      m[k.i] = mv;
      p[k.i] = pn;
      if (mirror16) mirror16[k.i] = (h16_t)pn;
    }
    for (int64_t j = t; j < k.n4; j += 256) {
      const int64_t o = k.a + 4 * j;
      const f32x4 pv = *(const f32x4*)(p + o), gv = *(const f32x4*)(g + o);
      f32x4 mv = *(const f32x4*)(m + o), pn;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float mq = mv[q];
        pn[q] = sgd_elem<AMP>(pv[q], gv[q], mq, inv, gscale, clip_mode, cf, cv, wd, mom, lr, nesterov);
        mv[q] = mq;
      }
      *(f32x4*)(m + o) = mv;
      *(f32x4*)(p + o) = pn;
      if (mirror16) st4(mirror16 + o, 0, pn);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// out = (mask_y ? (y > 0 ? dy : 0) : dy) * (scale ? scale[c] : 1)     on [M][C]
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_scale_k(const T* __restrict__ dy, const T* __restrict__ y,
                                                      const float* __restrict__ scale, T* __restrict__ out,
                                                      size_t n4, int C4) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    f32x4 g = ld4(dy, i);
    if (y) {
      const f32x4 yy = ld4(y, i);
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = yy[e] > 0.f ? g[e] : 0.f;
    }
    if (scale) {
      const f32x4 s = ((const f32x4*)scale)[i % C4];
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] *= s[e];
    }
    st4(out, i, g);
  }
}

// y = a + b (used for gradient fan-in)
__global__ __launch_bounds__(256) void add_f32(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o,
                                             size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) o[i] = a[i] + b[i];
}

// ---------------------------------------------------------------------------------------------
// Element i of an [N][H][W][C] tensor as (n, h, w, c); C counts whatever one lane moves (quads or octets of channels).  I: the index type
// the caller's loop runs in (size_t; unsigned for the kernel whose host check keeps it below 2^31).
struct Nhwc {
  int c, w, h, n;
};
template <typename I>
__device__ __forceinline__ Nhwc nhwc_split(I i, int C, int W, int H) {
  Nhwc s;
  s.c = (int)(i % C); i /= C;
  s.w = (int)(i % W); i /= W;
  s.h = (int)(i % H); i /= H;
  s.n = (int)i;
  return s;
}

// ---------------------------------------------------------------------------------------------
// 3x3 stride-2 pad-1 max pool, NHWC (ResNet stem; frozen => forward only)
// ATen's running maximum (`val > maxval || isnan(val)`): a NaN in the window is the window's maximum - fmaxf would drop it - so the
// forwards and the backward below name the same pixel.  pool_beats is that condition, pool_max the maximum it gives.
__device__ __forceinline__ bool pool_beats(float m, float v) { return v > m || v != v; }
__device__ __forceinline__ float pool_max(float m, float v) { return pool_beats(m, v) ? v : m; }

// the window of output pixel (n, oh, ow) in (kh, kw) scan order: f(dh * 3 + dw, pixel index of (n, ih, iw)) for each tap that exists
template <typename F>
__device__ __forceinline__ void pool_window(int n, int oh, int ow, int H, int W, F&& f) {
#pragma unroll
  for (int dh = 0; dh < 3; ++dh) {
    const int ih = oh * 2 - 1 + dh;
    if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
    for (int dw = 0; dw < 3; ++dw) {
      const int iw = ow * 2 - 1 + dw;
      if ((unsigned)iw >= (unsigned)W) continue;
      f(dh * 3 + dw, (size_t)(n * H + ih) * W + iw);
    }
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void maxpool3x3s2_nhwc_k(const TI* __restrict__ x, TO* __restrict__ y, int N, int H,
                                                         int W, int C4, int OH, int OW) {
  const size_t total = (size_t)N * OH * OW * C4;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const Nhwc o = nhwc_split(i, C4, OW, OH);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    pool_window(o.n, o.h, o.w, H, W, [&](int, size_t px) {
      const f32x4 v = ld4(x, px * C4 + o.c);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = pool_max(m[e], v[e]);
    });
    st4(y, i, m);
  }
}

// Backward of the 3x3 stride-2 pad-1 max pool (a trainable stem, MODEL.BACKBONE.FREEZE_AT < 1) as a GATHER: input pixel (h, w) collects
// dpool of every window whose arg-max it is - ATen's rule: the FIRST maximum in (kh, kw) scan order (`val > maxval`), so ties (frequent
// after a ReLU) go to one pixel, deterministically; relu != 0 also applies the mask x > 0 of the ReLU in front of the pool.
template <typename TX, typename TG>
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_nhwc_k(const TX* __restrict__ x, const TG* __restrict__ dpool, TG* __restrict__ dx, int N,
                                                             int H, int W, int C4, int OH, int OW, int relu) {
  const size_t total = (size_t)N * H * W * C4;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const Nhwc s = nhwc_split(i, C4, W, H);
    const int c = s.c, w = s.w, h = s.h, n = s.n;
    const f32x4 mine = ld4(x, i);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    // windows that contain (h, w): 2 oh - 1 <= h <= 2 oh + 1, i.e. oh = h / 2 (and h / 2 + 1 for odd h)
    for (int oh = h / 2; oh <= (h + 1) / 2; ++oh) {
      if (oh >= OH) continue;
      for (int ow = w / 2; ow <= (w + 1) / 2; ++ow) {
        if (ow >= OW) continue;
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        // ATen starts from the window's first existing tap: that is where the gradient of a window full of -inf goes
        const int first = (oh == 0 ? 3 : 0) + (ow == 0 ? 1 : 0);
        int arg[4] = {first, first, first, first};
        pool_window(n, oh, ow, H, W, [&](int tap, size_t px) {
          const f32x4 v = ld4(x, px * C4 + c);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (pool_beats(best[e], v[e])) { best[e] = v[e]; arg[e] = tap; }
        });
        const int me = (h - (oh * 2 - 1)) * 3 + (w - (ow * 2 - 1));
        const f32x4 d = ld4(dpool, ((size_t)(n * OH + oh) * OW + ow) * C4 + c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (arg[e] == me) g[e] += d[e];
      }
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = mine[e] > 0.f ? g[e] : 0.f;
    }
    st4(dx, i, g);
  }
}

// bf16 -> bf16 form with 8 channels (16 bytes) per thread and 32-bit index arithmetic (max is exact: same result as the generic kernel)
__global__ __launch_bounds__(256) void maxpool3x3s2_nhwc_bf16x8_k(const h16_t* __restrict__ x, h16_t* __restrict__ y, int N, int H, int W,
                                                                int C8, int OH, int OW) {
  const unsigned total = (unsigned)N * OH * OW * C8;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const Nhwc s = nhwc_split(i, C8, OW, OH);
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
    pool_window(s.n, s.h, s.w, H, W, [&](int, size_t px) {
      const bf16x8_t v = ((const bf16x8_t*)x)[px * C8 + s.c];
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = pool_max(m[e], (float)v[e]);
    });
    bf16x8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (h16_t)m[e];
    ((bf16x8_t*)y)[i] = o;
  }
}

// FPN top-down: out[n,h,w,:] = lateral[n,h,w,:] + top[n,h/2,w/2,:]   (nearest x2)
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_add_nhwc_k(const T* __restrict__ lat, const T* __restrict__ top,
                                                           T* __restrict__ out, int N, int H, int W, int C4) {
  const size_t total = (size_t)N * H * W * C4;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int TH = H >> 1, TW = W >> 1;
  for (; i < total; i += stride) {
    const Nhwc s = nhwc_split(i, C4, W, H);
    const f32x4 a = ld4(lat, i);
    const f32x4 b = ld4(top, ((size_t)(s.n * TH + (s.h >> 1)) * TW + (s.w >> 1)) * C4 + s.c);
    st4(out, i, a + b);
  }
}

// backward of the nearest x2 upsample: dtop[n,h,w,:] (+)= sum of the 2x2 block of g
template <typename T>
__global__ __launch_bounds__(256) void downsample2x_sum_nhwc_k(const T* __restrict__ g, T* __restrict__ dtop, int N,
                                                             int TH, int TW, int C4, int accumulate) {
  const size_t total = (size_t)N * TH * TW * C4;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int H = TH * 2, W = TW * 2;
  for (; i < total; i += stride) {
    const Nhwc o = nhwc_split(i, C4, TW, TH);
    const size_t b = ((size_t)(o.n * H + 2 * o.h) * W + 2 * o.w) * C4 + o.c;
    f32x4 s = ld4(g, b) + ld4(g, b + C4) + ld4(g, b + (size_t)W * C4) + ld4(g, b + (size_t)W * C4 + C4);
    if (accumulate) s += ld4(dtop, i);
    st4(dtop, i, s);
  }
}

// dgrad of a stride-2 1x1 conv: the compact gradient [N][TH][TW][C] lands on the even pixels of [N][H][W][C], zeros elsewhere
// is s an even pixel?  off = where its value sits in the compact tensor (in the caller's units of C)
__device__ __forceinline__ bool interleave_src(const Nhwc& s, int TH, int TW, int C, size_t& off) {
  if ((s.h | s.w) & 1) return false;
  off = ((size_t)(s.n * TH + (s.h >> 1)) * TW + (s.w >> 1)) * C + s.c;
  return true;
}

// the ReLU mask of NV values as a lane mask (the layout of a mask_bits byte): bit q set = mk[q] > 0 = value q passes
template <int NV, typename V>
__device__ __forceinline__ unsigned keep_bits(const V& mk) {
  unsigned mb = 0;
#pragma unroll
  for (int q = 0; q < NV; ++q) mb |= ((float)mk[q] > 0.f ? 1u : 0u) << q;
  return mb;
}

template <typename T>
__global__ __launch_bounds__(256) void zero_interleave2x_nhwc_k(const T* __restrict__ src, const T* __restrict__ mask, T* __restrict__ dst,
                                                              int N, int H, int W, int TH, int TW, int C4) {
  const size_t total = (size_t)N * H * W * C4;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    size_t off;
    if (interleave_src(nhwc_split(i, C4, W, H), TH, TW, C4, off)) {
      v = ld4(src, off);
      if (mask) {  // optional [N][H][W][C]: the gradient flows into a ReLU output, masked where it is made
        const unsigned mb = keep_bits<4>(ld4(mask, i));
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = ((mb >> q) & 1u) ? v[q] : 0.f;
      }
    }
    st4(dst, i, v);
  }
}

// The same on 16-bit tensors, 8 channels per thread, with the two fusions the stride-2 bottlenecks' backward wants: `add` (optional,
// [N][H][W][C]) is summed in (the gradient another consumer of the same activation produced: no elementwise add pass in autograd) and
// the ReLU mask of the even pixels can come as a bit plane (mask_bits, see epilogue_rows).  `add` is NOT masked here: its producer did.
__global__ __launch_bounds__(256) void zero_interleave2x_add_h16_k(const h16_t* __restrict__ src, const h16_t* __restrict__ mask,
                                                                  const unsigned char* __restrict__ mask_bits,
                                                                  const h16_t* __restrict__ add, h16_t* __restrict__ dst, int N, int H,
                                                                  int W, int TH, int TW, int C8) {
  const size_t total = (size_t)N * H * W * C8;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = 0.f;
    size_t off;
    if (interleave_src(nhwc_split(i, C8, W, H), TH, TW, C8, off)) {
      const bf16x8_t sv = *(const bf16x8_t*)(src + off * 8);
      unsigned mb = 0xffu;
      if (mask_bits) mb = mask_bits[i];
      else if (mask) mb = keep_bits<8>(*(const bf16x8_t*)(mask + i * 8));
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = ((mb >> q) & 1u) ? (float)sv[q] : 0.f;
    }
    bf16x8_t o;
    if (add) {
      const bf16x8_t a = *(const bf16x8_t*)(add + i * 8);
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = (h16_t)(v[q] + (float)a[q]);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = (h16_t)v[q];
    }
    *(bf16x8_t*)(dst + i * 8) = o;
  }
}

// ---------------------------------------------------------------------------------------------
// Image normalisation + CHW -> padded NHWC4 (one_stage_detector.py:88-90 / D2 preprocess_image +
// ImageList.from_tensors): dst[n,h,w,c] = (src[c,h,w] - mean[c]) / std[c] for h<H,w<W, else 0.
struct PreNorm {
  float m[3], s[3];   // pixel mean and std per channel
};

// pixel (h, w) of the canvas from a [3][H][W] image: the normalised channels (a division, as the reference divides), zero beyond the image
template <typename T>
__device__ __forceinline__ f32x4 pre_pixel(const T* __restrict__ src, int H, int W, int h, int w, const PreNorm& nm) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (h < H && w < W) {
    const size_t o = (size_t)h * W + w, hw = (size_t)H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ((float)src[c * hw + o] - nm.m[c]) / nm.s[c];
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void preprocess_chw_to_nhwc4(const T* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                             int Hp, int Wp, PreNorm nm) {
  const size_t total = (size_t)Hp * Wp;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) ((f32x4*)dst)[i] = pre_pixel(src, H, W, (int)(i / Wp), (int)(i % Wp), nm);
}

// bf16 form for the MFMA stem, a batch in ONE launch (blockIdx.y = image): image n lands at pixel offset (3, 3) of slot n of a
// [N][Hp+6][Wp+8][4] bf16 buffer whose border the caller zeroed once (rows pitch Wp+8); the padded canvas beyond the image is written as
// zeros here.  A training step preprocesses 12 + 4 images and each launch, with its gap, sat at the very start of the step's critical path.
#define PRE_MAX_IMGS 32
struct PreBatch {
  const void* src[PRE_MAX_IMGS];
  int H[PRE_MAX_IMGS], W[PRE_MAX_IMGS];
};
template <typename T>
__global__ __launch_bounds__(256) void preprocess_batch_bf16pad(PreBatch b, h16_t* __restrict__ dst, int Hp, int Wp, PreNorm nm) {
  const int n = blockIdx.y, H = b.H[n], W = b.W[n];
  const T* __restrict__ src = (const T*)b.src[n];
  h16_t* out = dst + (size_t)n * (Hp + 6) * (Wp + 8) * 4;
  const size_t total = (size_t)Hp * Wp;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int h = (int)(i / Wp), w = (int)(i % Wp);
    st4(out, (size_t)(h + 3) * (Wp + 8) + (w + 3), pre_pixel(src, H, W, h, w, nm));
  }
}

// ---------------------------------------------------------------------------------------------
// FrozenBatchNorm fold for every BN layer at once (D2 FrozenBatchNorm2d.forward [D2-recall]):
//   scale = w * rsqrt(var + eps);  shift = b - mean * scale
__global__ void frozenbn_fold_f32(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ mean,
                                  const float* __restrict__ var, float* __restrict__ scale, float* __restrict__ shift,
                                  int n, float eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float s = w[i] * (1.0f / sqrtf(var[i] + eps));
    scale[i] = s;
    shift[i] = b[i] - mean[i] * s;
  }
}

// ---------------------------------------------------------------------------------------------
// GroupNorm(G groups) + ReLU (fcos/fcos.py:263-264, 283) over SEGMENTS of a [rows][C] matrix: a segment is
// one (image, FPN level) = a run of consecutive rows that shares statistics, so ONE launch normalises every
// level of a shared tower.  Work is cut into chunks of GN_ROWS rows that never straddle a segment.
//   stage 1  per chunk: partial sum / sumsq per group            -> part[chunk][G][2]
//   stage 2  per (segment, group): mean / rstd (double combine)   -> mean, rstd [seg][G]
//   stage 3  per chunk: y = relu((x - mean) * rstd * gamma + beta)
#define GN_ROWS 256
#define GN_MAX_SEG 160
struct GnSegs {
  int nseg;
  int rev;                     // apply passes walk the chunks LAST to FIRST: the pass before them (statistics / partial sums, or the conv
                               // that wrote x) ended on the tensor's tail, which is what the 256 MB Infinity Cache still holds
  int row0[GN_MAX_SEG + 1];    // first row of each segment (prefix sums)
  int chunk0[GN_MAX_SEG + 1];  // first chunk of each segment
};

__device__ __forceinline__ void gn_locate(const GnSegs& sg, int chunk, int& seg, int& r0, int& r1) {
  int s = 0;
  for (int i = 1; i < sg.nseg; ++i)
    if (chunk >= sg.chunk0[i]) s = i;
  seg = s;
  r0 = sg.row0[s] + (chunk - sg.chunk0[s]) * GN_ROWS;
  r1 = r0 + GN_ROWS;
  if (r1 > sg.row0[s + 1]) r1 = sg.row0[s + 1];
}

// The row walk of every per-chunk pass: row lane rl of RL takes rows r0 + rl, r0 + rl + RL, ... < r1 in ascending order (the sums are
// fixed-order fp32 reductions).  Four rows are loaded before the four are consumed, then a rolled tail: with one dependent load per
// iteration the passes were latency-bound (the statistics at 2.5 TB/s), and inside the step they share the chip with the weight-gradient
// stream and get a fraction of the CUs, so the bandwidth one CU sustains decides their time (gn_bwd_apply: 324 us per launch in the step
// against ~100 alone).  load(row) -> the row's operands, use(operands, row).
template <typename Load, typename Use>
__device__ __forceinline__ void gn_walk_rows(int r0, int r1, int rl, int RL, Load load, Use use) {
  int row = r0 + rl;
  for (; row + 3 * RL < r1; row += 4 * RL) {
    decltype(load(row)) v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = load(row + u * RL);
#pragma unroll
    for (int u = 0; u < 4; ++u) use(v[u], row + u * RL);
  }
  for (; row < r1; row += RL) use(load(row), row);
}

struct GnGX { f32x4 g, x; };   // one row's operands of the backward passes: the gradient and the GroupNorm's input

// The forward's value before the ReLU.  Its sign is the ReLU mask the backward recomputes from x, so the forward and the mask share this
// one expression (the library is built with -ffp-contract=off: the same roundings wherever it is inlined).
__device__ __forceinline__ float gn_affine(float x, float m, float r, float ga, float be) { return (x - m) * r * ga + be; }

// gg where the forward's ReLU passed, 0 elsewhere.  remask (beta given): the sign of gn_affine recomputed from x - one tensor read less
// in each backward pass; otherwise the sign of the stored y at quad o.
template <typename T>
__device__ __forceinline__ f32x4 gn_relu_mask(f32x4 gg, const f32x4 xx, float m, float r, const f32x4 ga, const f32x4 be, bool remask,
                                              int relu, const T* __restrict__ y, size_t o) {
  if (remask) {
#pragma unroll
    for (int e = 0; e < 4; ++e) gg[e] = gn_affine(xx[e], m, r, ga[e], be[e]) > 0.f ? gg[e] : 0.f;
  } else if (relu) {
    const f32x4 yy = ld4(y, o);
#pragma unroll
    for (int e = 0; e < 4; ++e) gg[e] = yy[e] > 0.f ? gg[e] : 0.f;
  }
  return gg;
}

// mean / rstd of cnt values with sum s and sum of squares q, in double (var clamped at 0)
__device__ __forceinline__ void gn_mean_rstd(double s, double q, double cnt, float eps, float* mean, float* rstd) {
  const double m = s / cnt;
  double var = q / cnt - m * m;
  if (var < 0.0) var = 0.0;
  *mean = (float)m;
  *rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// Rows [r0, r1) of a segment against a grid of (1 << shift)-row blocks: the whole blocks [b0, b1) and the edge rows in front of the
// first, [r0, h1), and behind the last, [t0, r1).  A segment inside one block has no whole block and only "head" rows.
struct GnSplit { int b0, b1, h1, t0; };
__device__ __forceinline__ GnSplit gn_split(int r0, int r1, int shift) {
  GnSplit s;
  s.b0 = (r0 + (1 << shift) - 1) >> shift;
  s.b1 = r1 >> shift;
  if (s.b1 < s.b0) s.b1 = s.b0;
  s.h1 = (s.b0 << shift) < r1 ? (s.b0 << shift) : r1;
  s.t0 = (s.b1 << shift) > s.h1 ? (s.b1 << shift) : s.h1;
  return s;
}

template <typename T>
__global__ __launch_bounds__(256) void gn_stats_partial(GnSegs sg, const T* __restrict__ x, float* __restrict__ part, int C, int G) {
  // thread t owns channel quad c4 = t % C4 and row lane t / C4 (deterministic reduction order)
  __shared__ float red[2][256];
  int seg, r0, r1;
  gn_locate(sg, blockIdx.x, seg, r0, r1);
  const int C4 = C >> 2;
  const int cpg4 = (C / G) >> 2;  // channel quads per group
  const int c4 = threadIdx.x % C4, rl = threadIdx.x / C4, RL = blockDim.x / C4;
  float s = 0.f, q = 0.f;
  gn_walk_rows(r0, r1, rl, RL, [&](int row) { return ld4(x, (size_t)row * C4 + c4); },
               [&](const f32x4 v, int) {
                 s += (v[0] + v[1]) + (v[2] + v[3]);
                 q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
               });
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = q;
  __syncthreads();
  float* out = part + (size_t)blockIdx.x * G * 2;
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < RL; ++k)
      for (int j = 0; j < cpg4; ++j) {
        a += red[0][k * C4 + g * cpg4 + j];
        b += red[1][k * C4 + g * cpg4 + j];
      }
    out[g * 2] = a;
    out[g * 2 + 1] = b;
  }
}

// one block per segment: thread (g = t % G, lane = t / G) sums every (256/G)-th chunk, LDS-combined in order
__global__ __launch_bounds__(256) void gn_stats_final(GnSegs sg, const float* __restrict__ part, float* __restrict__ mean,
                                                    float* __restrict__ rstd, int G, int cpg, float eps) {
  __shared__ double red[2][256];
  const int seg = blockIdx.x;
  const int g = threadIdx.x % G, ln = threadIdx.x / G, L = blockDim.x / G;
  double s = 0.0, q = 0.0;
  for (int c = sg.chunk0[seg] + ln; c < sg.chunk0[seg + 1]; c += L) {
    const float* p = part + ((size_t)c * G + g) * 2;
    s += (double)p[0];
    q += (double)p[1];
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = q;
  __syncthreads();
  if (ln == 0) {
    for (int k = 1; k < L; ++k) { s += red[0][k * G + g]; q += red[1][k * G + g]; }
    gn_mean_rstd(s, q, (double)(sg.row0[seg + 1] - sg.row0[seg]) * cpg, eps, &mean[seg * G + g], &rstd[seg * G + g]);
  }
}

// The same from the conv epilogue's partials (epilogue_rows gn_part: fp32 [ceil(rows / 32)][G][2] per 32-row block and group; 8 channels
// per group): one block per segment; the 32-row blocks that lie inside the segment come from `part32`, the (< 32) rows in front of
// the first and behind the last whole block - segments start at arbitrary rows - are summed here from x itself.  Thread (g = t % G,
// lane = t / G); double accumulation, fixed order.
__global__ __launch_bounds__(256) void gn_stats_final_p32(GnSegs sg, const float* __restrict__ part32, const h16_t* __restrict__ x,
                                                        float* __restrict__ mean, float* __restrict__ rstd, int G, int C, float eps) {
  // grid (segments, G / 8): a workgroup owns 8 groups of one segment, thread (group, lane of 32) walks every 32nd block
  __shared__ double red[2][256];
  const int seg = blockIdx.x;
  const int gl = threadIdx.x & 7, ln = threadIdx.x >> 3, L = 32;
  const int g = blockIdx.y * 8 + gl;
  const int r0 = sg.row0[seg], r1 = sg.row0[seg + 1];
  const GnSplit sp = gn_split(r0, r1, 5);
  double s = 0.0, q = 0.0;
  if (g < G) {
    for (int b = sp.b0 + ln; b < sp.b1; b += L) {
      const float2 p = *(const float2*)(part32 + ((size_t)b * G + g) * 2);
      s += (double)p.x;
      q += (double)p.y;
    }
    for (int pass = 0; pass < 2; ++pass) {
      const int e0 = pass == 0 ? r0 : sp.t0, e1 = pass == 0 ? sp.h1 : r1;
      for (int r = e0 + ln; r < e1; r += L) {
        const bf16x8_t v = *(const bf16x8_t*)(x + (size_t)r * C + g * 8);
        float fs = 0.f, fq = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float f = (float)v[e]; fs += f; fq += f * f; }
        s += (double)fs;
        q += (double)fq;
      }
    }
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = q;
  __syncthreads();
  if (ln == 0 && g < G) {
    for (int k = 1; k < L; ++k) { s += red[0][k * 8 + gl]; q += red[1][k * 8 + gl]; }
    gn_mean_rstd(s, q, (double)(r1 - r0) * 8.0, eps, &mean[seg * G + g], &rstd[seg * G + g]);
  }
}

__device__ __forceinline__ int gn_chunk_of_block(const GnSegs& sg) {
  const int nch = sg.chunk0[sg.nseg], b = (int)blockIdx.x;
  return (sg.rev && b < nch) ? nch - 1 - b : b;
}

template <typename T>
__global__ __launch_bounds__(256) void gn_apply_relu(GnSegs sg, const T* __restrict__ x, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, T* __restrict__ y, int C, int G, int relu,
                                                   unsigned* __restrict__ bits = nullptr) {
  // bits (optional; C % 32 == 0): the ReLU mask as a bit plane, bit (row * C + c) = y > 0 BEFORE the rounding to T (the reference's ReLU
  // follows an fp32 GroupNorm under autocast; a positive value below T's range still passes its gradient) - the plane the conv epilogues
  // read in place of a sign tensor (common.h EpiBits).  8 neighbouring lanes (32 channels of one row) assemble one 32-bit word.
  int seg, r0, r1;
  gn_locate(sg, gn_chunk_of_block(sg), seg, r0, r1);
  const int C4 = C >> 2, cpg = C / G;
  const int c4 = threadIdx.x % C4, rl = threadIdx.x / C4, RL = blockDim.x / C4;
  const int g = (c4 * 4) / cpg;
  const float m = mean[seg * G + g], r = rstd[seg * G + g];
  const f32x4 ga = ((const f32x4*)gamma)[c4], be = ((const f32x4*)beta)[c4];
  auto apply = [&](const f32x4 v, int row) {
    const size_t i = (size_t)row * C4 + c4;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = gn_affine(v[e], m, r, ga[e], be[e]);
      o[e] = relu ? fmaxf(t, 0.f) : t;
    }
    st4(y, i, o);
    if (bits) {   // (wave-uniform; the 8 lanes of a word run the same rows)
      unsigned b = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) b |= (o[e] > 0.f ? 1u : 0u) << e;   // the fp32 value's sign: the mask gn_bwd_partial / gn_bwd_apply recompute from x
      b <<= 4 * (threadIdx.x & 7);
      b |= __shfl_xor(b, 1, 64);
      b |= __shfl_xor(b, 2, 64);
      b |= __shfl_xor(b, 4, 64);
      if ((threadIdx.x & 7) == 0) bits[i >> 3] = b;
    }
  };
  // gn_walk_rows written out: through the helper the fp32 instantiation of this kernel takes 52 VGPRs instead of 50
  int row = r0 + rl;
  for (; row + 3 * RL < r1; row += 4 * RL) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ld4(x, (size_t)(row + u * RL) * C4 + c4);
#pragma unroll
    for (int u = 0; u < 4; ++u) apply(v[u], row + u * RL);
  }
  for (; row < r1; row += RL) apply(ld4(x, (size_t)row * C4 + c4), row);
}

// backward stage 1: per (chunk, c): A = sum g*xhat, B = sum g   with g = dy * (y > 0)
template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_partial(GnSegs sg, const T* __restrict__ dy, const T* __restrict__ y,
                                                    const T* __restrict__ x, const float* __restrict__ mean,
                                                    const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ part, int C, int G,
                                                    int relu) {
  __shared__ float red[2][256 * 4];
  int seg, r0, r1;
  gn_locate(sg, blockIdx.x, seg, r0, r1);
  const int C4 = C >> 2, cpg = C / G;
  const int c4 = threadIdx.x % C4, rl = threadIdx.x / C4, RL = blockDim.x / C4;
  const int g = (c4 * 4) / cpg;
  const float m = mean[seg * G + g], r = rstd[seg * G + g];
  f32x4 A = {0.f, 0.f, 0.f, 0.f}, B = {0.f, 0.f, 0.f, 0.f};
  const bool remask = relu && beta != nullptr;   // see gn_relu_mask
  f32x4 ga = {0.f, 0.f, 0.f, 0.f}, be = {0.f, 0.f, 0.f, 0.f};
  if (remask) { ga = ((const f32x4*)gamma)[c4]; be = ((const f32x4*)beta)[c4]; }
  gn_walk_rows(r0, r1, rl, RL,
               [&](int row) {
                 const size_t o = (size_t)row * C4 + c4;
                 return GnGX{ld4(dy, o), ld4(x, o)};
               },
               [&](const GnGX v, int row) {
                 const f32x4 gg = gn_relu_mask(v.g, v.x, m, r, ga, be, remask, relu, y, (size_t)row * C4 + c4);
#pragma unroll
                 for (int e = 0; e < 4; ++e) {
                   A[e] += gg[e] * ((v.x[e] - m) * r);
                   B[e] += gg[e];
                 }
               });
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[0][threadIdx.x * 4 + e] = A[e];
    red[1][threadIdx.x * 4 + e] = B[e];
  }
  __syncthreads();
  if (rl == 0) {
    for (int k = 1; k < RL; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        A[e] += red[0][(k * C4 + c4) * 4 + e];
        B[e] += red[1][(k * C4 + c4) * 4 + e];
      }
    float* out = part + ((size_t)blockIdx.x * C + c4 * 4) * 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      out[e * 2] = A[e];
      out[e * 2 + 1] = B[e];
    }
  }
}

// backward stage 2: AB[seg][c][2] = sum over the segment's chunks; s1 = sum_c gamma*A, s2 = sum_c gamma*B per (seg, group).
// Grid (segments, C / 64): a workgroup owns 64 channels (whole groups: cpg divides 64) of one segment, thread (channel, lane) walks
// every 4th chunk with four loads in flight and the four lanes are combined in a fixed order - one block per segment with one walk per
// channel was pure load latency (78 us per launch on the backward's critical path for 0.3 MB of partials).
// (the tail both stage-2 kernels end on: thread `lead` of channel c = blockIdx.y * 64 + cl holds that channel's segment sums sa = A, sb = B)
__device__ __forceinline__ void gn_bwd_reduce_tail(bool lead, float sa, float sb, int seg, int c, int cl, const float* __restrict__ gamma,
                                                   float* __restrict__ AB, float* __restrict__ s12, int C, int G) {
  __shared__ float sh[64][2];
  const int cpg = C / G;
  if (lead) {
    AB[((size_t)seg * C + c) * 2] = sa;
    AB[((size_t)seg * C + c) * 2 + 1] = sb;
    sh[cl][0] = sa * gamma[c];
    sh[cl][1] = sb * gamma[c];
  }
  __syncthreads();
  const int gpb = 64 / cpg;   // groups per block
  if ((int)threadIdx.x < gpb && blockIdx.y * 64 + threadIdx.x * cpg < C) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < cpg; ++k) {
      s1 += sh[threadIdx.x * cpg + k][0];
      s2 += sh[threadIdx.x * cpg + k][1];
    }
    const int g = blockIdx.y * gpb + threadIdx.x;
    s12[(seg * G + g) * 2] = s1;
    s12[(seg * G + g) * 2 + 1] = s2;
  }
}

__global__ __launch_bounds__(256) void gn_bwd_reduce(GnSegs sg, const float* __restrict__ part, const float* __restrict__ gamma,
                                                   float* __restrict__ AB, float* __restrict__ s12, int C, int G) {
  __shared__ float ra[256], rb[256];
  const int seg = blockIdx.x, cl = threadIdx.x & 63, ln = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  const int k0 = sg.chunk0[seg], k1 = sg.chunk0[seg + 1];
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    for (int k = k0 + ln; k < k1; k += 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k + 4 * q < k1) {
          const float2 v = *(const float2*)(part + ((size_t)(k + 4 * q) * C + c) * 2);
          a[q] += v.x;
          b[q] += v.y;
        }
    }
  }
  ra[threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
  rb[threadIdx.x] = (b[0] + b[1]) + (b[2] + b[3]);
  __syncthreads();
  const bool lead = ln == 0 && c < C;
  float sa = 0.f, sb = 0.f;
  if (lead) {
    sa = (ra[cl] + ra[cl + 64]) + (ra[cl + 128] + ra[cl + 192]);
    sb = (rb[cl] + rb[cl + 64]) + (rb[cl + 128] + rb[cl + 192]);
  }
  gn_bwd_reduce_tail(lead, sa, sb, seg, c, cl, gamma, AB, s12, C, G);
}

// The same from the dgrad epilogue's partials (common.h EpiBits::gnb_part: fp32 [ceil(rows / 64)][C][2] = {sum g, sum g * x} per 64-row
// block and channel, g = dy * mask as stored in `g`): A = sum g * xhat = rstd * (sum g x - mean * sum g), B = sum g.  The 64-row blocks
// that lie inside the segment come from part64; the rows in front of the first and behind the last whole block - segments start at
// arbitrary rows - are summed here from g and x.  Same grid and outputs as gn_bwd_reduce; double accumulation, fixed order.
__global__ __launch_bounds__(256) void gn_bwd_reduce_p64(GnSegs sg, const float* __restrict__ part64, const h16_t* __restrict__ gy,
                                                       const h16_t* __restrict__ x, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       float* __restrict__ AB, float* __restrict__ s12, int C, int G) {
  __shared__ double r0s[256], r1s[256];
  const int seg = blockIdx.x, cl = threadIdx.x & 63, ln = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl, cpg = C / G;
  const int r0 = sg.row0[seg], r1 = sg.row0[seg + 1];
  const GnSplit sp = gn_split(r0, r1, 6);
  double t0 = 0.0, t1 = 0.0;
  if (c < C) {
    int k = sp.b0 + ln;
    for (; k + 12 < sp.b1; k += 16) {   // four loads in flight per thread
      float2 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = *(const float2*)(part64 + ((size_t)(k + 4 * q) * C + c) * 2);
#pragma unroll
      for (int q = 0; q < 4; ++q) { t0 += (double)v[q].x; t1 += (double)v[q].y; }
    }
    for (; k < sp.b1; k += 4) {
      const float2 v = *(const float2*)(part64 + ((size_t)k * C + c) * 2);
      t0 += (double)v.x;
      t1 += (double)v.y;
    }
    for (int pass = 0; pass < 2; ++pass) {
      const int e0 = pass == 0 ? r0 : sp.t0, e1 = pass == 0 ? sp.h1 : r1;
      for (int r = e0 + ln; r < e1; r += 4) {
        const float gv = (float)gy[(size_t)r * C + c], xv = (float)x[(size_t)r * C + c];
        t0 += (double)gv;
        t1 += (double)(gv * xv);
      }
    }
  }
  r0s[threadIdx.x] = t0;
  r1s[threadIdx.x] = t1;
  __syncthreads();
  const bool lead = ln == 0 && c < C;
  float sa = 0.f, sb = 0.f;
  if (lead) {
    const double S0 = (r0s[cl] + r0s[cl + 64]) + (r0s[cl + 128] + r0s[cl + 192]);
    const double S1 = (r1s[cl] + r1s[cl + 64]) + (r1s[cl + 128] + r1s[cl + 192]);
    const int g = c / cpg;
    sa = (float)((double)rstd[seg * G + g] * (S1 - (double)mean[seg * G + g] * S0));
    sb = (float)S0;
  }
  gn_bwd_reduce_tail(lead, sa, sb, seg, c, cl, gamma, AB, s12, C, G);
}

// dgamma / dbeta += sums of AB over the segments.  Runs as the prologue of the first cdiv(C, 64) workgroups of gn_bwd_apply: a launch of
// its own sat, with its gap, between gn_bwd_reduce and gn_bwd_apply on the backward's critical path although only the optimizer reads it.
__device__ __forceinline__ void gn_bwd_param(const float* __restrict__ AB, float* __restrict__ dgamma, float* __restrict__ dbeta, int S, int C,
                                             int block) {
  // 64 channels x 4 segment parts per block (one thread per channel walked the S segments alone: 16 us of pure load latency);
  // the parts are combined in a fixed order
  __shared__ float ra[256], rb[256];
  const int c = block * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
  float a = 0.f, b = 0.f;
  if (c < C)
    for (int n = part; n < S; n += 4) {
      const float2 v = *(const float2*)(AB + ((size_t)n * C + c) * 2);
      a += v.x;
      b += v.y;
    }
  ra[threadIdx.x] = a;
  rb[threadIdx.x] = b;
  __syncthreads();
  if (part == 0 && c < C) {
    dgamma[c] += (ra[threadIdx.x] + ra[threadIdx.x + 64]) + (ra[threadIdx.x + 128] + ra[threadIdx.x + 192]);
    dbeta[c] += (rb[threadIdx.x] + rb[threadIdx.x + 64]) + (rb[threadIdx.x + 128] + rb[threadIdx.x + 192]);
  }
}

// backward stage 3: dx = rstd * (g*gamma - (s2 + xhat*s1)/cnt)
template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_apply(GnSegs sg, const T* __restrict__ dy, const T* __restrict__ y,
                                                  const T* __restrict__ x, const float* __restrict__ mean,
                                                  const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, const float* __restrict__ s12,
                                                  T* __restrict__ dx, int C, int G, int relu, const float* __restrict__ AB,
                                                  float* __restrict__ dgamma, float* __restrict__ dbeta, int param_blocks,
                                                  float* __restrict__ colpart) {
  if ((int)blockIdx.x < param_blocks) gn_bwd_param(AB, dgamma, dbeta, sg.nseg, C, blockIdx.x);
  int seg, r0, r1;
  const int chunk = gn_chunk_of_block(sg);
  gn_locate(sg, chunk, seg, r0, r1);
  const int C4 = C >> 2, cpg = C / G;
  const int c4 = threadIdx.x % C4, rl = threadIdx.x / C4, RL = blockDim.x / C4;
  const int g = (c4 * 4) / cpg;
  const float m = mean[seg * G + g], r = rstd[seg * G + g];
  const float s1 = s12[(seg * G + g) * 2], s2 = s12[(seg * G + g) * 2 + 1];
  const float inv_cnt = 1.0f / ((float)(sg.row0[seg + 1] - sg.row0[seg]) * cpg);
  const f32x4 ga = ((const f32x4*)gamma)[c4];
  const bool remask = relu && beta != nullptr;
  f32x4 be = {0.f, 0.f, 0.f, 0.f};
  if (remask) be = ((const f32x4*)beta)[c4];
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};   // colpart: column sums of the rows this thread writes
  auto apply = [&](const GnGX v, int row) {
    const size_t i = (size_t)row * C4 + c4;
    const f32x4 gg = gn_relu_mask(v.g, v.x, m, r, ga, be, remask, relu, y, i);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (v.x[e] - m) * r;
      o[e] = r * (gg[e] * ga[e] - (s2 + xh * s1) * inv_cnt);
    }
    st4(dx, i, o);
    if (colpart) {
#pragma unroll
      for (int e = 0; e < 4; ++e) csum[e] += (float)(T)o[e];   // the value as stored (rounded to T)
    }
  };
  gn_walk_rows(r0, r1, rl, RL,
               [&](int row) {
                 const size_t i = (size_t)row * C4 + c4;
                 return GnGX{ld4(dy, i), ld4(x, i)};
               },
               apply);
  if (colpart) {   // colpart[chunk][c] = column sums of this chunk of dx, row lanes combined in a fixed order
    __shared__ float cred[256 * 4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cred[threadIdx.x * 4 + e] = csum[e];
    __syncthreads();
    if (rl == 0 && chunk < sg.chunk0[sg.nseg]) {
      for (int k = 1; k < RL; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) csum[e] += cred[(k * C4 + c4) * 4 + e];
      *(f32x4*)(colpart + (size_t)chunk * C + c4 * 4) = csum;
    }
  }
}

static const bool g_gn_reverse = env_on("UTV2_GN_REVERSE");   // A/B switch, read once

// chunks of nseg consecutive segments (a chunk never straddles a segment)
static int64_t gn_chunks(int nseg, const int* seg_rows) {
  int64_t c = 0;
  for (int s = 0; s < nseg; ++s) c += (seg_rows[s] + GN_ROWS - 1) / GN_ROWS;
  return c;
}

static int gn_fill(GnSegs& sg, int nseg, const int* seg_rows) {
  sg.nseg = nseg;
  sg.rev = g_gn_reverse ? 1 : 0;
  int r = 0, c = 0;
  for (int s = 0; s < nseg; ++s) {
    sg.row0[s] = r;
    sg.chunk0[s] = c;
    r += seg_rows[s];
    c += (int)gn_chunks(1, seg_rows + s);
  }
  for (int s = nseg; s <= GN_MAX_SEG; ++s) { sg.row0[s] = r; sg.chunk0[s] = c; }
  return c;
}

static int gn_check(int nseg, int C, int G) {
  return !(nseg < 1 || nseg > GN_MAX_SEG || G < 1 || C < 4 || (C & 3) || ((C / G) & 3) || C / 4 > 256 || (256 % (C / 4)) || (256 % G) || (C % G) || (64 % (C / G)));
}

// What every GroupNorm entry does with its segment arguments: checks them (gn_check; seg_rows_host given, no negative row count) and
// fills sg.  -> the chunk count, or -1 for an argument error.
static int gn_prepare(int nseg, const int* seg_rows_host, int C, int G, GnSegs& sg) {
  if (!seg_rows_host || !gn_check(nseg, C, G)) return -1;
  for (int s = 0; s < nseg; ++s)
    if (seg_rows_host[s] < 0) return -1;
  return gn_fill(sg, nseg, seg_rows_host);
}

// The backward's workspace, as offsets in floats: part [chunks][C][2] (gn_bwd_partial's sums), AB [nseg][C][2], s12 [nseg][G][2] (C
// floats per segment are set aside for it).  utv2_groupnorm_seg_workspace_floats returns `floats`; the forward's part [chunks][G][2]
// fits in it.
struct GnBwdWs { int64_t part, AB, s12, floats; };
static GnBwdWs gn_bwd_ws(int64_t chunks, int nseg, int C) {
  GnBwdWs w;
  w.part = 0;
  w.AB = w.part + chunks * C * 2;
  w.s12 = w.AB + (int64_t)nseg * C * 2;
  w.floats = w.s12 + (int64_t)nseg * C;
  return w;
}

static inline int grid_for(size_t n, int block = 256, int cap = 256 * 16) {
  size_t b = (n + block - 1) / block;
  if (b > (size_t)cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

static inline bool is_act_dtype(int dtype) { return dtype == UTV2_F32 || dtype == UTV2_BF16; }

// the mean3_host / std3_host arguments of the three preprocess entries; false: one of them is missing
static bool pre_norm(const float* mean3_host, const float* std3_host, PreNorm& nm) {
  if (!mean3_host || !std3_host) return false;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean3_host[c];
    nm.s[c] = std3_host[c];
  }
  return true;
}

static void pre_batch_launch(int is_u8, dim3 grid, const PreBatch& b, void* dst16, int Hp, int Wp, const PreNorm& nm, hipStream_t stream) {
  if (is_u8) hipLaunchKernelGGL((preprocess_batch_bf16pad<unsigned char>), grid, dim3(256), 0, stream, b, (h16_t*)dst16, Hp, Wp, nm);
  else hipLaunchKernelGGL((preprocess_batch_bf16pad<float>), grid, dim3(256), 0, stream, b, (h16_t*)dst16, Hp, Wp, nm);
}

// stage 3 of both backward entries: dx, and dgamma / dbeta in the first cdiv(C, 64) workgroups (a workgroup past the last chunk finds no rows)
template <typename T>
static void gn_bwd_apply_launch(const GnSegs& sg, int chunks, const void* dy, const void* y, const void* x, const float* mean,
                                const float* rstd, const float* gamma, const float* beta, void* dx, float* dgamma, float* dbeta,
                                const float* AB, const float* s12, int C, int G, int relu, float* colpart, hipStream_t stream) {
  const int pb = cdiv(C, 64);
  hipLaunchKernelGGL(gn_bwd_apply<T>, dim3(chunks > pb ? chunks : pb), dim3(256), 0, stream, sg, (const T*)dy, (const T*)y, (const T*)x, mean,
                     rstd, gamma, beta, s12, (T*)dx, C, G, relu, AB, dgamma, dbeta, pb, colpart);
}

extern "C" {

// mirror16 (optional, 8-byte aligned): mirror16[i] = the library's 16-bit rounding of the new teacher[i]
int utv2_ema_axpby(float* teacher, const float* student, void* mirror16, int64_t n, double keep_rate, hipStream_t stream) {
  if (!teacher || !student || n < 0) return UTV2_EARG;
  if (n == 0) return UTV2_OK;
  if ((((uintptr_t)teacher | (uintptr_t)student) & 15) || ((uintptr_t)mirror16 & 7)) return UTV2_EARG;
  const float a = (float)(1.0 - keep_rate), b = (float)keep_rate;
  hipLaunchKernelGGL(ema_axpby_f32, dim3(grid_for((size_t)n / 4)), dim3(256), 0, stream, teacher, student, (size_t)n / 4,
                     (size_t)n, a, b, (h16_t*)mirror16);
  return utv2_launch_status();
}

// mirror16 (optional; here and in utv2_sgd_momentum_amp): mirror16[i] = the library's 16-bit rounding of the new param[i]
int utv2_sgd_momentum(float* param, float* grad, float* mom_buf, void* mirror16, int64_t n, float lr, float momentum, float weight_decay,
                      float grad_scale, int zero_grad, hipStream_t stream) {
  if (!param || !grad || !mom_buf || n < 0) return UTV2_EARG;
  if (n == 0) return UTV2_OK;
  hipLaunchKernelGGL(sgd_momentum_f32<false>, dim3(grid_for((size_t)n)), dim3(256), 0, stream, param, grad, mom_buf, (size_t)n, lr,
                     momentum, weight_decay, grad_scale, zero_grad, (const float*)nullptr, (h16_t*)mirror16);
  return utv2_launch_status();
}

// state: device fp32[3] = {loss scale, found_inf flag, growth tracker} (see amp_found_inf_f32)
int utv2_amp_found_inf(const float* grad, int64_t n, float* state, hipStream_t stream) {
  if (!grad || !state || n < 0 || ((uintptr_t)grad & 15)) return UTV2_EARG;
  if (n == 0) return UTV2_OK;
  hipLaunchKernelGGL(amp_found_inf_f32, dim3(grid_for((size_t)n / 4 + 1)), dim3(256), 0, stream, grad, (size_t)n / 4, (size_t)n, state);
  return utv2_launch_status();
}

int utv2_sgd_momentum_amp(float* param, const float* grad, float* mom_buf, void* mirror16, int64_t n, float lr, float momentum,
                          float weight_decay, float grad_scale, const float* state, hipStream_t stream) {
  if (!param || !grad || !mom_buf || !state || n < 0) return UTV2_EARG;
  if (n == 0) return UTV2_OK;
  // (the AMP instantiation never writes grad: zero_grad belongs to the other one)
  hipLaunchKernelGGL(sgd_momentum_f32<true>, dim3(grid_for((size_t)n)), dim3(256), 0, stream, param, const_cast<float*>(grad), mom_buf,
                     (size_t)n, lr, momentum, weight_decay, grad_scale, 0, state, (h16_t*)mirror16);
  return utv2_launch_status();
}

int utv2_amp_update_scale(float* state, float growth_factor, float backoff_factor, int growth_interval, hipStream_t stream) {
  if (!state || growth_interval < 1) return UTV2_EARG;
  hipLaunchKernelGGL(amp_update_scale_f32, dim3(1), dim3(64), 0, stream, state, growth_factor, backoff_factor, growth_interval);
  return utv2_launch_status();
}

// the work list (see seg_norm_partial) is device memory the caller built and checked; here only what the host can see is checked
int utv2_grad_clip_coef(const float* grad, const int64_t* chunk_start, const int32_t* chunk_seg, int nchunks, const int32_t* seg_chunks,
                        int nseg, int norm_kind, double clip_value, float grad_scale, const float* amp_state, double* partial, float* coef,
                        hipStream_t stream) {
  if (!grad || !chunk_start || !chunk_seg || !seg_chunks || !partial || !coef || nchunks < 0 || nseg < 0) return UTV2_EARG;
  if (norm_kind < SEG_NORM_L2 || norm_kind > SEG_NORM_INF || !(clip_value > 0.0) || ((uintptr_t)grad & 15)) return UTV2_EARG;
  if (nseg == 0 || nchunks == 0) return UTV2_OK;
  const int grid = nchunks < 2048 ? nchunks : 2048;
#define SEG_NORM_LAUNCH(KIND)                                                                                                      \
  hipLaunchKernelGGL(seg_norm_partial<KIND>, dim3(grid), dim3(256), 0, stream, grad, chunk_start, chunk_seg, nchunks, partial);    \
  hipLaunchKernelGGL(seg_clip_coef<KIND>, dim3(nseg), dim3(64), 0, stream, partial, seg_chunks, nseg, clip_value, grad_scale,      \
                     amp_state, coef)
  if (norm_kind == SEG_NORM_L2) { SEG_NORM_LAUNCH(SEG_NORM_L2); }
  else if (norm_kind == SEG_NORM_L1) { SEG_NORM_LAUNCH(SEG_NORM_L1); }
  else { SEG_NORM_LAUNCH(SEG_NORM_INF); }
#undef SEG_NORM_LAUNCH
  return utv2_launch_status();
}

int utv2_sgd_segmented(float* param, const float* grad, float* mom_buf, void* mirror16, const int64_t* chunk_start,
                       const int32_t* chunk_seg, const float* chunk_wd, int nchunks, const float* coef, int clip_mode, float clip_value,
                       float lr, float momentum, float grad_scale, int nesterov, const float* amp_state, hipStream_t stream) {
  if (!param || !grad || !mom_buf || !chunk_start || !chunk_seg || !chunk_wd || nchunks < 0) return UTV2_EARG;
  if (clip_mode < SEG_CLIP_NONE || clip_mode > SEG_CLIP_NORM || (clip_mode == SEG_CLIP_NORM && !coef) ||
      (clip_mode == SEG_CLIP_VALUE && !(clip_value > 0.f)))
    return UTV2_EARG;
  if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)mom_buf) & 15) || ((uintptr_t)mirror16 & 7)) return UTV2_EARG;
  if (nchunks == 0) return UTV2_OK;
  const int grid = nchunks < 2048 ? nchunks : 2048;
  if (amp_state)
    hipLaunchKernelGGL(sgd_seg_f32<true>, dim3(grid), dim3(256), 0, stream, param, grad, mom_buf, (h16_t*)mirror16, chunk_start, chunk_seg,
                       chunk_wd, nchunks, coef, clip_mode, clip_value, lr, momentum, grad_scale, nesterov, amp_state);
  else
    hipLaunchKernelGGL(sgd_seg_f32<false>, dim3(grid), dim3(256), 0, stream, param, grad, mom_buf, (h16_t*)mirror16, chunk_start, chunk_seg,
                       chunk_wd, nchunks, coef, clip_mode, clip_value, lr, momentum, grad_scale, nesterov, amp_state);
  return utv2_launch_status();
}

// out[M][C] = (y? relu-mask by y : 1) * dy * (scale? scale[c] : 1).  C % 4 == 0.  dy / y / out are `dtype`.
int utv2_relu_bwd_scale(const void* dy, const void* y, const float* scale, void* out, int64_t M, int C, int dtype,
                        hipStream_t stream) {
  if (!dy || !out || (C & 3) || !is_act_dtype(dtype)) return UTV2_EARG;
  const size_t n4 = (size_t)M * C / 4;
  if (n4 == 0) return UTV2_OK;
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(relu_bwd_scale_k<T>, dim3(grid_for(n4)), dim3(256), 0, stream, (const T*)dy, (const T*)y, scale, (T*)out, n4, C / 4);
  });
  return utv2_launch_status();
}

int utv2_add(const float* a, const float* b, float* out, int64_t n, hipStream_t stream) {
  if (!a || !b || !out) return UTV2_EARG;
  if (n == 0) return UTV2_OK;
  hipLaunchKernelGGL(add_f32, dim3(grid_for((size_t)n)), dim3(256), 0, stream, a, b, out, (size_t)n);
  return utv2_launch_status();
}

// x is `x_dtype`, y is `y_dtype` (the stem conv writes fp32, the bf16 activation pipeline starts here)
// dx[n][h][w][c] = sum of dpool over the windows whose (first) arg-max pixel (h, w) is; relu: times (x > 0).  x: the pool's INPUT
// (x_dtype), dpool / dx: g_dtype.
int utv2_maxpool3x3s2_bwd_nhwc(const void* x, int x_dtype, const void* dpool, void* dx, int g_dtype, int N, int H, int W, int C, int OH,
                               int OW, int relu, hipStream_t stream) {
  if (!x || !dpool || !dx || (C & 3) || !is_act_dtype(x_dtype) || !is_act_dtype(g_dtype)) return UTV2_EARG;
  if (x_dtype == UTV2_F32 && g_dtype == UTV2_BF16) return UTV2_EARG;   // no 16-bit gradient of an fp32 pool
  const dim3 g(grid_for((size_t)N * H * W * C / 4, 256, 1 << 16)), b(256);
  with_types(x_dtype, g_dtype, [&](auto tx, auto tg) {
    using TX = TAG_T(tx);
    using TG = TAG_T(tg);
    if constexpr (sizeof(TX) <= sizeof(TG))   // (the pair refused above is not instantiated)
      hipLaunchKernelGGL((maxpool3x3s2_bwd_nhwc_k<TX, TG>), g, b, 0, stream, (const TX*)x, (const TG*)dpool, (TG*)dx, N, H, W, C / 4, OH, OW, relu);
  });
  return utv2_launch_status();
}

int utv2_maxpool3x3s2_nhwc(const void* x, int x_dtype, void* y, int y_dtype, int N, int H, int W, int C, int OH, int OW,
                           hipStream_t stream) {
  if (!x || !y || (C & 3) || !is_act_dtype(x_dtype) || !is_act_dtype(y_dtype)) return UTV2_EARG;
  if (x_dtype == UTV2_BF16 && y_dtype == UTV2_F32) return UTV2_EARG;   // no fp32 pool of a 16-bit tensor
  const dim3 g(grid_for((size_t)N * OH * OW * C / 4, 256, 1 << 16)), b(256);
  if (x_dtype == UTV2_BF16 && y_dtype == UTV2_BF16 && (C & 7) == 0 && (size_t)N * OH * OW * C / 8 < (1ull << 31) &&
      (size_t)N * H * W < (1ull << 31))
    hipLaunchKernelGGL(maxpool3x3s2_nhwc_bf16x8_k, dim3(grid_for((size_t)N * OH * OW * C / 8, 256, 1 << 16)), b, 0, stream,
                       (const h16_t*)x, (h16_t*)y, N, H, W, C / 8, OH, OW);
  else
    with_types(x_dtype, y_dtype, [&](auto ti, auto to) {
      using TI = TAG_T(ti);
      using TO = TAG_T(to);
      if constexpr (sizeof(TI) >= sizeof(TO))   // (the pair refused above is not instantiated)
        hipLaunchKernelGGL((maxpool3x3s2_nhwc_k<TI, TO>), g, b, 0, stream, (const TI*)x, (TO*)y, N, H, W, C / 4, OH, OW);
    });
  return utv2_launch_status();
}

int utv2_upsample2x_add_nhwc(const void* lateral, const void* top, void* out, int N, int H, int W, int C, int dtype,
                             hipStream_t stream) {
  if (!lateral || !top || !out || (C & 3) || (H & 1) || (W & 1) || !is_act_dtype(dtype)) return UTV2_EARG;
  const dim3 g(grid_for((size_t)N * H * W * C / 4, 256, 1 << 16)), b(256);
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(upsample2x_add_nhwc_k<T>, g, b, 0, stream, (const T*)lateral, (const T*)top, (T*)out, N, H, W, C / 4);
  });
  return utv2_launch_status();
}

int utv2_downsample2x_sum_nhwc(const void* g, void* dtop, int N, int TH, int TW, int C, int accumulate, int dtype,
                               hipStream_t stream) {
  if (!g || !dtop || (C & 3) || !is_act_dtype(dtype)) return UTV2_EARG;
  const dim3 gr(grid_for((size_t)N * TH * TW * C / 4, 256, 1 << 16)), b(256);
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(downsample2x_sum_nhwc_k<T>, gr, b, 0, stream, (const T*)g, (T*)dtop, N, TH, TW, C / 4, accumulate);
  });
  return utv2_launch_status();
}

// dst[n,2i,2j,:] = src[n,i,j,:], zero elsewhere.  TH = (H+1)/2, TW = (W+1)/2.
int utv2_zero_interleave2x_nhwc(const void* src, const void* mask, void* dst, int N, int H, int W, int C, int dtype, hipStream_t stream) {
  if (!src || !dst || (C & 3) || !is_act_dtype(dtype)) return UTV2_EARG;
  const int TH = (H + 1) / 2, TW = (W + 1) / 2;
  const dim3 g(grid_for((size_t)N * H * W * C / 4, 256, 1 << 16)), b(256);
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(zero_interleave2x_nhwc_k<T>, g, b, 0, stream, (const T*)src, (const T*)mask, (T*)dst, N, H, W, TH, TW, C / 4);
  });
  return utv2_launch_status();
}

// 16-bit tensors, C % 8 == 0: dst = add + (even pixel ? (mask ? src : 0) : 0); mask as a 16-bit tensor OR as a bit plane (uint8 [N][H][W][C / 8]);
// mask, mask_bits and add are optional
int utv2_zero_interleave2x_add_nhwc(const void* src, const void* mask, const void* mask_bits, const void* add, void* dst, int N, int H, int W,
                                    int C, hipStream_t stream) {
  if (!src || !dst || (C & 7) || (mask && mask_bits)) return UTV2_EARG;
  const int TH = (H + 1) / 2, TW = (W + 1) / 2;
  const dim3 g(grid_for((size_t)N * H * W * C / 8, 256, 1 << 16)), b(256);
  hipLaunchKernelGGL(zero_interleave2x_add_h16_k, g, b, 0, stream, (const h16_t*)src, (const h16_t*)mask, (const unsigned char*)mask_bits,
                     (const h16_t*)add, (h16_t*)dst, N, H, W, TH, TW, C / 8);
  return utv2_launch_status();
}

// src: one image [3][H][W], uint8 (is_u8) or fp32; dst: one padded NHWC4 image [Hp][Wp][4]
int utv2_preprocess_image(const void* src, int is_u8, float* dst, int H, int W, int Hp, int Wp, const float* mean3_host,
                          const float* std3_host, hipStream_t stream) {
  PreNorm nm;
  if (!src || !dst || H > Hp || W > Wp || !pre_norm(mean3_host, std3_host, nm)) return UTV2_EARG;
  const int g = grid_for((size_t)Hp * Wp, 256, 1 << 16);
  if (is_u8)
    hipLaunchKernelGGL((preprocess_chw_to_nhwc4<unsigned char>), dim3(g), dim3(256), 0, stream, (const unsigned char*)src,
                       dst, H, W, Hp, Wp, nm);
  else
    hipLaunchKernelGGL((preprocess_chw_to_nhwc4<float>), dim3(g), dim3(256), 0, stream, (const float*)src, dst, H, W, Hp, Wp, nm);
  return utv2_launch_status();
}

// dst16: one image slot [Hp+6][Wp+8][4] bf16 of the zero-bordered stem input (see utv2_conv2d_stem_fwd_bf16): a batch of one
int utv2_preprocess_image_bf16pad(const void* src, int is_u8, void* dst16, int H, int W, int Hp, int Wp, const float* mean3_host,
                                  const float* std3_host, hipStream_t stream) {
  PreNorm nm;
  if (!src || !dst16 || H > Hp || W > Wp || !pre_norm(mean3_host, std3_host, nm)) return UTV2_EARG;
  PreBatch b = {};
  b.src[0] = src;
  b.H[0] = H;
  b.W[0] = W;
  pre_batch_launch(is_u8, dim3(grid_for((size_t)Hp * Wp, 256, 1 << 16), 1), b, dst16, Hp, Wp, nm, stream);
  return utv2_launch_status();
}

// N <= 32 images (device pointers in src_host, sizes in H_host / W_host) into the N slots of dst16 = bf16 [N][Hp+6][Wp+8][4]
int utv2_preprocess_images_bf16pad(const void* const* src_host, int is_u8, void* dst16, const int* H_host, const int* W_host, int N,
                                   int Hp, int Wp, const float* mean3_host, const float* std3_host, hipStream_t stream) {
  PreNorm nm;
  if (!src_host || !dst16 || !H_host || !W_host || !pre_norm(mean3_host, std3_host, nm) || N < 1 || N > PRE_MAX_IMGS) return UTV2_EARG;
  PreBatch b;
  for (int i = 0; i < PRE_MAX_IMGS; ++i) {
    b.src[i] = i < N ? src_host[i] : nullptr;
    b.H[i] = i < N ? H_host[i] : 0;
    b.W[i] = i < N ? W_host[i] : 0;
    if (i < N && (!src_host[i] || H_host[i] > Hp || W_host[i] > Wp || H_host[i] < 0 || W_host[i] < 0)) return UTV2_EARG;
  }
  pre_batch_launch(is_u8, dim3(grid_for((size_t)Hp * Wp, 256, 1 << 12), N), b, dst16, Hp, Wp, nm, stream);
  return utv2_launch_status();
}

int utv2_frozenbn_fold(const float* w, const float* b, const float* mean, const float* var, float* scale, float* shift,
                       int n, float eps, hipStream_t stream) {
  if (!w || !b || !mean || !var || !scale || !shift) return UTV2_EARG;
  if (n == 0) return UTV2_OK;
  hipLaunchKernelGGL(frozenbn_fold_f32, dim3(cdiv(n, 256)), dim3(256), 0, stream, w, b, mean, var, scale, shift, n, eps);
  return utv2_launch_status();
}

// Segmented API: seg_rows_host = host int[nseg] (rows of each (image, level) segment, consecutive in memory).
int64_t utv2_groupnorm_seg_workspace_floats(int nseg, const int* seg_rows_host, int C) {
  return gn_bwd_ws(gn_chunks(nseg, seg_rows_host), nseg, C).floats;
}

int64_t utv2_groupnorm_seg_chunks(int nseg, const int* seg_rows_host) { return gn_chunks(nseg, seg_rows_host); }

// x,y: [rows][C] of `dtype`; mean,rstd: fp32 [nseg][G] (saved for backward).  Statistics and arithmetic are fp32.
int utv2_groupnorm_relu_seg_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                float* ws, int nseg, const int* seg_rows_host, int C, int G, float eps, int relu, int dtype,
                                hipStream_t stream) {
  GnSegs sg;
  const int chunks = gn_prepare(nseg, seg_rows_host, C, G, sg);
  if (!x || !y || !mean || !rstd || !ws || chunks < 0 || !is_act_dtype(dtype)) return UTV2_EARG;
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(gn_stats_partial<T>, dim3(chunks), dim3(256), 0, stream, sg, (const T*)x, ws, C, G);
    hipLaunchKernelGGL(gn_stats_final, dim3(nseg), dim3(256), 0, stream, sg, (const float*)ws, mean, rstd, G, C / G, eps);
    hipLaunchKernelGGL(gn_apply_relu<T>, dim3(chunks), dim3(256), 0, stream, sg, (const T*)x, (const float*)mean, (const float*)rstd,
                       gamma, beta, (T*)y, C, G, relu);
  });
  return utv2_launch_status();
}

// bf16 x with 8 channels per group whose statistics partials the producing conv left in part32 (utv2_conv2d_ml_fwd_bf16_g gn_part:
// fp32 [ceil(rows / 32)][G][2]): statistics from the partials (+ the segment-edge rows read from x), then the apply pass - one tensor
// pass less than utv2_groupnorm_relu_seg_fwd.
// relu_bits (optional; C % 32 == 0): [rows * C / 8] bytes, bit (row * C + c) = y > 0 in fp32 (before the 16-bit rounding; the mask
// utv2_groupnorm_relu_seg_bwd recomputes from x when it is given beta) - the plane utv2_conv2d_ml_fwd_bf16_gnb reads
int utv2_groupnorm_relu_seg_fwd_p32(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                    const float* part32, int nseg, const int* seg_rows_host, int C, int G, float eps, int relu,
                                    void* relu_bits, hipStream_t stream) {
  GnSegs sg;
  const int chunks = gn_prepare(nseg, seg_rows_host, C, G, sg);
  if (!x || !y || !mean || !rstd || !part32 || chunks < 0 || C != 8 * G || (relu_bits && (C & 31))) return UTV2_EARG;
  hipLaunchKernelGGL(gn_stats_final_p32, dim3(nseg, cdiv(G, 8)), dim3(256), 0, stream, sg, part32, (const h16_t*)x, mean, rstd, G, C, eps);
  hipLaunchKernelGGL(gn_apply_relu<h16_t>, dim3(chunks), dim3(256), 0, stream, sg, (const h16_t*)x, (const float*)mean, (const float*)rstd,
                     gamma, beta, (h16_t*)y, C, G, relu, (unsigned*)relu_bits);
  return utv2_launch_status();
}

// dx written (`dtype`, like dy / y / x); dgamma/dbeta (fp32) accumulated (+=).  The ReLU mask comes from y, or - when
// beta is given - is recomputed from x (y may then be null).
// colsum_part (optional, fp32 [utv2_groupnorm_seg_chunks()][C]): per-chunk column sums of dx as stored - the partial sums of the bias
// gradient of the convolution that produced x (its dY is this dx), for free while dx is in registers.
int utv2_groupnorm_relu_seg_bwd(const void* dy, const void* y, const void* x, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, void* dx, float* dgamma, float* dbeta, float* ws,
                                int nseg, const int* seg_rows_host, int C, int G, int relu, int dtype, float* colsum_part,
                                hipStream_t stream) {
  GnSegs sg;
  const int chunks = gn_prepare(nseg, seg_rows_host, C, G, sg);
  if (!dy || !x || !dx || !ws || chunks < 0 || !is_act_dtype(dtype) || (relu && !y && !beta)) return UTV2_EARG;
  const GnBwdWs w = gn_bwd_ws(chunks, nseg, C);
  with_type(dtype, [&](auto t) {
    using T = TAG_T(t);
    hipLaunchKernelGGL(gn_bwd_partial<T>, dim3(chunks), dim3(256), 0, stream, sg, (const T*)dy, (const T*)y, (const T*)x, mean, rstd,
                       gamma, beta, ws + w.part, C, G, relu);
    hipLaunchKernelGGL(gn_bwd_reduce, dim3(nseg, cdiv(C, 64)), dim3(256), 0, stream, sg, (const float*)(ws + w.part), gamma, ws + w.AB,
                       ws + w.s12, C, G);
    gn_bwd_apply_launch<T>(sg, chunks, dy, y, x, mean, rstd, gamma, beta, dx, dgamma, dbeta, ws + w.AB, ws + w.s12, C, G, relu,
                           colsum_part, stream);
  });
  return utv2_launch_status();
}

// GroupNorm (+ ReLU) backward whose first reduction the producing dgrad's epilogue already made (utv2_conv2d_ml_fwd_bf16_gnb): g = the
// gradient with the ReLU mask applied (16-bit [rows][C]), part64 = that conv's gnb_part.  Two launches (segment sums; apply) instead of
// three, and one pass over g and x instead of two.  Outputs and ws as utv2_groupnorm_relu_seg_bwd (the `part` range of ws stays unused).
int utv2_groupnorm_seg_bwd_p64(const void* g, const void* x, const float* mean, const float* rstd, const float* gamma, void* dx,
                               float* dgamma, float* dbeta, float* ws, int nseg, const int* seg_rows_host, int C, int G,
                               const float* part64, float* colsum_part, hipStream_t stream) {
  GnSegs sg;
  const int chunks = gn_prepare(nseg, seg_rows_host, C, G, sg);
  if (!g || !x || !dx || !ws || !part64 || !mean || !rstd || !gamma || chunks < 0) return UTV2_EARG;
  const GnBwdWs w = gn_bwd_ws(chunks, nseg, C);
  hipLaunchKernelGGL(gn_bwd_reduce_p64, dim3(nseg, cdiv(C, 64)), dim3(256), 0, stream, sg, part64, (const h16_t*)g, (const h16_t*)x, mean,
                     rstd, gamma, ws + w.AB, ws + w.s12, C, G);
  gn_bwd_apply_launch<h16_t>(sg, chunks, g, nullptr, x, mean, rstd, gamma, nullptr, dx, dgamma, dbeta, ws + w.AB, ws + w.s12, C, G, 0,
                             colsum_part, stream);
  return utv2_launch_status();
}

}  // extern "C"
