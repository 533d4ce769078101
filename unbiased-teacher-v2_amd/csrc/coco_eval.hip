// COCO box evaluation of a whole split on the device (evaluation/coco_eval_device.py), bit-identical to the host restatement
// evaluation/coco_eval.py (coco_box_ap / coco_box_eval).
//
// Layout: detections and ground truth are CSR by image in the evaluator's image order.  A (image, class) pair has the id
// pid = image * (K + 1) + class, where class K collects every class outside [0, K).  The host plumbing (ubteacher/hip.py:coco_box_eval)
// builds the orders with two stable sorts of the int64 keys written here:
//   key1 = pid << 32 | descending-score bits   ->  per (image, class) the detections by descending score, ties in output order
//                                                 (_evaluate_image: argsort(-scores, kind="mergesort")[:100])
//   key2 = class << 32 | descending-score bits ->  per class the detections of every image merged by descending score, ties in image
//                                                 order (coco_box_ap's concatenation + mergesort); pair ranks >= max_dets go to class K
// and the ground truth with one stable sort of pid (original order inside a pair).
//   match       one wave per (image, class) pair; lane a * 10 + t runs _evaluate_image's greedy loop for area range a and IoU
//               threshold t, in fp64 with _iou_matrix's operation order; writes the matched / ignored bit of every (detection, a, t)
//               and counts the non-ignored ground truth of every (class, area) with integer atomics
//   accumulate  one workgroup per (class, area, threshold) walks its class segment from the right in chunks: integer suffix counts
//               give the exact prefix counts tp / fp, pr = tp / max(tp + fp, eps) and rc = tp / npig in fp64, the reverse running max
//               of pr (the host's envelope loop), and every recall point is written by the one position that is its lower bound
// IEEE fp64 division; the build compiles with -ffp-contract=off, so nothing here is fused into an FMA.
#include "common.h"

#define COCO_T 10
#define COCO_R 101
#define COCO_A 4
#define COCO_LANES (COCO_T * COCO_A)
#define COCO_ACC_THREADS 256
#define COCO_ACC_PER 4
#define COCO_ACC_CHUNK (COCO_ACC_THREADS * COCO_ACC_PER)

struct CocoMatchConsts {
  double iou[COCO_T];
  double lo[COCO_A], hi[COCO_A];
};

struct CocoRecConsts {
  double rec[COCO_R];
};

// descending-score key bits: ascending order of the result = descending order of the score; -0 counts as +0 (numpy compares them equal)
__device__ __forceinline__ unsigned long long coco_desc_bits(float s) {
  if (s == 0.0f) s = 0.0f;
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (unsigned long long)(~u);
}

__global__ __launch_bounds__(256) void coco_pair_keys_kernel(const float* __restrict__ scores, const int* __restrict__ cls,
                                                             const long long* __restrict__ off, int K, long long* __restrict__ keys) {
  const int img = blockIdx.x;
  const long long b = off[img], e = off[img + 1];
  for (long long i = b + threadIdx.x; i < e; i += blockDim.x) {
    const int c = cls[i];
    const long long pid = (long long)img * (K + 1) + ((c >= 0 && c < K) ? c : K);
    keys[i] = (long long)(((unsigned long long)pid << 32) | (scores ? coco_desc_bits(scores[i]) : 0ull));
  }
}

// off[s] = first i with (keys[i] >> 32) >= s, s in [0, nseg]; segment ids above nseg count as nseg.  keys ascending.
__global__ __launch_bounds__(256) void coco_seg_offsets_kernel(const long long* __restrict__ keys, long long n, long long nseg,
                                                               long long* __restrict__ off) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (long long)gridDim.x * blockDim.x) {
    long long prev = -1, cur = nseg;
    if (i > 0) { prev = keys[i - 1] >> 32; if (prev > nseg) prev = nseg; }
    if (i < n) { cur = keys[i] >> 32; if (cur > nseg) cur = nseg; }
    for (long long s = prev + 1; s <= cur; ++s) off[s] = i;
  }
}

__global__ __launch_bounds__(256) void coco_rank_keys_kernel(const long long* __restrict__ key1, const long long* __restrict__ pair_off,
                                                             long long D, int K, int max_dets, long long* __restrict__ key2,
                                                             unsigned char* __restrict__ rank) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < D; p += (long long)gridDim.x * blockDim.x) {
    const long long k1 = key1[p];
    const long long pid = k1 >> 32;
    const int c = (int)(pid % (K + 1));
    const long long r = p - pair_off[pid];
    const bool keep = c < K && r < max_dets;
    key2[p] = keep ? (long long)(((unsigned long long)c << 32) | ((unsigned long long)k1 & 0xffffffffull)) : ((long long)K << 32);
    rank[p] = keep ? (unsigned char)r : (unsigned char)255;
  }
}

__device__ __forceinline__ double coco_box_area(const double* b) { return (b[2] - b[0]) * (b[3] - b[1]); }

// one 64-lane workgroup per (image, class < K) pair; taken[w * 40 + lane] = ground truth 32w..32w+31 of the pair taken at that lane's
// (area, threshold).  words * 32 >= the pair's ground-truth count (the launcher sizes it from the host-known bound).
__global__ __launch_bounds__(64) void coco_match_kernel(const float* __restrict__ dbox, const long long* __restrict__ dperm,
                                                        const long long* __restrict__ dpair_off, const double* __restrict__ gbox,
                                                        const unsigned char* __restrict__ gcrowd, const double* __restrict__ garea,
                                                        const long long* __restrict__ gperm, const long long* __restrict__ gpair_off,
                                                        int K, int max_dets, int words, CocoMatchConsts cs,
                                                        unsigned long long* __restrict__ mbits, unsigned long long* __restrict__ ibits,
                                                        int* __restrict__ npig) {
  extern __shared__ unsigned taken[];
  __shared__ double s_iou[COCO_T], s_lo[COCO_A], s_hi[COCO_A];
  const int lane = threadIdx.x;
#pragma unroll
  for (int i = 0; i < COCO_T; ++i)
    if (lane == i) s_iou[i] = cs.iou[i];
#pragma unroll
  for (int i = 0; i < COCO_A; ++i)
    if (lane == i) { s_lo[i] = cs.lo[i]; s_hi[i] = cs.hi[i]; }
  __syncthreads();
  const long long pair = blockIdx.x;
  const long long img = pair / K;
  const int c = (int)(pair % K);
  const long long pid = img * (K + 1) + c;
  const long long d0 = dpair_off[pid], g0 = gpair_off[pid];
  long long nd = dpair_off[pid + 1] - d0;
  if (nd > max_dets) nd = max_dets;
  const long long ng = gpair_off[pid + 1] - g0;
  if ((nd == 0 && ng == 0) || ng > (long long)words * 32) return;   // (the second: a launcher bound violated - never reached)
  const bool active = lane < COCO_LANES;
  const int a = active ? lane / COCO_T : 0, t = active ? lane % COCO_T : 0;
  const double lo = s_lo[a], hi = s_hi[a];
  const int nw = (int)((ng + 31) / 32);
  if (active) {
    int cnt = 0;
    for (long long g = 0; g < ng; ++g) {
      const long long gi = gperm[g0 + g];
      const double ar = garea ? garea[gi] : coco_box_area(gbox + 4 * gi);
      cnt += !(gcrowd[gi] || ar < lo || ar > hi);
    }
    if (t == 0 && cnt) atomicAdd(&npig[c * COCO_A + a], cnt);
    for (int w = 0; w < nw; ++w) taken[w * COCO_LANES + lane] = 0u;
  }
  const double thr0 = s_iou[t] < 1.0 - 1e-10 ? s_iou[t] : 1.0 - 1e-10;
  for (long long d = 0; d < nd; ++d) {
    const long long j = dperm[d0 + d];
    const double x0 = (double)dbox[4 * j], y0 = (double)dbox[4 * j + 1], x1 = (double)dbox[4 * j + 2], y1 = (double)dbox[4 * j + 3];
    const double ad = (x1 - x0) * (y1 - y0);
    bool matched = false, mign = false;
    if (active) {
      double best = thr0;
      long long m = -1;
      // the stable partition of _evaluate_image: the non-ignored ground truth first, then the ignored; the ignored are only reached
      // when no regular one matched (the host loop breaks at the first ignored box once it holds a regular match)
      for (int pass = 0; pass < 2 && m < 0; ++pass) {
        for (long long g = 0; g < ng; ++g) {
          const long long gi = gperm[g0 + g];
          const double* gb = gbox + 4 * gi;
          const bool crowd = gcrowd[gi] != 0;
          const double ar = garea ? garea[gi] : coco_box_area(gb);
          const bool ign = crowd || ar < lo || ar > hi;
          if ((int)ign != pass) continue;
          if (!crowd && ((taken[(g >> 5) * COCO_LANES + lane] >> (g & 31)) & 1u)) continue;
          const double ag = coco_box_area(gb);
          const double mx0 = x0 > gb[0] ? x0 : gb[0], mx1 = x1 < gb[2] ? x1 : gb[2];
          const double my0 = y0 > gb[1] ? y0 : gb[1], my1 = y1 < gb[3] ? y1 : gb[3];
          double iw = mx1 - mx0, ih = my1 - my0;
          iw = iw > 0.0 ? iw : 0.0;
          ih = ih > 0.0 ? ih : 0.0;
          const double inter = iw * ih;
          const double uni = crowd ? ad : (ad + ag) - inter;
          const double iou = inter / (uni > 1e-12 ? uni : 1e-12);
          if (iou < best) continue;
          best = iou;
          m = g;
          mign = ign;
        }
      }
      if (m >= 0) {
        matched = true;
        taken[(m >> 5) * COCO_LANES + lane] |= 1u << (m & 31);
      } else {
        mign = ad < lo || ad > hi;   // unmatched and outside the area range
      }
    }
    const unsigned long long mb = __ballot(matched), ib = __ballot(active && mign);
    if (lane == 0) { mbits[d0 + d] = mb; ibits[d0 + d] = ib; }
  }
}

// 256-thread block scans (4 waves): exclusive prefix of the per-thread values in thread order
__device__ __forceinline__ int coco_block_excl_sum(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int run = inc - v, tot = 0;
  for (int i = 0; i < COCO_ACC_THREADS / 64; ++i) {
    if (i < w) run += wsum[i];
    tot += wsum[i];
  }
  *total = tot;
  __syncthreads();
  return run;
}

__device__ __forceinline__ double coco_block_excl_max(double v, double* wmax, double* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(inc, o, 64);
    if (lane >= o && u > inc) inc = u;
  }
  double ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = -1.0;
  if (lane == 63) wmax[w] = inc;
  __syncthreads();
  double run = ex, tot = -1.0;
  for (int i = 0; i < COCO_ACC_THREADS / 64; ++i) {
    if (i < w && wmax[i] > run) run = wmax[i];
    if (wmax[i] > tot) tot = wmax[i];
  }
  *total = tot;
  __syncthreads();
  return run;
}

__device__ __forceinline__ int coco_block_sum(int v, int* wsum) {
  int tot;
  (void)coco_block_excl_sum(v, wsum, &tot);
  return tot;
}

// one workgroup per (class k, area a, threshold t): block index (k * 4 + a) * 10 + t
__global__ __launch_bounds__(COCO_ACC_THREADS) void coco_accumulate_kernel(const long long* __restrict__ perm2,
                                                                           const long long* __restrict__ cat_off,
                                                                           const unsigned char* __restrict__ rank,
                                                                           const unsigned long long* __restrict__ mbits,
                                                                           const unsigned long long* __restrict__ ibits,
                                                                           const int* __restrict__ npig, int K, CocoRecConsts rc_consts,
                                                                           double* __restrict__ precision, double* __restrict__ recall) {
  __shared__ double s_rec[COCO_R], s_q[COCO_R];
  __shared__ int wsum[COCO_ACC_THREADS / 64];
  __shared__ double wmax[COCO_ACC_THREADS / 64];
  const int t = blockIdx.x % COCO_T, a = (blockIdx.x / COCO_T) % COCO_A, k = blockIdx.x / (COCO_T * COCO_A);
  const int bit = a * COCO_T + t;
  const int np = npig[k * COCO_A + a];
#pragma unroll
  for (int i = 0; i < COCO_R; ++i)
    if ((int)threadIdx.x == i) { s_rec[i] = rc_consts.rec[i]; s_q[i] = np == 0 ? -1.0 : 0.0; }
  __syncthreads();
  double* rec_out = recall + (((size_t)t * K + k) * COCO_A + a) * 3;
  if (np > 0) {
    const long long s0 = cat_off[k], n = cat_off[k + 1] - s0;
    int tp_all = 0, fp_all = 0, tp1 = 0, tp10 = 0;
    for (long long q = threadIdx.x; q < n; q += COCO_ACC_THREADS) {
      const long long src = perm2[s0 + q];
      const unsigned long long mb = mbits[src] >> bit, ib = ibits[src] >> bit;
      const int tpb = (int)(mb & ~ib & 1ull), fpb = (int)(~mb & ~ib & 1ull);
      const int r = rank[src];
      tp_all += tpb;
      fp_all += fpb;
      tp1 += r < 1 ? tpb : 0;
      tp10 += r < 10 ? tpb : 0;
    }
    const int TP = coco_block_sum(tp_all, wsum), FP = coco_block_sum(fp_all, wsum);
    const int TP1 = coco_block_sum(tp1, wsum), TP10 = coco_block_sum(tp10, wsum);
    if (threadIdx.x == 0) {   // pycocotools: rc[-1] at maxDets 1 / 10 / 100 (0 without detections, = 0 / npig)
      rec_out[0] = (double)TP1 / (double)np;
      rec_out[1] = (double)TP10 / (double)np;
      rec_out[2] = (double)TP / (double)np;
    }
    // chunks from the right: thread i owns the positions c1 - 1 - (4 i + u), u = 0..3 (descending)
    int carry_tp = 0, carry_fp = 0;
    double carry_e = -1.0;
    const double eps = 2.220446049250313e-16;   // np.spacing(1)
    for (long long c1 = n; c1 > 0; c1 -= COCO_ACC_CHUNK) {
      int tpb[COCO_ACC_PER], fpb[COCO_ACC_PER];
      int ltp = 0, lfp = 0;
#pragma unroll
      for (int u = 0; u < COCO_ACC_PER; ++u) {
        const long long p = c1 - 1 - (threadIdx.x * COCO_ACC_PER + u);
        tpb[u] = fpb[u] = 0;
        if (p >= 0) {
          const long long src = perm2[s0 + p];
          const unsigned long long mb = mbits[src] >> bit, ib = ibits[src] >> bit;
          tpb[u] = (int)(mb & ~ib & 1ull);
          fpb[u] = (int)(~mb & ~ib & 1ull);
        }
        ltp += tpb[u];
        lfp += fpb[u];
      }
      int ctp, cfp;
      const int xtp = coco_block_excl_sum(ltp, wsum, &ctp);
      const int xfp = coco_block_excl_sum(lfp, wsum, &cfp);
      // suffix counts S(p) = sum over q >= p; the inclusive prefix count at p is then TOTAL - S(p) + bit(p)
      int stp = carry_tp + xtp, sfp = carry_fp + xfp;
      double pr[COCO_ACC_PER];
      int tpv[COCO_ACC_PER];
      double lmax = -1.0;
#pragma unroll
      for (int u = 0; u < COCO_ACC_PER; ++u) {
        stp += tpb[u];
        sfp += fpb[u];
        const int tp = TP - stp + tpb[u], fp = FP - sfp + fpb[u];
        tpv[u] = tp;
        const double den = (double)tp + (double)fp;
        pr[u] = (double)tp / (den > eps ? den : eps);
        const long long p = c1 - 1 - (threadIdx.x * COCO_ACC_PER + u);
        if (p < 0) pr[u] = -1.0;
        if (pr[u] > lmax) lmax = pr[u];
        pr[u] = lmax;                               // running max from the right inside the thread
      }
      double cmax;
      const double xmax = coco_block_excl_max(lmax, wmax, &cmax);
      const double base = xmax > carry_e ? xmax : carry_e;
#pragma unroll
      for (int u = 0; u < COCO_ACC_PER; ++u) {
        const long long p = c1 - 1 - (threadIdx.x * COCO_ACC_PER + u);
        if (p < 0 || (p > 0 && !tpb[u])) continue;    // rc only rises where a true positive is
        const double env = pr[u] > base ? pr[u] : base;
        const double rc = (double)tpv[u] / (double)np;
        int j = 0;
        if (p > 0) {                                 // first recall point above rc[p - 1]
          const double rcp = (double)(tpv[u] - tpb[u]) / (double)np;
          int lo = 0, hi = COCO_R;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_rec[mid] > rcp) hi = mid; else lo = mid + 1;
          }
          j = lo;
        }
        for (; j < COCO_R && s_rec[j] <= rc; ++j) s_q[j] = env;
      }
      carry_tp += ctp;
      carry_fp += cfp;
      if (cmax > carry_e) carry_e = cmax;
    }
    __syncthreads();
  } else if (threadIdx.x == 0) {
    rec_out[0] = rec_out[1] = rec_out[2] = -1.0;
  }
  for (int r = threadIdx.x; r < COCO_R; r += COCO_ACC_THREADS)
    precision[(((size_t)t * COCO_R + r) * K + k) * COCO_A + a] = s_q[r];
}

extern "C" {

int utv2_coco_pair_keys(const float* scores, const int* cls, const long long* off, int N, int K, long long* keys, hipStream_t stream) {
  if (!cls || !off || !keys || N <= 0 || K <= 0 || (long long)N * (K + 1) >= (1ll << 31)) return UTV2_EARG;
  hipLaunchKernelGGL(coco_pair_keys_kernel, dim3(N), dim3(256), 0, stream, scores, cls, off, K, keys);
  return utv2_launch_status();
}

int utv2_coco_seg_offsets(const long long* keys, int64_t n, int64_t nseg, long long* off, hipStream_t stream) {
  if (!off || n < 0 || nseg < 0 || (n > 0 && !keys)) return UTV2_EARG;
  int grid = cdiv(n + 1, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(coco_seg_offsets_kernel, dim3(grid), dim3(256), 0, stream, keys, (long long)n, (long long)nseg, off);
  return utv2_launch_status();
}

int utv2_coco_rank_keys(const long long* key1, const long long* pair_off, int64_t D, int K, int max_dets, long long* key2,
                        unsigned char* rank, hipStream_t stream) {
  if (D < 0 || K <= 0 || max_dets < 1 || max_dets > 254 || !pair_off) return UTV2_EARG;
  if (D == 0) return UTV2_OK;
  if (!key1 || !key2 || !rank) return UTV2_EARG;
  int grid = cdiv(D, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(coco_rank_keys_kernel, dim3(grid), dim3(256), 0, stream, key1, pair_off, (long long)D, K, max_dets, key2, rank);
  return utv2_launch_status();
}

static inline size_t coco_align(size_t n) { return (n + 255) & ~(size_t)255; }

int64_t utv2_coco_eval_workspace_bytes(int64_t D, int K) {
  return (int64_t)(2 * coco_align((size_t)(D > 0 ? D : 1) * sizeof(unsigned long long)) + coco_align((size_t)K * COCO_A * sizeof(int)));
}

#define COCO_MATCH_MAX_WORDS 400   // 40 lanes x 400 words x 4 B = 64000 B of LDS: up to 12800 ground-truth boxes per (image, class)

int utv2_coco_match(const float* dbox, const long long* dperm, const long long* dpair_off, const double* gbox, const unsigned char* gcrowd,
                    const double* garea, const long long* gperm, const long long* gpair_off, int N, int K, int64_t D, int max_dets,
                    int max_gt, const double* iou_thrs_host, const double* area_rng_host, void* ws, hipStream_t stream) {
  if (N <= 0 || K <= 0 || D < 0 || max_dets < 1 || max_gt < 0 || !dpair_off || !gpair_off || !iou_thrs_host || !area_rng_host || !ws)
    return UTV2_EARG;
  if ((long long)N * (K + 1) >= (1ll << 31)) return UTV2_EARG;
  if (D > 0 && (!dbox || !dperm)) return UTV2_EARG;
  if (max_gt > 0 && (!gbox || !gcrowd || !gperm)) return UTV2_EARG;
  const int words = max_gt > 0 ? (max_gt + 31) / 32 : 1;
  if (words > COCO_MATCH_MAX_WORDS) return UTV2_EARG;
  char* w = (char*)ws;
  unsigned long long* mbits = (unsigned long long*)w;
  w += coco_align((size_t)(D > 0 ? D : 1) * sizeof(unsigned long long));
  unsigned long long* ibits = (unsigned long long*)w;
  w += coco_align((size_t)(D > 0 ? D : 1) * sizeof(unsigned long long));
  int* npig = (int*)w;
  hipError_t e = hipMemsetAsync(npig, 0, (size_t)K * COCO_A * sizeof(int), stream);
  if (e != hipSuccess) return -(int)e;
  CocoMatchConsts cs;
  for (int i = 0; i < COCO_T; ++i) cs.iou[i] = iou_thrs_host[i];
  for (int i = 0; i < COCO_A; ++i) { cs.lo[i] = area_rng_host[2 * i]; cs.hi[i] = area_rng_host[2 * i + 1]; }
  const size_t lds = (size_t)words * COCO_LANES * sizeof(unsigned);
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)((long long)N * K)), dim3(64), lds, stream, dbox, dperm, dpair_off, gbox, gcrowd,
                     garea, gperm, gpair_off, K, max_dets, words, cs, mbits, ibits, npig);
  return utv2_launch_status();
}

int utv2_coco_accumulate(const long long* perm2, const long long* cat_off, const unsigned char* rank, int K, int64_t D,
                         const double* rec_thrs_host, const void* ws, double* precision, double* recall, hipStream_t stream) {
  if (K <= 0 || D < 0 || !cat_off || !rec_thrs_host || !ws || !precision || !recall) return UTV2_EARG;
  if (D > 0 && (!perm2 || !rank)) return UTV2_EARG;
  const char* w = (const char*)ws;
  const unsigned long long* mbits = (const unsigned long long*)w;
  w += coco_align((size_t)(D > 0 ? D : 1) * sizeof(unsigned long long));
  const unsigned long long* ibits = (const unsigned long long*)w;
  w += coco_align((size_t)(D > 0 ? D : 1) * sizeof(unsigned long long));
  const int* npig = (const int*)w;
  CocoRecConsts rc;
  for (int i = 0; i < COCO_R; ++i) rc.rec[i] = rec_thrs_host[i];
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3(K * COCO_A * COCO_T), dim3(COCO_ACC_THREADS), 0, stream, perm2, cat_off, rank, mbits, ibits,
                     npig, K, rc, precision, recall);
  return utv2_launch_status();
}

}  // extern "C"
