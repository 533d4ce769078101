// Test-time augmentation (TEST.AUG): the return trip of every view's detections into the original image's frame and the packing of
// all views into ONE candidate set for the merge NMS (Detectron2 GeneralizedRCNNWithTTA._inverse_augmented_boxes + the head of
// _merge_detections [D2-recall]; ubteacher/modeling/test_time_augmentation.py).
// One thread per (view, slot): a few loads, a dozen fp32 operations, one float4 store - latency-bound glue whose point is that the
// 18 views' results never visit the host.  No loops over device data, no atomics, every index < V * D.
// Builds with -ffp-contract=off: W - x and the two multiplications per coordinate must stay separate roundings.
#include "common.h"
#include "utv2.h"

struct TtaViews {
  const float* boxes[UTV2_TTA_MAX_VIEWS];          // [D][4] xyxy in the view's own pixel frame
  const float* scores[UTV2_TTA_MAX_VIEWS];         // [D]
  const int* classes[UTV2_TTA_MAX_VIEWS];          // [D]
  const unsigned char* valid[UTV2_TTA_MAX_VIEWS];  // [D]
};

// Transform.inverse() of the view's chain applied in reverse order, as TransformList.apply_box does it (the four corners through
// apply_coords, then min / max): un-flip, the view's resize back to the loader image, the leading resize back to the original.
__device__ __forceinline__ float4 tta_return_trip(float4 b, const float* __restrict__ t) {
  float xa = b.x, xb = b.z;
  if (t[UTV2_TTA_FLIP] != 0.f) {  // HFlipTransform.apply_coords: x <- W_view - x
    xa = t[UTV2_TTA_WVIEW] - xa;
    xb = t[UTV2_TTA_WVIEW] - xb;
  }
  float x1 = fminf(xa, xb), x2 = fmaxf(xa, xb);
  float y1 = fminf(b.y, b.w), y2 = fmaxf(b.y, b.w);
  // ResizeTransform.apply_coords per step: one multiplication by the step's own fp32 ratio (positive: the order is kept)
  x1 = x1 * t[UTV2_TTA_RX_VIEW]; x2 = x2 * t[UTV2_TTA_RX_VIEW];
  y1 = y1 * t[UTV2_TTA_RY_VIEW]; y2 = y2 * t[UTV2_TTA_RY_VIEW];
  x1 = x1 * t[UTV2_TTA_RX_LEAD]; x2 = x2 * t[UTV2_TTA_RX_LEAD];
  y1 = y1 * t[UTV2_TTA_RY_LEAD]; y2 = y2 * t[UTV2_TTA_RY_LEAD];
  // Boxes.clip to the original (height, width)
  const float h = t[UTV2_TTA_ORIG_H], w = t[UTV2_TTA_ORIG_W];
  return make_float4(fminf(fmaxf(x1, 0.f), w), fminf(fmaxf(y1, 0.f), h), fminf(fmaxf(x2, 0.f), w), fminf(fmaxf(y2, 0.f), h));
}

__global__ __launch_bounds__(256) void tta_collect_kernel(TtaViews in, const float* __restrict__ table, int view0, int nviews, int D,
                                                         float4* __restrict__ oboxes, float* __restrict__ oscores,
                                                         int* __restrict__ oclasses, unsigned char* __restrict__ ovalid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (view of this launch, slot)
  if (i >= nviews * D) return;
  const int v = i / D, d = i - v * D;
  const size_t o = (size_t)(view0 + v) * D + d;         // view-major slot of the packed set: < V * D
  const float s = in.scores[v][d];
  // fast_rcnn_inference_single_image(score_thresh=1e-8): strictly above, in fp32
  const bool ok = in.valid[v][d] != 0 && s > 1e-8f;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) b = tta_return_trip(((const float4*)in.boxes[v])[d], table + (size_t)(view0 + v) * UTV2_TTA_STRIDE);
  oboxes[o] = b;
  oscores[o] = ok ? s : 0.f;
  oclasses[o] = ok ? in.classes[v][d] : 0;
  ovalid[o] = ok ? 1 : 0;
}

extern "C" {

int utv2_tta_collect(const void* const* boxes_host, const void* const* scores_host, const void* const* classes_host,
                     const void* const* valid_host, const float* table, int V, int D, float* oboxes, float* oscores, int* oclasses,
                     unsigned char* ovalid, hipStream_t stream) {
  if (!boxes_host || !scores_host || !classes_host || !valid_host || !table || !oboxes || !oscores || !oclasses || !ovalid) return UTV2_EARG;
  if (V < 1 || D < 1 || (int64_t)V * D >= ((int64_t)1 << 31)) return UTV2_EARG;
  for (int v = 0; v < V; ++v)
    if (!boxes_host[v] || !scores_host[v] || !classes_host[v] || !valid_host[v] || ((uintptr_t)boxes_host[v] & 15)) return UTV2_EARG;
  if ((uintptr_t)oboxes & 15) return UTV2_EARG;
  // the views' pointers travel as kernel arguments, UTV2_TTA_MAX_VIEWS per launch (the default 9 sizes x flip = 18 views: one launch)
  for (int v0 = 0; v0 < V; v0 += UTV2_TTA_MAX_VIEWS) {
    const int nv = V - v0 < UTV2_TTA_MAX_VIEWS ? V - v0 : UTV2_TTA_MAX_VIEWS;
    TtaViews in;
    for (int v = 0; v < UTV2_TTA_MAX_VIEWS; ++v) {
      const int u = v0 + (v < nv ? v : 0);   // unused entries repeat a valid pointer; no thread reads them
      in.boxes[v] = (const float*)boxes_host[u];
      in.scores[v] = (const float*)scores_host[u];
      in.classes[v] = (const int*)classes_host[u];
      in.valid[v] = (const unsigned char*)valid_host[u];
    }
    hipLaunchKernelGGL(tta_collect_kernel, dim3(cdiv((int64_t)nv * D, 256)), dim3(256), 0, stream, in, table, v0, nv, D, (float4*)oboxes,
                       oscores, oclasses, ovalid);
  }
  return utv2_launch_status();
}

}  // extern "C"
