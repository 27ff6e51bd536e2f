// The IoU of class-aware NMS (reference csrc/cuda/ml_nms.cu:15-26): legacy "+1" widths, fp32, one operation at a time.  One statement for the
// bit-mask NMS (nms.hip) and the per-class NMS of the TTA merge (tta.hip): their keep flags are compared byte for byte.
// Other IoUs of the library are other operations and stay where they are: tta_iou1 (soft-NMS's comparisons, which treat NaN differently
// from fmaxf), ap_iou (fp64, crowds), atss_iou, the Flickr IoU.
#pragma once

// two corner quadruples with their precomputed +1 areas
__device__ __forceinline__ float box_iou_area(float ax1, float ay1, float ax2, float ay2, float sa, float bx1, float by1, float bx2, float by2,
                                              float sb) {
#pragma clang fp contract(off)
  const float left = fmaxf(ax1, bx1), right = fminf(ax2, bx2);
  const float top = fmaxf(ay1, by1), bottom = fminf(ay2, by2);
  const float w = fmaxf(right - left + 1.f, 0.f), h = fmaxf(bottom - top + 1.f, 0.f);
  const float inter = w * h;
  return inter / (sa + sb - inter);
}

// boxes a, b as (x1, y1, x2, y2) with their labels: 0 across labels
__device__ __forceinline__ float ml_iou(const float* a, int la, const float* b, int lb) {
#pragma clang fp contract(off)
  if (la != lb) return 0.f;
  const float sa = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
  const float sb = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
  return box_iou_area(a[0], a[1], a[2], a[3], sa, b[0], b[1], b[2], b[3], sb);
}
