// What the Detect decode kernel (detect.hip) and the sparse box-branch kernel
// (head_box.hip) share: the by-value level table and the box arithmetic (DFL
// softmax expectation, dist2bbox, xywh2xyxy), so a candidate's box is the
// same bits whichever kernel computes it.
#pragma once
#include "conv.h"
#include "conv_common.h"

namespace rv {

struct HeadLevels {
  HeadLevel lv[4];
  int start[5];  // first anchor of each level
  int blk[5];    // first 64-anchor block of each level
  int nlv;
};

// The level table of a launch; false (and the error set) unless the levels
// have the decode's geometry: 1..4 levels, reg_max 16, one logits row stride
// (a multiple of 4)
inline bool head_levels(const HeadLevel* lv, int nlv, int reg_max, HeadLevels& h) {
  if (nlv < 1 || nlv > 4 || reg_max != 16) {
    set_error("detect decode: nlv=%d reg_max=%d unsupported", nlv, reg_max);
    return false;
  }
  h.nlv = nlv;
  h.start[0] = 0;
  h.blk[0] = 0;
  const int cs = lv[0].cs;
  for (int i = 0; i < nlv; ++i) {
    h.lv[i] = lv[i];
    h.start[i + 1] = h.start[i] + lv[i].H * lv[i].W;
    h.blk[i + 1] = h.blk[i] + ceil_div(lv[i].H * lv[i].W, 64);
    if (lv[i].cs != cs || cs % 4 != 0) {
      set_error("detect decode: head channel strides differ / not a multiple of 4");
      return false;
    }
  }
  return true;
}

// DFL side: softmax expectation over the REG bins at p (16-B aligned)
template <int REG>
__device__ __forceinline__ float dfl_side(const float* p) {
  float v[REG];
  float mx = -INFINITY;
  // ds_read_b128s
#pragma unroll
  for (int i = 0; i < REG; i += 4) {
    const f32x4 q = *(const f32x4*)(p + i);
    v[i] = q[0];
    v[i + 1] = q[1];
    v[i + 2] = q[2];
    v[i + 3] = q[3];
  }
#pragma unroll
  for (int i = 0; i < REG; ++i) mx = fmaxf(mx, v[i]);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < REG; ++i) {
    v[i] = __expf(v[i] - mx);
    sum += v[i];
  }
  // softmax probabilities by one reciprocal (v_rcp_f32, <= 1 ulp from
  // v / sum; the decode tolerance is 2e-3 px)
  const float rs = __builtin_amdgcn_rcpf(sum);
  float e = 0.f;
#pragma unroll
  for (int i = 0; i < REG; ++i) e += (float)i * (v[i] * rs);
  return e;
}

// dist2bbox (xywh) * stride of the anchor at map position (x, y) from its
// four DFL distances (left, top, right, bottom)
struct BoxXYWH {
  float cx, cy, w, h;
};
__device__ __forceinline__ BoxXYWH dist2bbox(float d0, float d1, float d2, float d3, int x, int y,
                                             float stride) {
  const float ax = (float)x + 0.5f, ay = (float)y + 0.5f;
  const float x1 = ax - d0, y1 = ay - d1, x2 = ax + d2, y2 = ay + d3;
  return BoxXYWH{(x1 + x2) / 2.0f * stride, (y1 + y2) / 2.0f * stride, (x2 - x1) * stride,
                 (y2 - y1) * stride};
}
// xywh2xyxy: the candidate row's x1, y1, x2, y2
__device__ __forceinline__ f32x4 xywh2xyxy(const BoxXYWH& b) {
  const float hw = b.w / 2.0f, hh = b.h / 2.0f;
  return f32x4{b.cx - hw, b.cy - hh, b.cx + hw, b.cy + hh};
}

}  // namespace rv
