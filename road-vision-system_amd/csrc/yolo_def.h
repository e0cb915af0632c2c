// YOLOv8 / YOLOv5u / YOLO11 model definition (yolo_def.hip): the canonical conv list
// of a variant (Ultralytics state_dict order, BN already fused into conv
// weight + bias) and the layout of its packed weight blob.  Host code only.
#pragma once
#include <string>
#include <vector>
#include "conv.h"

namespace rv {

struct ConvSpec {
  std::string name;
  int cin, cout, k, s, act;
  size_t w_off = 0, b_off = 0;  // byte offsets in the packed blob
  size_t ws_off = 0;            // fp8 convs: per-cout weight scales (f32)
  bool f8 = false;              // fp8 weights / inputs (RV_YOLO_DTYPE_FP8 plans)
  // widths the plan launches the conv with: cin / cout, but for the Detect
  // class branch of a plan whose c3d is no multiple of 8 (Variant::c3p).  The
  // packed rows / columns beyond cout / cin are zero, so the extra channels
  // are exact zeros and every logical channel keeps its sums.
  int pcin = 0, pcout = 0;
  // 1: dense; cin (= cout): depthwise (YOLO11's DWConv), state_dict weight
  // [cout][1][k][k], packed for dwconv.hip as bf16 [k * k][pcout] (tap-major,
  // zero beyond cout) instead of the dense layout
  int groups = 1;
};

struct Variant {
  int c1, c2, c3, c4, c5;   // backbone widths (P1..P5)
  int h12, h15, h18, h21;   // head widths
  int nb, nm;               // C2f repeats for "3" and "6"
  int nx = 0;               // YOLOv5u: C3 repeats for "9" (model.6)
  int family = 0;           // kFamilyV8 (C2f graph, yolov8.yaml) / kFamilyV5u (C3 graph, yolov5.yaml) /
                            // kFamilyV11 (C3k2 + C2PSA graph, yolo11.yaml)
  bool c3k = false;         // YOLO11 m, l, x: every C3k2 nests C3k blocks
  int c2d, c3d;             // Detect branch widths (the Ultralytics ones)
  int nc = 80, reg = 16;
  int c3p;                  // c3d as the plan runs it: padded to a multiple of 8
  int hcs;                  // f32 logits row stride: 4 * reg + nc padded to a multiple of 4
};

// Variants 0..4: YOLOv8 n, s, m, l, x; 5..9: YOLOv5u n, s, m, l, x (the
// anchor-free re-release of YOLOv5: yolov5.yaml's C3 graph under the YOLOv8
// Detect head).  For YOLOv5u h15 / h18 / h21 are the Detect inputs' widths
// (model.17 / 20 / 23: c3, c4, c5) and h12 is model.14's (c3).
// Variants 20..24: YOLO11 n, s, m, l, x (yolo11.yaml); 10..19 are no variant.
// There h12 / h15 / h18 / h21 are the widths of model.13 / 16 / 19 / 22 (c4,
// c3, c4, c5), nb is the repeat count of every C3k2 and of C2PSA.
constexpr int kFamilyV8 = 0, kFamilyV5u = 1, kFamilyV11 = 2;
constexpr int kV11Base = 20;
inline bool variant_known(int variant) {
  return (variant >= 0 && variant < 10) || (variant >= kV11Base && variant < kV11Base + 5);
}
inline int family_of(int variant) {
  return variant >= kV11Base ? kFamilyV11 : (variant >= 5 ? kFamilyV5u : kFamilyV8);
}

// class counts a plan supports: the NMS class mask is 4 x 32 bits wide
constexpr int kMinClasses = 1, kMaxClasses = 128;

struct ModelDef {
  Variant v;
  int dtype = 0;  // RV_YOLO_DTYPE_BF16 / RV_YOLO_DTYPE_FP8
  std::vector<ConvSpec> convs;
  // conv 0's integer form (the i8 MFMA conv0, conv.h Conv0Q), after every
  // conv's block.  YOLOv8 (k3): digits [3][C0][64] i8, scales [C0] f32,
  // biases [C0] f32, accumulator starts [3][C0] i32.  YOLOv5u (k6 s2 p2,
  // Conv0Q with three 64-deep K blocks per digit): digits [3][C0][3][64] i8
  // -- digit t, channel o, row pair p = ky / 2, K slot 32 (ky & 1) + 3 kx + ch
  // over the window row's 18 BGR bytes, slots 18..31 and 50..63 zero --, then
  // scales [C0] f32, biases [C0] f32, accumulator starts [3][C0] i32
  // (128 x the digit's sum over all 108 taps).
  size_t q_off = 0, q_bytes = 0;
  std::string head = "model.22.";  // the Detect module's state_dict prefix
  int add(const std::string& n, int ci, int co, int k, int s, int act = 1) {
    convs.push_back(ConvSpec{n, ci, co, k, s, act});
    convs.back().pcin = ci;
    convs.back().pcout = co;
    return (int)convs.size() - 1;
  }
  void c2f(const std::string& p, int c1, int c2, int n) {
    const int c = c2 / 2;
    add(p + ".cv1", c1, 2 * c, 1, 1);
    add(p + ".cv2", (2 + n) * c, c2, 1, 1);
    for (int i = 0; i < n; ++i) {
      add(p + ".m." + std::to_string(i) + ".cv1", c, c, 3, 1);
      add(p + ".m." + std::to_string(i) + ".cv2", c, c, 3, 1);
    }
  }
  // C3(c1, c2, n): cv1, cv2 (c1 -> c2 / 2, 1x1, both on the block's input),
  // cv3 (c2 -> c2, 1x1 on [bottleneck chain | cv2]), then the bottlenecks
  // (1x1 then 3x3 at width c2 / 2) -- the state_dict order
  void c3(const std::string& p, int c1, int c2, int n) {
    const int c = c2 / 2;
    add(p + ".cv1", c1, c, 1, 1);
    add(p + ".cv2", c1, c, 1, 1);
    add(p + ".cv3", 2 * c, c2, 1, 1);
    for (int i = 0; i < n; ++i) {
      add(p + ".m." + std::to_string(i) + ".cv1", c, c, 1, 1);
      add(p + ".m." + std::to_string(i) + ".cv2", c, c, 3, 1);
    }
  }
  // YOLO11 C3k2(c1, c2, n, c3k, e): a C2f (cv1, cv2 on [y0 | y1 | m.i ...])
  // whose m.i is Bottleneck(c, c) with hidden width c / 2 (3x3, 3x3), or with
  // c3k a C3k(c, c): cv1, cv2 (c -> c / 2, 1x1), cv3 (c -> c, 1x1), two
  // bottlenecks (3x3, 3x3) at width c / 2 -- the state_dict order
  void c3k2(const std::string& p, int c1, int c2, int n, bool c3k, int e4 = 2) {
    const int c = c2 * e4 / 4, h = c / 2;  // e = e4 / 4: 0.5 or 0.25
    add(p + ".cv1", c1, 2 * c, 1, 1);
    add(p + ".cv2", (2 + n) * c, c2, 1, 1);
    for (int i = 0; i < n; ++i) {
      const std::string q = p + ".m." + std::to_string(i);
      if (!c3k) {
        add(q + ".cv1", c, h, 3, 1);
        add(q + ".cv2", h, c, 3, 1);
        continue;
      }
      add(q + ".cv1", c, h, 1, 1);
      add(q + ".cv2", c, h, 1, 1);
      add(q + ".cv3", 2 * h, c, 1, 1);
      for (int j = 0; j < 2; ++j) {
        add(q + ".m." + std::to_string(j) + ".cv1", h, h, 3, 1);
        add(q + ".m." + std::to_string(j) + ".cv2", h, h, 3, 1);
      }
    }
  }
  int add_dw(const std::string& n, int c, int act) {  // DWConv(c, c, 3)
    const int i = add(n, c, c, 3, 1, act);
    convs[i].groups = c;
    return i;
  }
  // YOLO11 C2PSA(C, C, n): cv1 (C -> 2c, c = C / 2, split a | b), n PSA
  // blocks on b (attn.qkv c -> 2c, attn.proj c -> c, attn.pe depthwise 3x3,
  // all without activation; ffn.0 c -> 2c SiLU, ffn.1 2c -> c none), cv2
  void c2psa(const std::string& p, int C, int n) {
    const int c = C / 2;
    add(p + ".cv1", C, 2 * c, 1, 1);
    add(p + ".cv2", 2 * c, C, 1, 1);
    for (int i = 0; i < n; ++i) {
      const std::string q = p + ".m." + std::to_string(i);
      add(q + ".attn.qkv", c, 2 * c, 1, 1, 0);
      add(q + ".attn.proj", c, c, 1, 1, 0);
      add_dw(q + ".attn.pe", c, 0);
      add(q + ".ffn.0", c, 2 * c, 1, 1);
      add(q + ".ffn.1", 2 * c, c, 1, 1, 0);
    }
  }
  int find(const std::string& n) const {
    for (size_t i = 0; i < convs.size(); ++i)
      if (convs[i].name == n) return (int)i;
    return -1;
  }
};

// false: unknown variant / dtype, or nc outside [kMinClasses, kMaxClasses]
bool build_def(int variant, ModelDef& m, int dtype = RV_YOLO_DTYPE_BF16, int nc = 80);
// RV_OK, or RV_EINVAL with rv_last_error naming what is wrong with
// (variant, dtype, nc): the range of nc, fp8 with nc != 80 or a YOLOv5u /
// YOLO11 variant
int check_plan_args(int variant, int dtype, int nc);
size_t packed_bytes(const ModelDef& m);
size_t flat_floats(const ModelDef& m);

}  // namespace rv
