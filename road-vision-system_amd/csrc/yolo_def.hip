// YOLOv8 / YOLOv5u / YOLO11 model definition + weight packer (restating the
// Ultralytics yolov8.yaml graph: Conv / C2f / SPPF / Detect(DFL), the
// yolov5.yaml graph of the "u" models: Conv k6 / C3 / SPPF under the same
// Detect, and the yolo11.yaml graph: C3k2 / C2PSA and a Detect whose class
// branch is depthwise-separable) and the C ABI entries that need no handle.
// Host code only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "yolo_def.h"

namespace rv {

static int make_div8(double x) { return (int)(std::ceil(x / 8.0) * 8); }

static bool variant_widths(int variant, Variant& v) {
  // yolov8.yaml scales: n [0.33, 0.25, 1024], s [0.33, 0.50, 1024],
  // m [0.67, 0.75, 768], l [1.00, 1.00, 512], x [1.00, 1.25, 512]
  static const double S[5][3] = {{0.33, 0.25, 1024}, {0.33, 0.50, 1024}, {0.67, 0.75, 768},
                                 {1.00, 1.00, 512},  {1.00, 1.25, 512}};
  // yolov5.yaml scales (variants 5..9): depth, width, max channels 1024
  static const double S5[5][3] = {{0.33, 0.25, 1024}, {0.33, 0.50, 1024}, {0.67, 0.75, 1024},
                                  {1.00, 1.00, 1024}, {1.33, 1.25, 1024}};
  // yolo11.yaml scales (variants 20..24): depth, width, max channels
  static const double S11[5][3] = {{0.50, 0.25, 1024}, {0.50, 0.50, 1024}, {0.50, 1.00, 512},
                                   {1.00, 1.00, 512},  {1.00, 1.50, 512}};
  if (!variant_known(variant)) return false;
  v.family = family_of(variant);
  if (v.family == kFamilyV11) {
    const int sc = variant - kV11Base;
    const double d = S11[sc][0], w = S11[sc][1], mc = S11[sc][2];
    auto ch = [&](int c) { return make_div8(std::min((double)c, mc) * w); };
    v.c1 = ch(64);
    v.c2 = ch(128);
    v.c3 = ch(256);
    v.c4 = ch(512);
    v.c5 = ch(1024);
    v.h12 = v.c4;  // model.13
    v.h15 = v.c3;  // model.16 -> Detect P3
    v.h18 = v.c4;  // model.19 -> Detect P4
    v.h21 = v.c5;  // model.22 -> Detect P5
    v.nb = v.nm = std::max((int)std::lround(2 * d), 1);
    v.c3k = sc >= 2;
    v.c2d = std::max(std::max(16, v.h15 / 4), v.reg * 4);
    v.c3d = std::max(v.h15, std::min(v.nc, 100));
    v.c3p = (v.c3d + 7) & ~7;
    v.hcs = (4 * v.reg + v.nc + 3) & ~3;
    return true;
  }
  if (v.family == kFamilyV5u) {
    const double d = S5[variant - 5][0], w = S5[variant - 5][1], mc = S5[variant - 5][2];
    auto ch = [&](int c) { return make_div8(std::min((double)c, mc) * w); };
    auto rep = [&](int n) { return std::max((int)std::lround(n * d), 1); };
    v.c1 = ch(64);
    v.c2 = ch(128);
    v.c3 = ch(256);
    v.c4 = ch(512);
    v.c5 = ch(1024);
    v.h12 = v.c3;  // model.14
    v.h15 = v.c3;  // model.17 -> Detect P3
    v.h18 = v.c4;  // model.20 -> Detect P4
    v.h21 = v.c5;  // model.23 -> Detect P5
    v.nb = rep(3);
    v.nm = rep(6);
    v.nx = rep(9);
    v.c2d = std::max(std::max(16, v.h15 / 4), v.reg * 4);
    v.c3d = std::max(v.h15, std::min(v.nc, 100));
    v.c3p = (v.c3d + 7) & ~7;
    v.hcs = (4 * v.reg + v.nc + 3) & ~3;
    return true;
  }
  const double d = S[variant][0], w = S[variant][1], mc = S[variant][2];
  auto ch = [&](int c) { return make_div8(std::min((double)c, mc) * w); };
  auto rep = [&](int n) { return std::max((int)std::lround(n * d), 1); };
  v.c1 = ch(64);
  v.c2 = ch(128);
  v.c3 = ch(256);
  v.c4 = ch(512);
  v.c5 = ch(1024);
  v.h12 = ch(512);
  v.h15 = ch(256);
  v.h18 = ch(512);
  v.h21 = ch(1024);
  v.nb = rep(3);
  v.nm = rep(6);
  v.c2d = std::max(std::max(16, v.h15 / 4), v.reg * 4);
  v.c3d = std::max(v.h15, std::min(v.nc, 100));
  v.c3p = (v.c3d + 7) & ~7;
  v.hcs = (4 * v.reg + v.nc + 3) & ~3;
  return true;
}

static size_t conv0q_bytes(int C0) { return 3 * (size_t)C0 * 64 + 20 * (size_t)C0; }
static size_t conv0q6_bytes(int C0) { return 9 * (size_t)C0 * 64 + 20 * (size_t)C0; }

int check_plan_args(int variant, int dtype, int nc) {
  RV_CHECK_ARG(variant_known(variant), "unknown variant %d", variant);
  RV_CHECK_ARG(dtype == RV_YOLO_DTYPE_BF16 || dtype == RV_YOLO_DTYPE_FP8, "unknown dtype %d", dtype);
  RV_CHECK_ARG(nc >= kMinClasses && nc <= kMaxClasses, "nc = %d outside the supported range %d..%d",
               nc, kMinClasses, kMaxClasses);
  RV_CHECK_ARG(dtype != RV_YOLO_DTYPE_FP8 || nc == 80,
               "fp8 plans support nc = 80 only (got nc = %d): the fp8 parity rests on the 80-class "
               "calibration; use the bf16 plan", nc);
  RV_CHECK_ARG(dtype != RV_YOLO_DTYPE_FP8 || family_of(variant) != kFamilyV5u,
               "YOLOv5u plans (variant %d) are bf16 only: there is no fp8 YOLOv5u plan", variant);
  RV_CHECK_ARG(dtype != RV_YOLO_DTYPE_FP8 || family_of(variant) != kFamilyV11,
               "YOLO11 plans (variant %d) are bf16 only: there is no fp8 YOLO11 plan", variant);
  return RV_OK;
}

// The Detect head (the same module in both families) on maps of widths chs
static void add_detect(ModelDef& m, const int (&chs)[3]) {
  const Variant& v = m.v;
  for (int i = 0; i < 3; ++i) {
    const std::string p = m.head + "cv2." + std::to_string(i);
    m.add(p + ".0", chs[i], v.c2d, 3, 1);
    m.add(p + ".1", v.c2d, v.c2d, 3, 1);
    m.add(p + ".2", v.c2d, 4 * v.reg, 1, 1, 0);
  }
  for (int i = 0; i < 3; ++i) {
    const std::string p = m.head + "cv3." + std::to_string(i);
    // the plan runs the branch c3p wide (c3d padded to 8: 16-byte feature
    // rows); the state_dict shapes and the packed layout keep c3d
    m.convs[m.add(p + ".0", chs[i], v.c3d, 3, 1)].pcout = v.c3p;
    ConvSpec& c1 = m.convs[m.add(p + ".1", v.c3d, v.c3d, 3, 1)];
    c1.pcin = c1.pcout = v.c3p;
    m.convs[m.add(p + ".2", v.c3d, v.nc, 1, 1, 0)].pcin = v.c3p;
  }
}

// yolov5.yaml (the "u" models): layer numbers as in the yaml; Upsample (11,
// 15) and Concat (12, 16, 19, 22) hold no weights
static void build_v5u(ModelDef& m) {
  const Variant& v = m.v;
  m.head = "model.24.";
  m.add("model.0", 3, v.c1, 6, 2);
  m.add("model.1", v.c1, v.c2, 3, 2);
  m.c3("model.2", v.c2, v.c2, v.nb);
  m.add("model.3", v.c2, v.c3, 3, 2);
  m.c3("model.4", v.c3, v.c3, v.nm);
  m.add("model.5", v.c3, v.c4, 3, 2);
  m.c3("model.6", v.c4, v.c4, v.nx);
  m.add("model.7", v.c4, v.c5, 3, 2);
  m.c3("model.8", v.c5, v.c5, v.nb);
  m.add("model.9.cv1", v.c5, v.c5 / 2, 1, 1);
  m.add("model.9.cv2", v.c5 / 2 * 4, v.c5, 1, 1);
  m.add("model.10", v.c5, v.c4, 1, 1);
  m.c3("model.13", 2 * v.c4, v.c4, v.nb);
  m.add("model.14", v.c4, v.c3, 1, 1);
  m.c3("model.17", 2 * v.c3, v.c3, v.nb);
  m.add("model.18", v.c3, v.c3, 3, 2);
  m.c3("model.20", 2 * v.c3, v.c4, v.nb);
  m.add("model.21", v.c4, v.c4, 3, 2);
  m.c3("model.23", 2 * v.c4, v.c5, v.nb);
  add_detect(m, {v.h15, v.h18, v.h21});
}

// yolo11.yaml: layer numbers as in the yaml; Upsample (11, 14) and Concat
// (12, 15, 18, 21) hold no weights.  The Detect class branch is
// DWConv 3x3 -> Conv 1x1, twice, then the plain 1x1 (the box branch is
// YOLOv8's); state_dict order: all of cv2, then all of cv3.
static void build_v11(ModelDef& m) {
  const Variant& v = m.v;
  m.head = "model.23.";
  m.add("model.0", 3, v.c1, 3, 2);
  m.add("model.1", v.c1, v.c2, 3, 2);
  m.c3k2("model.2", v.c2, v.c3, v.nb, v.c3k, 1);
  m.add("model.3", v.c3, v.c3, 3, 2);
  m.c3k2("model.4", v.c3, v.c4, v.nb, v.c3k, 1);
  m.add("model.5", v.c4, v.c4, 3, 2);
  m.c3k2("model.6", v.c4, v.c4, v.nb, true);
  m.add("model.7", v.c4, v.c5, 3, 2);
  m.c3k2("model.8", v.c5, v.c5, v.nb, true);
  m.add("model.9.cv1", v.c5, v.c5 / 2, 1, 1);
  m.add("model.9.cv2", v.c5 / 2 * 4, v.c5, 1, 1);
  m.c2psa("model.10", v.c5, v.nb);
  m.c3k2("model.13", v.c5 + v.c4, v.h12, v.nb, v.c3k);
  m.c3k2("model.16", v.h12 + v.c4, v.h15, v.nb, v.c3k);
  m.add("model.17", v.h15, v.h15, 3, 2);
  m.c3k2("model.19", v.h15 + v.h12, v.h18, v.nb, v.c3k);
  m.add("model.20", v.h18, v.h18, 3, 2);
  m.c3k2("model.22", v.h18 + v.c5, v.h21, v.nb, true);
  const int chs[3] = {v.h15, v.h18, v.h21};
  for (int i = 0; i < 3; ++i) {
    const std::string p = m.head + "cv2." + std::to_string(i);
    m.add(p + ".0", chs[i], v.c2d, 3, 1);
    m.add(p + ".1", v.c2d, v.c2d, 3, 1);
    m.add(p + ".2", v.c2d, 4 * v.reg, 1, 1, 0);
  }
  for (int i = 0; i < 3; ++i) {
    const std::string p = m.head + "cv3." + std::to_string(i);
    // as in add_detect: the plan runs the branch c3p wide behind its first 1x1
    m.add_dw(p + ".0.0", chs[i], 1);
    m.convs[m.add(p + ".0.1", chs[i], v.c3d, 1, 1)].pcout = v.c3p;
    ConvSpec& d1 = m.convs[m.add_dw(p + ".1.0", v.c3d, 1)];
    d1.pcin = d1.pcout = v.c3p;
    ConvSpec& c1 = m.convs[m.add(p + ".1.1", v.c3d, v.c3d, 1, 1)];
    c1.pcin = c1.pcout = v.c3p;
    m.convs[m.add(p + ".2", v.c3d, v.nc, 1, 1, 0)].pcin = v.c3p;
  }
}

// yolov8.yaml
static void build_v8(ModelDef& m) {
  const Variant& v = m.v;
  m.add("model.0", 3, v.c1, 3, 2);
  m.add("model.1", v.c1, v.c2, 3, 2);
  m.c2f("model.2", v.c2, v.c2, v.nb);
  m.add("model.3", v.c2, v.c3, 3, 2);
  m.c2f("model.4", v.c3, v.c3, v.nm);
  m.add("model.5", v.c3, v.c4, 3, 2);
  m.c2f("model.6", v.c4, v.c4, v.nm);
  m.add("model.7", v.c4, v.c5, 3, 2);
  m.c2f("model.8", v.c5, v.c5, v.nb);
  m.add("model.9.cv1", v.c5, v.c5 / 2, 1, 1);
  m.add("model.9.cv2", v.c5 / 2 * 4, v.c5, 1, 1);
  m.c2f("model.12", v.c5 + v.c4, v.h12, v.nb);
  m.c2f("model.15", v.h12 + v.c3, v.h15, v.nb);
  m.add("model.16", v.h15, v.h15, 3, 2);
  m.c2f("model.18", v.h15 + v.h12, v.h18, v.nb);
  m.add("model.19", v.h18, v.h18, 3, 2);
  m.c2f("model.21", v.h18 + v.c5, v.h21, v.nb);
  add_detect(m, {v.h15, v.h18, v.h21});
}

bool build_def(int variant, ModelDef& m, int dtype, int nc) {
  if (nc < kMinClasses || nc > kMaxClasses) return false;
  m.v.nc = nc;
  if (!variant_widths(variant, m.v)) return false;
  if (dtype != RV_YOLO_DTYPE_BF16 && dtype != RV_YOLO_DTYPE_FP8) return false;
  if (dtype == RV_YOLO_DTYPE_FP8 && m.v.family != kFamilyV8) return false;
  m.dtype = dtype;
  const Variant& v = m.v;
  if (v.family == kFamilyV11)
    build_v11(m);
  else if (v.family == kFamilyV5u)
    build_v5u(m);
  else
    build_v8(m);
  // packed layout: conv 0 keeps f32 OIHW (VALU conv), the rest bf16
  // [Cout_pad16][ky][kx][Cin_pad32]; biases f32 [Cout_pad16]; 256-B aligned.
  // Depthwise convs (YOLO11): bf16 [ky * 3 + kx][pcout], bias as the others.
  // fp8 plans: every conv but conv 0 and the Detect head's last 1x1 stage
  // (run inside the decode kernel on bf16 features) is fp8 e4m3
  // [Cout_pad16][ky][kx][Cin_pad64] + f32 per-cout scales [Cout_pad16].
  size_t off = 0;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  for (size_t i = 0; i < m.convs.size(); ++i) {
    ConvSpec& c = m.convs[i];
    c.f8 = dtype == RV_YOLO_DTYPE_FP8 && i > 0 &&
           !(c.name.compare(0, m.head.size(), m.head) == 0 && c.name.size() > 2 &&
             c.name.compare(c.name.size() - 2, 2, ".2") == 0);
    const int cop = (c.cout + 15) & ~15;
    const int cip = c.f8 ? (c.cin + 63) & ~63 : (c.cin + 31) & ~31;
    c.w_off = off;
    off = al(off + (i == 0 ? (size_t)c.cout * c.cin * c.k * c.k * 4
                    : c.groups > 1 ? (size_t)c.k * c.k * c.pcout * 2
                                   : (size_t)cop * c.k * c.k * cip * (c.f8 ? 1 : 2)));
    c.b_off = off;
    off = al(off + (size_t)cop * 4);
    if (c.f8) {
      c.ws_off = off;
      off = al(off + (size_t)cop * 4);
    }
  }
  m.q_off = off;
  m.q_bytes = v.family == kFamilyV5u ? conv0q6_bytes(m.convs[0].cout) : conv0q_bytes(m.convs[0].cout);
  return true;
}

size_t packed_bytes(const ModelDef& m) { return (m.q_off + m.q_bytes + 255) & ~(size_t)255; }

// Integer form of conv 0 (conv.h Conv0Q): per output channel o, the f64
// weights V[k] = w[o][2-ch][ky][kx] / 255 (RGB order and 1/255 folded in;
// k = 16 ky + 3 kx + ch over the window's BGR bytes, k % 16 >= 9 zero) as
// integers Q[k] = round(V[k] / s), s = max|V| / (127 * 2^16), split into
// balanced base-256 digits Q = 65536 D0 + 256 D1 + D2 (each in [-128, 127]).
// The kernel feeds x - 128 (the byte XOR 0x80) to one i8 MFMA per digit,
// starting each accumulator at 128 sum_k D_i[k], so it holds T_i = sum_k
// D_i[k] x[k] exactly (|T_i| <= 27 * 128 * 255 < 2^24: exact in f32 too);
// the value is s (65536 T0 + 256 T1 + T2) + b, f32 to 2^-23 of the weight
// scale with no offset cancellation.
static void pack_conv0q(const float* w, const float* b, int C0, uint8_t* dst) {
  int8_t* D = (int8_t*)dst;
  float* S = (float*)(dst + 3 * (size_t)C0 * 64);
  float* Bv = S + C0;
  int32_t* Cq = (int32_t*)(Bv + C0);
  for (int o = 0; o < C0; ++o) {
    double V[64] = {0.0}, M = 0.0;
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx)
        for (int ch = 0; ch < 3; ++ch) {
          const double v = (double)w[((o * 3 + (2 - ch)) * 3 + ky) * 3 + kx] / 255.0;
          V[16 * ky + 3 * kx + ch] = v;
          M = std::max(M, std::fabs(v));
        }
    const float s = M > 0.0 ? (float)(M / (127.0 * 65536.0)) : 1.0f;
    long long sd[3] = {0, 0, 0};
    for (int k = 0; k < 64; ++k) {
      const long long q = std::llround(V[k] / (double)s);
      const long long d2 = ((q + 128) & 255) - 128;
      const long long q1 = (q - d2) / 256;
      const long long d1 = ((q1 + 128) & 255) - 128;
      const long long d0 = (q1 - d1) / 256;
      const long long d[3] = {d0, d1, d2};
      for (int t = 0; t < 3; ++t) {
        D[((size_t)t * C0 + o) * 64 + k] = (int8_t)d[t];
        sd[t] += d[t];
      }
    }
    S[o] = s;
    Bv[o] = b[o];
    for (int t = 0; t < 3; ++t) Cq[t * C0 + o] = (int32_t)(128 * sd[t]);
  }
}

// Integer form of YOLOv5u's conv 0 (k6 s2 p2; conv.h Conv0Q, yolo_def.h for
// the layout): the rule of pack_conv0q over the 6 x 6 x 3 = 108 taps.  Window
// row ky is 18 contiguous BGR bytes j = 3 kx + ch; rows 2p and 2p + 1 share
// the 64-deep K block p (slots 32 (ky & 1) + j), every other slot zero.
// |T_i| <= 108 * 128 * 255 < 2^24, so the digit sums stay exact in i32 and f32.
static void pack_conv0q6(const float* w, const float* b, int C0, uint8_t* dst) {
  int8_t* D = (int8_t*)dst;
  float* S = (float*)(dst + 9 * (size_t)C0 * 64);
  float* Bv = S + C0;
  int32_t* Cq = (int32_t*)(Bv + C0);
  for (int o = 0; o < C0; ++o) {
    double V[192] = {0.0}, M = 0.0;
    for (int ky = 0; ky < 6; ++ky)
      for (int kx = 0; kx < 6; ++kx)
        for (int ch = 0; ch < 3; ++ch) {
          const double v = (double)w[((o * 3 + (2 - ch)) * 6 + ky) * 6 + kx] / 255.0;
          V[64 * (ky / 2) + 32 * (ky & 1) + 3 * kx + ch] = v;
          M = std::max(M, std::fabs(v));
        }
    const float s = M > 0.0 ? (float)(M / (127.0 * 65536.0)) : 1.0f;
    long long sd[3] = {0, 0, 0};
    for (int k = 0; k < 192; ++k) {
      const long long q = std::llround(V[k] / (double)s);
      const long long d2 = ((q + 128) & 255) - 128;
      const long long q1 = (q - d2) / 256;
      const long long d1 = ((q1 + 128) & 255) - 128;
      const long long d0 = (q1 - d1) / 256;
      const long long d[3] = {d0, d1, d2};
      for (int t = 0; t < 3; ++t) {
        D[((size_t)t * C0 + o) * 192 + k] = (int8_t)d[t];
        sd[t] += d[t];
      }
    }
    S[o] = s;
    Bv[o] = b[o];
    for (int t = 0; t < 3; ++t) Cq[t * C0 + o] = (int32_t)(128 * sd[t]);
  }
}

size_t flat_floats(const ModelDef& m) {
  size_t n = 0;
  for (const ConvSpec& c : m.convs) n += (size_t)c.cout * (c.cin / c.groups) * c.k * c.k + c.cout;
  return n;
}

// OCP e4m3fn code of x (|x| saturated to 448, round to nearest even,
// subnormals in 2^-9 steps) -- the rounding of v_cvt_pk_fp8_f32
static uint8_t host_f2e4m3(float x) {
  const uint8_t sgn = std::signbit(x) ? 0x80 : 0;
  double a = std::fabs((double)x);
  if (a > 448.0) a = 448.0;
  if (a < std::ldexp(1.0, -6)) return sgn | (uint8_t)std::nearbyint(a * 512.0);  // 8 -> 2^-6
  int e;
  const double m = std::frexp(a, &e);  // a = m 2^e, m in [0.5, 1)
  int q = (int)std::nearbyint((m * 2.0 - 1.0) * 8.0);
  int E = e - 1 + 7;
  if (q == 8) {
    q = 0;
    ++E;
  }
  return sgn | (uint8_t)((E << 3) | q);
}

// smallest power of two s with amax / s <= 448 (1 for amax == 0)
static float pow2_scale(double amax) {
  if (!(amax > 0.0)) return 1.0f;
  return (float)std::ldexp(1.0, (int)std::ceil(std::log2(amax / 448.0)));
}

static uint16_t host_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)(u >> 16);  // inf/nan
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

}  // namespace rv

using namespace rv;

extern "C" int rv_yolo_num_convs(int variant) { return rv_yolo_num_convs_nc(variant, 80); }

extern "C" int rv_yolo_num_convs_nc(int variant, int nc) {
  if (const int st = check_plan_args(variant, RV_YOLO_DTYPE_BF16, nc)) return st;
  ModelDef m;
  if (!build_def(variant, m, RV_YOLO_DTYPE_BF16, nc)) return RV_EINVAL;
  return (int)m.convs.size();
}

extern "C" int rv_yolo_conv_info(int variant, int idx, int* info, char* name, int name_cap) {
  return rv_yolo_conv_info_nc(variant, 80, idx, info, name, name_cap);
}

extern "C" int rv_yolo_conv_info_nc(int variant, int nc, int idx, int* info, char* name,
                                    int name_cap) {
  if (const int st = check_plan_args(variant, RV_YOLO_DTYPE_BF16, nc)) return st;
  ModelDef m;
  RV_CHECK_ARG(build_def(variant, m, RV_YOLO_DTYPE_BF16, nc), "unknown variant %d", variant);
  RV_CHECK_ARG(idx >= 0 && idx < (int)m.convs.size() && info, "bad conv index %d", idx);
  const ConvSpec& c = m.convs[idx];
  info[0] = c.cin;
  info[1] = c.cout;
  info[2] = c.k;
  info[3] = c.s;
  info[4] = c.act;
  if (name && name_cap > 0) {
    strncpy(name, c.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  return RV_OK;
}

extern "C" int rv_yolo_conv_groups(int variant, int nc, int idx) {
  if (const int st = check_plan_args(variant, RV_YOLO_DTYPE_BF16, nc)) return st;
  ModelDef m;
  RV_CHECK_ARG(build_def(variant, m, RV_YOLO_DTYPE_BF16, nc), "unknown variant %d", variant);
  RV_CHECK_ARG(idx >= 0 && idx < (int)m.convs.size(), "bad conv index %d", idx);
  return m.convs[idx].groups;
}

extern "C" size_t rv_yolo_flat_floats(int variant) { return rv_yolo_flat_floats_nc(variant, 80); }

extern "C" size_t rv_yolo_flat_floats_nc(int variant, int nc) {
  ModelDef m;
  if (check_plan_args(variant, RV_YOLO_DTYPE_BF16, nc) ||
      !build_def(variant, m, RV_YOLO_DTYPE_BF16, nc))
    return 0;
  return flat_floats(m);
}

extern "C" size_t rv_yolo_packed_bytes2(int variant, int dtype) {
  ModelDef m;
  if (!build_def(variant, m, dtype)) return 0;
  return packed_bytes(m);
}

extern "C" size_t rv_yolo_packed_bytes3(int variant, int dtype, int nc) {
  ModelDef m;
  if (check_plan_args(variant, dtype, nc) || !build_def(variant, m, dtype, nc)) return 0;
  return packed_bytes(m);
}

extern "C" size_t rv_yolo_packed_bytes(int variant) {
  return rv_yolo_packed_bytes2(variant, RV_YOLO_DTYPE_BF16);
}

extern "C" float rv_fp8_scale(double amax) { return pow2_scale(amax); }

extern "C" int rv_yolo_pack(int variant, const float* flat, size_t n, void* host_out,
                            size_t out_bytes) {
  return rv_yolo_pack2(variant, RV_YOLO_DTYPE_BF16, flat, n, host_out, out_bytes);
}

extern "C" int rv_yolo_pack2(int variant, int dtype, const float* flat, size_t n, void* host_out,
                             size_t out_bytes) {
  return rv_yolo_pack3(variant, dtype, 80, flat, n, host_out, out_bytes);
}

extern "C" int rv_yolo_pack3(int variant, int dtype, int nc, const float* flat, size_t n,
                             void* host_out, size_t out_bytes) {
  if (const int st = check_plan_args(variant, dtype, nc)) return st;
  ModelDef m;
  RV_CHECK_ARG(build_def(variant, m, dtype, nc), "unknown variant %d / dtype %d", variant, dtype);
  RV_CHECK_ARG(flat && host_out, "null pointer");
  RV_CHECK_ARG(n == flat_floats(m), "flat weights: got %zu floats, need %zu (variant %d, nc %d)", n,
               flat_floats(m), variant, nc);
  RV_CHECK_ARG(out_bytes >= packed_bytes(m), "packed buffer too small");
  uint8_t* out = (uint8_t*)host_out;
  memset(out, 0, packed_bytes(m));
  const float* p = flat;
  for (size_t i = 0; i < m.convs.size(); ++i) {
    const ConvSpec& c = m.convs[i];
    const size_t nw = (size_t)c.cout * (c.cin / c.groups) * c.k * c.k;
    const float* w = p;
    const float* b = p + nw;
    p += nw + c.cout;
    if (i == 0) {
      memcpy(out + c.w_off, w, nw * 4);
      if (m.v.family == kFamilyV5u)
        pack_conv0q6(w, b, c.cout, out + m.q_off);
      else
        pack_conv0q(w, b, c.cout, out + m.q_off);
    } else if (c.groups > 1) {
      uint16_t* dst = (uint16_t*)(out + c.w_off);
      for (int o = 0; o < c.cout; ++o)
        for (int t = 0; t < c.k * c.k; ++t) dst[(size_t)t * c.pcout + o] = host_f2bf(w[o * c.k * c.k + t]);
    } else if (c.f8) {
      // per output channel: scale = 2^ceil(log2(amax / 448)), codes RNE
      const int cip = (c.cin + 63) & ~63;
      const int kk = c.k * c.k;
      uint8_t* dst = out + c.w_off;
      float* wsc = (float*)(out + c.ws_off);
      for (int o = 0; o < c.cout; ++o) {
        double amax = 0.0;
        for (size_t j = 0; j < (size_t)c.cin * kk; ++j)
          amax = std::max(amax, (double)std::fabs(w[(size_t)o * c.cin * kk + j]));
        const float sc = pow2_scale(amax);
        wsc[o] = sc;
        for (int ky = 0; ky < c.k; ++ky)
          for (int kx = 0; kx < c.k; ++kx)
            for (int ci = 0; ci < c.cin; ++ci)
              dst[((size_t)o * kk + ky * c.k + kx) * cip + ci] =
                  host_f2e4m3(w[(((size_t)o * c.cin + ci) * c.k + ky) * c.k + kx] / sc);
      }
    } else {
      const int cip = (c.cin + 31) & ~31;
      uint16_t* dst = (uint16_t*)(out + c.w_off);
      for (int o = 0; o < c.cout; ++o)
        for (int ky = 0; ky < c.k; ++ky)
          for (int kx = 0; kx < c.k; ++kx)
            for (int ci = 0; ci < c.cin; ++ci)
              dst[((size_t)o * c.k * c.k + ky * c.k + kx) * cip + ci] =
                  host_f2bf(w[(((size_t)o * c.cin + ci) * c.k + ky) * c.k + kx]);
    }
    memcpy(out + c.b_off, b, (size_t)c.cout * 4);
  }
  return RV_OK;
}
