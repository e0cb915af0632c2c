// YOLOv8 / YOLOv5u / YOLO11 model plan + forward (the detector backend behind
// src/detect/yolo_ultralytics.py:7-53; the model definition and the weight
// packer are in yolo_def.hip).
//
// The plan is built natively here: the activation-buffer layout in one
// caller-owned HBM workspace and the launch sequence of a forward.  Concats
// are free (producers write into channel slices of the concat buffers);
// nearest-2x upsamples are extra epilogue writes of the producing conv.
#include <cmath>
#include <cstring>
#include "yolo_model.h"

namespace rv {

// The Detect head's buffers (both families) and the anchor count
static void plan_heads(Model& M) {
  const Variant& v = M.def.v;
  for (int i = 0; i < 3; ++i) {
    const std::string l = std::to_string(i);
    // class branch c3p wide, logits rows hcs floats: the padding channels
    // (none in the 80-class plans) hold exact zeros
    M.DA[i] = M.newbuf("DA" + l, 3 + i, v.c2d + v.c3p);
    M.DB[i] = M.newbuf("DB" + l, 3 + i, v.c2d + v.c3p, false, true);  // bf16: the decode's features
    M.HD[i] = M.newbuf("HD" + l, 3 + i, v.hcs, true);
  }
  M.nA = M.map_h[3] * M.map_w[3] + M.map_h[4] * M.map_w[4] + M.map_h[5] * M.map_w[5];
}

// YOLOv5u (yolov5.yaml): one buffer per activation.  A C3 block's concat
// buffer holds [last bottleneck's output | cv2's output] (2c wide, cv3's
// input); t_i = "prefix.t.i" is the input of bottleneck i (t_0 = cv1's
// output) and "prefix.m.i" the output of its 1x1 conv.  CAT17 / CAT20 are the
// yaml's concats 19 = [model.18 | model.14] and 22 = [model.21 | model.10];
// concats 12 and 16 (behind the two Upsamples) are never materialised.
static void plan_v5u(Model& M) {
  const Variant& v = M.def.v;
  M.CAT14 = M.CAT11 = -1;
  M.X0 = M.newbuf("X0", 1, v.c1);
  M.X1 = M.newbuf("X1", 2, v.c2);
  M.C2 = M.newbuf("C2", 2, v.c2);
  M.X2 = M.newbuf("X2", 2, v.c2);
  M.X3 = M.newbuf("X3", 3, v.c3);
  M.C4 = M.newbuf("C4", 3, v.c3);
  M.X4 = M.newbuf("X4", 3, v.c3);
  M.X5 = M.newbuf("X5", 4, v.c4);
  M.C6 = M.newbuf("C6", 4, v.c4);
  M.X6 = M.newbuf("X6", 4, v.c4);
  M.X7 = M.newbuf("X7", 5, v.c5);
  M.C8 = M.newbuf("C8", 5, v.c5);
  M.X8 = M.newbuf("X8", 5, v.c5);
  M.SP = M.newbuf("SP", 5, 4 * (v.c5 / 2));
  M.X9 = M.newbuf("X9", 5, v.c5);
  M.CAT20 = M.newbuf("CAT20", 5, 2 * v.c4);
  M.C12 = M.newbuf("C12", 4, v.c4);
  M.X13 = M.newbuf("X13", 4, v.c4);
  M.CAT17 = M.newbuf("CAT17", 4, 2 * v.c3);
  M.C15 = M.newbuf("C15", 3, v.c3);
  M.X15 = M.newbuf("X15", 3, v.c3);
  M.C18 = M.newbuf("C18", 4, v.c4);
  M.X18 = M.newbuf("X18", 4, v.c4);
  M.C21 = M.newbuf("C21", 5, v.c5);
  M.X21 = M.newbuf("X21", 5, v.c5);
  plan_heads(M);
  struct C3Def {
    const char* p;
    int level, c2, n;
  };
  const C3Def cs[] = {{"model.2", 2, v.c2, v.nb},  {"model.4", 3, v.c3, v.nm},
                      {"model.6", 4, v.c4, v.nx},  {"model.8", 5, v.c5, v.nb},
                      {"model.13", 4, v.c4, v.nb}, {"model.17", 3, v.c3, v.nb},
                      {"model.20", 4, v.c4, v.nb}, {"model.23", 5, v.c5, v.nb}};
  for (const C3Def& c : cs)
    for (int i = 0; i < c.n; ++i) {
      M.newbuf(std::string(c.p) + ".t." + std::to_string(i), c.level, c.c2 / 2);
      M.newbuf(std::string(c.p) + ".m." + std::to_string(i), c.level, c.c2 / 2);
    }
}

// The C3k2 blocks of a YOLO11 plan: state_dict prefix, map level, hidden
// width c (= int(c2 e)) and whether the block nests C3k
struct C3k2Def {
  const char* p;
  int level, c;
  bool c3k;
};
static std::vector<C3k2Def> c3k2_blocks(const Variant& v) {
  return {{"model.2", 2, v.c3 / 4, v.c3k},  {"model.4", 3, v.c4 / 4, v.c3k},
          {"model.6", 4, v.c4 / 2, true},   {"model.8", 5, v.c5 / 2, true},
          {"model.13", 4, v.h12 / 2, v.c3k}, {"model.16", 3, v.h15 / 2, v.c3k},
          {"model.19", 4, v.h18 / 2, v.c3k}, {"model.22", 5, v.h21 / 2, true}};
}

// YOLO11 (yolo11.yaml): one buffer per activation.  A C3k2 block's concat
// buffer C<n> holds [y0 | y1 | m.0's output | ...] as a C2f's; "prefix.m.i"
// is bottleneck i's hidden map (width c / 2), and for a nested C3k
// "prefix.m.i.t.j" the input of its bottleneck j (t.0 = its cv1's output),
// "prefix.m.i.m.j" that bottleneck's hidden map and "prefix.m.i.cat" its
// [chain | cv2] concat.  C2PSA: "PA" = cv1's output [a | b]; per PSA block
// "model.10.m.i.qkv", ".o" (the attention output), ".ope" (o + pe(v)), ".x"
// (b + proj), ".f" (ffn.0) and ".b" (x + ffn.1: the block's output); cv2 reads
// [a | last b] as a virtual concat into CAT20 (the yaml's concat 21 = [model.20
// | model.10]); CAT17 is concat 18 = [model.17 | model.13].  Concats 12 and 15
// (behind the two Upsamples) are never materialised.  "DW<i>a" / "DW<i>b" are
// the outputs of the Detect class branch's two depthwise convs at level i.
static void plan_v11(Model& M) {
  const Variant& v = M.def.v;
  const int n = v.nb;
  M.CAT14 = M.CAT11 = -1;
  M.X0 = M.newbuf("X0", 1, v.c1);
  M.X1 = M.newbuf("X1", 2, v.c2);
  M.C2 = M.newbuf("C2", 2, (2 + n) * (v.c3 / 4));
  M.X2 = M.newbuf("X2", 2, v.c3);
  M.X3 = M.newbuf("X3", 3, v.c3);
  M.C4 = M.newbuf("C4", 3, (2 + n) * (v.c4 / 4));
  M.X4 = M.newbuf("X4", 3, v.c4);
  M.X5 = M.newbuf("X5", 4, v.c4);
  M.C6 = M.newbuf("C6", 4, (2 + n) * (v.c4 / 2));
  M.X6 = M.newbuf("X6", 4, v.c4);
  M.X7 = M.newbuf("X7", 5, v.c5);
  M.C8 = M.newbuf("C8", 5, (2 + n) * (v.c5 / 2));
  M.X8 = M.newbuf("X8", 5, v.c5);
  M.SP = M.newbuf("SP", 5, 4 * (v.c5 / 2));
  M.X9 = M.newbuf("X9", 5, v.c5);
  M.newbuf("PA", 5, v.c5);
  for (int i = 0; i < n; ++i) {
    const std::string q = "model.10.m." + std::to_string(i);
    M.newbuf(q + ".qkv", 5, v.c5);
    M.newbuf(q + ".o", 5, v.c5 / 2);
    M.newbuf(q + ".ope", 5, v.c5 / 2);
    M.newbuf(q + ".x", 5, v.c5 / 2);
    M.newbuf(q + ".f", 5, v.c5);
    M.newbuf(q + ".b", 5, v.c5 / 2);
  }
  M.CAT20 = M.newbuf("CAT20", 5, v.h18 + v.c5);
  M.C12 = M.newbuf("C12", 4, (2 + n) * (v.h12 / 2));
  M.CAT17 = M.newbuf("CAT17", 4, v.h15 + v.h12);
  M.C15 = M.newbuf("C15", 3, (2 + n) * (v.h15 / 2));
  M.X15 = M.newbuf("X15", 3, v.h15);
  M.C18 = M.newbuf("C18", 4, (2 + n) * (v.h18 / 2));
  M.X18 = M.newbuf("X18", 4, v.h18);
  M.C21 = M.newbuf("C21", 5, (2 + n) * (v.h21 / 2));
  M.X21 = M.newbuf("X21", 5, v.h21);
  plan_heads(M);
  const int chs[3] = {v.h15, v.h18, v.h21};
  for (int i = 0; i < 3; ++i) {
    M.newbuf("DW" + std::to_string(i) + "a", 3 + i, chs[i]);
    M.newbuf("DW" + std::to_string(i) + "b", 3 + i, v.c3p);
  }
  for (const C3k2Def& c : c3k2_blocks(v))
    for (int i = 0; i < n; ++i) {
      const std::string q = std::string(c.p) + ".m." + std::to_string(i);
      if (!c.c3k) {
        M.newbuf(q, c.level, c.c / 2);
        continue;
      }
      M.newbuf(q + ".cat", c.level, c.c);
      for (int j = 0; j < 2; ++j) {
        M.newbuf(q + ".t." + std::to_string(j), c.level, c.c / 2);
        M.newbuf(q + ".m." + std::to_string(j), c.level, c.c / 2);
      }
    }
}

static void plan(Model& M) {
  const Variant& v = M.def.v;
  for (int i = 0; i < 6; ++i) {
    M.map_h[i] = M.H >> i;
    M.map_w[i] = M.W >> i;
  }
  if (v.family == kFamilyV5u) return plan_v5u(M);
  if (v.family == kFamilyV11) return plan_v11(M);
  M.X0 = M.newbuf("X0", 1, v.c1);
  M.X1 = M.newbuf("X1", 2, v.c2);
  M.C2 = M.newbuf("C2", 2, (2 + v.nb) * (v.c2 / 2));
  M.X2 = M.newbuf("X2", 2, v.c2);
  M.X3 = M.newbuf("X3", 3, v.c3);
  M.C4 = M.newbuf("C4", 3, (2 + v.nm) * (v.c3 / 2));
  M.CAT14 = M.newbuf("CAT14", 3, v.h12 + v.c3);
  M.X5 = M.newbuf("X5", 4, v.c4);
  M.C6 = M.newbuf("C6", 4, (2 + v.nm) * (v.c4 / 2));
  M.CAT11 = M.newbuf("CAT11", 4, v.c5 + v.c4);
  M.X7 = M.newbuf("X7", 5, v.c5);
  M.C8 = M.newbuf("C8", 5, (2 + v.nb) * (v.c5 / 2));
  M.X8 = M.newbuf("X8", 5, v.c5);
  M.SP = M.newbuf("SP", 5, 4 * (v.c5 / 2));
  M.CAT20 = M.newbuf("CAT20", 5, v.h18 + v.c5);
  M.C12 = M.newbuf("C12", 4, (2 + v.nb) * (v.h12 / 2));
  M.CAT17 = M.newbuf("CAT17", 4, v.h15 + v.h12);
  M.C15 = M.newbuf("C15", 3, (2 + v.nb) * (v.h15 / 2));
  M.X15 = M.newbuf("X15", 3, v.h15);
  M.C18 = M.newbuf("C18", 4, (2 + v.nb) * (v.h18 / 2));
  M.X18 = M.newbuf("X18", 4, v.h18);
  M.C21 = M.newbuf("C21", 5, (2 + v.nb) * (v.h21 / 2));
  M.X21 = M.newbuf("X21", 5, v.h21);
  plan_heads(M);
  // one temp per bottleneck (its first conv's output), named "prefix.m.i":
  // no buffer is ever overwritten inside a forward, so every layer stays
  // inspectable
  struct C2fDef {
    const char* p;
    int level, c2, n;
  };
  const C2fDef cs[] = {{"model.2", 2, v.c2, v.nb},  {"model.4", 3, v.c3, v.nm},
                       {"model.6", 4, v.c4, v.nm},  {"model.8", 5, v.c5, v.nb},
                       {"model.12", 4, v.h12, v.nb}, {"model.15", 3, v.h15, v.nb},
                       {"model.18", 4, v.h18, v.nb}, {"model.21", 5, v.h21, v.nb}};
  for (const C2fDef& c : cs)
    for (int i = 0; i < c.n; ++i)
      M.newbuf(std::string(c.p) + ".m." + std::to_string(i), c.level, c.c2 / 2);
}

static const View NO_VIEW{-1, 0, 0};

// RV_YOLO_OPT_HEAD_SPARSE = 2 (auto): the sparse head runs when the call's
// conf is at least kSparseAutoConf and its batch at least kSparseAutoBatch
// ("Sparse box branch", has the measured curves behind both).
constexpr float kSparseAutoConf = 0.1f;
constexpr int kSparseAutoBatch = 8;

// What one conv reads and writes: input view at map level li -> up to two
// output views (up: a nearest-2x upsampled copy), an optional residual, and
// for a 1x1 conv an optional virtual concat input that stands in for `in`.
struct ConvIO {
  View in;
  int li;
  View o0;
  int up0 = 0;
  View o1 = NO_VIEW;
  int up1 = 0;
  View res = NO_VIEW;
  const VIn* vin = nullptr;
};

// One forward (or forward part) of a plan on a workspace
struct Exec {
  Model* M;
  uint8_t* ws;
  int B;
  hipStream_t s;
  std::vector<size_t> off;  // Model::offsets(B)
  int status = 0;
  // this forward may fuse launches: a bf16 plan, unless a raw parity forward
  // keeps every activation (RV_YOLO_OPT_RAW_UNFUSED)
  bool f8, fusing;
  // fused C2f chains (c2f.hip) unless RV_YOLO_OPT_FUSE_C2F = 0.  The
  // hidden-width-32 chains (model.4, model.15 of YOLOv8n) measured faster
  // unfused since the patch kernel's buffer-DMA / fast-epilogue work (r03:
  // 188 + 86 us per 128-frame unit fused, 142 + 79 unfused): only the C = 16
  // chain (model.2 at P2, 122 fused vs 191 unfused) stays fused unless
  // RV_YOLO_OPT_FUSE_C2F = 2
  bool fuse_c2f, fuse_c2f32;
  int cat14, cat11, cat20, cat17;  // concat buffer widths

  Exec(Model* m, void* ws_, int B_, void* stream, std::vector<size_t> off_, bool raw)
      : M(m), ws((uint8_t*)ws_), B(B_), s(as_stream(stream)), off(std::move(off_)) {
    const Variant& v = M->def.v;
    f8 = M->def.dtype == RV_YOLO_DTYPE_FP8;
    fusing = !f8 && !(raw && M->raw_unfused);
    fuse_c2f = fusing && M->fuse_c2f;
    fuse_c2f32 = fuse_c2f && M->fuse_c2f == 2;
    cat14 = v.h12 + v.c3, cat11 = v.c5 + v.c4, cat20 = v.h18 + v.c5, cat17 = v.h15 + v.h12;
    if (v.family == kFamilyV5u) cat14 = cat17 = 2 * v.c3, cat11 = cat20 = 2 * v.c4;
  }

  void* ptr(int buf) const { return ws + off[buf]; }
  const bf16_t* wptr(const ConvSpec& c) const { return (const bf16_t*)(M->dev + c.w_off); }
  const float* bptr(const ConvSpec& c) const { return (const float*)(M->dev + c.b_off); }
  const float* wsptr(const ConvSpec& c) const {
    return c.f8 ? (const float*)(M->dev + c.ws_off) : nullptr;
  }
  float scale(int buf) const { return buf >= 0 ? M->act_scale[buf] : 1.0f; }

  const ConvSpec* spec(const std::string& name) {  // nullptr (and an error status): no such conv
    const int idx = M->def.find(name);
    if (idx < 0 && !status) {
      set_error("plan: unknown conv %s", name.c_str());
      status = RV_EINVAL;
    }
    return idx < 0 ? nullptr : &M->def.convs[idx];
  }
  int index(const ConvSpec& c) const { return (int)(&c - M->def.convs.data()); }

  static int out_dim(const ConvSpec& c, int n) { return (n + 2 * (c.k / 2) - c.k) / c.s + 1; }

  ConvArgs args(const ConvSpec& c, const ConvIO& io) const {
    const View in = io.vin ? io.vin->a : io.in, o0 = io.o0, o1 = io.o1, res = io.res;
    ConvArgs a = {};
    a.in = (const bf16_t*)ptr(in.buf);
    a.in_cs = in.cs;
    a.in_co = in.co;
    a.Hin = M->map_h[io.li];
    a.Win = M->map_w[io.li];
    a.Cin = c.pcin;
    a.w = wptr(c);
    a.bias = bptr(c);
    a.Cout = c.pcout;
    a.k = c.k;
    a.stride = c.s;
    a.pad = c.k / 2;
    a.Ho = out_dim(c, a.Hin);
    a.Wo = out_dim(c, a.Win);
    a.B = B;
    a.out0 = ptr(o0.buf);
    a.out0_cs = o0.cs;
    a.out0_co = o0.co;
    a.out0_up = io.up0;
    if (o1.buf >= 0) {
      a.out1 = ptr(o1.buf);
      a.out1_cs = o1.cs;
      a.out1_co = o1.co;
      a.out1_up = io.up1;
    }
    a.out_f32 = M->bufs[o0.buf].f32 ? 1 : 0;
    if (res.buf >= 0) {
      a.res = (const bf16_t*)ptr(res.buf);
      a.res_cs = res.cs;
      a.res_co = res.co;
    }
    a.act = c.act;
    if (c.f8) {
      a.in8 = 1;
      a.s_in = scale(in.buf);
      a.wscale = wsptr(c);
      a.out0_8 = M->bufs[o0.buf].esize == 1;
      a.s_out0 = scale(o0.buf);
      if (o1.buf >= 0) {
        a.out1_8 = M->bufs[o1.buf].esize == 1;
        a.s_out1 = scale(o1.buf);
      }
      if (res.buf >= 0) a.s_res = scale(res.buf);
    }
    if (io.vin) {
      a.in_up = io.vin->up;
      a.in2 = (const bf16_t*)ptr(io.vin->b.buf);
      a.in2_cs = io.vin->b.cs;
      a.in2_co = io.vin->b.co;
      a.split = io.vin->split;
    }
    return a;
  }

  // one record per conv spec (layer-wise parity tests read these back)
  void trace(const ConvSpec& c, const ConvIO& io) {
    const VIn* vi = io.vin;
    const int Hin = M->map_h[io.li], Win = M->map_w[io.li];
    M->trace.push_back(TraceRec{index(c), vi ? vi->a : io.in, Hin, Win, out_dim(c, Hin),
                                out_dim(c, Win), io.o0, io.up0, io.o1, io.up1, io.res,
                                vi ? vi->up : 0, vi ? vi->b : NO_VIEW, vi ? vi->split : 0});
  }

  // Algorithmic HBM bytes of one conv launch: every input channel slice it
  // reads (once), every output / upsampled copy it writes, the residual it
  // adds and its packed weights -- each byte once, however the kernel tiles.
  static double launch_bytes(const ConvArgs& a) {
    const double px_in = (double)a.B * a.Hin * a.Win, px_out = (double)a.B * a.Ho * a.Wo;
    if (a.split > 0 || a.in_up) {  // virtual concat: each source read once
      const double cin1 = a.split > 0 ? a.split : a.Cin;
      const double src = (a.in_up ? px_in / 4 : px_in) * cin1 + px_in * (a.Cin - cin1);
      const double outs = (a.out0 ? (a.out0_up ? 4 : 1) : 0) + (a.out1 ? (a.out1_up ? 4 : 1) : 0);
      return 2.0 * src + 2.0 * px_out * a.Cout * outs + 2.0 * a.Cout * a.Cin;
    }
    const bool g2 = a.g2_cout0 > 0;
    const int cout1 = g2 ? a.g2_cout0 : a.Cout, cout2 = g2 ? a.Cout - a.g2_cout0 : 0;
    double in_ch = a.Cin;
    if (g2 && (a.g2_in_co != a.in_co || a.g2_Cin != a.Cin)) in_ch += a.g2_Cin;
    const double eb = a.in8 ? 1.0 : 2.0;  // input / residual / weight element bytes
    auto ob = [&](int o8) { return a.out_f32 ? 4.0 : (o8 ? 1.0 : 2.0); };
    const double outs = (a.out0 ? (a.out0_up ? 4 : 1) * ob(a.out0_8) : 0) +
                        (a.out1 ? (a.out1_up ? 4 : 1) * ob(a.out1_8) : 0);
    const double w = eb * a.k * a.k * ((double)cout1 * a.Cin + (double)cout2 * (g2 ? a.g2_Cin : 0)) +
                     (a.ch_w ? 2.0 * a.Cout * a.Cout : 0.0);  // a chained 1x1's weights
    return px_in * in_ch * eb + px_out * a.Cout * outs + (a.res ? px_out * a.Cout * eb : 0.0) + w;
  }

  double flops_of(const ConvSpec& c, int li) const {  // conv c on the level-li map
    return 2.0 * B * out_dim(c, M->map_h[li]) * out_dim(c, M->map_w[li]) * (double)c.cout * c.cin *
           c.k * c.k;
  }

  // One kernel launch standing for conv c (and what is fused into it:
  // flops and bytes are the launch's algorithmic totals): the autotuned
  // configuration of this launch index if there is a valid one, else the
  // default; live HIP-event timing when profiling is on.
  void launch(const ConvArgs& a, const ConvSpec& c, double flops, double bytes) {
    const int li_ = M->li_base + (int)M->launches.size();
    M->launches.push_back(a);
    status = M->prof.timed(li_, s, index(c), flops, bytes, [&] {
      if (a.fused > 0) {
        const Model::FusedC2f& f = M->fused[a.fused - 1];
        return launch_c2f_chain(f.a, f.C, f.N, f.shortcut, s);
      }
      if (li_ < (int)M->tuned.size() && M->tuned[li_].mr > 0 && conv_cfg_ok(a, M->tuned[li_]))
        return launch_conv_cfg(a, M->tuned[li_], s);
      return launch_conv(a, s);
    });
  }

  void conv(const std::string& name, const ConvIO& io) {
    if (status) return;
    const ConvSpec* c = spec(name);
    if (!c) return;
    const ConvArgs a = args(*c, io);
    trace(*c, io);
    launch(a, *c, flops_of(*c, io.li), launch_bytes(a));
  }

  // Conv `name` of a sparse-head forward: not launched (it runs per candidate
  // inside the sparse box-branch kernel).  Its trace record stays, with no
  // output view (out0.buf = -1: the map is never written), and so does its
  // launch index: a placeholder (ConvArgs::fused = -1) in the launch list with
  // no profile slot, so the per-index tuned configurations line up between
  // dense and sparse forwards of one handle.
  void conv_in_sparse(const std::string& name, const ConvIO& io) {
    if (status) return;
    const ConvSpec* c = spec(name);
    if (!c) return;
    ConvArgs a = args(*c, io);
    a.fused = -1;
    trace(*c, {io.in, io.li, NO_VIEW});
    M->launches.push_back(a);
  }

  // Two convs that share their input buffer, kernel size, stride and
  // activation and write adjacent channel slices of one output view -- the
  // Detect head's cv2 / cv3 branches -- as one grouped launch
  // (ConvArgs::g2_*).  Default: grouped in fp8 plans only.  bf16 plans launch
  // the branches separately: with the 8-wave patch kernel each branch runs
  // as ONE cout tile of its own width (box 64, class 80) reading the input
  // once, where the grouped launch's 64-wide tiles padded the class branch
  // to 128 (r04: P3 head 306 -> 260 us per 128-frame unit,
  // profiles/r04/conv_table_eager_*).
  void conv_pair(const std::string& n1, View in1, const std::string& n2, View in2, int li,
                 View o0) {
    if (status) return;
    const ConvSpec *p1 = spec(n1), *p2 = spec(n2);
    if (!p1 || !p2) return;
    const ConvSpec &c1 = *p1, &c2 = *p2;
    const ConvIO io1{in1, li, o0}, io2{in2, li, View{o0.buf, o0.cs, o0.co + c1.cout}};
    if (!c1.f8 || in1.buf != in2.buf || in1.cs != in2.cs || c1.k != c2.k || c1.s != c2.s ||
        c1.act != c2.act || c1.cout % 64 != 0) {
      conv(n1, io1);
      conv(n2, io2);
      return;
    }
    ConvArgs a = args(c1, io1);
    trace(c1, io1);
    trace(c2, io2);
    a.Cout = c1.pcout + c2.pcout;
    a.g2_cout0 = c1.pcout;
    a.g2_in_co = in2.co;
    a.g2_Cin = c2.pcin;
    a.g2_w = wptr(c2);
    a.g2_bias = bptr(c2);
    a.g2_wscale = wsptr(c2);
    launch(a, c1, flops_of(c1, li) + flops_of(c2, li), launch_bytes(a));
  }

  // conv n1 (3x3, output view `mid`, never written) with the 1x1 conv n2
  // (Cout -> Cout, SiLU: a C2f cv1) chained inside the same launch
  // (ConvArgs::ch_w, conv_patch_kernel CH form) writing view o0.  false
  // when the pair does not have the chained form's shape (the caller then
  // runs them as two launches).
  bool conv_chain(const std::string& n1, View in, int li, View mid, const std::string& n2,
                  View o0) {
    if (status) return false;
    const int i1 = M->def.find(n1), i2 = M->def.find(n2);
    if (i1 < 0 || i2 < 0) return false;
    const ConvSpec& c1 = M->def.convs[i1];
    const ConvSpec& c2 = M->def.convs[i2];
    if (c1.f8 || c2.f8 || c1.k != 3 || c1.cout != 64 || c2.k != 1 || c2.cin != c1.cout ||
        c2.cout != c1.cout || !c1.act || !c2.act)
      return false;
    ConvArgs a = args(c1, {in, li, o0});
    ConvCfg probe{4, 1, 1, 1, 1, 0};
    a.ch_w = wptr(c2);
    a.ch_b = bptr(c2);
    if (!conv_cfg_ok(a, probe)) return false;
    // trace records: the two convs as the unfused plan runs them
    trace(c1, {in, li, mid});
    trace(c2, {mid, li + 1, o0});
    launch(a, c1, flops_of(c1, li) + flops_of(c2, li + 1), launch_bytes(a));
    return true;
  }

  static bool c2f_will_fuse(int c, int n, bool fuse, int up0, View o1, View o0) {
    return fuse && up0 == 0 && o1.buf < 0 && c2f_fusable(c, n, 2 * c, 0, o0.cs, o0.co);
  }

  // C2f(prefix): the block's input (io.in / io.vin at map io.li) -> concat
  // buffer cb -> the block's outputs (io.o0 / io.o1).  With `fuse`, narrow
  // blocks run cv1 and then one fused launch for the bottlenecks + cv2
  // (c2f.hip; intermediates stay in LDS).
  void c2f(const std::string& p, const ConvIO& io, int cb, int c2, int n, bool shortcut,
           bool fuse = false, bool cv1_done = false) {
    const int c = c2 / 2, li = io.li;
    // a fused chain keeps z_i in LDS, so its concat buffer holds y0, y1
    // only: pixel stride 2c (denser cv1 stores and chain reads)
    const bool fused = c2f_will_fuse(c, n, fuse, io.up0, io.o1, io.o0);
    const int cs_u = (2 + n) * c, cs = fused ? 2 * c : cs_u;
    if (!cv1_done) conv(p + ".cv1", {io.in, li, View{cb, cs, 0}, 0, NO_VIEW, 0, NO_VIEW, io.vin});
    // bottleneck i over a concat buffer of pixel stride st: its two convs
    struct Bneck {
      std::string q;
      ConvIO a, b;
    };
    auto bneck = [&](int i, int st) {
      const std::string q = p + ".m." + std::to_string(i);
      const View bin{cb, st, (1 + i) * c}, tmp{M->buf_of(q), c, 0};
      return Bneck{q, {bin, li, tmp},
                   {tmp, li, View{cb, st, (2 + i) * c}, 0, NO_VIEW, 0, shortcut ? bin : NO_VIEW}};
    };
    if (fused && !status) {
      Model::FusedC2f f{{}, c, n, shortcut};
      f.a.cat = (const bf16_t*)ptr(cb);
      f.a.cat_cs = cs;
      f.a.cat_co = 0;
      f.a.H = M->map_h[li];
      f.a.W = M->map_w[li];
      f.a.B = B;
      f.a.tap_pairs = M->c2f_tap_pairs;
      double flops = 0.0;
      for (int i = 0; i < n; ++i) {
        // trace records keep the layer list complete (the buffers are not
        // written: parity forwards run unfused; the records show the unfused
        // concat layout)
        const Bneck m = bneck(i, cs_u);
        const ConvSpec *pa = spec(m.q + ".cv1"), *pb = spec(m.q + ".cv2");
        if (!pa || !pb) return;
        const ConvSpec &ca = *pa, &cbv = *pb;
        f.a.wa[i] = wptr(ca);
        f.a.ba[i] = bptr(ca);
        f.a.wb[i] = wptr(cbv);
        f.a.bb[i] = bptr(cbv);
        trace(ca, m.a);
        trace(cbv, m.b);
        flops += flops_of(ca, li) + flops_of(cbv, li);
      }
      const ConvSpec* p2 = spec(p + ".cv2");
      if (!p2) return;
      const ConvSpec& c2s = *p2;
      f.a.w2 = wptr(c2s);
      f.a.b2 = bptr(c2s);
      f.a.out = (bf16_t*)ptr(io.o0.buf);
      f.a.out_cs = io.o0.cs;
      f.a.out_co = io.o0.co;
      const ConvIO io2{View{cb, cs_u, 0}, li, io.o0};  // cv2's Cin: the unfused concat width
      ConvArgs rec = args(c2s, io2);  // the chain's entry in the launch list
      trace(c2s, io2);
      flops += flops_of(c2s, li);
      M->fused.push_back(f);
      rec.fused = (int)M->fused.size();
      // algorithmic bytes: y0 + y1 read once, cv2's output written once,
      // every weight of the chain read once
      const double wbytes = n * (2.0 * 2 * 9 * c * 32) + 2.0 * c2 * ((cs_u + 31) / 32 * 32);
      launch(rec, c2s, flops, (double)B * f.a.H * f.a.W * (2.0 * c * 2 + 2.0 * c2) + wbytes);
      return;
    }
    for (int i = 0; i < n; ++i) {
      const Bneck m = bneck(i, cs);
      conv(m.q + ".cv1", m.a);
      conv(m.q + ".cv2", m.b);
    }
    conv(p + ".cv2", {View{cb, cs, 0}, li, io.o0, io.up0, io.o1, io.up1});
  }

  // C3(prefix), YOLOv5u: the block's input (io.in / io.vin at map io.li) ->
  // cv1 -> n bottlenecks (1x1 then 3x3, t + ... with shortcut), the last one
  // writing channels [0, c) of the concat buffer cb; cv2 on the same input
  // -> [c, 2c); cv3 on cb -> the block's outputs.  One launch per conv.
  void c3(const std::string& p, const ConvIO& io, int cb, int c2, int n, bool shortcut) {
    const int c = c2 / 2, li = io.li;
    auto tbuf = [&](int i) { return View{M->buf_of(p + ".t." + std::to_string(i)), c, 0}; };
    conv(p + ".cv1", {io.in, li, tbuf(0), 0, NO_VIEW, 0, NO_VIEW, io.vin});
    for (int i = 0; i < n; ++i) {
      const std::string q = p + ".m." + std::to_string(i);
      const View tin = tbuf(i), tmp{M->buf_of(q), c, 0};
      const View tout = i + 1 < n ? tbuf(i + 1) : View{cb, 2 * c, 0};
      conv(q + ".cv1", {tin, li, tmp});
      conv(q + ".cv2", {tmp, li, tout, 0, NO_VIEW, 0, shortcut ? tin : NO_VIEW});
    }
    conv(p + ".cv2", {io.in, li, View{cb, 2 * c, c}, 0, NO_VIEW, 0, NO_VIEW, io.vin});
    conv(p + ".cv3", {View{cb, 2 * c, 0}, li, io.o0, io.up0, io.o1, io.up1});
  }

  // A launch that is no conv-launcher launch (a depthwise conv, an attention):
  // it keeps a launch index -- a placeholder in the launch list (ConvArgs::fused
  // = -2 depthwise, -3 attention) that the autotuner skips, so the per-index
  // tuned configurations stay aligned -- and is timed in that index's slot.
  template <class F>
  void other_launch(ConvArgs a, int kind, int conv, double flops, double bytes, F&& run) {
    const int li_ = M->li_base + (int)M->launches.size();
    a.fused = kind;
    M->launches.push_back(a);
    status = M->prof.timed(li_, s, conv, flops, bytes, run);
  }

  // Depthwise 3x3 conv `name` (dwconv.hip): input view `in` at map li -- with
  // gw > 0 in the group form, gw channels every gs -- -> o0, + res.  Its trace
  // record is a conv's; the virtual-concat fields carry the group form
  // (in2 = {-1, gs, 0}, split = gw).
  void dw(const std::string& name, View in, int gw, int gs, int li, View o0, View res = NO_VIEW) {
    if (status) return;
    const ConvSpec* c = spec(name);
    if (!c) return;
    const int H = M->map_h[li], W = M->map_w[li], C = c->pcout;
    M->trace.push_back(TraceRec{index(*c), in, H, W, H, W, o0, 0, NO_VIEW, 0, res, 0,
                                View{-1, gs, 0}, gw});
    const double px = (double)B * H * W;
    other_launch(args(*c, {in, li, o0, 0, NO_VIEW, 0, res}), -2, index(*c), 2.0 * px * C * 9,
                 2.0 * px * C * (res.buf >= 0 ? 3 : 2) + 2.0 * 9 * C, [&] {
                   return launch_dwconv3x3((const bf16_t*)ptr(in.buf), in.cs, in.co, gw, gs, wptr(*c),
                                           bptr(*c), B, H, W, C, c->act,
                                           res.buf >= 0 ? (const bf16_t*)ptr(res.buf) : nullptr,
                                           res.cs, res.co, (bf16_t*)ptr(o0.buf), o0.cs, o0.co, s);
                 });
  }

  // Self-attention over the level-li map (attn.hip): qkv view -> o.  `conv`:
  // the block's attn.qkv conv, under whose index the launch is profiled.
  void attn(View qkv, int heads, int li, View o, int conv) {
    if (status) return;
    const int H = M->map_h[li], W = M->map_w[li];
    const double N = (double)H * W;
    M->attn_trace.push_back(AttnRec{qkv, heads, H, W, o});
    ConvArgs a = {};
    a.B = B;
    other_launch(a, -3, conv, 2.0 * B * heads * N * N * (32 + 64), 2.0 * B * N * heads * (128 + 64),
                 [&] {
                   return launch_psa_attention((const bf16_t*)ptr(qkv.buf), B, H * W, heads, qkv.cs,
                                               qkv.co, (bf16_t*)ptr(o.buf), o.cs, o.co, s);
                 });
  }

  // C3k2(prefix), YOLO11: a C2f over the concat buffer cb ((2 + n) c wide)
  // whose m.i is a bottleneck with hidden width c / 2 (3x3, 3x3, shortcut) or,
  // with c3k, a C3k: cv1 -> two bottlenecks at width c / 2 -> [chain | cv2] ->
  // cv3.  One launch per conv (plan_v11 names the buffers).
  void c3k2(const std::string& p, const ConvIO& io, int cb, int c, int n, bool c3k) {
    const int li = io.li, cs = (2 + n) * c, h = c / 2;
    conv(p + ".cv1", {io.in, li, View{cb, cs, 0}, 0, NO_VIEW, 0, NO_VIEW, io.vin});
    for (int i = 0; i < n; ++i) {
      const std::string q = p + ".m." + std::to_string(i);
      const View bin{cb, cs, (1 + i) * c}, bout{cb, cs, (2 + i) * c};
      if (!c3k) {
        const View tmp{M->buf_of(q), h, 0};
        conv(q + ".cv1", {bin, li, tmp});
        conv(q + ".cv2", {tmp, li, bout, 0, NO_VIEW, 0, bin});
        continue;
      }
      const int cat = M->buf_of(q + ".cat");
      auto tb = [&](int j) { return View{M->buf_of(q + ".t." + std::to_string(j)), h, 0}; };
      conv(q + ".cv1", {bin, li, tb(0)});
      for (int j = 0; j < 2; ++j) {
        const std::string r = q + ".m." + std::to_string(j);
        const View tmp{M->buf_of(r), h, 0};
        conv(r + ".cv1", {tb(j), li, tmp});
        conv(r + ".cv2", {tmp, li, j == 0 ? tb(1) : View{cat, 2 * h, 0}, 0, NO_VIEW, 0, tb(j)});
      }
      conv(q + ".cv2", {bin, li, View{cat, 2 * h, h}});
      conv(q + ".cv3", {View{cat, 2 * h, 0}, li, bout});
    }
    conv(p + ".cv2", {View{cb, cs, 0}, li, io.o0, io.up0, io.o1, io.up1});
  }

  // C2PSA(prefix), YOLO11: cv1 -> [a | b]; n PSA blocks on b (b += proj(attn(b)
  // + pe(v)), b += ffn(b)); cv2 on [a | b] (a virtual concat) -> out
  void c2psa(const std::string& p, View in, int li, View out, int n) {
    const int c = M->def.v.c5 / 2, heads = c / 64, pa = M->buf_of("PA");
    conv(p + ".cv1", {in, li, View{pa, 2 * c, 0}});
    View b{pa, 2 * c, c};
    for (int i = 0; i < n && !status; ++i) {
      const std::string q = p + ".m." + std::to_string(i);
      const View qkv{M->buf_of(q + ".qkv"), 2 * c, 0}, o{M->buf_of(q + ".o"), c, 0},
          ope{M->buf_of(q + ".ope"), c, 0}, x{M->buf_of(q + ".x"), c, 0},
          f{M->buf_of(q + ".f"), 2 * c, 0}, bo{M->buf_of(q + ".b"), c, 0};
      conv(q + ".attn.qkv", {b, li, qkv});
      attn(qkv, heads, li, o, M->def.find(q + ".attn.qkv"));
      // pe on v (64 channels of every head's 128, in o's channel order), + o
      dw(q + ".attn.pe", View{qkv.buf, 2 * c, 64}, 64, 128, li, ope, o);
      conv(q + ".attn.proj", {ope, li, x, 0, NO_VIEW, 0, b});
      conv(q + ".ffn.0", {x, li, f});
      conv(q + ".ffn.1", {f, li, bo, 0, NO_VIEW, 0, x});
      b = bo;
    }
    const VIn vin{View{pa, 2 * c, 0}, 0, b, c};
    conv(p + ".cv2", {View{pa, 2 * c, 0}, li, out, 0, NO_VIEW, 0, NO_VIEW, &vin});
  }
};

// YOLO11, segment A: model.0 (YOLOv8's k3 s2 conv on the u8 letterbox),
// model.1, model.2
static int seg_stem_v11(Exec& E, const uint8_t* lb) {
  Model* M = E.M;
  const Variant& v = M->def.v;
  const View x0{M->X0, v.c1, 0}, x1{M->X1, v.c2, 0}, x2{M->X2, v.c3, 0};
  const ConvSpec& c0 = M->def.convs[0];
  const uint8_t* qb = M->dev + M->def.q_off;
  const float* qs = (const float*)(qb + 3 * (size_t)c0.cout * 64);
  const Conv0Q q0{(const int8_t*)qb, qs, qs + c0.cout, (const int32_t*)(qs + 2 * c0.cout)};
  const double px0 = (double)E.B * M->map_h[1] * M->map_w[1];
  // timed like the other families' stems: profile slot per_fwd - 1
  E.status = M->prof.timed(M->prof.per_fwd - 1, E.s, 0, 2.0 * px0 * c0.cout * 27,
                           (double)E.B * M->H * M->W * 3 + M->def.q_bytes + px0 * 2.0 * c0.cout, [&] {
                             return launch_conv0(lb, E.B, M->H, M->W, q0, c0.cout,
                                                 (bf16_t*)E.ptr(M->X0), v.c1, E.s);
                           });
  E.conv("model.1", {x0, 1, x1});
  E.c3k2("model.2", {x1, 2, x2}, M->C2, v.c3 / 4, v.nb, v.c3k);
  return E.status;
}

// YOLO11, segment B: model.3 .. model.16 (the rest of the backbone, SPPF,
// C2PSA and the top-down neck).  The yaml's Upsample + Concat pairs (11-12,
// 14-15) are virtual concat inputs of model.13.cv1 / model.16.cv1.
static int seg_backbone_v11(Exec& E) {
  Model* M = E.M;
  const Variant& v = M->def.v;
  const int sc = v.c5 / 2;
  const View x2{M->X2, v.c3, 0}, x3{M->X3, v.c3, 0}, p3{M->X4, v.c4, 0}, x5{M->X5, v.c4, 0},
      p4{M->X6, v.c4, 0}, x7{M->X7, v.c5, 0}, x8{M->X8, v.c5, 0}, sp{M->SP, 4 * sc, 0},
      x9{M->X9, v.c5, 0};
  // model.10 / model.13 as the bottom-up concats 21 / 18 hold them
  const View t10{M->CAT20, E.cat20, v.h18}, t13{M->CAT17, E.cat17, v.h15};
  const VIn vin13{t10, 1, p4, v.c5}, vin16{t13, 1, p3, v.h12};
  E.conv("model.3", {x2, 2, x3});
  E.c3k2("model.4", {x3, 3, p3}, M->C4, v.c4 / 4, v.nb, v.c3k);
  E.conv("model.5", {p3, 3, x5});
  E.c3k2("model.6", {x5, 4, p4}, M->C6, v.c4 / 2, v.nb, true);
  E.conv("model.7", {p4, 4, x7});
  E.c3k2("model.8", {x7, 5, x8}, M->C8, v.c5 / 2, v.nb, true);
  E.conv("model.9.cv1", {x8, 5, sp});
  if (!E.status)
    E.status = launch_sppf_pool((bf16_t*)E.ptr(M->SP), E.B, M->map_h[5], M->map_w[5], sc, E.s);
  E.conv("model.9.cv2", {sp, 5, x9});
  E.c2psa("model.10", x9, 5, t10, v.nb);
  E.c3k2("model.13", {t10, 4, t13, 0, NO_VIEW, 0, NO_VIEW, &vin13}, M->C12, v.h12 / 2, v.nb, v.c3k);
  E.c3k2("model.16", {t13, 3, View{M->X15, v.h15, 0}, 0, NO_VIEW, 0, NO_VIEW, &vin16}, M->C15,
         v.h15 / 2, v.nb, v.c3k);
  return E.status;
}

// YOLOv5u, segment A: model.0 (k6 s2 p2 from the u8 letterbox, its own
// kernel: Exec::out_dim's pad = k / 2 does not hold for it), model.1, model.2
static int seg_stem_v5u(Exec& E, const uint8_t* lb) {
  Model* M = E.M;
  const Variant& v = M->def.v;
  const View x0{M->X0, v.c1, 0}, x1{M->X1, v.c2, 0}, x2{M->X2, v.c2, 0};
  const ConvSpec& c0 = M->def.convs[0];
  const uint8_t* qb = M->dev + M->def.q_off;
  const float* qs = (const float*)(qb + 9 * (size_t)c0.cout * 64);
  const Conv0Q q0{(const int8_t*)qb, qs, qs + c0.cout, (const int32_t*)(qs + 2 * c0.cout)};
  const double px0 = (double)E.B * M->map_h[1] * M->map_w[1];
  const double px1 = (double)E.B * M->map_h[2] * M->map_w[2];
  const double f0 = 2.0 * px0 * c0.cout * 108, by_in = (double)E.B * M->H * M->W * 3 + M->def.q_bytes;
  // both forms are timed like the YOLOv8 fused stem: profile slot
  // per_fwd - 1, which no conv launch index reaches
  const int slot = M->prof.per_fwd - 1;
  // conv0-k6 + model.1 fused (YOLOv5nu; the P1 map stays in LDS) unless the
  // caller asked for the raw prediction with RV_YOLO_OPT_RAW_UNFUSED set
  const int i1 = M->def.find("model.1");
  if (E.fusing && M->stem6_fused && c0.cout == 16 && v.c2 == 32 && i1 >= 0) {
    const ConvSpec& c1 = M->def.convs[i1];
    E.trace(c1, {x0, 1, x1});
    E.status = M->prof.timed(slot, E.s, 0, f0 + 2.0 * px1 * c1.cout * c1.cin * 9,
                             by_in + px1 * 2.0 * c1.cout + 2.0 * c1.cout * 9 * 32, [&] {
                               return launch_stem(lb, E.B, M->H, M->W, q0, c0.cout, E.wptr(c1),
                                                  E.bptr(c1), c1.cout, (bf16_t*)E.ptr(M->X1), v.c2,
                                                  E.s, nullptr, nullptr, nullptr, 0, true);
                             });
  } else {
    E.status = M->prof.timed(slot, E.s, 0, f0, by_in + px0 * 2.0 * c0.cout, [&] {
      return launch_conv0_k6(lb, E.B, M->H, M->W, q0, c0.cout, (bf16_t*)E.ptr(M->X0), v.c1, E.s);
    });
    E.conv("model.1", {x0, 1, x1});
  }
  E.c3("model.2", {x1, 2, x2}, M->C2, v.c2, v.nb, true);
  return E.status;
}

// YOLOv5u, segment B: model.3 .. model.17 (the rest of the backbone, SPPF and
// the top-down neck).  The yaml's Upsample + Concat pairs (11-12, 15-16) are
// virtual concat inputs of the two 1x1 convs that read each of them.
static int seg_backbone_v5u(Exec& E) {
  Model* M = E.M;
  const Variant& v = M->def.v;
  const int sc = v.c5 / 2;
  const View x2{M->X2, v.c2, 0}, x3{M->X3, v.c3, 0}, p3{M->X4, v.c3, 0}, x5{M->X5, v.c4, 0},
      p4{M->X6, v.c4, 0}, x7{M->X7, v.c5, 0}, x8{M->X8, v.c5, 0}, sp{M->SP, 4 * sc, 0},
      x9{M->X9, v.c5, 0}, x13{M->X13, v.c4, 0};
  // model.10 / model.14 as the bottom-up concats 22 / 19 hold them
  const View t10{M->CAT20, E.cat20, v.c4}, t14{M->CAT17, E.cat17, v.c3};
  const VIn vin13{t10, 1, p4, v.c4}, vin17{t14, 1, p3, v.c3};
  E.conv("model.3", {x2, 2, x3});
  E.c3("model.4", {x3, 3, p3}, M->C4, v.c3, v.nm, true);
  E.conv("model.5", {p3, 3, x5});
  E.c3("model.6", {x5, 4, p4}, M->C6, v.c4, v.nx, true);
  E.conv("model.7", {p4, 4, x7});
  E.c3("model.8", {x7, 5, x8}, M->C8, v.c5, v.nb, true);
  E.conv("model.9.cv1", {x8, 5, sp});
  if (!E.status)
    E.status = launch_sppf_pool((bf16_t*)E.ptr(M->SP), E.B, M->map_h[5], M->map_w[5], sc, E.s);
  E.conv("model.9.cv2", {sp, 5, x9});
  E.conv("model.10", {x9, 5, t10});
  E.c3("model.13", {t10, 4, x13, 0, NO_VIEW, 0, NO_VIEW, &vin13}, M->C12, v.c4, v.nb, false);
  E.conv("model.14", {x13, 4, t14});
  E.c3("model.17", {t14, 3, View{M->X15, v.h15, 0}, 0, NO_VIEW, 0, NO_VIEW, &vin17}, M->C15, v.c3,
       v.nb, false);
  return E.status;
}

// A forward is three consecutive segments over one Exec, each returning
// E.status.  Segment A: the stem (model.0, model.1) and model.2
static int seg_stem(Exec& E, const uint8_t* lb) {
  Model* M = E.M;
  const Variant& v = M->def.v;
  const int B = E.B;
  const View x0{M->X0, v.c1, 0}, x1{M->X1, v.c2, 0}, x2{M->X2, v.c2, 0};
  const ConvSpec& c0 = M->def.convs[0];
  const uint8_t* qb = M->dev + M->def.q_off;
  const float* qs = (const float*)(qb + 3 * (size_t)c0.cout * 64);
  const Conv0Q q0{(const int8_t*)qb, qs, qs + c0.cout, (const int32_t*)(qs + 2 * c0.cout)};
  // conv0 + model.1 fused (the P1 map stays in LDS) unless the caller asked
  // for the raw prediction with RV_YOLO_OPT_RAW_UNFUSED set (layer parity
  // forwards keep every activation in the workspace)
  const int i1 = M->def.find("model.1");
  const bool fuse_stem = E.fusing && c0.cout == 16 && v.c2 == 32 && i1 >= 0;
  // the fused stem also runs model.2.cv1 (32 -> 32 1x1) from its registers
  // into the model.2 concat buffer when the shapes allow
  const int i2cv1 = M->def.find("model.2.cv1");
  const int c2cs = E.c2f_will_fuse(v.c2 / 2, v.nb, E.fuse_c2f, 0, NO_VIEW, x2)
                       ? v.c2
                       : (2 + v.nb) * (v.c2 / 2);
  const bool stem_cv1 = fuse_stem && i2cv1 >= 0 && M->def.convs[i2cv1].cin == 32 &&
                        M->def.convs[i2cv1].cout == 32 && M->def.convs[i2cv1].k == 1;
  if (fuse_stem) {
    const ConvSpec& c1 = M->def.convs[i1];
    E.trace(c1, {x0, 1, x1});
    const ConvSpec* cv = stem_cv1 ? &M->def.convs[i2cv1] : nullptr;
    if (cv) E.trace(*cv, {x1, 2, View{M->C2, c2cs, 0}});
    const bool x1_out = !cv || M->stem_x1;
    const double px0 = (double)B * M->map_h[1] * M->map_w[1];
    const double px1 = (double)B * M->map_h[2] * M->map_w[2];
    const double flops = 2.0 * px0 * c0.cout * 27 + 2.0 * px1 * c1.cout * c1.cin * 9 +
                         (cv ? 2.0 * px1 * cv->cout * cv->cin : 0.0);
    // letterbox read once, X1 / the cv1 slice written once, weights once
    const double bytes = (double)B * M->H * M->W * 3 + px1 * 2.0 * (x1_out ? c1.cout : 0) +
                         (cv ? px1 * 2.0 * cv->cout : 0.0) + M->def.q_bytes +
                         2.0 * c1.cout * 9 * 32 + (cv ? 2.0 * cv->cout * 32 : 0.0);
    // the stem is timed with the conv launches (profile slot per_fwd - 1,
    // which no conv launch index reaches: a forward has fewer launches than
    // convs)
    E.status = M->prof.timed(M->prof.per_fwd - 1, E.s, 0, flops, bytes, [&] {
      return launch_stem(lb, B, M->H, M->W, q0, c0.cout, E.wptr(c1), E.bptr(c1), c1.cout,
                         x1_out ? (bf16_t*)E.ptr(M->X1) : nullptr, v.c2, E.s,
                         cv ? E.wptr(*cv) : nullptr, cv ? E.bptr(*cv) : nullptr,
                         cv ? (bf16_t*)E.ptr(M->C2) : nullptr, c2cs);
    });
  } else {
    E.status = E.f8 ? launch_conv0_fp8(lb, B, M->H, M->W, q0, c0.cout, (uint8_t*)E.ptr(M->X0),
                                       v.c1, E.scale(M->X0), E.s)
                    : launch_conv0(lb, B, M->H, M->W, q0, c0.cout, (bf16_t*)E.ptr(M->X0), v.c1,
                                   E.s);
    E.conv("model.1", {x0, 1, x1});
  }
  E.c2f("model.2", {x1, 2, x2}, M->C2, v.c2, v.nb, true, E.fuse_c2f, stem_cv1);
  return E.status;
}

// Segment B: model.3 .. model.15 (the rest of the backbone, SPPF and the
// top-down neck)
static int seg_backbone(Exec& E) {
  Model* M = E.M;
  const Variant& v = M->def.v;
  const int cat14 = E.cat14, cat11 = E.cat11, sc = v.c5 / 2;
  const View x2{M->X2, v.c2, 0}, x3{M->X3, v.c3, 0}, x5{M->X5, v.c4, 0}, x7{M->X7, v.c5, 0},
      x8{M->X8, v.c5, 0}, sp{M->SP, 4 * sc, 0};
  // P3 / P4 / P5 as the neck's concats hold them, and the whole concats
  const View p3{M->CAT14, cat14, v.h12}, p4{M->CAT11, cat11, v.c5}, p5{M->CAT20, E.cat20, v.h18},
      n4{M->CAT17, E.cat17, v.h15}, c11{M->CAT11, cat11, 0}, c14{M->CAT14, cat14, 0};
  // The neck's two Upsample + Concat pairs (yolov8.yaml layers 10-11 and
  // 13-14): bf16 plans read the upsampled half of model.12.cv1's and
  // model.15.cv1's input straight from the half-resolution map (a virtual
  // concat, ConvArgs::split / in_up), so the 4x upsampled copies are never
  // written; fp8 plans (patch kernel only) materialise them into
  // CAT11[0, c5) / CAT14[0, h12).
  const bool vcat = !E.f8;
  const VIn vin12{p5, 1, p4, v.c5}, vin15{n4, 1, p3, v.h12};
  // model.3 + model.4.cv1 in one launch (the chained 1x1: model.3's output
  // map is only ever read by model.4.cv1) unless a raw parity forward keeps
  // every activation (RV_YOLO_OPT_RAW_UNFUSED) or RV_YOLO_OPT_FUSE_CV1 = 0
  const int c4 = v.c3 / 2;
  const bool f4 = c4 == 16 ? E.fuse_c2f : E.fuse_c2f32;
  const int c4cs = E.c2f_will_fuse(c4, v.nm, f4, 0, NO_VIEW, p3) ? 2 * c4 : (2 + v.nm) * c4;
  const bool chained = M->fuse_cv1 && E.fusing &&
                       E.conv_chain("model.3", x2, 2, x3, "model.4.cv1", View{M->C4, c4cs, 0});
  if (!chained) E.conv("model.3", {x2, 2, x3});
  E.c2f("model.4", {x3, 3, p3}, M->C4, v.c3, v.nm, true, f4, chained);
  E.conv("model.5", {p3, 3, x5});
  E.c2f("model.6", {x5, 4, p4}, M->C6, v.c4, v.nm, true);
  E.conv("model.7", {p4, 4, x7});
  E.c2f("model.8", {x7, 5, x8}, M->C8, v.c5, v.nb, true);
  // SPPF
  E.conv("model.9.cv1", {x8, 5, sp});
  if (!E.status)
    E.status =
        E.f8 ? launch_sppf_pool_fp8((uint8_t*)E.ptr(M->SP), E.B, M->map_h[5], M->map_w[5], sc, E.s)
             : launch_sppf_pool((bf16_t*)E.ptr(M->SP), E.B, M->map_h[5], M->map_w[5], sc, E.s);
  E.conv("model.9.cv2", {sp, 5, p5, 0, vcat ? NO_VIEW : c11, vcat ? 0 : 1});
  // head: the top-down neck.  Part 1 ends after model.15: it is the busier
  // half (its stream 70 % busy against 45 % in the r04 trace), but moving
  // the top-down neck's C2f blocks into part 2 measured slower (three A/B
  // triples, r04: 44.6-45.1k ending here, 43.9-45.2k after model.12,
  // 43.6-44.7k after SPPF)
  E.c2f("model.12", {c11, 4, n4, 0, vcat ? NO_VIEW : c14, vcat ? 0 : 1, NO_VIEW, vcat ? &vin12 : nullptr},
        M->C12, v.h12, v.nb, false);
  E.c2f("model.15", {c14, 3, View{M->X15, v.h15, 0}, 0, NO_VIEW, 0, NO_VIEW, vcat ? &vin15 : nullptr},
        M->C15, v.h15, v.nb, false, v.h15 / 2 == 16 ? E.fuse_c2f : E.fuse_c2f32);
  return E.status;
}

// Segment C: the bottom-up neck, the Detect heads and the decode
static int seg_heads(Exec& E, float* raw_out, float conf, void* cand, int cand_cap, int* cand_n) {
  Model* M = E.M;
  const Variant& v = M->def.v;
  const int B = E.B;
  const View c17{M->CAT17, E.cat17, 0}, c20{M->CAT20, E.cat20, 0};
  // Detect head of level i: box (cv2) and class (cv3) branches, one grouped
  // launch per stage; the last 1x1 stage runs inside the decode kernel
  // (heads whose widths are not multiples of 8: separate launches and f32
  // logits in HBM).  The P3 and P4 heads are forked onto side streams as
  // soon as their input map exists, so they overlap the rest of the neck
  // (small, latency-bound launches);
  // RV_YOLO_OPT_HEAD_STREAMS = 0 (a pipelined caller: its stages already
  // overlap, and two more streams per handle share the process's 4 hardware
  // queues -- r04: +3 % in the pipeline with the heads on the caller's
  // stream) keeps everything on the caller's stream.
  const View P[3] = {View{M->X15, v.h15, 0}, View{M->X18, v.h18, 0}, View{M->X21, v.h21, 0}};
  const int dcs = v.c2d + v.c3p, hcs = v.hcs;
  const bool fuse_head = v.c2d % 8 == 0 && v.c3p % 8 == 0;
  // profiled forwards time every launch alone (per-launch roofline), so the
  // heads stay on the caller's stream there; so do batches under 8, whose
  // few-us head launches gain less from the overlap than the fork / join
  // event round trips cost (batch 1, r05: 0.356 -> 0.308 ms device time per
  // forward, launch submission 284 -> 218 us, tools/c2_host.py)
  const bool fork =
      M->head_streams && B >= 8 && M->side[0] && M->side[1] && !M->prof.active();
  const hipStream_t main_s = E.s;
  // Sparse head: the box branch behind cv2.i.0 runs at the candidates only
  // (head_box.hip) after a class-only decode.  Only where the decode takes
  // its fixed form (bf16 plan, 64-wide box branch, 80 or <= 64 classes, no
  // raw output / logits copy) and a candidate list is asked for; auto picks
  // it for pipeline-sized batches at a conf where candidates are sparse.
  // YOLO11 heads are dense only (their class branch is not the two 3x3 convs)
  const bool v11 = v.family == kFamilyV11;
  const bool fixed_head = fuse_head && !E.f8 && !v11 && !raw_out && cand && v.c2d == 64 &&
                          (v.nc == 80 || v.nc <= 64) && v.c3p == (v.nc == 80 ? 80 : 64);
  const bool sparse =
      fixed_head && (M->head_sparse == 1 ||
                     (M->head_sparse == 2 && conf >= kSparseAutoConf && B >= kSparseAutoBatch));
  HeadLevel hl[3] = {};
  HeadBoxLevel hbx[3] = {};
  auto head_level = [&](int i) {
    const std::string a = M->def.head + "cv2." + std::to_string(i),
                      c = M->def.head + "cv3." + std::to_string(i);
    const View da{M->DA[i], dcs, 0}, fb{M->DB[i], dcs, 0}, fc{M->DB[i], dcs, v.c2d},
        lg{M->HD[i], hcs, 0};
    if (v11) {
      // class branch: DWConv 3x3 -> Conv 1x1, twice, beside the box branch's 3x3s
      const std::string l = std::to_string(i);
      const View wa{M->buf_of("DW" + l + "a"), P[i].cs, 0}, wb{M->buf_of("DW" + l + "b"), v.c3p, 0};
      E.conv(a + ".0", {P[i], 3 + i, da});
      E.dw(c + ".0.0", P[i], 0, 0, 3 + i, wa);
      E.conv(c + ".0.1", {wa, 3 + i, View{M->DA[i], dcs, v.c2d}});
      E.conv(a + ".1", {da, 3 + i, fb});
      E.dw(c + ".1.0", View{M->DA[i], dcs, v.c2d}, 0, 0, 3 + i, wb);
      E.conv(c + ".1.1", {wb, 3 + i, fc});
    } else if (sparse) {
      E.conv_pair(a + ".0", P[i], c + ".0", P[i], 3 + i, da);
      const ConvSpec* p1 = E.spec(a + ".1");
      if (!p1) return E.status;
      E.conv_in_sparse(a + ".1", {da, 3 + i, fb});
      E.conv(c + ".1", {View{M->DA[i], dcs, v.c2d}, 3 + i, fc});
      hbx[i] = HeadBoxLevel{(const bf16_t*)E.ptr(M->DA[i]), dcs, E.wptr(*p1), E.bptr(*p1)};
    } else {
      E.conv_pair(a + ".0", P[i], c + ".0", P[i], 3 + i, da);
      E.conv_pair(a + ".1", da, c + ".1", View{M->DA[i], dcs, v.c2d}, 3 + i, fb);
    }
    HeadLevel& L = hl[i];
    L.logits = (const float*)E.ptr(M->HD[i]);
    L.H = M->map_h[3 + i];
    L.W = M->map_w[3 + i];
    L.cs = hcs;
    L.stride = (float)(8 << i);
    if (!fuse_head) {
      E.conv_pair(a + ".2", fb, c + ".2", fc, 3 + i, lg);
      return E.status;
    }
    // run inside the decode kernel; trace records keep the layer list complete
    const ConvSpec *pa = E.spec(a + ".2"), *pc = E.spec(c + ".2");
    if (!pa || !pc) return E.status;
    const ConvSpec &sa = *pa, &sc = *pc;
    E.trace(sa, {fb, 3 + i, lg});
    E.trace(sc, {fc, 3 + i, View{M->HD[i], hcs, 4 * v.reg}});
    L.feat = (const bf16_t*)E.ptr(M->DB[i]);
    L.feat_cs = dcs;
    L.cin_b = sa.pcin;
    L.cin_c = sc.pcin;
    L.w_box = E.wptr(sa);
    L.w_cls = E.wptr(sc);
    L.b_box = E.bptr(sa);
    L.b_cls = E.bptr(sc);
    L.logits_out = raw_out ? (float*)E.ptr(M->HD[i]) : nullptr;
    return E.status;
  };
  auto forked_head = [&](int i) {  // level i's head on side stream i (joined before decode)
    if (!fork) return head_level(i);
    int e = hip_check(hipEventRecord(M->ev_fork[i], main_s), "head fork hipEventRecord");
    if (!e) e = hip_check(hipStreamWaitEvent(M->side[i], M->ev_fork[i], 0), "head fork wait");
    if (e) return E.status = e;
    E.s = M->side[i];
    const int r = head_level(i);
    e = hip_check(hipEventRecord(M->ev_join[i], M->side[i]), "head join hipEventRecord");
    E.s = main_s;
    if (!r && e) E.status = e;
    return r ? r : e;
  };
  // the bottom-up neck: a stride-2 conv into the level's concat, then its
  // block (YOLOv8: model.16, C2f 18, model.19, C2f 21; YOLOv5u: model.18,
  // C3 20, model.21, C3 23; YOLO11: model.17, C3k2 19, model.20, C3k2 22)
  const bool v5 = v.family == kFamilyV5u;
  if (E.status || forked_head(0)) return E.status;
  E.conv(v11 ? "model.17" : (v5 ? "model.18" : "model.16"), {P[0], 3, c17});
  if (v11)
    E.c3k2("model.19", {c17, 4, P[1]}, M->C18, v.h18 / 2, v.nb, v.c3k);
  else if (v5)
    E.c3("model.20", {c17, 4, P[1]}, M->C18, v.h18, v.nb, false);
  else
    E.c2f("model.18", {c17, 4, P[1]}, M->C18, v.h18, v.nb, false);
  if (E.status || forked_head(1)) return E.status;
  E.conv(v11 ? "model.20" : (v5 ? "model.21" : "model.19"), {P[1], 4, c20});
  if (v11)
    E.c3k2("model.22", {c20, 5, P[2]}, M->C21, v.h21 / 2, v.nb, true);
  else if (v5)
    E.c3("model.23", {c20, 5, P[2]}, M->C21, v.h21, v.nb, false);
  else
    E.c2f("model.21", {c20, 5, P[2]}, M->C21, v.h21, v.nb, false);
  if (E.status || head_level(2)) return E.status;
  if (fork)
    for (int i = 0; i < 2 && !E.status; ++i)
      E.status = hip_check(hipStreamWaitEvent(main_s, M->ev_join[i], 0), "head join wait");
  if (E.status) return E.status;
  if (M->prof.active()) M->prof.n_fwd++;
  const int st = launch_detect_decode(hl, 3, B, v.nc, v.reg, conf, raw_out, (Cand*)cand, cand_cap,
                                      cand_n, E.s, &M->head_form, sparse);
  if (st || !sparse) return st;
  return launch_head_box(hl, hbx, 3, B, v.reg, (Cand*)cand, cand_cap, cand_n, E.s);
}

// Part 4 must continue the handle's last part 3, part 2 its last part 0 / 1 / 4:
// the same batch on the same workspace
static int check_resume(const Model& M, int part, int B, const void* ws) {
  if (part != 2 && part != 4) return RV_OK;
  const Resume& r = part == 4 ? M.after_stem : M.after_neck;
  RV_CHECK_ARG(r.n >= 0, "forward part %d before any %s of this handle", part,
               part == 4 ? "part 3" : "part 0 / part 1 forward");
  RV_CHECK_ARG(B == r.B && ws == r.ws,
               "forward part %d (B=%d, ws %p) does not continue the last part %d of this handle "
               "(B=%d, ws %p)", part, B, ws, part == 4 ? 3 : 1, r.B, r.ws);
  return RV_OK;
}

}  // namespace rv

using namespace rv;

extern "C" int rv_yolo_create(int variant, const void* dev_packed, int max_B, int in_h, int in_w,
                              void** handle) {
  return rv_yolo_create2(variant, RV_YOLO_DTYPE_BF16, dev_packed, max_B, in_h, in_w, handle);
}

extern "C" int rv_yolo_create2(int variant, int dtype, const void* dev_packed, int max_B, int in_h,
                               int in_w, void** handle) {
  return rv_yolo_create3(variant, dtype, 80, dev_packed, max_B, in_h, in_w, handle);
}

extern "C" int rv_yolo_create3(int variant, int dtype, int nc, const void* dev_packed, int max_B,
                               int in_h, int in_w, void** handle) {
  RV_CHECK_ARG(handle && dev_packed, "null pointer");
  if (const int st = check_plan_args(variant, dtype, nc)) return st;
  RV_CHECK_ARG(max_B > 0 && in_h > 0 && in_w > 0 && in_h % 32 == 0 && in_w % 32 == 0,
               "input %dx%d must be positive multiples of 32", in_h, in_w);
  Model* M = new Model();
  if (!build_def(variant, M->def, dtype, nc)) {
    delete M;
    set_error("unknown variant %d / dtype %d", variant, dtype);
    return RV_EINVAL;
  }
  M->dev = (const uint8_t*)dev_packed;
  for (int i = 0; i < 2; ++i) {
    if (hipStreamCreateWithFlags(&M->side[i], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&M->ev_fork[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&M->ev_join[i], hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      M->side[0] = M->side[1] = nullptr;  // sequential heads
    }
  }
  M->max_B = max_B;
  M->H = in_h;
  M->W = in_w;
  plan(*M);
  M->act_scale.assign(M->bufs.size(), 1.0f);
  M->scales_set = dtype == RV_YOLO_DTYPE_BF16;
  *handle = M;
  return RV_OK;
}

extern "C" int rv_yolo_set_act_scales(void* h, const float* scales, int n) {
  RV_CHECK_ARG(h && scales, "null pointer");
  Model* M = (Model*)h;
  RV_CHECK_ARG(n == (int)M->bufs.size(), "got %d scales, the plan has %d buffers", n,
               (int)M->bufs.size());
  for (int i = 0; i < n; ++i) {
    if (M->bufs[i].esize != 1) continue;
    int e;
    const float f = std::frexp(scales[i], &e);
    RV_CHECK_ARG(scales[i] > 0.f && std::isfinite(scales[i]) && f == 0.5f,
                 "buffer %d: scale %g is not a positive power of two", i, (double)scales[i]);
  }
  for (int i = 0; i < n; ++i) M->act_scale[i] = M->bufs[i].esize == 1 ? scales[i] : 1.0f;
  M->scales_set = true;
  return RV_OK;
}

extern "C" int rv_yolo_buffer_name(void* h, int buf, char* name, int cap) {
  RV_CHECK_ARG(h && name && cap > 0, "bad args");
  Model* M = (Model*)h;
  RV_CHECK_ARG(buf >= 0 && buf < (int)M->bufs.size(), "bad buffer %d", buf);
  strncpy(name, M->bufs[buf].name.c_str(), cap - 1);
  name[cap - 1] = 0;
  return RV_OK;
}

extern "C" int rv_yolo_buffer_esize(void* h, int buf) {
  RV_CHECK_ARG(h, "null handle");
  Model* M = (Model*)h;
  RV_CHECK_ARG(buf >= 0 && buf < (int)M->bufs.size(), "bad buffer %d", buf);
  return M->bufs[buf].esize;
}

extern "C" int rv_yolo_destroy(void* h) {
  delete (Model*)h;
  return RV_OK;
}

extern "C" int rv_yolo_set_option(void* h, int opt, int value) {
  RV_CHECK_ARG(h, "null handle");
  Model* M = (Model*)h;
  switch (opt) {
    case RV_YOLO_OPT_RAW_UNFUSED:
      M->raw_unfused = value != 0;
      return RV_OK;
    case RV_YOLO_OPT_FUSE_C2F:
      M->fuse_c2f = value < 0 ? 0 : (value > 2 ? 2 : value);
      return RV_OK;
    case RV_YOLO_OPT_STEM_X1:
      M->stem_x1 = value != 0;
      return RV_OK;
    case RV_YOLO_OPT_HEAD_STREAMS:
      M->head_streams = value != 0;
      return RV_OK;
    case RV_YOLO_OPT_FUSE_CV1:
      M->fuse_cv1 = value != 0;
      return RV_OK;
    case RV_YOLO_OPT_C2F_TAP_PAIRS:
      M->c2f_tap_pairs = value != 0;
      return RV_OK;
    case RV_YOLO_OPT_STEM6_FUSED:
      M->stem6_fused = value != 0;
      return RV_OK;
    case RV_YOLO_OPT_HEAD_SPARSE:
      RV_CHECK_ARG(value >= 0 && value <= 2, "head sparse option %d not in {0, 1, 2}", value);
      M->head_sparse = value;
      return RV_OK;
    default:
      set_error("unknown yolo option %d", opt);
      return RV_EINVAL;
  }
}

extern "C" size_t rv_yolo_ws_bytes(void* h, int B) {
  if (!h || B <= 0) return 0;
  return ((Model*)h)->ws_bytes(B);
}

extern "C" int rv_yolo_num_anchors(void* h) { return h ? ((Model*)h)->nA : 0; }

extern "C" int rv_yolo_num_classes(void* h) { return h ? ((Model*)h)->def.v.nc : 0; }

extern "C" int rv_yolo_head_form(void* h) { return h ? ((Model*)h)->head_form : RV_EINVAL; }

extern "C" int rv_yolo_cand_segments(void* h) {
  if (!h) return 0;
  const Model* M = (const Model*)h;
  HeadLevel hl[3];
  for (int i = 0; i < 3; ++i) {
    hl[i].H = M->map_h[3 + i];
    hl[i].W = M->map_w[3 + i];
  }
  return decode_segments(hl, 3);
}

extern "C" int rv_yolo_forward(void* h, const uint8_t* lb, int B, void* ws, size_t ws_bytes,
                               float* raw_out, float conf, void* cand, int cand_cap, int* cand_n,
                               void* stream) {
  return rv_yolo_forward_part(h, lb, B, ws, ws_bytes, raw_out, conf, cand, cand_cap, cand_n, stream,
                              0);
}

// part 0: the whole forward (segments A-C).  part 1: A-B, stem .. model.15
// (YOLOv5u: .. model.17, YOLO11: .. model.16; their segments end at the same
// places of the graph)
// (the backbone and the top-down neck: the bandwidth-heavy P2/P3 layers).
// part 2: C, the rest (the bottom-up neck, the Detect heads and the decode:
// small latency-bound launches), reading part 1's activations from the same
// workspace.  A pipelined caller with two workspaces runs part 2 of step j-1
// beside part 1 of step j.  part 3: A (the stem and model.2: the VALU-heavy
// start of part 1) and part 4: B split part 1 in two.
extern "C" int rv_yolo_forward_part(void* h, const uint8_t* lb, int B, void* ws, size_t ws_bytes,
                                    float* raw_out, float conf, void* cand, int cand_cap,
                                    int* cand_n, void* stream, int part) {
  RV_CHECK_ARG(h && ws && (lb || part == 2 || part == 4), "null pointer");
  RV_CHECK_ARG(part >= 0 && part <= 4, "part %d not in {0, 1, 2, 3, 4}", part);
  Model* M = (Model*)h;
  if (const int st = check_resume(*M, part, B, ws)) return st;
  RV_CHECK_ARG((part != 1 && part != 3 && part != 4) || !raw_out,
               "raw_out needs the whole forward (part 0)");
  RV_CHECK_ARG(B > 0 && B <= M->max_B, "B=%d outside (0, %d]", B, M->max_B);
  std::vector<size_t> off = M->offsets(B);
  RV_CHECK_ARG(ws_bytes >= off.back(), "workspace %zu < %zu bytes", ws_bytes, off.back());
  RV_CHECK_ARG(!cand || (cand_n && cand_cap > 0), "candidate buffers incomplete");
  RV_CHECK_ARG(M->scales_set, "fp8 plan: activation scales not set (rv_yolo_set_act_scales)");
  Exec E(M, ws, B, stream, std::move(off), raw_out != nullptr);
  M->trace.clear();
  M->attn_trace.clear();
  M->launches.clear();
  M->fused.clear();
  M->li_base = part == 2 ? M->after_neck.n : (part == 4 ? M->after_stem.n : 0);
  static const int SEGS[5] = {7, 3, 4, 1, 2};  // per part: bit 0 = segment A, 1 = B, 2 = C
  const int segs = SEGS[part];
  auto here = [&] { return Resume{M->li_base + (int)M->launches.size(), B, ws}; };
  const bool v5 = M->def.v.family == kFamilyV5u, v11 = M->def.v.family == kFamilyV11;
  if ((segs & 1) && (v11 ? seg_stem_v11(E, lb) : v5 ? seg_stem_v5u(E, lb) : seg_stem(E, lb)))
    return E.status;
  if (part == 3) {
    M->after_stem = here();
    // part 3 rewrote the start of the workspace: a part 2 now needs the part 4
    // that finishes this forward, not the part 1 of an earlier one
    M->after_neck = Resume{};
  }
  if (segs & 2) {
    if (v11 ? seg_backbone_v11(E) : v5 ? seg_backbone_v5u(E) : seg_backbone(E)) return E.status;
    M->after_neck = here();
  }
  return (segs & 4) ? seg_heads(E, raw_out, conf, cand, cand_cap, cand_n) : RV_OK;
}

// ---- introspection (parity tests / debugging) ------------------------------
extern "C" int rv_yolo_num_buffers(void* h) { return h ? (int)((Model*)h)->bufs.size() : 0; }

extern "C" int rv_yolo_buffer_info(void* h, int B, int buf, int* info, size_t* off_bytes) {
  RV_CHECK_ARG(h && info && off_bytes && B > 0, "bad args");
  Model* M = (Model*)h;
  RV_CHECK_ARG(buf >= 0 && buf < (int)M->bufs.size(), "bad buffer %d", buf);
  *off_bytes = M->offsets(B)[buf];
  const Buf& b = M->bufs[buf];
  info[0] = b.h;
  info[1] = b.w;
  info[2] = b.c;
  info[3] = b.f32 ? 1 : 0;
  return RV_OK;
}

// One TraceRec (24 ints) per conv spec run by the last forward; returns the
// record count
extern "C" int rv_yolo_trace(void* h, int* recs, int max_recs) {
  if (!h) return RV_EINVAL;
  Model* M = (Model*)h;
  const int n = (int)M->trace.size();
  static_assert(sizeof(TraceRec) == 24 * sizeof(int), "rv_yolo_trace: 24 ints per record");
  if (recs)
    for (int i = 0; i < n && i < max_recs; ++i) memcpy(recs + 24 * i, &M->trace[i], 24 * sizeof(int));
  return n;
}

// One AttnRec (9 ints: qkv view {buf, cs, co}, heads, H, W, output view {buf,
// cs, co}) per attention launch of the last forward (YOLO11's PSA blocks, in
// launch order); returns the record count
extern "C" int rv_yolo_attn_trace(void* h, int* recs, int max_recs) {
  if (!h) return RV_EINVAL;
  Model* M = (Model*)h;
  const int n = (int)M->attn_trace.size();
  static_assert(sizeof(AttnRec) == 9 * sizeof(int), "rv_yolo_attn_trace: 9 ints per record");
  if (recs)
    for (int i = 0; i < n && i < max_recs; ++i)
      memcpy(recs + 9 * i, &M->attn_trace[i], 9 * sizeof(int));
  return n;
}
