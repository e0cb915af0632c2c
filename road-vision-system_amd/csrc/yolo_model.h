// The YOLOv8 plan handle behind the rv_yolo_* entries: what yolo.hip (plan and
// forward), yolo_profile.hip (timing) and yolo_tune.hip (autotuner) share.
#pragma once
#include <string>
#include <vector>
#include "yolo_def.h"

namespace rv {

// Activation buffers: element offsets into the caller's workspace, per B
struct View {
  int buf;  // buffer id
  int cs, co;
};

struct Buf {
  std::string name;
  int h, w, c;  // map size, channels
  size_t elems_per_img;
  bool f32;
  int esize;  // bytes per element: 4 (f32 logits), 2 (bf16), 1 (fp8 codes)
};

struct TraceRec {  // 24 ints: rv_yolo_trace copies them out as they lie
  int conv;
  View in;
  int Hin, Win, Ho, Wo;
  View out0;
  int up0;
  View out1;
  int up1;
  View res;
  int in_up;  // virtual concat input (ConvArgs::split): in2 = {-1, 0, 0} without one
  View in2;
  int split;
};

struct AttnRec {  // 9 ints: rv_yolo_attn_trace copies them out as they lie
  View qkv;       // the qkv map: head h in channels co + 128 h + [0, 128)
  int heads, H, W;
  View out;       // o: head h in channels co + 64 h + [0, 64)
};

// A 1x1 conv's virtual concat input (ConvArgs::in2 / split / in_up):
// channels [0, split) from view a (read upsampled 2x when up), the rest
// from view b.
struct VIn {
  View a;
  int up;
  View b;
  int split;
};

// Live per-launch timing of conv_mfma (bench roofline): one hipEvent pair
// per conv launch per forward, recorded on the launch stream.
struct Profile {
  bool on = false;
  int cap_fwd = 0, n_fwd = 0, per_fwd = 0;
  int reps = 1;  // launches of each conv between its event pair (rv_yolo_profile_reps)
  std::vector<hipEvent_t> ev;     // [cap_fwd][per_fwd][2]
  std::vector<double> flops;      // per conv launch index (algorithmic, 2*M*N*K)
  std::vector<double> bytes;      // per conv launch index (algorithmic HBM bytes, launch_bytes)
  std::vector<int> conv_of;       // conv spec index per launch index
  Profile() = default;
  Profile(const Profile&) = delete;
  ~Profile() { reset(0, 0, 1); }
  // off, every event destroyed, then room for max_forwards x slots launches
  int reset(int max_forwards, int slots, int reps_);
  hipEvent_t event(int fwd, int slot, int end) const {
    return ev[((size_t)fwd * per_fwd + slot) * 2 + end];
  }
  bool active() const { return on && n_fwd < cap_fwd; }  // the next forward is recorded
  bool recording(int slot) const { return active() && slot >= 0 && slot < per_fwd; }
  // One slot of the forward being recorded: `run` (a kernel launch returning
  // its status) between the slot's event pair on stream s, `reps` times back
  // to back (the same inputs, the same output: the pair then times reps
  // kernels, not reps dispatch latencies); once when the slot is not recorded.
  // The first forward also notes what the slot stands for.
  template <class F>
  int timed(int slot, hipStream_t s, int conv, double fl, double by, F&& run) {
    const bool rec = recording(slot);
    int st = rec ? hip_check(hipEventRecord(event(n_fwd, slot, 0), s), "profile hipEventRecord")
                 : RV_OK;
    for (int r = 0; r < (rec ? reps : 1) && !st; ++r) st = run();
    if (rec && !st)
      st = hip_check(hipEventRecord(event(n_fwd, slot, 1), s), "profile hipEventRecord");
    if (rec && n_fwd == 0) {
      flops[slot] = fl;
      bytes[slot] = by;
      conv_of[slot] = conv;
    }
    return st;
  }
};

struct Resume {  // where a forward part stopped: what the next part must continue
  int n = -1;    // launches so far (-1: nothing to continue)
  int B = 0;
  const void* ws = nullptr;
};

// YOLOv5nu's fused k6 stem (conv0-k6 + model.1): the default of
// RV_YOLO_OPT_STEM6_FUSED, set by the measurement in DESIGN.md "YOLOv5u"
constexpr int kStem6FusedDefault = 1;

struct Model {
  ModelDef def;
  Profile prof;
  std::vector<TraceRec> trace;  // conv specs run by the last forward (one record each)
  std::vector<AttnRec> attn_trace;  // attention launches of the last forward (YOLO11)
  std::vector<ConvArgs> launches;  // conv kernel launches of the last forward
  std::vector<ConvCfg> tuned;      // per launch index: autotuned config (mr 0 = default)
  struct FusedC2f {
    C2fArgs a;
    int C, N;
    bool shortcut;
  };
  std::vector<FusedC2f> fused;     // fused C2f chains of the last forward (ConvArgs::fused)
  const uint8_t* dev = nullptr;  // packed weights (caller-owned device memory)
  // side streams + events for the forked P3 / P4 Detect heads
  hipStream_t side[2] = {nullptr, nullptr};
  hipEvent_t ev_fork[2] = {nullptr, nullptr}, ev_join[2] = {nullptr, nullptr};
  ~Model() {
    for (int i = 0; i < 2; ++i) {
      // teardown: a failure here leaves nothing to report or undo
      if (side[i]) (void)hipStreamDestroy(side[i]);
      if (ev_fork[i]) (void)hipEventDestroy(ev_fork[i]);
      if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
    }
  }
  int max_B = 0, H = 0, W = 0;
  // forward parts (rv_yolo_forward_part): launch index base of this call (a
  // later part continues the launch numbering) and where part 3 (after_stem)
  // and part 0 / 1 / 4 (after_neck) stopped
  int li_base = 0;
  Resume after_stem, after_neck;
  // fp8 plans: per-buffer activation scales (value = code * scale), powers
  // of two; set by rv_yolo_set_act_scales before the first forward
  std::vector<float> act_scale;
  bool scales_set = false;
  // RV_YOLO_OPT_RAW_UNFUSED: forwards that return the raw prediction run the
  // unfused stem, so every activation (X0 included) is in the workspace
  int raw_unfused = 1;
  // RV_YOLO_OPT_FUSE_C2F: narrow C2f blocks as cv1 + one fused chain launch
  // (1: the hidden-width-16 chains only, 2: width 16 and 32, 0: none)
  int fuse_c2f = 1;
  // RV_YOLO_OPT_STEM_X1: the fused stem also writes X1 (parity tests)
  int stem_x1 = 0;
  int head_streams = 1;            // RV_YOLO_OPT_HEAD_STREAMS
  int fuse_cv1 = 1;                // RV_YOLO_OPT_FUSE_CV1
  int c2f_tap_pairs = 1;           // RV_YOLO_OPT_C2F_TAP_PAIRS
  int head_sparse = 2;             // RV_YOLO_OPT_HEAD_SPARSE: 0 dense, 1 sparse, 2 auto
  int stem6_fused = kStem6FusedDefault;  // RV_YOLO_OPT_STEM6_FUSED
  // decode form of the last forward that reached the decode (rv_yolo_head_form;
  // -1 before one): 0 unfused last stage, 1 fused + LDS class scan, 2 fused
  // with register-resident class scores, 3 the class-only form 2 followed by
  // the sparse box-branch kernel
  int head_form = -1;
  std::vector<Buf> bufs;
  int nA = 0;
  int map_h[6], map_w[6];  // stride 2^i maps

  int newbuf(const std::string& name, int s, int c, bool f32 = false, bool bf16 = false) {
    const int esize = f32 ? 4 : (def.dtype == RV_YOLO_DTYPE_FP8 && !bf16 ? 1 : 2);
    bufs.push_back(Buf{name, map_h[s], map_w[s], c, (size_t)map_h[s] * map_w[s] * c, f32, esize});
    return (int)bufs.size() - 1;
  }
  int buf_of(const std::string& name) const {  // -1: no such buffer
    for (size_t i = 0; i < bufs.size(); ++i)
      if (bufs[i].name == name) return (int)i;
    return -1;
  }
  // buffer ids
  int X0, X1, C2, X2, X3, C4, CAT14, X5, C6, CAT11, X7, C8, X8, SP, CAT20, C12, CAT17, C15,
      X15, C18, X18, C21, X21;
  // YOLOv5u plans: the outputs of model.4 / 6 / 9 / 13 (P3, P4, SPPF and the
  // top-down P4 block), which no concat buffer holds there; CAT14 and CAT11
  // are -1 (both Upsample + Concat pairs are virtual), CAT17 / CAT20 are the
  // yaml's concats 19 / 22 and X15 / X18 / X21 the Detect inputs 17 / 20 / 23.
  // YOLO11 plans: X4 / X6 / X9 likewise (model.4 / 6 / 9), X13 unused (model.13
  // lives in CAT17); CAT17 / CAT20 are the yaml's concats 18 / 21 and X15 / X18
  // / X21 the Detect inputs 16 / 19 / 22 (yolo.hip plan_v11 names the rest)
  int X4 = -1, X6 = -1, X9 = -1, X13 = -1;
  int DA[3], DB[3], HD[3];

  // byte offset of every buffer in a workspace for batch B (256-B aligned),
  // then the workspace size
  std::vector<size_t> offsets(int B) const {
    std::vector<size_t> off(bufs.size() + 1, 0);
    for (size_t i = 0; i < bufs.size(); ++i)
      off[i + 1] = (off[i] + bufs[i].elems_per_img * B * bufs[i].esize + 255) & ~(size_t)255;
    return off;
  }
  size_t ws_bytes(int B) const { return offsets(B).back(); }
};

}  // namespace rv
