// YOLOv8 conv kernels for gfx950 (the SPPF pool is sppf.hip, the Detect
// decode detect.hip).
//
// Reference: the YOLOv8 graph Ultralytics runs inside model.predict
// (src/detect/yolo_ultralytics.py:28-35; Conv = conv + fused BN + SiLU,
// C2f, SPPF, Detect with DFL).  Layout: NHWC bf16 activations, weights packed
// [Cout_pad16][ky][kx][Cin_pad32] bf16 so every MFMA operand fragment is one
// 16-byte load.
//
// The kernels, in the order launch_conv tries them: conv1x1_direct_kernel
// (1x1 convs with a virtual concat input, and tuned 1x1 layers),
// conv_patch_kernel (the LDS-staged implicit GEMM every k in {1,3},
// s in {1,2} layer of the plans runs) and conv_mfma_kernel, the generic
// fallback for the shapes rv_conv_bf16 supports but the patch kernel has no
// configuration for (a 1x1 stride-2 conv, images of Hin*Win >= 2^24 pixels).
// Each kernel has its own translation unit (conv_direct.hip, conv_patch.hip,
// conv_generic.hip) with its launcher; this file chooses and checks the
// configuration; conv_kernels.h is what they share.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include "conv_kernels.h"

namespace rv {

// a virtual concat / upsampled input (ConvArgs::split, in_up) is read by
// the direct 1x1 kernel only
static bool vcat(const ConvArgs& a) { return a.split > 0 || a.in_up; }

// (MR, NR) tiles built for the patch and the direct kernel
#define RV_TILE_ROW(M_, N_) {M_, N_},
static const int kTiles[][2] = {RV_TILES(RV_TILE_ROW)};
#undef RV_TILE_ROW

// Is c a valid configuration of layer a?  For the patch kernel (kinds 0 and
// 2) also its geometry and LDS bytes: a launch resolves them once, here.
static bool resolve(const ConvArgs& a, const ConvCfg& c, PatchGeo& g, size_t& smem) {
  if (a.ch_w &&  // chained 1x1: the patch kernel's CH form, one cout tile covering Cout
      (c.kind == 1 || a.in8 || 16 * c.mr < a.Cout || 16 * c.mr - a.Cout >= 16 || a.res || a.out1 ||
       a.out0_up || a.g2_cout0 > 0 || vcat(a) || !epi_fast(a)))
    return false;
  if (c.kind == 1) return !a.in8 && direct_ok(a, c);
  if ((c.kind != 0 && c.kind != 2) || vcat(a)) return false;
  if (!patch_built(c.kind == 2 ? 8 : 4, a.in8 != 0, a.ch_w != nullptr, c.mr, c.nr, a.k, a.stride,
                   c.resw != 0))
    return false;
  if (a.in8 && (a.Cin % 16 || a.in_co % 16 || a.in_cs % 16 ||
                 (a.g2_cout0 > 0 && (a.g2_Cin % 16 || a.g2_in_co % 16))))
    return false;  // whole 16-B quarters of fp8 channels
  const int T = (a.Cout + 15) / 16;
  if (c.mr > T && c.mr > 1) return false;
  if (a.g2_cout0 > 0 && a.g2_cout0 % (16 * c.mr) != 0) return false;  // tiles inside one group
  return patch_geo(a, c, g, smem);
}

bool conv_cfg_ok(const ConvArgs& a, const ConvCfg& c) {
  PatchGeo g;
  size_t sm;
  return resolve(a, c, g, sm);
}

int launch_conv_cfg(const ConvArgs& a, const ConvCfg& c, hipStream_t s) {
  PatchGeo g;
  size_t sm;
  if (!resolve(a, c, g, sm)) {
    set_error("conv config MR=%d NR=%d G=%d resw=%d not valid for this layer", c.mr, c.nr, c.G,
              c.resw);
    return RV_EINVAL;
  }
  return c.kind == 1 ? launch_conv_direct(a, c, s) : launch_conv_patch(a, c, g, sm, s);
}

// (conv_kernels.h, at ConvLaunchState)
int conv_grid_x(ConvLaunchState& st, const void* fn, int threads, size_t smem, int ytiles, int ntiles,
                int persist) {
  if (!st.attr) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      set_error("hipFuncSetAttribute: %s", hipGetErrorString(e));
      return -(int)e;
    }
    st.attr = true;
  }
  int occ = 0;
  for (int i = 0; i < 16; ++i)
    if (st.occ_smem[i] == smem) occ = st.occ_val[i];
  if (!occ) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, threads, smem) != hipSuccess || occ < 1)
      occ = 1;
    (void)hipGetLastError();
    for (int i = 0; i < 16; ++i)
      if (st.occ_smem[i] == 0) {
        st.occ_smem[i] = smem;
        st.occ_val[i] = occ;
        break;
      }
  }
  return xcd_grid(std::max(1, num_cus() * occ / ytiles), ntiles, persist != 0);
}

// Every valid configuration of this layer (the autotuner's search space):
// each tile with resident weights (largest G that fits) and with staged
// weights (the largest G that fits, and G = 1); persistent grid or one
// block per pixel tile.
int conv_candidates(const ConvArgs& a, ConvCfg* out, int cap) {
  int n = 0;
  const int nch = conv_nch(a);
  for (const auto& t : kTiles) {
    for (int kind = 0; kind <= 2; kind += 2)  // 4- and 8-wave patch kernels
      for (int resw = 1; resw >= 0; --resw) {
        int gbest = 0;
        for (int G = nch; G >= 1 && !gbest; --G)
          if (conv_cfg_ok(a, ConvCfg{t[0], t[1], G, resw, 1, kind})) gbest = G;
        if (!gbest) continue;
        // persistent grid, and (for layers with few tiles) one block per tile
        for (int persist = 1; persist >= 0; --persist) {
          if (n < cap) out[n] = ConvCfg{t[0], t[1], gbest, resw, persist, kind};
          ++n;
          if (!resw && gbest > 1) {
            if (n < cap) out[n] = ConvCfg{t[0], t[1], 1, resw, persist, kind};
            ++n;
          }
        }
      }
    // 1x1 layers: the direct-B kernel
    for (int persist = 1; persist >= 0; --persist) {
      const ConvCfg d{t[0], t[1], 1, 1, persist, 1};
      if (!a.in8 && direct_ok(a, d)) {
        if (n < cap) out[n] = d;
        ++n;
      }
    }
  }
  return n;
}

// Default (untuned) choice: the largest wave tile that still fills the
// machine (blocks >= 3/4 of CUs x co-resident blocks), resident weights and
// the largest chunk group that fit.
static bool default_cfg(const ConvArgs& a, ConvCfg& best) {
  const int T = (a.Cout + 15) / 16;
  double best_fill = -1.0;
  bool found = false;
  for (const auto& t : kTiles) {
    if (ceil_div(T, t[0]) * t[0] - T > (t[0] > 1 ? 1 : 0)) continue;
    if (a.k == 3 && t[0] > 5) continue;  // keep 3x3 weight stages modest
    ConvCfg cand{0, 0, 0, 0, 1};
    PatchGeo g;
    size_t sm = 0;
    bool ok = false;
    for (int resw = 1; resw >= 0 && !ok; --resw)
      for (int G = conv_nch(a); G >= 1 && !ok; --G) {
        cand = ConvCfg{t[0], t[1], G, resw, 1};
        ok = resolve(a, cand, g, sm);
      }
    if (!ok) continue;
    const long blocks = (long)a.B * g.tiles_x * g.tiles_y * ceil_div(T, t[0]);
    const int bpc = std::max(1, std::min(4, (int)((160 * 1024) / sm)));
    const double fill = (double)blocks / (256.0 * bpc);
    if (fill >= 0.75) {
      best = cand;
      return true;
    }
    if (fill > best_fill) {
      best_fill = fill;
      best = cand;
      found = true;
    }
  }
  return found;
}

int launch_conv(const ConvArgs& a, hipStream_t s) {
  if (vcat(a)) {  // the direct 1x1 kernel: the widest channel tile that divides Cout and fits
    const int T = (a.Cout + 15) / 16;
    ConvCfg c{1, 1, 1, 1, 1, 1};
    for (const int mr : {8, 4, 2})
      if (T % mr == 0 && conv_cfg_ok(a, ConvCfg{mr, 1, 1, 1, 1, 1})) {
        c.mr = mr;
        break;
      }
    if (!conv_cfg_ok(a, c)) {
      set_error("virtual concat input (split %d, up %d) needs a bf16 1x1 conv", a.split, a.in_up);
      return RV_EINVAL;
    }
    return launch_conv_cfg(a, c, s);
  }
  ConvCfg c{0, 0, 1, 0, 1};
  if (default_cfg(a, c)) {
    static const int dbg = getenv("RV_CONV_DEBUG") ? atoi(getenv("RV_CONV_DEBUG")) : 0;
    if (dbg)
      fprintf(stderr, "[conv] %dx%d k%d s%d Cin %d Cout %d -> MR=%d NR=%d G=%d resw=%d\n", a.Ho, a.Wo,
              a.k, a.stride, a.Cin, a.Cout, c.mr, c.nr, c.G, c.resw);
    return launch_conv_cfg(a, c, s);
  }
  if (a.ch_w) {
    set_error("chained 1x1 conv (Cout %d, k%d s%d) has no patch-kernel configuration", a.Cout, a.k,
              a.stride);
    return RV_EINVAL;
  }
  if (a.in8) {
    set_error("fp8 conv (Cin %d, Cout %d, k%d s%d) has no patch-kernel configuration", a.Cin,
              a.Cout, a.k, a.stride);
    return RV_EINVAL;
  }
  if (a.g2_cout0 > 0) {
    set_error("grouped conv (Cout %d, split %d) has no patch-kernel configuration", a.Cout,
              a.g2_cout0);
    return RV_EINVAL;
  }
  return launch_conv_generic(a, s);
}

// One bf16 conv (k 1 or 3, pad k / 2, SiLU optional, optional bf16 residual
// of the output's shape) through the production launcher, for layer tests:
// the weights packed as yolo_def.hip packs them ([Cout_pad16][k*k][Cin_pad32]
// bf16), the bias padded to Cout_pad16.  cfg6 (nullable): an explicit
// {MR, NR, G, resw, persist, kind} configuration.  The supported channel
// counts, strides and alignments are checked here (include/rvhip.h).
}  // namespace rv
extern "C" int rv_conv_bf16(const void* in, int B, int Hin, int Win, int Cin, int in_cs,
                            const void* w, const float* bias, int Cout, int k, int stride, void* out,
                            int out_cs, const void* res, int res_cs, int act, const int* cfg6,
                            void* stream) {
  using namespace rv;
  RV_CHECK_ARG(in && w && bias && out, "null pointer");
  RV_CHECK_ARG(B >= 1 && Hin >= 1 && Win >= 1 && Cin >= 1 && Cout >= 1, "bad shape");
  RV_CHECK_ARG((k == 1 || k == 3) && (stride == 1 || stride == 2), "k %d stride %d", k, stride);
  RV_CHECK_ARG(in_cs >= Cin && out_cs >= Cout && (!res || res_cs >= Cout), "channel strides");
  // the kernels' access widths (include/rvhip.h): 16-byte input loads of 8
  // channels, 8-byte output stores / residual loads of 4 channels
  RV_CHECK_ARG(Cin % 8 == 0 && in_cs % 8 == 0 && (uintptr_t)in % 16 == 0,
               "input: Cin %d and in_cs %d must be multiples of 8, in 16-byte aligned", Cin, in_cs);
  RV_CHECK_ARG(Cout % 4 == 0 && out_cs % 4 == 0 && (uintptr_t)out % 8 == 0,
               "output: Cout %d and out_cs %d must be multiples of 4, out 8-byte aligned", Cout,
               out_cs);
  RV_CHECK_ARG(!res || (res_cs % 4 == 0 && (uintptr_t)res % 8 == 0),
               "residual: res_cs %d must be a multiple of 4, res 8-byte aligned", res_cs);
  RV_CHECK_ARG((uintptr_t)w % 16 == 0 && (uintptr_t)bias % 16 == 0,
               "w and bias must be 16-byte aligned");
  // 32-bit element indices in the kernels
  RV_CHECK_ARG((double)B * Hin * Win * in_cs < 2147483648.0 &&
                   (double)B * Hin * Win * out_cs < 2147483648.0 &&
                   (!res || (double)B * Hin * Win * res_cs < 2147483648.0),
               "view of B=%d %dx%d pixels exceeds 2^31 elements", B, Hin, Win);
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.in = (const bf16_t*)in;
  a.in_cs = in_cs;
  a.Hin = Hin;
  a.Win = Win;
  a.Cin = Cin;
  a.w = (const bf16_t*)w;
  a.bias = bias;
  a.Cout = Cout;
  a.k = k;
  a.stride = stride;
  a.pad = k / 2;
  a.Ho = (Hin + 2 * a.pad - k) / stride + 1;
  a.Wo = (Win + 2 * a.pad - k) / stride + 1;
  a.B = B;
  a.out0 = out;
  a.out0_cs = out_cs;
  a.res = (const bf16_t*)res;
  a.res_cs = res_cs;
  a.act = act ? 1 : 0;
  const hipStream_t s = (hipStream_t)stream;
  if (cfg6) {
    const ConvCfg c{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5]};
    return launch_conv_cfg(a, c, s);
  }
  return launch_conv(a, s);
}
