// What the preprocess translation units share: the CLAHE geometry and blend
// (clahe.hip's appliers, median.hip's fused passes) and the launchers the
// pass runners of preprocess.hip call.  Each kernel lives in the file that
// launches it (-fno-gpu-rdc).
#pragma once
#include "common.h"
#include "lbgeo.h"

// Cache policy of the preprocess's streaming traffic: the frames are read
// twice (LUT pass, then the median pass) and proc is written once and never
// read back on the device.  Non-temporal loads / stores (global_* nt) keep
// those ~600 MB per 32-frame step from evicting the detector's activations
// out of L2 / the Infinity Cache while the passes overlap the forward:
// +1.5 % frames/s in the bench (5 interleaved runs each, profiles/r06/).
// The letterbox output (read by the stem) stays temporal.  Build with
// -DRV_PRE_TEMPORAL for plain loads / stores (A/B).
#ifndef RV_PRE_TEMPORAL
#define RV_LUT_LD(p) __builtin_nontemporal_load(p)
#define RV_MED_LD(p) __builtin_nontemporal_load(p)
#define RV_MED_ST(p, v) __builtin_nontemporal_store((v), (p))
#else
#define RV_LUT_LD(p) (*(p))
#define RV_MED_LD(p) (*(p))
#define RV_MED_ST(p, v) (*(p) = (v))
#endif

namespace rv {

struct ClaheGeo {
  int tiles;       // tiles per axis
  int tw, th;      // tile size in the (possibly reflect-101 extended) image
  int clip_limit;  // integer clip (0 = no clipping)
  float lut_scale; // 255.f / (tw*th)
  float inv_tw, inv_th;
};

// cv::CLAHE_Impl::apply geometry (imgproc/src/clahe.cpp): when either axis
// is not divisible by the grid, BOTH axes are extended by
// tiles - (n % tiles) (a full extra tile-row of padding on a divisible axis).
inline ClaheGeo make_geo(int H, int W, int tiles, double clip) {
  ClaheGeo g;
  g.tiles = tiles;
  if (W % tiles == 0 && H % tiles == 0) {
    g.tw = W / tiles;
    g.th = H / tiles;
  } else {
    g.tw = (W + tiles - (W % tiles)) / tiles;
    g.th = (H + tiles - (H % tiles)) / tiles;
  }
  int area = g.tw * g.th;
  g.lut_scale = 255.0f / (float)area;
  g.clip_limit = 0;
  if (clip > 0.0) {
    g.clip_limit = (int)(clip * area / 256);
    if (g.clip_limit < 1) g.clip_limit = 1;
  }
  g.inv_tw = 1.0f / (float)g.tw;
  g.inv_th = 1.0f / (float)g.th;
  return g;
}

enum ClaheSpace { kYCrCb = 0, kLab = 1 };  // = RV_CHAIN_YCRCB / RV_CHAIN_LAB

// B x tiles^2 LUTs of 256 bytes
inline size_t lut_bytes(int B, int tiles) { return (size_t)B * tiles * tiles * 256; }

// CLAHE_Interpolation_Body per-axis coefficients.
struct Interp {
  int i1, i2;   // clamped tile indices
  float a, a1;  // weight of i2 / of i1
};
__device__ __forceinline__ Interp interp_axis(int p, float inv, int tiles) {
  Interp r;
  const float f = (float)p * inv - 0.5f;
  const int i1 = (int)floorf(f);
  r.a = f - (float)i1;
  r.a1 = 1.0f - r.a;
  r.i1 = i1 < 0 ? 0 : i1;
  r.i2 = (i1 + 1) > tiles - 1 ? tiles - 1 : i1 + 1;
  return r;
}

// res = (L11*xa1 + L12*xa)*ya1 + (L21*xa1 + L22*xa)*ya, then cvRound+saturate.
__device__ __forceinline__ int clahe_blend(int l11, int l12, int l21, int l22, const Interp& ix,
                                           const Interp& iy) {
  const float res = ((float)l11 * ix.a1 + (float)l12 * ix.a) * iy.a1 +
                    ((float)l21 * ix.a1 + (float)l22 * ix.a) * iy.a;
  return sat_u8(__float2int_rn(res));
}

// The launchers.  flags: nullptr, or the chain gate's per-frame flags
// (flags[b] == 0: a frame the gate passed through, which is skipped).

// clahe.hip: the LUTs of every frame, and the standalone applier in -> out.
void launch_clahe_lut(int space, const uint8_t* in, uint8_t* lut, int B, int H, int W, int pitch,
                      const ClaheGeo& g, const int* flags, hipStream_t s);
void launch_clahe_apply(int space, const uint8_t* in, uint8_t* out, const uint8_t* lut, int B,
                        int H, int W, int pitch, const ClaheGeo& g, const int* flags,
                        hipStream_t s);
// Upload the Lab tables to the current device once.  Synchronous: call it
// (rv_lab_init) before a capture.
int ensure_lab_tables();

// median.hip.  The 128 x 32 pass takes CLAHE (`clahe`) when med3_cells_fit(g)
// and emits the letterbox too (lb, lb_out: nullable, and only with `clahe`)
// when med3_lb_fits.  pass_copy (with flags): a passed-through frame's blocks
// copy their raw tile to `out` and letterbox it instead of returning.
bool med3_cells_fit(const ClaheGeo& g);
bool med3_lb_fits(const LbGeo& G, int H, int W);
// CLAHE(YCrCb) + k x k median run as one pass (either median kernel takes it)
bool clahe_median_fuses(const ClaheGeo& g, int k);
void launch_med3(bool clahe, const uint8_t* in, uint8_t* out, const uint8_t* lut, int B, int H,
                 int W, int pitch, const ClaheGeo& g, const LbGeo* lb, uint8_t* lb_out,
                 const int* flags, int pass_copy, hipStream_t s);
template <bool CLAHE>
void dispatch_median(int k, const uint8_t* in, uint8_t* out, const uint8_t* lut, int B, int H,
                     int W, int pitch, const ClaheGeo& g, hipStream_t s,
                     const int* flags = nullptr);

}  // namespace rv
