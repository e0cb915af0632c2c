// CLAHE for gfx950: the per-tile LUT kernels and the standalone appliers, in
// YCrCb luma and in Lab L (the fused CLAHE + median passes are median.hip's).
//
// Reference interface: src/preprocess/ops/clahe_dehaze.py:13-32 (CLAHEDehaze).
// The arithmetic it delegates to OpenCV is restated here:
//   * BGR<->YCrCb 8U: 14-bit fixed point (common.h); BGR<->Lab 8U: lab.h
//   * cv::CLAHE 8UC1: per-tile 256-bin histogram, integer clip +
//     redistribution, float CDF LUT, float bilinear blend of 4 tile LUTs
//     (cvRound = round-half-even).  Compiled with -ffp-contract=off so the
//     blend rounds exactly like the scalar C++.
//
// The LUT workspace is B x tiles^2 x 256 u8 (16 KB per frame at 8x8).
#include <cstring>
#include <mutex>
#include "clahe.h"
#include "lab.h"

namespace rv {

// Lab tables (lab.h) in device memory, filled once on first LAB use.  Every
// kernel that reads them and the upload live in this translation unit.
__device__ LabTables g_lab;

template <int SPACE>
__device__ __forceinline__ int clahe_luma(int b, int g, int r) {
  if (SPACE == kLab) return lab_l(g_lab, b, g, r);
  return bgr_to_y(b, g, r);
}

// ---------------------------------------------------------------------------
// Kernel A: per (tile, frame) histogram of Y -> clip -> redistribute -> LUT.
// One 256-thread workgroup per tile.
// PACKED (every tile whose counts fit 16 bits; the default at 1080p): 32
// LDS histogram copies, copy = lane & 31, two bins per word as u16 counts:
// bin y of copy c is half y & 1 of word 32 (y >> 1) + c.  An atomic add's
// bank is then (word mod 32/64) = c + 32 ((y >> 1) & 1): the 32 lanes of a
// lane group always hit 32 different banks and never one address, whatever
// the image -- conflict-free.  The reduction reads a row's 32 words as 8
// rotated 16-B quads (conflict-free) and, for tiles below 2^16 pixels, adds
// whole words before extracting the bin's half.  16 KB of LDS, as before.
// Otherwise (tiles of > 2M pixels): 16 u32 copies, copy = lane & 15, word
// 257 c + y.
// (r02/r03: copy = wave x lane & 3, bin-major -- a wave reached only 16 banks
// and up to 16 lanes hit one address, SQ_LDS_BANK_CONFLICT /
// SQ_LDS_IDX_ACTIVE 0.78; the 257-word form alone: 0.68.  r02's one copy
// per lane with u16 counters in 33 KB halved the resident blocks: slower.)
// ---------------------------------------------------------------------------
template <int SPACE, bool PACKED>
__device__ __forceinline__ void clahe_lut_body(const uint8_t* __restrict__ in,
                                               uint8_t* __restrict__ lut, int H, int W, int pitch,
                                               const ClaheGeo& g, int tile, int b, int t) {
  constexpr int kCopies = PACKED ? 32 : 16;
  constexpr int kStride = PACKED ? 0 : 257;  // u32 form: words per copy
  constexpr int kWords = PACKED ? 128 * 32 : kStride * kCopies;
  __shared__ __attribute__((aligned(16))) int hist[kWords];
  __shared__ int wsum[4], wtot[4];
  const int wave = t >> 6;
  const int r_lo = 0, r_hi = g.th;
  const int ty = tile / g.tiles, tx = tile - (tile / g.tiles) * g.tiles;
  const int x0 = tx * g.tw, y0 = ty * g.th;
  const uint8_t* frame = in + (size_t)b * H * pitch;

  for (int i = t; i < kWords; i += 256) hist[i] = 0;
  __syncthreads();

  const bool inside = (x0 + g.tw <= W) && (y0 + g.th <= H);
  const bool vec = inside && (g.tw % 4 == 0) && (pitch % 4 == 0) &&
                   ((((uintptr_t)frame) + (uintptr_t)x0 * 3) % 4 == 0);
  int* h = hist + (t & (kCopies - 1)) * (PACKED ? 1 : kStride);
  auto bump = [&](int y) {
    if constexpr (PACKED)
      atomicAdd(&h[(y >> 1) * 32], 1 << ((y & 1) << 4));
    else
      atomicAdd(&h[y], 1);
  };
  if (vec) {
    // thread t takes the 4-pixel groups i = t + 256 k of the tile (row i /
    // groups, column i % groups), two batches of 4 in flight: batch k + 1's
    // loads are issued before batch k's pixels are binned, and a group's
    // byte offset is stepped incrementally (a division per group was ~20 VALU
    // of the ~70 a group costs)
    const int groups = g.tw >> 2, rows = r_hi - r_lo;
    const int dr = 256 / groups, dg = 256 - dr * groups;  // block-uniform steps
    const int step_b = dr * pitch + dg * 12, wrap_b = pitch - groups * 12;
    const uint8_t* base = frame + (size_t)(y0 + r_lo) * pitch + (size_t)x0 * 3;
    int r = t / groups, gi = t - (t / groups) * groups;
    int off = r * pitch + gi * 12;
    auto advance = [&]() {
      off += step_b;
      r += dr;
      gi += dg;
      if (gi >= groups) {
        gi -= groups;
        ++r;
        off += wrap_b;
      }
    };
    auto load4 = [&](uint32_t (&w)[4][3], bool (&ok)[4]) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ok[u] = r < rows;
        w[u][0] = w[u][1] = w[u][2] = 0;
        if (ok[u]) {
          const uint32_t* q = (const uint32_t*)(base + off);
          w[u][0] = RV_LUT_LD(q);
          w[u][1] = RV_LUT_LD(q + 1);
          w[u][2] = RV_LUT_LD(q + 2);
        }
        advance();
      }
    };
    auto bin4 = [&](const uint32_t (&w)[4][3], const bool (&ok)[4]) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!ok[u]) break;
        const uint32_t w0 = w[u][0], w1 = w[u][1], w2 = w[u][2];
        // bytes little-endian: w0 = b0 g0 r0 b1 | w1 = g1 r1 b2 g2 | w2 = r2 b3 g3 r3
        bump(clahe_luma<SPACE>(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255));
        bump(clahe_luma<SPACE>(w0 >> 24, w1 & 255, (w1 >> 8) & 255));
        bump(clahe_luma<SPACE>((w1 >> 16) & 255, w1 >> 24, w2 & 255));
        bump(clahe_luma<SPACE>((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24));
      }
    };
    uint32_t wa[4][3], wb[4][3];
    bool oka[4], okb[4];
    load4(wa, oka);
    while (oka[0]) {  // groups are in row order: once one is past the tile, so are the rest
      load4(wb, okb);
      bin4(wa, oka);
      if (!okb[0]) break;
      load4(wa, oka);
      bin4(wb, okb);
    }
  } else {
    const int total = g.tw * (r_hi - r_lo);
    for (int i = t; i < total; i += 256) {
      const int r = r_lo + i / g.tw;
      const int c = i - r * g.tw;
      int sy = y0 + r;
      if (sy >= H) sy = reflect101(sy, H);
      int sx = x0 + c;
      if (sx >= W) sx = reflect101(sx, W);
      const uint8_t* p = frame + (size_t)sy * pitch + (size_t)sx * 3;
      bump(clahe_luma<SPACE>(p[0], p[1], p[2]));
    }
  }
  __syncthreads();

  int v = 0;
  if constexpr (PACKED) {
    // bin t = half t & 1 of the 32 copies' words of row t >> 1, read as 8
    // 16-B quads (quad j rotated by the row: lanes of one ds_read_b128 group
    // cover 8 rows x 2 bin halves on 16 distinct bank slots)
    const int rw = t >> 1, sh = (t & 1) << 4;
    const uint4* row = (const uint4*)(hist + rw * 32);
    if ((long)g.tw * g.th <= 65535) {
      // the low halves' sum is the bin's count (<= tile pixels < 2^16): add
      // whole words, extract once
      uint32_t sum = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint4 q = row[(j + rw) & 7];
        sum += q.x + q.y + q.z + q.w;
      }
      v = (int)((sum >> sh) & 0xFFFF);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint4 q = row[(j + rw) & 7];
        v += (int)(((q.x >> sh) & 0xFFFF) + ((q.y >> sh) & 0xFFFF) + ((q.z >> sh) & 0xFFFF) +
                   ((q.w >> sh) & 0xFFFF));
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < kCopies; ++c) v += hist[c * kStride + t];
  }
  if (g.clip_limit > 0) {
    int ex = v > g.clip_limit ? v - g.clip_limit : 0;
    v = v > g.clip_limit ? g.clip_limit : v;
    // block sum of the clipped excess
    for (int off = 32; off > 0; off >>= 1) ex += __shfl_xor(ex, off);
    if ((t & 63) == 0) wsum[wave] = ex;
    __syncthreads();
    const int clipped = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const int batch = clipped / 256;
    const int residual = clipped - batch * 256;
    v += batch;
    if (residual != 0) {
      int step = 256 / residual;
      if (step < 1) step = 1;
      if (t % step == 0 && t / step < residual) v += 1;
    }
  }
  // inclusive prefix sum over the 256 bins: wave scans, then the totals of
  // the lower waves
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(v, off);
    if ((t & 63) >= off) v += y;
  }
  if ((t & 63) == 63) wtot[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += wtot[w];
  const float f = (float)v * g.lut_scale;
  uint8_t* dst = lut + ((size_t)b * g.tiles * g.tiles + tile) * 256;
  dst[t] = (uint8_t)sat_u8(__float2int_rn(f));
}

template <int SPACE, bool PACKED>
__global__ __launch_bounds__(256) void clahe_lut_kernel(const uint8_t* __restrict__ in,
                                                        uint8_t* __restrict__ lut, int H, int W,
                                                        int pitch, ClaheGeo g) {
  clahe_lut_body<SPACE, PACKED>(in, lut, H, W, pitch, g, blockIdx.x, blockIdx.y, threadIdx.x);
}

// u16 counts per (copy, bin) fit: a copy is shared by 8 threads (lanes c,
// c + 32 of 4 waves), each bumping at most 4 ceil(tw/4 th / 256) (vector
// path) or ceil(tw th / 256) pixels
static bool clahe_packed_ok(const ClaheGeo& g) {
  const long per_thread = 4L * (((long)(g.tw / 4) * g.th + 255) / 256) + ((long)g.tw * g.th + 255) / 256;
  return 8 * per_thread <= 65535;
}

// Gate-aware form (rv_preprocess_chain_u8): flags[b] == 0 marks a frame the
// low-contrast gate passed through; its LUTs are never read.
template <int SPACE, bool PACKED>
__global__ __launch_bounds__(256) void clahe_lut_gate_kernel(const uint8_t* __restrict__ in,
                                                             uint8_t* __restrict__ lut, int H,
                                                             int W, int pitch, ClaheGeo g,
                                                             const int* __restrict__ flags) {
  if (flags[blockIdx.y] == 0) return;
  clahe_lut_body<SPACE, PACKED>(in, lut, H, W, pitch, g, blockIdx.x, blockIdx.y, threadIdx.x);
}

template <int SPACE, bool PACKED>
static void launch_clahe_lut_as(const uint8_t* in, uint8_t* lut, int B, int H, int W, int pitch,
                                const ClaheGeo& g, const int* flags, hipStream_t s) {
  const dim3 grid(g.tiles * g.tiles, B);
  if (flags)
    clahe_lut_gate_kernel<SPACE, PACKED><<<grid, 256, 0, s>>>(in, lut, H, W, pitch, g, flags);
  else
    clahe_lut_kernel<SPACE, PACKED><<<grid, 256, 0, s>>>(in, lut, H, W, pitch, g);
}

void launch_clahe_lut(int space, const uint8_t* in, uint8_t* lut, int B, int H, int W, int pitch,
                      const ClaheGeo& g, const int* flags, hipStream_t s) {
  const bool packed = clahe_packed_ok(g);
  if (space == kLab)
    (packed ? launch_clahe_lut_as<kLab, true> : launch_clahe_lut_as<kLab, false>)(
        in, lut, B, H, W, pitch, g, flags, s);
  else
    (packed ? launch_clahe_lut_as<kYCrCb, true> : launch_clahe_lut_as<kYCrCb, false>)(
        in, lut, B, H, W, pitch, g, flags, s);
}

// ---------------------------------------------------------------------------
// Kernel B (standalone CLAHEDehaze): per pixel YCrCb, blend of the 4 tile
// LUTs (read through L2), YCrCb->BGR.  One workgroup per 8-row strip.
// ---------------------------------------------------------------------------
constexpr int kApplyRows = 8;

template <int SPACE>
__global__ __launch_bounds__(256) void clahe_apply_kernel(const uint8_t* __restrict__ in,
                                                          uint8_t* __restrict__ out,
                                                          const uint8_t* __restrict__ lut, int H,
                                                          int W, int pitch, ClaheGeo g,
                                                          const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] == 0) return;  // a frame the gate passed through
  const uint8_t* fin = in + (size_t)b * H * pitch;
  uint8_t* fout = out + (size_t)b * H * pitch;
  const uint8_t* flut = lut + (size_t)b * g.tiles * g.tiles * 256;
  const int yb = blockIdx.y * kApplyRows;
  const int ye = min(H, yb + kApplyRows);
  for (int y = yb; y < ye; ++y) {
    const Interp iy = interp_axis(y, g.inv_th, g.tiles);
    const uint8_t* r1 = flut + (size_t)iy.i1 * g.tiles * 256;
    const uint8_t* r2 = flut + (size_t)iy.i2 * g.tiles * 256;
    const uint8_t* src = fin + (size_t)y * pitch;
    uint8_t* dst = fout + (size_t)y * pitch;
    for (int x = threadIdx.x; x < W; x += 256) {
      const Interp ix = interp_axis(x, g.inv_tw, g.tiles);
      int Y, Cr, Cb;  // (L, a, b) for SPACE == kLab
      if (SPACE == kLab)
        bgr_to_lab(g_lab, src[3 * x], src[3 * x + 1], src[3 * x + 2], Y, Cr, Cb);
      else
        bgr_to_ycrcb(src[3 * x], src[3 * x + 1], src[3 * x + 2], Y, Cr, Cb);
      const int y2 = clahe_blend(r1[ix.i1 * 256 + Y], r1[ix.i2 * 256 + Y], r2[ix.i1 * 256 + Y],
                                 r2[ix.i2 * 256 + Y], ix, iy);
      int bb, gg, rr;
      if (SPACE == kLab)
        lab_to_bgr(g_lab, y2, Cr, Cb, bb, gg, rr);
      else
        ycrcb_to_bgr(y2, Cr, Cb, bb, gg, rr);
      dst[3 * x] = (uint8_t)bb;
      dst[3 * x + 1] = (uint8_t)gg;
      dst[3 * x + 2] = (uint8_t)rr;
    }
  }
}

void launch_clahe_apply(int space, const uint8_t* in, uint8_t* out, const uint8_t* lut, int B,
                        int H, int W, int pitch, const ClaheGeo& g, const int* flags,
                        hipStream_t s) {
  const dim3 grid(1, ceil_div(H, kApplyRows), B);
  if (space == kLab)
    clahe_apply_kernel<kLab><<<grid, 256, 0, s>>>(in, out, lut, H, W, pitch, g, flags);
  else
    clahe_apply_kernel<kYCrCb><<<grid, 256, 0, s>>>(in, out, lut, H, W, pitch, g, flags);
}

static LabTables g_lab_host;
static std::once_flag g_lab_built;
static std::mutex g_lab_mu;
static uint64_t g_lab_devices = 0;  // bit d: tables uploaded to device d

// Upload the Lab tables to the current device once (per device: a process
// may drive several GPUs).  Synchronous; call rv_lab_init() before capture.
int ensure_lab_tables() {
  std::call_once(g_lab_built, [] { build_lab_tables(g_lab_host); });
  int dev = 0;
  int st = hip_check(hipGetDevice(&dev), "hipGetDevice");
  if (st) return st;
  RV_CHECK_ARG(dev >= 0 && dev < 64, "device %d out of range", dev);
  std::lock_guard<std::mutex> lock(g_lab_mu);
  if (g_lab_devices >> dev & 1) return RV_OK;
  st = hip_check(hipMemcpyToSymbol(HIP_SYMBOL(g_lab), &g_lab_host, sizeof(LabTables)),
                 "Lab table upload");
  if (!st) g_lab_devices |= 1ull << dev;
  return st;
}

}  // namespace rv

using namespace rv;

extern "C" int rv_lab_init(void) { return ensure_lab_tables(); }

extern "C" int rv_lab_tables_host(void* out, size_t bytes) {
  RV_CHECK_ARG(out != nullptr && bytes == sizeof(LabTables), "need %zu bytes",
               sizeof(LabTables));
  LabTables t;
  build_lab_tables(t);
  memcpy(out, &t, sizeof(t));
  return RV_OK;
}

