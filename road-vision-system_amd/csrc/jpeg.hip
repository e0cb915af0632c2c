// Baseline JPEG, device half: coefficient records (jpeg_host.h entropy-decodes
// them on the reader threads; layout in include/rvhip.h) -> interleaved BGR.
// Restates libjpeg's default decode arithmetic bit for bit: dequantise, the
// "islow" 8x8 IDCT (13-bit constants, column pass descaled by 11, row pass by
// 18), "fancy" triangle chroma upsampling, 16-bit fixed-point YCbCr -> RGB.
//
// One fused kernel.  A workgroup owns a 128 x 64 pixel tile of one frame:
//   1. IDCT of every block the tile needs into planar u8 tiles in LDS, eight
//      lanes per block: lane t loads coefficient row t (one 16-byte load) and
//      its quant row, the 8x8 goes through a stride-9 LDS scratch for the
//      column pass and back for the row pass (conflict-free both ways: 9 t +
//      72 b hits 64 distinct banks over a wave).  Subsampled chroma also gets
//      the ring of blocks around the tile, for the one-sample halo the
//      triangle filter reads across MCU borders (4:2:0: 248 blocks for 192).
//   2. upsample + colour from LDS, four pixels per lane, 12-byte stores of
//      consecutive lanes (non-temporal: the frame is read next by another
//      kernel, never by this one).
// Nothing branches on block content; edge replication is an index clamp to
// the cropped plane, so every LDS read lands in a block that was decoded.
#include "common.h"
#include "jpeg_host.h"

namespace rv {

namespace {

constexpr int kTileW = 128, kTileH = 64;  // pixels per workgroup
constexpr int kBlocksPerPass = 32;        // 256 lanes / 8 lanes per block
constexpr int kScrStride = 72;            // dwords per block of transpose scratch (8 rows of 9)

__device__ __forceinline__ int opaque(int v) {  // see ingest.hip: keeps v_ashr_pk_u8_i32 away
  asm volatile("" : "+v"(v));
  return v;
}

// libjpeg jidctint.c butterfly on eight values, descaled by s
__device__ __forceinline__ void idct8(int (&x)[8], int s) {
  int z1 = (x[2] + x[6]) * 4433;
  const int t2 = z1 - x[6] * 15137, t3 = z1 + x[2] * 6270;
  const int t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * 9633;
  a0 *= 2446;
  a1 *= 16819;
  a2 *= 25172;
  a3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  const int r = 1 << (s - 1);
  x[0] = (t10 + a3 + r) >> s;
  x[7] = (t10 - a3 + r) >> s;
  x[1] = (t11 + a2 + r) >> s;
  x[6] = (t11 - a2 + r) >> s;
  x[2] = (t12 + a1 + r) >> s;
  x[5] = (t12 - a1 + r) >> s;
  x[3] = (t13 + a0 + r) >> s;
  x[4] = (t13 - a0 + r) >> s;
}

// Geometry of one component inside a tile, for sampling factors FH x FV
// (1 or 2: full-resolution samples per component sample).
template <int FH, int FV>
struct TileGeom {
  static constexpr int kHaloX = FH == 2 ? 1 : 0, kHaloY = FV == 2 ? 1 : 0;
  static constexpr int kNbx = kTileW / 8 / FH + 2 * kHaloX, kNby = kTileH / 8 / FV + 2 * kHaloY;
  static constexpr int kBlocks = kNbx * kNby;
  static constexpr int kStride = kNbx * 8;  // bytes per row of the LDS plane
  static_assert(kStride * kNby * 8 <= kTileW * kTileH, "plane tile larger than its LDS slot");
};

struct CompArgs {
  const uint8_t* coef;  // this component's block grid in the record
  const uint8_t* qt;    // its quant table
  int gw, gh;           // block grid size
  int dw, dh;           // cropped plane size in samples
};

// Four horizontally adjacent samples of a component, upsampled to full
// resolution, for pixels (gx .. gx + 3, gy); gx is a multiple of four.
template <int FH, int FV>
__device__ __forceinline__ void sample4(const uint8_t* plane, const CompArgs& a, int tx, int ty,
                                        int gx, int gy, int (&out)[4]) {
  using G = TileGeom<FH, FV>;
  const int ox = (tx * (kTileW / 8 / FH) - G::kHaloX) * 8;
  const int oy = (ty * (kTileH / 8 / FV) - G::kHaloY) * 8;
  if (FH == 1) {
    const uint32_t w = *(const uint32_t*)(plane + (gy / FV - oy) * G::kStride + (gx - ox));
    out[0] = w & 255;
    out[1] = (w >> 8) & 255;
    out[2] = (w >> 16) & 255;
    out[3] = w >> 24;
    return;
  }
  const int cy = gy / FV, cx = gx >> 1;
  const uint8_t* r0 = plane + (cy - oy) * G::kStride - ox;
  if (a.dw <= 2) {  // libjpeg replicates when the plane is at most two samples wide
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = r0[min((gx + i) >> 1, a.dw - 1)];
    return;
  }
  const int c0 = max(cx - 1, 0), c1 = min(cx, a.dw - 1), c2 = min(cx + 1, a.dw - 1),
            c3 = min(cx + 2, a.dw - 1);
  if (FV == 1) {
    const int p0 = r0[c0], p1 = r0[c1], p2 = r0[c2], p3 = r0[c3];
    out[0] = (3 * p1 + p0 + 1) >> 2;
    out[1] = (3 * p1 + p2 + 2) >> 2;
    out[2] = (3 * p2 + p1 + 1) >> 2;
    out[3] = (3 * p2 + p3 + 2) >> 2;
  } else {
    const int cyn = (gy & 1) ? min(cy + 1, a.dh - 1) : max(cy - 1, 0);
    const uint8_t* r1 = plane + (cyn - oy) * G::kStride - ox;
    const int s0 = 3 * r0[c0] + r1[c0], s1 = 3 * r0[c1] + r1[c1], s2 = 3 * r0[c2] + r1[c2],
              s3 = 3 * r0[c3] + r1[c3];
    out[0] = (3 * s1 + s0 + 8) >> 4;
    out[1] = (3 * s1 + s2 + 7) >> 4;
    out[2] = (3 * s2 + s1 + 8) >> 4;
    out[3] = (3 * s2 + s3 + 7) >> 4;
  }
}

// Where block j of a component's tile list lies: in the LDS plane (lbx, lby)
// and in the record's block grid (gbx, gby).
template <int FH, int FV>
__device__ __forceinline__ void locate(int j, int tx, int ty, int& lbx, int& lby, int& gbx,
                                       int& gby, int& stride) {
  using G = TileGeom<FH, FV>;
  lbx = j % G::kNbx;
  lby = j / G::kNbx;
  gbx = tx * (kTileW / 8 / FH) - G::kHaloX + lbx;
  gby = ty * (kTileH / 8 / FV) - G::kHaloY + lby;
  stride = G::kStride;
}

// IDCT of one block by eight lanes (t = 0..7) into its LDS plane.  Called by
// every lane of the workgroup in uniform control flow (it has barriers);
// lanes whose block lies outside the grid only keep step.
__device__ __forceinline__ void idct_block(uint8_t* plane, int stride, int* scr, const CompArgs& a,
                                           int lbx, int lby, int gbx, int gby, int t) {
  const bool inside = gbx >= 0 && gbx < a.gw && gby >= 0 && gby < a.gh;
  int x[8];
  if (inside) {
    const int4 c = *(const int4*)(a.coef + ((size_t)gby * a.gw + gbx) * 128 + t * 16);
    const uint4 q = *(const uint4*)(a.qt + t * 16);
    x[0] = (int)(short)c.x * (int)(q.x & 0xFFFF);
    x[1] = (c.x >> 16) * (int)(q.x >> 16);
    x[2] = (int)(short)c.y * (int)(q.y & 0xFFFF);
    x[3] = (c.y >> 16) * (int)(q.y >> 16);
    x[4] = (int)(short)c.z * (int)(q.z & 0xFFFF);
    x[5] = (c.z >> 16) * (int)(q.z >> 16);
    x[6] = (int)(short)c.w * (int)(q.w & 0xFFFF);
    x[7] = (c.w >> 16) * (int)(q.w >> 16);
#pragma unroll
    for (int u = 0; u < 8; ++u) scr[t * 9 + u] = x[u];  // row t of the dequantised block
  }
  __syncthreads();
  if (inside) {
#pragma unroll
    for (int v = 0; v < 8; ++v) x[v] = scr[v * 9 + t];  // column t
    idct8(x, 11);
#pragma unroll
    for (int v = 0; v < 8; ++v) scr[v * 9 + t] = x[v];
  }
  __syncthreads();
  if (inside) {
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = scr[t * 9 + u];  // row t of the column pass
    idct8(x, 18);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      lo |= (uint32_t)opaque(sat_u8(x[u] + 128)) << (8 * u);
      hi |= (uint32_t)opaque(sat_u8(x[u + 4] + 128)) << (8 * u);
    }
    *(uint2*)(plane + (lby * 8 + t) * stride + lbx * 8) = make_uint2(lo, hi);
  }
}

template <int SAMP>
__device__ __forceinline__ void decode_tile(const uint8_t* rec, uint8_t* out, int W, int H,
                                            uint8_t (*planes)[kTileW * kTileH],
                                            int (*scratch)[kScrStride]) {
  constexpr int FH = SAMP == 1 || SAMP == 2 ? 2 : 1, FV = SAMP == 2 ? 2 : 1;
  constexpr int NC = SAMP == 3 ? 1 : 3;
  using GY = TileGeom<1, 1>;
  using GC = TileGeom<FH, FV>;
  const int tx = blockIdx.x, ty = blockIdx.y, tid = threadIdx.x;
  const int mx = (W + 8 * FH - 1) / (8 * FH), my = (H + 8 * FV - 1) / (8 * FV);
  CompArgs a[NC];
  {
    const uint8_t* p = rec + rvjpeg::kHeaderBytes + NC * 128;
    for (int c = 0; c < NC; ++c) {
      a[c].gw = c == 0 ? mx * FH : mx;
      a[c].gh = c == 0 ? my * FV : my;
      a[c].dw = c == 0 ? W : (W + FH - 1) / FH;
      a[c].dh = c == 0 ? H : (H + FV - 1) / FV;
      a[c].coef = p;
      a[c].qt = rec + rvjpeg::kHeaderBytes + c * 128;
      p += (size_t)a[c].gw * a[c].gh * 128;
    }
  }
  constexpr int kTotal = GY::kBlocks + (NC - 1) * GC::kBlocks;
  const int t = tid & 7;
  int* scr = scratch[tid >> 3];
  for (int base = 0; base < kTotal; base += kBlocksPerPass) {
    // lanes past the list's end redo its last block (same values to the same
    // addresses), so the barriers in idct_block stay uniform
    const int i = min(base + (tid >> 3), kTotal - 1);
    int c = 0, lbx, lby, gbx, gby, stride;
    if (NC == 1 || i < GY::kBlocks) {
      locate<1, 1>(i, tx, ty, lbx, lby, gbx, gby, stride);
    } else {
      const int j = i - GY::kBlocks;
      c = j < GC::kBlocks ? 1 : 2;
      locate<FH, FV>(j - (c - 1) * GC::kBlocks, tx, ty, lbx, lby, gbx, gby, stride);
    }
    CompArgs ca = a[0];
#pragma unroll
    for (int k = 1; k < NC; ++k)
      if (c == k) ca = a[k];
    idct_block(planes[c], stride, scr, ca, lbx, lby, gbx, gby, t);
  }
  __syncthreads();

  for (int u = tid; u < (kTileW / 4) * kTileH; u += 256) {
    const int ly = u / (kTileW / 4), lx = (u % (kTileW / 4)) * 4;
    const int gx = tx * kTileW + lx, gy = ty * kTileH + ly;
    if (gx >= W || gy >= H) continue;
    int y[4], cb[4], cr[4];
    sample4<1, 1>(planes[0], a[0], tx, ty, gx, gy, y);
    uint32_t px[4];
    if (NC == 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) px[i] = (uint32_t)y[i] * 0x010101u;
    } else {
      sample4<FH, FV>(planes[1], a[NC > 1 ? 1 : 0], tx, ty, gx, gy, cb);
      sample4<FH, FV>(planes[2], a[NC > 1 ? 2 : 0], tx, ty, gx, gy, cr);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u8 = cb[i] - 128, v8 = cr[i] - 128;
        const int r = opaque(sat_u8(y[i] + ((91881 * v8 + 32768) >> 16)));
        const int g = opaque(sat_u8(y[i] + ((-22554 * u8 - 46802 * v8 + 32768) >> 16)));
        const int b = opaque(sat_u8(y[i] + ((116130 * u8 + 32768) >> 16)));
        px[i] = (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
      }
    }
    uint8_t* d = out + ((size_t)gy * W + gx) * 3;
    if (gx + 4 <= W && ((uintptr_t)d & 3) == 0) {
      uint32_t* d4 = (uint32_t*)d;
      __builtin_nontemporal_store(px[0] | (px[1] << 24), d4);
      __builtin_nontemporal_store((px[1] >> 8) | (px[2] << 16), d4 + 1);
      __builtin_nontemporal_store((px[2] >> 16) | (px[3] << 8), d4 + 2);
    } else {
      const int n = min(4, W - gx);
      for (int i = 0; i < n; ++i) {
        d[3 * i] = px[i] & 255;
        d[3 * i + 1] = (px[i] >> 8) & 255;
        d[3 * i + 2] = (px[i] >> 16) & 255;
      }
    }
  }
}

// Bytes of a W x H record with this sampling code (jpeg_host.cpp layout()).
__device__ __forceinline__ size_t record_bytes_dev(int W, int H, int samp) {
  const int fh = samp == 1 || samp == 2 ? 2 : 1, fv = samp == 2 ? 2 : 1, nc = samp == 3 ? 1 : 3;
  const size_t mx = (W + 8 * fh - 1) / (8 * fh), my = (H + 8 * fv - 1) / (8 * fv);
  return rvjpeg::kHeaderBytes + (size_t)nc * 128 + mx * my * (fh * fv + nc - 1) * 128;
}

__global__ __launch_bounds__(256) void jpeg_coef_to_bgr_kernel(const uint8_t* __restrict__ records,
                                                               size_t stride,
                                                               uint8_t* __restrict__ bgr, int W,
                                                               int H) {
  __shared__ __attribute__((aligned(16))) uint8_t planes[3][kTileW * kTileH];
  __shared__ int scratch[kBlocksPerPass][kScrStride];
  const uint8_t* rec = records + (size_t)blockIdx.z * stride;
  const int* hdr = (const int*)rec;
  // a record that is not a W x H record of this stride leaves its frame
  // unwritten: nothing below depends on anything else the record says
  const int samp = hdr[3];
  if ((uint32_t)hdr[0] != rvjpeg::kMagic || hdr[1] != W || hdr[2] != H || samp < 0 || samp > 3 ||
      record_bytes_dev(W, H, samp) > stride)
    return;
  uint8_t* out = bgr + (size_t)blockIdx.z * H * W * 3;
  switch (samp) {  // uniform over the workgroup
    case 0: decode_tile<0>(rec, out, W, H, planes, scratch); break;
    case 1: decode_tile<1>(rec, out, W, H, planes, scratch); break;
    case 2: decode_tile<2>(rec, out, W, H, planes, scratch); break;
    default: decode_tile<3>(rec, out, W, H, planes, scratch); break;
  }
}

thread_local char g_jpeg_err[rvjpeg::kErrLen];

}  // namespace

extern "C" int rv_jpeg_probe(const uint8_t* data, size_t n, int* info) {
  RV_CHECK_ARG(data != nullptr && info != nullptr, "null pointer");
  rvjpeg::Info i;
  if (rvjpeg::probe(data, n, &i, g_jpeg_err) != rvjpeg::kOk) {
    set_error("%s", g_jpeg_err);
    return RV_EINVAL;
  }
  info[0] = i.W;
  info[1] = i.H;
  info[2] = i.sampling;
  info[3] = i.ncomp;
  return RV_OK;
}

extern "C" size_t rv_jpeg_record_bytes(int W, int H, int sampling) {
  rvjpeg::Layout l;
  return rvjpeg::layout(W, H, sampling, &l) == rvjpeg::kOk ? l.record_bytes : 0;
}

extern "C" int rv_jpeg_record_layout(int W, int H, int sampling, int64_t* layout) {
  RV_CHECK_ARG(layout != nullptr, "null pointer");
  rvjpeg::Layout l;
  RV_CHECK_ARG(rvjpeg::layout(W, H, sampling, &l) == rvjpeg::kOk,
               "JPEG record of %dx%d, sampling code %d", W, H, sampling);
  layout[0] = (int64_t)l.record_bytes;
  layout[1] = l.ncomp;
  layout[2] = (int64_t)l.qt_off;
  for (int c = 0; c < 3; ++c) {
    layout[3 + c] = (int64_t)l.coef_off[c];
    layout[6 + c] = l.blocks_w[c];
    layout[9 + c] = l.blocks_h[c];
  }
  return RV_OK;
}

extern "C" int rv_jpeg_decode_coef(const uint8_t* data, size_t n, uint8_t* record, size_t cap) {
  RV_CHECK_ARG(data != nullptr && record != nullptr, "null pointer");
  if (rvjpeg::decode(data, n, record, cap, nullptr, g_jpeg_err) != rvjpeg::kOk) {
    set_error("%s", g_jpeg_err);
    return RV_EINVAL;
  }
  return RV_OK;
}

extern "C" int rv_jpeg_coef_to_bgr_u8(const uint8_t* records, size_t record_stride, int S, int W,
                                      int H, uint8_t* bgr, void* stream) {
  RV_CHECK_ARG(records != nullptr && bgr != nullptr, "null pointer");
  RV_CHECK_ARG(S >= 0 && S <= 65535 && W >= 1 && H >= 1 && W <= 65535 && H <= 65535,
               "bad JPEG batch S=%d W=%d H=%d", S, W, H);
  RV_CHECK_ARG(record_stride % 16 == 0 && (uintptr_t)records % 16 == 0,
               "records and their stride must be 16-byte aligned");
  RV_CHECK_ARG(record_stride >= rv_jpeg_record_bytes(W, H, RV_JPEG_GRAY),
               "record stride %zu too small for %dx%d", record_stride, W, H);
  if (S == 0) return RV_OK;
  const dim3 grid(ceil_div(W, kTileW), ceil_div(H, kTileH), S);
  jpeg_coef_to_bgr_kernel<<<grid, 256, 0, as_stream(stream)>>>(records, record_stride, bgr, W, H);
  return launch_status("rv_jpeg_coef_to_bgr_u8");
}

}  // namespace rv
