// Directional rain-streak removal in integer arithmetic, bit for bit
// tests/streak_ref.py: rv_streak_derain_u8 and the streak pass of
// rv_preprocess_chain_u8 (include/rvhip.h states the arithmetic).
//
//   streak_row_kernel     T = the thresholded horizontal white top-hat of the
//                         gray, one row segment per block, four pixels a thread
//   streak_erode_kernel   E = emin_n(hmax_k(T)): a 64 x 64 tile with its line
//                         halo in LDS, the k-wide maximum taken there
//   streak_dilate_kernel  D = emax_n(E), the same tile form (max_len only)
//   streak_final_kernel   emax_L(E_L) from an LDS tile, S = min(T, .), the
//                         rejection by hmax_9(D_M), the recovery, four pixels
//                         a thread
//
// The planes are u8 with a pitch of W rounded up to 16, in the workspace:
// [T | E | max_len > 0: E_M | D_M].
#include "derain.h"

namespace rv {
namespace {

constexpr int kTile = 64;   // output tile of the line kernels, 64 x 64
constexpr int kSeg = 1024;  // outputs per block of the row kernel
constexpr int kRowPad = 16;  // room for the halo of width - 1 <= 14 pixels
constexpr int kReject = RV_STREAK_REJECT_W;

// o_j of the header: the column offset of the line's sample j rows away.
__device__ __forceinline__ int line_off(int j, int slant) {
  const int a = j * slant;
  return a >= 0 ? (a + 2) >> 2 : -((2 - a) >> 2);
}
__host__ __device__ __forceinline__ int line_reach(int hn, int slant) {
  return (hn * (slant < 0 ? -slant : slant) + 2) >> 2;
}

// One row segment of kSeg outputs, four adjacent ones per thread.  g and m
// keep pixel xs + i at index kRowPad + i, so that a thread's four are a word.
// vec: the frame rows are 4-byte aligned (12 bytes of BGR as three words).
__global__ __launch_bounds__(256) void streak_row_kernel(const uint8_t* __restrict__ in,
                                                         uint8_t* __restrict__ T, int H, int W,
                                                         int pitch, int Wp, int nseg, int w,
                                                         int thr, int vec,
                                                         const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] == 0) return;
  const int tid = threadIdx.x, hw = w >> 1, h = 2 * hw;
  const int xs = (blockIdx.x % nseg) * kSeg, y = blockIdx.x / nseg;
  const uint8_t* row = in + ((size_t)b * H + y) * pitch;
  __shared__ __attribute__((aligned(16))) uint8_t g[kSeg + 2 * kRowPad], m[kSeg + 2 * kRowPad];
  auto gray_at = [&](int x) {  // 255 outside the frame takes no part in a minimum
    return (x >= 0 && x < W) ? bgr_to_y(row[3 * x], row[3 * x + 1], row[3 * x + 2]) : 255;
  };
  const int x4 = xs + 4 * tid, i4 = kRowPad + 4 * tid;
  if (vec && x4 + 4 <= W) {
    const uint32_t* q = (const uint32_t*)(row + 3 * x4);
    const uint32_t a = q[0], c = q[1], d = q[2];
    const int g0 = bgr_to_y(a & 255, (a >> 8) & 255, (a >> 16) & 255);
    const int g1 = bgr_to_y(a >> 24, c & 255, (c >> 8) & 255);
    const int g2 = bgr_to_y((c >> 16) & 255, c >> 24, d & 255);
    const int g3 = bgr_to_y((d >> 8) & 255, (d >> 16) & 255, d >> 24);
    *(uint32_t*)(g + i4) = (uint32_t)g0 | (uint32_t)g1 << 8 | (uint32_t)g2 << 16 | (uint32_t)g3 << 24;
  } else {
    for (int k = 0; k < 4; ++k) g[i4 + k] = (uint8_t)gray_at(x4 + k);
  }
  if (tid < 2 * h) {  // the halo of h pixels either side
    const int i = tid < h ? tid - h : kSeg + tid - h;
    g[kRowPad + i] = (uint8_t)gray_at(xs + i);
  }
  __syncthreads();
  auto hmin_at = [&](int i) {  // 0 outside the frame takes no part in a maximum
    const int x = xs + i;
    int v = 0;
    if (x >= 0 && x < W) {
      v = 255;
      for (int d = -hw; d <= hw; ++d) v = min(v, (int)g[kRowPad + i + d]);
    }
    return v;
  };
  {
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k) v |= (uint32_t)hmin_at(4 * tid + k) << (8 * k);
    *(uint32_t*)(m + i4) = v;
  }
  if (tid < 2 * hw) {
    const int i = tid < hw ? tid - hw : kSeg + tid - hw;
    m[kRowPad + i] = (uint8_t)hmin_at(i);
  }
  __syncthreads();
  if (x4 >= W) return;
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k) {
    int mx = 0;
    for (int d = -hw; d <= hw; ++d) mx = max(mx, (int)m[i4 + k + d]);
    const int t0 = (int)g[i4 + k] - mx;
    v |= (uint32_t)(t0 >= thr ? t0 : 0) << (8 * k);
  }
  // the plane's rows are padded to 16: a whole word fits, what lies past W is never read
  *(uint32_t*)(T + ((size_t)b * H + y) * Wp + x4) = v;
}

// The rows [y0 - hn, y0 + kTile + hn) and columns [x0 - rxr, x0 + kTile + rxr)
// of one frame's plane into LDS (stride = kTile + 2 rxr, rxr a multiple of 4),
// `fill` outside the frame.  Returns whether this thread loaded a non-zero byte.
__device__ __forceinline__ bool load_tile(uint8_t* dst, const uint8_t* plane, int H, int W, int Wp,
                                          int y0, int x0, int hn, int rxr, int fill) {
  const int nw = (kTile + 2 * rxr) >> 2, total = (kTile + 2 * hn) * nw;
  const uint32_t fillw = (uint32_t)fill * 0x01010101u;
  uint32_t acc = 0;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int r = i / nw, wd = i - r * nw;
    const int y = y0 - hn + r, x = x0 - rxr + 4 * wd;
    uint32_t v = fillw;
    if (y >= 0 && y < H && x + 3 >= 0 && x < W) {
      const uint8_t* src = plane + (size_t)y * Wp;
      if (x >= 0 && x + 4 <= W) {
        v = *(const uint32_t*)(src + x);
      } else {
        v = 0;
        for (int k = 0; k < 4; ++k) {
          const int xx = x + k;
          const uint32_t byte = (xx >= 0 && xx < W) ? src[xx] : (uint32_t)fill;
          v |= byte << (8 * k);
        }
      }
    }
    acc |= v;
    ((uint32_t*)dst)[i] = v;
  }
  return acc != 0;
}

// E = emin_n(hmax_k(T)) on one tile.  Dynamic LDS: two tiles of
// (kTile + 2 hn) x (kTile + 2 rxr) bytes.
__global__ __launch_bounds__(256) void streak_erode_kernel(const uint8_t* __restrict__ T,
                                                           uint8_t* __restrict__ E, int H, int W,
                                                           int Wp, int tilesX, int n, int k,
                                                           int slant, const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] == 0) return;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hn = n >> 1, hk = k >> 1;
  const int rxr = (line_reach(hn, slant) + hk + 3) & ~3;
  const int rows = kTile + 2 * hn, stride = kTile + 2 * rxr;
  const int x0 = (blockIdx.x % tilesX) * kTile, y0 = (blockIdx.x / tilesX) * kTile;
  const size_t fo = (size_t)b * H * Wp;
  uint8_t* raw = lds;
  uint8_t* A = lds + rows * stride;

  const bool any = __syncthreads_or(load_tile(raw, T + fo, H, W, Wp, y0, x0, hn, rxr, 0));
  if (!any) {  // T = 0 on the whole tile and its halo: E = 0
    for (int r = wv; r < kTile; r += 4)
      if (y0 + r < H && x0 + lane < W) E[fo + (size_t)(y0 + r) * Wp + x0 + lane] = 0;
    return;
  }
  // A = hmax_k(T) inside the frame, 255 outside (no part in a minimum); a word
  // of four at a time, and nothing to take where T = 0 in the words around it
  const int nw = stride >> 2;
  for (int i = tid; i < rows * nw; i += 256) {
    const int r = i / nw, c4 = 4 * (i - r * nw);
    const int y = y0 - hn + r;
    const uint32_t* rw = (const uint32_t*)(raw + r * stride + c4);
    const uint32_t near = rw[0] | (c4 > 0 ? rw[-1] : 0u) | (c4 + 4 < stride ? rw[1] : 0u);
    uint32_t v = 0;
    for (int u = 0; u < 4; ++u) {
      const int c = c4 + u, x = x0 - rxr + c;
      int a = 255;
      if (y >= 0 && y < H && x >= 0 && x < W && c >= hk && c < stride - hk) {
        a = 0;
        if (near != 0)
          for (int d = -hk; d <= hk; ++d) a = max(a, (int)raw[r * stride + c + d]);
      }
      v |= (uint32_t)a << (8 * u);
    }
    *(uint32_t*)(A + r * stride + c4) = v;
  }
  __syncthreads();
  for (int i = tid; i < kTile * (kTile / 4); i += 256) {  // four adjacent outputs per thread
    const int r = i >> 4, c4 = 4 * (i & 15);
    const int y = y0 + r, x = x0 + c4;
    if (y >= H || x >= W) continue;
    const int base = (r + hn) * stride + c4 + rxr;
    uint32_t v = 0;
    if (*(const uint32_t*)(A + base) != 0) {
      for (int u = 0; u < 4 && x + u < W; ++u) {
        int mn = A[base + u];
        for (int j = 1; j <= hn && mn > 0; ++j) {  // o_-j = -o_j
          const int o = j * stride + line_off(j, slant);
          mn = min(mn, min((int)A[base + u + o], (int)A[base + u - o]));
        }
        v |= (uint32_t)mn << (8 * u);
      }
    }
    // the plane's rows are padded to 16: a whole word fits, what lies past W is never read
    *(uint32_t*)(E + fo + (size_t)y * Wp + x) = v;
  }
}

// max over the line through tile pixel `base` of the LDS tile t (0 outside the frame).
__device__ __forceinline__ int line_max(const uint8_t* t, int base, int stride, int hn, int slant) {
  int mx = t[base];
  for (int j = 1; j <= hn; ++j) {
    const int o = j * stride + line_off(j, slant);
    mx = max(mx, max((int)t[base + o], (int)t[base - o]));
  }
  return mx;
}

// D = emax_n(E) on one tile.  Dynamic LDS: one tile.
__global__ __launch_bounds__(256) void streak_dilate_kernel(const uint8_t* __restrict__ E,
                                                            uint8_t* __restrict__ D, int H, int W,
                                                            int Wp, int tilesX, int n, int slant,
                                                            const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] == 0) return;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int hn = n >> 1, rxr = (line_reach(hn, slant) + 3) & ~3, stride = kTile + 2 * rxr;
  const int x0 = (blockIdx.x % tilesX) * kTile, y0 = (blockIdx.x / tilesX) * kTile;
  const size_t fo = (size_t)b * H * Wp;
  const bool any = __syncthreads_or(load_tile(lds, E + fo, H, W, Wp, y0, x0, hn, rxr, 0));
  for (int r = wv; r < kTile; r += 4) {
    const int y = y0 + r, x = x0 + lane;
    if (y >= H || x >= W) continue;
    const int v = any ? line_max(lds, (r + hn) * stride + lane + rxr, stride, hn, slant) : 0;
    D[fo + (size_t)y * Wp + x] = (uint8_t)v;
  }
}

// S = min(T, emax_L(E)), S = 0 where hmax_9(DM) > 0 (DM: nullptr for
// max_len 0), and the recovery.  Dynamic LDS: one tile of E.  vec: the rows
// of in and out are 4-byte aligned (four pixels as three words).
__global__ __launch_bounds__(256) void streak_final_kernel(
    const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const uint8_t* __restrict__ T,
    const uint8_t* __restrict__ E, const uint8_t* __restrict__ DM, int H, int W, int pitch, int Wp,
    int tilesX, int n, int slant, int vec, uint8_t* __restrict__ s_out,
    const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] == 0) return;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int hn = n >> 1, rxr = (line_reach(hn, slant) + 3) & ~3, stride = kTile + 2 * rxr;
  const int x0 = (blockIdx.x % tilesX) * kTile, y0 = (blockIdx.x / tilesX) * kTile;
  const size_t fo = (size_t)b * H * Wp;
  const bool any = __syncthreads_or(load_tile(lds, E + fo, H, W, Wp, y0, x0, hn, rxr, 0));
  for (int i = threadIdx.x; i < kTile * (kTile / 4); i += 256) {  // four adjacent pixels per thread
    const int r = i >> 4, c4 = 4 * (i & 15);
    const int y = y0 + r, x = x0 + c4;
    if (y >= H || x >= W) continue;
    const size_t po = fo + (size_t)y * Wp;
    const int np = min(4, W - x);
    int S[4] = {0, 0, 0, 0};
    uint32_t tw = any ? *(const uint32_t*)(T + po + x) : 0u;
    if (np < 4) tw &= (1u << (8 * np)) - 1;  // what lies past W in the plane is not T
    if (tw != 0) {
      for (int k = 0; k < np; ++k) {
        const int t = (tw >> (8 * k)) & 255;
        if (t == 0) continue;
        int v = min(t, line_max(lds, (r + hn) * stride + c4 + k + rxr, stride, hn, slant));
        if (v > 0 && DM != nullptr) {
          int R = 0;
          for (int xx = max(x + k - kReject / 2, 0); xx <= min(x + k + kReject / 2, W - 1); ++xx)
            R = max(R, (int)DM[po + xx]);
          if (R > 0) v = 0;
        }
        S[k] = v;
      }
    }
    const uint8_t* I = in + ((size_t)b * H + y) * pitch + 3 * x;
    uint8_t* O = out + ((size_t)b * H + y) * pitch + 3 * x;
    const bool words = vec && np == 4;
    uint32_t q[3] = {0, 0, 0};
    uint8_t px[12];
    if (words) {
      for (int k = 0; k < 3; ++k) q[k] = ((const uint32_t*)I)[k];
      for (int k = 0; k < 12; ++k) px[k] = (uint8_t)(q[k >> 2] >> (8 * (k & 3)));
    } else {
      for (int k = 0; k < 3 * np; ++k) px[k] = I[k];
    }
    if ((S[0] | S[1] | S[2] | S[3]) != 0) {
      for (int k = 0; k < np; ++k) {
        if (S[k] == 0) continue;  // the inverse of I' = I + (255 - I) a with a = S / (255 - g)
        const int i0 = px[3 * k], i1 = px[3 * k + 1], i2 = px[3 * k + 2];
        const unsigned den = (unsigned)max(1, 255 - bgr_to_y(i0, i1, i2)), half = den >> 1;
        px[3 * k] = (uint8_t)max(0, i0 - (int)(((unsigned)(S[k] * (255 - i0)) + half) / den));
        px[3 * k + 1] = (uint8_t)max(0, i1 - (int)(((unsigned)(S[k] * (255 - i1)) + half) / den));
        px[3 * k + 2] = (uint8_t)max(0, i2 - (int)(((unsigned)(S[k] * (255 - i2)) + half) / den));
      }
      if (words)
        for (int k = 0; k < 3; ++k)
          q[k] = (uint32_t)px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 |
                 (uint32_t)px[4 * k + 3] << 24;
    }
    if (words) {
      for (int k = 0; k < 3; ++k) ((uint32_t*)O)[k] = q[k];
    } else {
      for (int k = 0; k < 3 * np; ++k) O[k] = px[k];
    }
    if (s_out != nullptr)
      for (int k = 0; k < np; ++k) s_out[((size_t)b * H + y) * W + x + k] = (uint8_t)S[k];
  }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
int plane_pitch(int W) { return (W + 15) & ~15; }

size_t tile_bytes(int n, int k, int slant) {
  const int hn = n >> 1, rxr = (line_reach(hn, slant) + (k >> 1) + 3) & ~3;
  return (size_t)(kTile + 2 * hn) * (kTile + 2 * rxr);
}

}  // namespace

int streak_check(const StreakParams& p, const char* what) {
  RV_CHECK_ARG(p.width >= 3 && p.width <= 15 && (p.width & 1), "%s: width %d must be odd in 3..15",
               what, p.width);
  RV_CHECK_ARG(p.min_len >= 3 && p.min_len <= 33 && (p.min_len & 1),
               "%s: min_len %d must be odd in 3..33", what, p.min_len);
  RV_CHECK_ARG(p.max_len == 0 || (p.max_len > p.min_len && p.max_len <= 97 && (p.max_len & 1)),
               "%s: max_len %d must be 0 or odd in min_len+2..97", what, p.max_len);
  RV_CHECK_ARG(p.slant >= -4 && p.slant <= 4, "%s: slant %d not in -4..4", what, p.slant);
  RV_CHECK_ARG(p.thr >= 1 && p.thr <= 255, "%s: thr %d not in 1..255", what, p.thr);
  return RV_OK;
}

// [T | E | max_len > 0: E_M | D_M], each B x H x pitch16(W) bytes
size_t streak_ws_bytes(int B, int H, int W, int max_len) {
  return (max_len > 0 ? 4 : 2) * align256((size_t)B * H * plane_pitch(W));
}

void launch_streak(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                   const StreakParams& p, void* ws, uint8_t* s_out, const int* flags,
                   hipStream_t s) {
  const int Wp = plane_pitch(W);
  const size_t Pn = align256((size_t)B * H * Wp);
  uint8_t* T = (uint8_t*)ws;
  uint8_t* E = T + Pn;
  uint8_t* EM = E + Pn;
  uint8_t* DM = EM + Pn;
  const int nseg = ceil_div(W, kSeg), tilesX = ceil_div(W, kTile);
  const dim3 tiles(tilesX * ceil_div(H, kTile), 1, B);
  const int vec = (pitch % 4 == 0) && ((uintptr_t)in % 4 == 0) && ((uintptr_t)out % 4 == 0);
  streak_row_kernel<<<dim3(nseg * H, 1, B), 256, 0, s>>>(in, T, H, W, pitch, Wp, nseg, p.width,
                                                        p.thr, vec, flags);
  streak_erode_kernel<<<tiles, 256, 2 * tile_bytes(p.min_len, 3, p.slant), s>>>(
      T, E, H, W, Wp, tilesX, p.min_len, 3, p.slant, flags);
  if (p.max_len > 0) {
    streak_erode_kernel<<<tiles, 256, 2 * tile_bytes(p.max_len, kReject, p.slant), s>>>(
        T, EM, H, W, Wp, tilesX, p.max_len, kReject, p.slant, flags);
    streak_dilate_kernel<<<tiles, 256, tile_bytes(p.max_len, 1, p.slant), s>>>(
        EM, DM, H, W, Wp, tilesX, p.max_len, p.slant, flags);
  }
  streak_final_kernel<<<tiles, 256, tile_bytes(p.min_len, 1, p.slant), s>>>(
      in, out, T, E, p.max_len > 0 ? DM : nullptr, H, W, pitch, Wp, tilesX, p.min_len, p.slant, vec,
      s_out, flags);
}

}  // namespace rv

using namespace rv;

extern "C" size_t rv_streak_ws_bytes(int B, int H, int W, int max_len) {
  if (B <= 0 || H <= 0 || W <= 0 || max_len < 0 || max_len > 97) return 0;
  return streak_ws_bytes(B, H, W, max_len);
}

extern "C" int rv_streak_derain_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                                   int width, int min_len, int max_len, int slant, int thr,
                                   void* ws, size_t ws_bytes, uint8_t* s_out, void* stream) {
  RV_CHECK_ARG(in != nullptr && out != nullptr, "null frame pointer");
  RV_CHECK_ARG(B >= 0 && B <= 65535 && H > 0 && W > 0, "bad frame shape B=%d H=%d W=%d", B, H, W);
  RV_CHECK_ARG(pitch >= 3 * W, "pitch %d < 3*W", pitch);
  RV_CHECK_ARG((const void*)in != (const void*)out, "in and out must not alias");
  const StreakParams p{width, min_len, max_len, slant, thr};
  const int st = streak_check(p, "rv_streak_derain_u8");
  if (st) return st;
  const size_t need = B > 0 ? streak_ws_bytes(B, H, W, max_len) : 0;
  RV_CHECK_ARG(need == 0 || (ws != nullptr && ws_bytes >= need),
               "workspace too small: %zu bytes, rv_streak_ws_bytes says %zu", ws_bytes, need);
  RV_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  if (B == 0) return RV_OK;
  launch_streak(in, out, B, H, W, pitch, p, ws, s_out, nullptr, as_stream(stream));
  return launch_status("rv_streak_derain_u8");
}
