// Dark-channel-prior dehaze (He, Sun, Tang) in integer arithmetic, bit for
// bit tests/dcp_ref.py: rv_dcp_dehaze_u8 and the DCP pass of
// rv_preprocess_chain_u8 (include/rvhip.h states the arithmetic).
//
//   dcp_min_kernel<0>   d = p x p minimum of min(B,G,R); per-frame histogram of
//                       d with the channel sums of each level (airlight)
//   dcp_airlight_kernel suffix sums of the histogram -> L, cnt, A
//   dcp_min_kernel<1>   nd = p x p minimum of the normalised channels -> t0
//                       (radius 0: recovery here); writes the t0 and gray planes
//   dcp_vsum_kernel<R>  running sums down the columns, (2r+1) clipped rows
//   dcp_hsum_kernel<R>  sums along the rows by an LDS prefix scan; round 1 ends
//                       in the aq/bq divisions, round 2 in t and the recovery
//
// Every sum is an exact integer, so the order of the atomics and of the
// running sums does not show in the result.
#include "dehaze.h"

namespace rv {
namespace {

constexpr int kTW = 128, kTH = 32;  // output tile of the minimum filter
constexpr int kHaloMax = 15;        // patch <= 31
constexpr int kAH = kTH + 2 * kHaloMax;  // rows of the value tile
// Row strides of the value tile (158 columns used, words read up to byte 159)
// and of the transposed row minima (62 rows used, words up to byte 63): an odd
// number of dwords, so that lanes on consecutive rows fall on different banks.
constexpr int kAW = 164, kRT = 68;
constexpr int kRawStride = 512;     // bytes of BGR per tile row, 16-byte chunks
constexpr int kBand = 64;           // rows per block of the column sums
constexpr int kSeg = 512;           // outputs per block of the row sums
constexpr int kEnt = 768;           // scan entries per block: kSeg + 2 * 64 <= 3 * 256
constexpr int kMaxPixels = 1 << 24;

__device__ __forceinline__ int64_t floordiv64(int64_t a, int64_t b) {  // b > 0
  int64_t q = a / b;
  if (a - q * b < 0) --q;
  return q;
}

// Step 6: clamp(A + floor(((I - A) * 510 + tt) / (2 tt)), 0, 255), tt in 1..255.
// The numerator is moved up by 65536 * 2 tt so that the division is unsigned.
__device__ __forceinline__ int dcp_recover(int I, int A, int tt) {
  const unsigned den = 2u * (unsigned)tt;
  const unsigned num = (unsigned)((I - A) * 510 + tt + 65536 * (int)den);
  return sat_u8(A + (int)(num / den) - 65536);
}

__global__ void dcp_zero_kernel(unsigned* __restrict__ p, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

__device__ __forceinline__ int min4(uint32_t w) {
  return min(min(w & 255, (w >> 8) & 255), min((w >> 16) & 255, w >> 24));
}

// Four adjacent outputs of the 1-D minimum over 2 hp + 1 bytes: output k is the
// minimum of src[k .. k + 2 hp], src 4-byte aligned.  The bytes 3 .. 2 hp are in
// all four windows and are taken a word at a time; the three bytes before and
// the three after them go to the windows that hold them.  Reads whole words up
// to byte 4 * ((2 hp + 1) / 4) + 7 (hp >= 2) of which it uses those up to
// 2 hp + 3.
__device__ __forceinline__ void min_run4(const uint8_t* src, int hp, int (&o)[4]) {
  const uint32_t* w = (const uint32_t*)src;
  const uint32_t w0 = w[0];
  const int b0 = w0 & 255, b1 = (w0 >> 8) & 255, b2 = (w0 >> 16) & 255, b3 = w0 >> 24;
  if (hp == 1) {
    const uint32_t w1 = w[1];
    const int t0 = w1 & 255, t1 = (w1 >> 8) & 255;
    o[0] = min(b0, min(b1, b2));
    o[1] = min(b1, min(b2, b3));
    o[2] = min(b2, min(b3, t0));
    o[3] = min(b3, min(t0, t1));
    return;
  }
  const int mt = (2 * hp + 1) >> 2;  // the first word that is not in all four windows
  int core = b3;
  for (int m = 1; m < mt; ++m) core = min(core, min4(w[m]));
  const uint32_t u = w[mt];
  const int t0 = u & 255, t1 = (u >> 8) & 255, t2 = (u >> 16) & 255, t3 = u >> 24;
  int p0, p1, p2, p3;  // what of the words from mt on is in windows 0..3
  if ((hp & 1) == 0) {  // 2 hp = 4 mt: window k ends at byte k of word mt
    p0 = t0;
    p1 = min(p0, t1);
    p2 = min(p1, t2);
    p3 = min(p2, t3);
  } else {              // 2 hp = 4 mt + 2: window k ends at byte k + 2
    const uint32_t u1 = w[mt + 1];
    p0 = min(t0, min(t1, t2));
    p1 = min(p0, t3);
    p2 = min(p1, (int)(u1 & 255));
    p3 = min(p2, (int)((u1 >> 8) & 255));
  }
  o[3] = min(core, p3);
  o[2] = min(min(b2, core), p2);
  o[1] = min(min(b1, b2), min(core, p1));
  o[0] = min(min(b0, min(b1, b2)), min(core, p0));
}

// 1-D minimum along the lines of src (nlines lines of `sstride` bytes, nwords
// words of four outputs per line), written transposed: output c of line l to
// dst[c * dstride + l].  Consecutive lanes take consecutive lines.
__device__ __forceinline__ void min_pass(const uint8_t* src, int sstride, int nlines, int nwords,
                                         uint8_t* dst, int dstride, int hp) {
  for (int i = threadIdx.x; i < nlines * nwords; i += 256) {
    const int wd = i / nlines, l = i - wd * nlines;
    int o[4];
    min_run4(src + l * sstride + 4 * wd, hp, o);
    for (int k = 0; k < 4; ++k) dst[(4 * wd + k) * dstride + l] = (uint8_t)o[k];
  }
}

// One kTW x kTH tile of the separable p x p minimum.  PASS 0: of min(B,G,R),
// feeding the histogram; PASS 1: of the channels normalised by the airlight.
template <int PASS>
__global__ __launch_bounds__(256) void dcp_min_kernel(
    const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int pitch, int vec,
    int tilesX, DcpParams p, unsigned* __restrict__ hist, const int* __restrict__ air,
    uint8_t* __restrict__ gpl, uint8_t* __restrict__ t0pl, int Wp, uint8_t* __restrict__ t_out,
    const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] == 0) return;
  const int tid = threadIdx.x;
  const int hp = p.patch >> 1;
  const int x0 = (blockIdx.x % tilesX) * kTW, y0 = (blockIdx.x / tilesX) * kTH;
  const uint8_t* frame = in + (size_t)b * H * pitch;

  __shared__ __attribute__((aligned(16))) uint8_t raw[kAH * kRawStride];
  __shared__ __attribute__((aligned(16))) uint8_t a[kAH * kAW];
  __shared__ __attribute__((aligned(16))) uint8_t rmT[kTW * kRT];  // row minima, transposed
  uint8_t* res = a;  // the tile's minima, [kTH][kTW], once the value tile is spent
  __shared__ uint8_t lut[PASS == 1 ? 3 * 256 : 1];
  __shared__ unsigned lh[PASS == 0 ? 4 * 256 : 1];

  int A[3] = {1, 1, 1};
  if (PASS == 1) {
    for (int c = 0; c < 3; ++c) A[c] = air[8 * b + c];
    for (int i = tid; i < 3 * 256; i += 256) {
      const int c = i >> 8, v = i & 255;
      lut[i] = (uint8_t)min(255u, (510u * v + A[c]) / (2u * A[c]));
    }
  } else {
    for (int i = tid; i < 4 * 256; i += 256) lh[i] = 0;
  }

  // the tile's rows and columns inside the frame, and their BGR bytes
  const int cx0 = max(x0 - hp, 0), cx1 = min(x0 + kTW + hp, W);
  const int ry0 = max(y0 - hp, 0), ry1 = min(y0 + kTH + hp, H);
  const int bs = (3 * cx0) & ~15, be = 3 * cx1;
  const int nchunk = (be - bs + 15) >> 4, nrows = ry1 - ry0;
  for (int i = tid; i < nrows * 32; i += 256) {
    const int j = i >> 5, c = i & 31;
    if (c >= nchunk) continue;
    const int off = bs + 16 * c;
    const uint8_t* src = frame + (size_t)(ry0 + j) * pitch + off;
    uint8_t* dst = raw + j * kRawStride + 16 * c;
    if (vec && off + 16 <= 3 * W) {
      *(uint4*)dst = *(const uint4*)src;
    } else {
      const int n = min(16, 3 * W - off);
      for (int k = 0; k < n; ++k) dst[k] = src[k];
    }
  }
  __syncthreads();

  // value tile; 255 outside the frame takes no part in a minimum
  const int aw = kTW + 2 * hp, ah = kTH + 2 * hp;
  for (int i = tid; i < ah * 160; i += 256) {
    const int j = i / 160, c = i - j * 160;
    if (c >= aw) continue;
    const int y = y0 - hp + j, x = x0 - hp + c;
    int v = 255;
    if (y >= ry0 && y < ry1 && x >= cx0 && x < cx1) {
      const uint8_t* q = raw + (y - ry0) * kRawStride + (3 * x - bs);
      if (PASS == 0) v = min((int)q[0], min((int)q[1], (int)q[2]));
      else v = min((int)lut[q[0]], min((int)lut[256 + q[1]], (int)lut[512 + q[2]]));
    }
    a[j * kAW + c] = (uint8_t)v;
  }
  __syncthreads();
  min_pass(a, kAW, ah, kTW / 4, rmT, kRT, hp);   // along the rows
  __syncthreads();
  min_pass(rmT, kRT, kTW, kTH / 4, res, kTW, hp);  // down the columns
  __syncthreads();

  for (int i = tid; i < kTH * kTW; i += 256) {  // a wave is 64 pixels of one row
    const int j = i >> 7, c = i & (kTW - 1);
    const int y = y0 + j, x = x0 + c;
    const bool valid = y < H && x < W;
    const int v = res[i];
    int I[3] = {0, 0, 0};
    if (valid) {
      const uint8_t* q = raw + (y - ry0) * kRawStride + (3 * x - bs);
      I[0] = q[0], I[1] = q[1], I[2] = q[2];
    }
    if (PASS == 0) {
      // d is piecewise constant: a wave that holds one level adds once
      const int key = valid ? v : -1;
      const int first = __builtin_amdgcn_readfirstlane(key);
      if (__all(key == first)) {
        if (first >= 0) {
          int s0 = I[0], s1 = I[1], s2 = I[2];
          for (int off = 32; off > 0; off >>= 1) {
            s0 += __shfl_xor(s0, off);
            s1 += __shfl_xor(s1, off);
            s2 += __shfl_xor(s2, off);
          }
          if ((tid & 63) == 0) {
            atomicAdd(&lh[first], 64u);
            atomicAdd(&lh[256 + first], (unsigned)s0);
            atomicAdd(&lh[512 + first], (unsigned)s1);
            atomicAdd(&lh[768 + first], (unsigned)s2);
          }
        }
      } else if (valid) {
        atomicAdd(&lh[v], 1u);
        atomicAdd(&lh[256 + v], (unsigned)I[0]);
        atomicAdd(&lh[512 + v], (unsigned)I[1]);
        atomicAdd(&lh[768 + v], (unsigned)I[2]);
      }
    } else if (valid) {
      const int t0 = 255 - ((p.wq * v + 128) >> 8);
      if (p.radius > 0) {
        const size_t o = ((size_t)b * H + y) * Wp + x;
        t0pl[o] = (uint8_t)t0;
        gpl[o] = (uint8_t)bgr_to_y(I[0], I[1], I[2]);
      } else {
        const int tt = max(t0, p.tq);
        uint8_t* o = out + ((size_t)b * H + y) * pitch + 3 * x;
        for (int c2 = 0; c2 < 3; ++c2) o[c2] = (uint8_t)dcp_recover(I[c2], A[c2], tt);
        if (t_out != nullptr) t_out[((size_t)b * H + y) * W + x] = (uint8_t)t0;
      }
    }
  }
  if (PASS == 0) {
    __syncthreads();
    for (int i = tid; i < 4 * 256; i += 256)
      if (lh[i] != 0) atomicAdd(&hist[(size_t)b * 1024 + i], lh[i]);
  }
}

// Step 2 from the histogram: one block per frame.  air: {A_b, A_g, A_r, L,
// cnt, 0, 0, 0} per frame in the workspace; air_out: 5 ints per frame.
__global__ __launch_bounds__(256) void dcp_airlight_kernel(const unsigned* __restrict__ hist,
                                                           int n, int* __restrict__ air,
                                                           int32_t* __restrict__ air_out,
                                                           const int* __restrict__ flags) {
  const int b = blockIdx.x, i = threadIdx.x;
  if (flags != nullptr && flags[b] == 0) return;
  __shared__ unsigned long long s[4][256];
  for (int q = 0; q < 4; ++q) s[q][i] = hist[(size_t)b * 1024 + 256 * q + i];
  for (int off = 1; off < 256; off <<= 1) {  // suffix sums: s[q][i] = sum over levels >= i
    __syncthreads();
    unsigned long long v[4];
    for (int q = 0; q < 4; ++q) v[q] = i + off < 256 ? s[q][i + off] : 0;
    __syncthreads();
    for (int q = 0; q < 4; ++q) s[q][i] += v[q];
  }
  __syncthreads();
  const unsigned long long need = (unsigned long long)n;
  if (s[0][i] >= need && (i == 255 || s[0][i + 1] < need)) {  // the largest such level
    const unsigned long long cnt = s[0][i];
    int r[5];
    for (int c = 0; c < 3; ++c) r[c] = max(1, (int)((2 * s[1 + c][i] + cnt) / (2 * cnt)));
    r[3] = i;
    r[4] = (int)cnt;
    for (int k = 0; k < 8; ++k) air[8 * b + k] = k < 5 ? r[k] : 0;
    if (air_out != nullptr)
      for (int k = 0; k < 5; ++k) air_out[5 * b + k] = r[k];
  }
}

// Running sums down four adjacent columns per thread over the rows
// [y - r, y + r] clipped to the frame, for the kBand rows of one band.
// ROUND 1: of g, t0, g*t0, g*g (u8 planes) -> {Sg | Sp << 16}, Sgp, Sgg (u32).
// ROUND 2: of aq, bq (i32 planes) -> SA (i32), SB (i64).
template <int ROUND>
__global__ __launch_bounds__(64) void dcp_vsum_kernel(const void* __restrict__ src0,
                                                      const void* __restrict__ src1,
                                                      uint8_t* __restrict__ vs, size_t Pn, int H,
                                                      int Wp, int r, int ngroups,
                                                      const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] == 0) return;
  const int x = ((blockIdx.x % ngroups) * 64 + threadIdx.x) * 4;
  if (x >= Wp) return;  // Wp is a multiple of 16: x + 3 < Wp
  const int y0 = (blockIdx.x / ngroups) * kBand, y1 = min(y0 + kBand, H);
  const size_t fo = (size_t)b * H * Wp + x;  // this thread's columns in row 0 of the frame

  if (ROUND == 1) {
    const uint8_t* g = (const uint8_t*)src0;
    const uint8_t* t = (const uint8_t*)src1;
    unsigned sg[4] = {}, sp[4] = {}, sgp[4] = {}, sgg[4] = {};
    auto add = [&](int y, int sign) {
      const uint32_t gw = *(const uint32_t*)(g + fo + (size_t)y * Wp);
      const uint32_t tw = *(const uint32_t*)(t + fo + (size_t)y * Wp);
      for (int k = 0; k < 4; ++k) {
        const unsigned gv = (gw >> (8 * k)) & 255, tv = (tw >> (8 * k)) & 255;
        sg[k] += sign * gv;  // unsigned wrap-around: the running sums never go negative
        sp[k] += sign * tv;
        sgp[k] += sign * (gv * tv);
        sgg[k] += sign * (gv * gv);
      }
    };
    for (int y = max(y0 - r, 0); y <= min(y0 + r, H - 1); ++y) add(y, 1);
    uint32_t* v0 = (uint32_t*)vs;
    uint32_t* v1 = (uint32_t*)(vs + 4 * Pn);
    uint32_t* v2 = (uint32_t*)(vs + 8 * Pn);
    for (int y = y0; y < y1; ++y) {
      const size_t o = fo + (size_t)y * Wp;
      *(uint4*)(v0 + o) = make_uint4(sg[0] | sp[0] << 16, sg[1] | sp[1] << 16, sg[2] | sp[2] << 16,
                                     sg[3] | sp[3] << 16);
      *(uint4*)(v1 + o) = make_uint4(sgp[0], sgp[1], sgp[2], sgp[3]);
      *(uint4*)(v2 + o) = make_uint4(sgg[0], sgg[1], sgg[2], sgg[3]);
      if (y + 1 + r < H) add(y + 1 + r, 1);
      if (y - r >= 0) add(y - r, -1);
    }
  } else {
    const int32_t* aq = (const int32_t*)src0;
    const int32_t* bq = (const int32_t*)src1;
    int sa[4] = {};
    int64_t sb[4] = {};
    auto add = [&](int y, int sign) {
      const int4 av = *(const int4*)(aq + fo + (size_t)y * Wp);
      const int4 bv = *(const int4*)(bq + fo + (size_t)y * Wp);
      sa[0] += sign * av.x, sa[1] += sign * av.y, sa[2] += sign * av.z, sa[3] += sign * av.w;
      sb[0] += sign * bv.x, sb[1] += sign * bv.y, sb[2] += sign * bv.z, sb[3] += sign * bv.w;
    };
    for (int y = max(y0 - r, 0); y <= min(y0 + r, H - 1); ++y) add(y, 1);
    int32_t* vA = (int32_t*)vs;
    int64_t* vB = (int64_t*)(vs + 4 * Pn);
    for (int y = y0; y < y1; ++y) {
      const size_t o = fo + (size_t)y * Wp;
      *(int4*)(vA + o) = make_int4(sa[0], sa[1], sa[2], sa[3]);
      *(longlong2*)(vB + o) = make_longlong2(sb[0], sb[1]);
      *(longlong2*)(vB + o + 2) = make_longlong2(sb[2], sb[3]);
      if (y + 1 + r < H) add(y + 1 + r, 1);
      if (y - r >= 0) add(y - r, -1);
    }
  }
}

// Exclusive prefix of one value per thread over the block of 256 (four waves).
template <typename T>
__device__ __forceinline__ T block_excl_scan(T s, T* wave_tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = s;
  for (int off = 1; off < 64; off <<= 1) {
    const T u = __shfl_up(incl, off);
    if (lane >= off) incl += u;
  }
  if (lane == 63) wave_tot[w] = incl;
  __syncthreads();
  T base = 0;
  for (int k = 0; k < w; ++k) base += wave_tot[k];
  return base + incl - s;
}

// Prefix sums P[0..n] of one row's entries (three per thread) into LDS.
template <typename T>
__device__ __forceinline__ void row_prefix(const T (&v)[3], T* P, T* wave_tot) {
  T e = block_excl_scan<T>(v[0] + v[1] + v[2], wave_tot);
  const int k = 3 * threadIdx.x;
  P[k] = e;
  P[k + 1] = e + v[0];
  P[k + 2] = e + v[0] + v[1];
}

// Sums along one row segment of the column sums: the (2r+1)^2 clipped box.
// ROUND 1 ends in aq and bq; ROUND 2 in t, t_out and the recovered pixel.
template <int ROUND>
__global__ __launch_bounds__(256) void dcp_hsum_kernel(
    const uint8_t* __restrict__ vs, size_t Pn, int H, int W, int Wp, int nseg, DcpParams p,
    int32_t* __restrict__ aqp, int32_t* __restrict__ bqp, const uint8_t* __restrict__ gpl,
    const int* __restrict__ air, const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
    int pitch, uint8_t* __restrict__ t_out, const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] == 0) return;
  const int tid = threadIdx.x, r = p.radius;
  const int xs = (blockIdx.x % nseg) * kSeg, y = blockIdx.x / nseg;
  const int c0 = max(xs - r, 0), c1 = min(xs + kSeg + r, W);  // columns scanned: [c0, c1)
  const int n = c1 - c0;
  const size_t ro = ((size_t)b * H + y) * Wp;
  const int ny = min(y + r, H - 1) - max(y - r, 0) + 1;

  if (ROUND == 1) {
    __shared__ unsigned P[4][kEnt];
    __shared__ unsigned wt[4][4];
    const uint32_t* v0 = (const uint32_t*)vs + ro;
    const uint32_t* v1 = (const uint32_t*)(vs + 4 * Pn) + ro;
    const uint32_t* v2 = (const uint32_t*)(vs + 8 * Pn) + ro;
    unsigned e[4][3];
    for (int k = 0; k < 3; ++k) {
      const int c = 3 * tid + k;
      const bool ok = c < n;
      const unsigned w = ok ? v0[c0 + c] : 0;
      e[0][k] = w & 0xffff;
      e[1][k] = w >> 16;
      e[2][k] = ok ? v1[c0 + c] : 0;
      e[3][k] = ok ? v2[c0 + c] : 0;
    }
    for (int q = 0; q < 4; ++q) row_prefix<unsigned>(e[q], P[q], wt[q]);
    __syncthreads();
    for (int u = 0; u < kSeg / 256; ++u) {
      const int x = xs + tid + 256 * u;
      if (x >= W) break;
      const int lo = max(x - r, 0) - c0, hi = min(x + r, W - 1) + 1 - c0;
      const int64_t N = (int64_t)(hi - lo) * ny;
      // the prefixes wrap modulo 2^32; a box sum is below 2^31
      const int64_t Sg = P[0][hi] - P[0][lo], Sp = P[1][hi] - P[1][lo];
      const int64_t Sgp = P[2][hi] - P[2][lo], Sgg = P[3][hi] - P[3][lo];
      const int64_t num = N * Sgp - Sg * Sp;
      const int64_t den = N * Sgg - Sg * Sg + (int64_t)p.eq * N * N;
      const int64_t aq = floordiv64(num * 16384, den);
      const int64_t bq = floordiv64(Sp * 16384 - aq * Sg, N);
      aqp[ro + x] = (int32_t)aq;
      bqp[ro + x] = (int32_t)bq;
    }
  } else {
    __shared__ int64_t P[2][kEnt];
    __shared__ int64_t wt[2][4];
    const int32_t* vA = (const int32_t*)vs + ro;
    const int64_t* vB = (const int64_t*)(vs + 4 * Pn) + ro;
    int64_t e[2][3];
    for (int k = 0; k < 3; ++k) {
      const int c = 3 * tid + k;
      const bool ok = c < n;
      e[0][k] = ok ? vA[c0 + c] : 0;
      e[1][k] = ok ? vB[c0 + c] : 0;
    }
    for (int q = 0; q < 2; ++q) row_prefix<int64_t>(e[q], P[q], wt[q]);
    __syncthreads();
    int A[3];
    for (int c = 0; c < 3; ++c) A[c] = air[8 * b + c];
    for (int u = 0; u < kSeg / 256; ++u) {
      const int x = xs + tid + 256 * u;
      if (x >= W) break;
      const int lo = max(x - r, 0) - c0, hi = min(x + r, W - 1) + 1 - c0;
      const int N = (hi - lo) * ny;
      const int64_t SA = P[0][hi] - P[0][lo], SB = P[1][hi] - P[1][lo];
      const int g = gpl[ro + x];
      // floor(X / (N << 14)) = floor((X >> 14) / N), and |X >> 14| < 2^31
      const int X = (int)((SA * g + SB + ((int64_t)N << 13)) >> 14);
      int q = X / N;
      if (X - q * N < 0) --q;
      const int t = sat_u8(q);
      const int tt = max(t, p.tq);
      const uint8_t* I = in + ((size_t)b * H + y) * pitch + 3 * x;
      uint8_t* o = out + ((size_t)b * H + y) * pitch + 3 * x;
      for (int c = 0; c < 3; ++c) o[c] = (uint8_t)dcp_recover(I[c], A[c], tt);
      if (t_out != nullptr) t_out[((size_t)b * H + y) * W + x] = (uint8_t)t;
    }
  }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
int plane_pitch(int W) { return (W + 15) & ~15; }

}  // namespace

int dcp_check(const DcpParams& p, int H, int W, const char* what) {
  RV_CHECK_ARG(p.patch >= 3 && p.patch <= 31 && (p.patch & 1), "%s: patch %d must be odd in 3..31",
               what, p.patch);
  RV_CHECK_ARG(p.wq >= 1 && p.wq <= 256, "%s: wq %d not in 1..256", what, p.wq);
  RV_CHECK_ARG(p.tq >= 1 && p.tq <= 255, "%s: tq %d not in 1..255", what, p.tq);
  RV_CHECK_ARG(p.radius >= 0 && p.radius <= 64, "%s: radius %d not in 0..64", what, p.radius);
  RV_CHECK_ARG(p.eq >= 1 && p.eq <= (1 << 20), "%s: eq %d not in 1..2^20", what, p.eq);
  RV_CHECK_ARG(H <= 0 || W <= 0 || (int64_t)H * W <= kMaxPixels,
               "%s: %d x %d frame has more than 2^24 pixels", what, W, H);
  return RV_OK;
}

// [histogram | airlight | radius > 0: gray | t0 | aq | bq | column sums]
size_t dcp_ws_bytes(int B, int H, int W, int radius) {
  size_t n = align256((size_t)B * 1024 * sizeof(unsigned)) + align256((size_t)B * 8 * sizeof(int));
  if (radius > 0) {
    const size_t Pn = (size_t)B * H * plane_pitch(W);
    n += 2 * align256(Pn) + 2 * align256(4 * Pn) + align256(12 * Pn);
  }
  return n;
}

void launch_dcp(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                const DcpParams& p, void* ws, int32_t* air_out, uint8_t* t_out, const int* flags,
                hipStream_t s) {
  const int Wp = plane_pitch(W);
  const size_t Pn = (size_t)B * H * Wp;
  uint8_t* w = (uint8_t*)ws;
  unsigned* hist = (unsigned*)w;
  w += align256((size_t)B * 1024 * sizeof(unsigned));
  int* air = (int*)w;
  w += align256((size_t)B * 8 * sizeof(int));
  uint8_t* gpl = w;
  uint8_t* t0pl = gpl + align256(Pn);
  int32_t* aq = (int32_t*)(t0pl + align256(Pn));
  int32_t* bq = (int32_t*)((uint8_t*)aq + align256(4 * Pn));
  uint8_t* vs = (uint8_t*)bq + align256(4 * Pn);

  const int vec = (pitch % 16 == 0) && (((uintptr_t)in) % 16 == 0);
  const int tilesX = ceil_div(W, kTW);
  const dim3 tiles(tilesX * ceil_div(H, kTH), 1, B);
  const size_t nh = (size_t)B * 1024;
  dcp_zero_kernel<<<(unsigned)((nh + 255) / 256), 256, 0, s>>>(hist, nh);
  dcp_min_kernel<0><<<tiles, 256, 0, s>>>(in, nullptr, H, W, pitch, vec, tilesX, p, hist, nullptr,
                                         nullptr, nullptr, Wp, nullptr, flags);
  const int n = max(1, (int)((int64_t)H * W / 1000));
  dcp_airlight_kernel<<<B, 256, 0, s>>>(hist, n, air, air_out, flags);
  dcp_min_kernel<1><<<tiles, 256, 0, s>>>(in, out, H, W, pitch, vec, tilesX, p, nullptr, air, gpl,
                                         t0pl, Wp, t_out, flags);
  if (p.radius == 0) return;
  const int ngroups = ceil_div(Wp, 256), nseg = ceil_div(W, kSeg);
  const dim3 vgrid(ngroups * ceil_div(H, kBand), 1, B), hgrid(nseg * H, 1, B);
  dcp_vsum_kernel<1><<<vgrid, 64, 0, s>>>(gpl, t0pl, vs, Pn, H, Wp, p.radius, ngroups, flags);
  dcp_hsum_kernel<1><<<hgrid, 256, 0, s>>>(vs, Pn, H, W, Wp, nseg, p, aq, bq, nullptr, nullptr,
                                          nullptr, nullptr, 0, nullptr, flags);
  dcp_vsum_kernel<2><<<vgrid, 64, 0, s>>>(aq, bq, vs, Pn, H, Wp, p.radius, ngroups, flags);
  dcp_hsum_kernel<2><<<hgrid, 256, 0, s>>>(vs, Pn, H, W, Wp, nseg, p, nullptr, nullptr, gpl, air,
                                          in, out, pitch, t_out, flags);
}

}  // namespace rv

using namespace rv;

extern "C" size_t rv_dcp_ws_bytes(int B, int H, int W, int radius) {
  if (B <= 0 || H <= 0 || W <= 0 || radius < 0 || radius > 64 || (int64_t)H * W > kMaxPixels)
    return 0;
  return dcp_ws_bytes(B, H, W, radius);
}

extern "C" int rv_dcp_dehaze_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                                int patch, int wq, int tq, int radius, int eq, void* ws,
                                size_t ws_bytes, int32_t* air_out, uint8_t* t_out, void* stream) {
  RV_CHECK_ARG(in != nullptr && out != nullptr, "null frame pointer");
  RV_CHECK_ARG(B >= 0 && B <= 65535 && H > 0 && W > 0, "bad frame shape B=%d H=%d W=%d", B, H, W);
  RV_CHECK_ARG(pitch >= 3 * W, "pitch %d < 3*W", pitch);
  RV_CHECK_ARG((const void*)in != (const void*)out, "in and out must not alias");
  const DcpParams p{patch, wq, tq, radius, eq};
  int st = dcp_check(p, H, W, "rv_dcp_dehaze_u8");
  if (st) return st;
  const size_t need = B > 0 ? dcp_ws_bytes(B, H, W, radius) : 0;
  RV_CHECK_ARG(need == 0 || (ws != nullptr && ws_bytes >= need),
               "workspace too small: %zu bytes, rv_dcp_ws_bytes says %zu", ws_bytes, need);
  RV_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  if (B == 0) return RV_OK;
  launch_dcp(in, out, B, H, W, pitch, p, ws, air_out, t_out, nullptr, as_stream(stream));
  return launch_status("rv_dcp_dehaze_u8");
}
