// Baseline JPEG, device encoder: interleaved BGR -> coefficient records ->
// complete JPEG images, byte for byte what libjpeg writes with its default
// settings and a restart interval of one MCU row (Pillow: quality=q,
// subsampling=s, restart_marker_rows=1).  The mirror image of jpeg.hip; the
// arithmetic is restated in jpeg_enc_math.h, the tables in jpeg_tables.h, the
// file header comes from jpeg_host.cpp.
//
// Three kernels, all stream-ordered, none read by the host:
//   1. jpeg_bgr_to_coef_kernel: eight lanes per 8x8 block.  Lane t converts,
//      edge-replicates and downsamples row t, runs the row DCT, the block goes
//      through a stride-9 LDS scratch (9 t + 72 b: 64 distinct banks over a
//      wave, as in jpeg.hip) for the column DCT and the quantiser, and back so
//      that lane t stores coefficient row t with one 16-byte store.
//   2. jpeg_entropy_kernel: one workgroup per restart segment (= MCU row).
//      One lane per block, 256 blocks at a time: count the block's bits,
//      workgroup scan, then every lane ORs its codes into an LDS bit buffer at
//      its own offset; whole words leave for a per-segment workspace in global
//      memory, the partial word carries into the next 256 blocks.  The segment
//      ends padded with 1-bits; its length with and without the 0x00 that
//      follows every 0xFF goes to a small table.
//   3. jpeg_compact_kernel: one workgroup per segment again.  It sums the
//      table for its offset inside the image, copies its bytes behind the
//      header prefix while inserting the stuffing zeros (scan of per-lane byte
//      counts), and appends RSTm or EOI; segment 0 also writes the prefix and
//      the stream header.  Every byte store is checked against the capacity.
// Nothing branches on block content except the entropy coder's symbol
// decisions (zero / non-zero coefficient, run of sixteen, end of block).
#include <string.h>

#include "common.h"
#include "jpeg_enc_math.h"
#include "jpeg_host.h"
#include "jpeg_tables.h"

namespace rv {

namespace {

using rvjpeg::EncGeom;

constexpr int kThreads = 256;
constexpr int kBlocksPerPass = 32;  // 256 lanes / 8 lanes per block
constexpr int kScrStride = 72;      // dwords per block of transpose scratch (8 rows of 9)
// words of the LDS bit buffer: 256 blocks of at most kBlockBitsMax bits, the
// carried partial word in front and one word of slack behind
constexpr int kBitWords = (kThreads * rvjpeg::kBlockBitsMax + 31) / 32 + 2;
constexpr int kStreamHeader = RV_JPEG_STREAM_HEADER_BYTES;

struct QuantArg {
  uint16_t q[2][64];  // luma, chroma; natural order
};

struct FileHeader {
  uint32_t w[rvjpeg::kFileHeaderMax / 4];  // SOI .. SOS, little-endian packed bytes
  int n;
};

// Bytes of a W x H record with this sampling code (jpeg_host.cpp layout()).
__host__ __device__ inline size_t record_bytes_of(const EncGeom& g) {
  return rvjpeg::kHeaderBytes + (size_t)3 * 128 +
         (size_t)g.mx * g.my * g.blocks_per_mcu() * 128;
}

__host__ __device__ inline size_t coef_offset(const EncGeom& g, int c) {
  size_t off = rvjpeg::kHeaderBytes + (size_t)3 * 128;
  if (c >= 1) off += (size_t)g.grid_w(0) * g.grid_h(0) * 128;
  if (c >= 2) off += (size_t)g.grid_w(1) * g.grid_h(1) * 128;
  return off;
}

__global__ __launch_bounds__(kThreads) void jpeg_bgr_to_coef_kernel(
    const uint8_t* __restrict__ bgr, uint8_t* __restrict__ records, size_t stride, int W, int H,
    int samp, QuantArg qa) {
  __shared__ int scratch[kBlocksPerPass][kScrStride];
  __shared__ int qtab[2][64];
  const int tid = threadIdx.x, t = tid & 7;
  const EncGeom g(W, H, samp);
  const int row = blockIdx.y;
  uint8_t* rec = records + (size_t)blockIdx.z * stride;
  const uint8_t* frame = bgr + (size_t)blockIdx.z * H * W * 3;
  if (tid < 128) qtab[tid >> 6][tid & 63] = qa.q[tid >> 6][tid & 63];
  if (blockIdx.x == 0 && row == 0) {
    if (tid < 8) {
      const int hdr[8] = {(int)rvjpeg::kMagic, W, H, samp, 3, 0, 0, 0};
      ((int*)rec)[tid] = hdr[tid];
    }
    if (tid < 192)
      ((uint16_t*)(rec + rvjpeg::kHeaderBytes))[tid] = qa.q[tid >= 64 ? 1 : 0][tid & 63];
  }
  const int ny = g.grid_w(0) * g.fv, total = ny + 2 * g.mx;  // blocks of this MCU row
  // lanes past the list's end redo its last block (same values to the same
  // addresses), so the barriers below stay uniform
  const int i = min((int)blockIdx.x * kBlocksPerPass + (tid >> 3), total - 1);
  int c, bx, by;
  if (i < ny) {
    c = 0;
    by = row * g.fv + i / g.grid_w(0);
    bx = i % g.grid_w(0);
  } else {
    const int j = i - ny;
    c = 1 + j / g.mx;
    bx = j % g.mx;
    by = row;
  }
  int sbx, sby;
  const bool dummy = g.source(c, bx, by, sbx, sby);
  int* scr = scratch[tid >> 3];
  int x[8];
  rvjpeg::sample_row(frame, g, c, sbx, sby, t, x);
  rvjpeg::fdct8<1>(x);
#pragma unroll
  for (int u = 0; u < 8; ++u) scr[t * 9 + u] = x[u];
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 8; ++v) x[v] = scr[v * 9 + t];  // column t
  rvjpeg::fdct8<2>(x);
  const int* q = qtab[c == 0 ? 0 : 1];
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const int k = rvjpeg::quantise(x[v], q[v * 8 + t]);
    scr[v * 9 + t] = dummy && (v | t) != 0 ? 0 : k;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 8; ++u) x[u] = scr[t * 9 + u];  // coefficient row t
  uint4 o;
  o.x = (uint32_t)(x[0] & 0xFFFF) | ((uint32_t)x[1] << 16);
  o.y = (uint32_t)(x[2] & 0xFFFF) | ((uint32_t)x[3] << 16);
  o.z = (uint32_t)(x[4] & 0xFFFF) | ((uint32_t)x[5] << 16);
  o.w = (uint32_t)(x[6] & 0xFFFF) | ((uint32_t)x[7] << 16);
  *(uint4*)(rec + coef_offset(g, c) + ((size_t)by * g.grid_w(c) + bx) * 128 + t * 16) = o;
}

// ---- entropy coding --------------------------------------------------------

// Exclusive scan of v over the workgroup's 256 lanes; total -> every lane.
__device__ __forceinline__ int block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) {
    const int s = wsum[k];
    if (k < wv) base += s;
    total += s;
  }
  __syncthreads();
  return base + x - v;
}

__device__ __forceinline__ int count_ff(uint32_t w, int nbytes) {  // among the low nbytes bytes
  int n = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) n += (j < nbytes && ((w >> (8 * j)) & 255) == 255) ? 1 : 0;
  return n;
}

struct BitCount {
  int bits = 0;
  __device__ __forceinline__ void put(uint32_t, int n) { bits += n; }
};

// Bits into the LDS buffer from bit offset `start`, MSB first inside a word.
// Words are shared with the neighbouring blocks, hence the atomic OR.
struct BitEmit {
  uint32_t* buf;
  uint64_t acc = 0;
  int cnt, w;
  __device__ __forceinline__ BitEmit(uint32_t* b, int start) : buf(b), cnt(start & 31), w(start >> 5) {}
  __device__ __forceinline__ void put(uint32_t v, int n) {  // n <= 31, v < 2^n
    acc = (acc << n) | v;
    cnt += n;
    if (cnt >= 32) {
      atomicOr(&buf[w++], (uint32_t)(acc >> (cnt - 32)));
      cnt -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (cnt) atomicOr(&buf[w], (uint32_t)(acc << (32 - cnt)));
  }
};

__device__ __forceinline__ int category(int v) {  // bits of |v|
  const int a = v < 0 ? -v : v;
  return 32 - __clz(a);  // __clz(0) = 32
}

// One block's codes in order: the DC difference, then run / size symbols with
// ZRL for sixteen zeros and EOB unless coefficient 63 is non-zero.
template <class Sink>
__device__ __forceinline__ void code_block(const uint32_t (&c)[32], int pred, const uint32_t* dc,
                                           const uint32_t* ac, Sink& sink) {
  const int diff = (int)(short)(c[0] & 0xFFFF) - pred;
  int s = category(diff);
  uint32_t e = dc[s];
  sink.put(((e & 0xFFFF) << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)),
           (int)(e >> 16) + s);
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const int n = zz[k];
    const int v = (n & 1) ? (int)c[n >> 1] >> 16 : (int)(short)(c[n >> 1] & 0xFFFF);
    if (v == 0) {
      ++run;
    } else {
      while (run >= 16) {
        e = ac[0xF0];
        sink.put(e & 0xFFFF, (int)(e >> 16));
        run -= 16;
      }
      // -32768 alone has 16 bits: no image holds it, and as category 15 (which
      // has no code either) it keeps the index and the block's bit count in range
      s = min(category(v), 15);
      e = ac[(run << 4) | s];
      sink.put(((e & 0xFFFF) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1)),
               (int)(e >> 16) + s);
      run = 0;
    }
  }
  if (run) {
    e = ac[0];
    sink.put(e & 0xFFFF, (int)(e >> 16));
  }
}

__device__ const rvjpeg::HuffEnc g_huff = rvjpeg::make_huff_enc();

// Does the record say W x H with this sampling, three components, and fit?
__device__ __forceinline__ bool record_ok(const uint8_t* rec, size_t stride, const EncGeom& g,
                                          int samp) {
  const int* hdr = (const int*)rec;
  return (uint32_t)hdr[0] == rvjpeg::kMagic && hdr[1] == g.W && hdr[2] == g.H && hdr[3] == samp &&
         hdr[4] == 3 && record_bytes_of(g) <= stride;
}

// Workspace of rv_jpeg_coef_to_stream: uint2 {raw bytes, stuffed bytes} per
// segment, then `seg_ws` bytes of unstuffed entropy data per segment.
__host__ __device__ inline size_t seg_ws_bytes(const EncGeom& g) {
  const size_t bits = (size_t)g.mx * g.blocks_per_mcu() * rvjpeg::kBlockBitsMax;
  return ((bits + 7) / 8 + 8 + 15) / 16 * 16;
}
__host__ __device__ inline size_t seg_table_bytes(const EncGeom& g, int S) {
  return ((size_t)S * g.my * sizeof(uint2) + 255) / 256 * 256;
}

__global__ __launch_bounds__(kThreads) void jpeg_entropy_kernel(
    const uint8_t* __restrict__ records, size_t stride, int W, int H, int samp,
    uint8_t* __restrict__ ws, int S) {
  __shared__ uint32_t buf[kBitWords];
  __shared__ uint32_t tab_dc[2][32], tab_ac[2][256];
  __shared__ int wsum[kThreads / 64];
  __shared__ int ff_total;
  const int tid = threadIdx.x, row = blockIdx.x, frame = blockIdx.y;
  const EncGeom g(W, H, samp);
  const uint8_t* rec = records + (size_t)frame * stride;
  uint2* info = (uint2*)ws + (size_t)frame * g.my + row;
  if (!record_ok(rec, stride, g, samp)) {  // uniform over the workgroup
    if (tid == 0) *info = make_uint2(0, 0);
    return;
  }
  uint32_t* raw =
      (uint32_t*)(ws + seg_table_bytes(g, S) + ((size_t)frame * g.my + row) * seg_ws_bytes(g));
  if (tid < 64) ((uint32_t*)tab_dc)[tid] = ((const uint32_t*)g_huff.dc)[tid];
  for (int k = tid; k < 512; k += kThreads) ((uint32_t*)tab_ac)[k] = ((const uint32_t*)g_huff.ac)[k];
  if (tid == 0) ff_total = 0;
  __syncthreads();

  const int bpm = g.blocks_per_mcu(), ny = g.fh * g.fv;
  const int nblk = g.mx * bpm;
  int total_bits = 0, ff = 0;
  uint32_t carry = 0;
  for (int base = 0; base < nblk; base += kThreads) {
    const int i = base + tid;
    const bool valid = i < nblk;
    uint32_t c[32];
    int pred = 0, t = 0;
    if (valid) {
      const int mcu = i / bpm, j = i % bpm;
      int comp, bx, by, pbx = -1, pby = 0;  // the block whose DC predicts this one's
      if (j < ny) {
        comp = 0;
        bx = mcu * g.fh + j % g.fh;
        by = row * g.fv + j / g.fh;
        if (j > 0) {
          pbx = mcu * g.fh + (j - 1) % g.fh;
          pby = row * g.fv + (j - 1) / g.fh;
        } else if (mcu > 0) {
          pbx = mcu * g.fh - 1;
          pby = row * g.fv + g.fv - 1;
        }
      } else {
        comp = 1 + j - ny;
        t = 1;
        bx = mcu;
        by = row;
        if (mcu > 0) {
          pbx = mcu - 1;
          pby = row;
        }
      }
      const uint8_t* plane = rec + coef_offset(g, comp);
      const int gw = g.grid_w(comp);
      const uint4* src = (const uint4*)(plane + ((size_t)by * gw + bx) * 128);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint4 v = src[k];
        c[4 * k] = v.x;
        c[4 * k + 1] = v.y;
        c[4 * k + 2] = v.z;
        c[4 * k + 3] = v.w;
      }
      if (pbx >= 0) pred = *(const short*)(plane + ((size_t)pby * gw + pbx) * 128);
    }
    BitCount cnt;
    if (valid) code_block(c, pred, tab_dc[t], tab_ac[t], cnt);
    int chunk_bits;
    const int off = block_scan(cnt.bits, wsum, chunk_bits);
    const int lead = total_bits & 31;
    const int nfull = (lead + chunk_bits) >> 5;  // whole words this chunk completes
    for (int w = tid; w <= nfull; w += kThreads) buf[w] = w == 0 ? carry : 0;
    __syncthreads();
    if (valid) {
      BitEmit em(buf, lead + off);
      code_block(c, pred, tab_dc[t], tab_ac[t], em);
      em.finish();
    }
    __syncthreads();
    const int wbase = total_bits >> 5;
    for (int w = tid; w < nfull; w += kThreads) {
      const uint32_t v = __builtin_bswap32(buf[w]);  // first bit -> first byte
      raw[wbase + w] = v;
      ff += count_ff(v, 4);
    }
    carry = buf[nfull];
    total_bits += chunk_bits;
    __syncthreads();
  }
  const int rem = total_bits & 31;
  if (tid == 0 && rem) {  // pad the last byte with 1-bits
    const int pad = (8 - (rem & 7)) & 7;
    const uint32_t v =
        __builtin_bswap32(carry | (((1u << pad) - 1) << (32 - rem - pad)));
    raw[total_bits >> 5] = v;
    ff += count_ff(v, (rem + pad) >> 3);
  }
  if (ff) atomicAdd(&ff_total, ff);
  __syncthreads();
  if (tid == 0) {
    const uint32_t nraw = (uint32_t)((total_bits + 7) >> 3);
    *info = make_uint2(nraw, nraw + (uint32_t)ff_total);
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_compact_kernel(
    const uint8_t* __restrict__ records, size_t stride, int W, int H, int samp,
    const uint8_t* __restrict__ ws, int S, uint8_t* __restrict__ streams, size_t stream_stride,
    size_t cap, FileHeader fh) {
  __shared__ int wsum[kThreads / 64];
  __shared__ unsigned long long sums[2];
  const int tid = threadIdx.x, row = blockIdx.x, frame = blockIdx.y;
  const EncGeom g(W, H, samp);
  uint8_t* out = streams + (size_t)frame * stream_stride;
  if (!record_ok(records + (size_t)frame * stride, stride, g, samp)) {
    if (row == 0 && tid == 0) {
      uint32_t* sh = (uint32_t*)out;
      sh[0] = RV_JPEG_STREAM_MAGIC;
      sh[1] = 0;
      sh[2] = RV_JPEG_STREAM_BAD_RECORD;
      sh[3] = 0;
    }
    return;
  }
  const uint2* info = (const uint2*)ws + (size_t)frame * g.my;
  if (tid < 2) sums[tid] = 0;
  __syncthreads();
  unsigned long long before = 0, all = 0;
  for (int k = tid; k < g.my; k += kThreads) {
    const unsigned s = info[k].y;
    all += s;
    if (k < row) before += s;
  }
  if (before) atomicAdd(&sums[0], before);
  if (all) atomicAdd(&sums[1], all);
  __syncthreads();
  // image: header prefix, segments with RSTm between them, EOI
  const size_t image = (size_t)fh.n + sums[1] + 2 * (size_t)g.my;
  size_t pos = (size_t)kStreamHeader + fh.n + sums[0] + 2 * (size_t)row;
  if (row == 0) {
    for (int k = tid; k < fh.n; k += kThreads)
      if ((size_t)kStreamHeader + k < cap)
        out[kStreamHeader + k] = (uint8_t)(fh.w[k >> 2] >> (8 * (k & 3)));
    if (tid == 0) {
      uint32_t* sh = (uint32_t*)out;
      sh[0] = RV_JPEG_STREAM_MAGIC;
      sh[1] = (uint32_t)image;
      sh[2] = kStreamHeader + image > cap ? RV_JPEG_STREAM_OVERFLOW : 0;
      sh[3] = (uint32_t)g.my;
    }
  }
  const int nraw = (int)info[row].x;
  const uint32_t* raw = (const uint32_t*)(ws + seg_table_bytes(g, S) +
                                          ((size_t)frame * g.my + row) * seg_ws_bytes(g));
  for (int base = 0; base < nraw; base += 4 * kThreads) {
    const int o = base + 4 * tid;
    const int nv = min(max(nraw - o, 0), 4);
    const uint32_t w = nv > 0 ? raw[o >> 2] : 0;
    int chunk;
    const int excl = block_scan(nv + count_ff(w, nv), wsum, chunk);
    size_t p = pos + excl;
    for (int j = 0; j < nv; ++j) {
      const uint32_t b = (w >> (8 * j)) & 255;
      if (p < cap) out[p] = (uint8_t)b;
      ++p;
      if (b == 255) {
        if (p < cap) out[p] = 0;
        ++p;
      }
    }
    pos += chunk;
  }
  if (tid == 0) {
    if (pos < cap) out[pos] = 0xFF;
    if (pos + 1 < cap) out[pos + 1] = (uint8_t)(row + 1 < g.my ? 0xD0 + (row & 7) : 0xD9);
  }
}

thread_local char g_enc_err[rvjpeg::kErrLen];

bool check_geometry(int S, int W, int H, int sampling) {
  if (S < 0 || S > 65535 || W < 1 || H < 1 || W > 65535 || H > 65535) {
    set_error("bad JPEG batch S=%d W=%d H=%d", S, W, H);
    return false;
  }
  if (sampling != RV_JPEG_444 && sampling != RV_JPEG_422 && sampling != RV_JPEG_420) {
    set_error("the device JPEG encoder takes sampling 4:4:4, 4:2:2 or 4:2:0, not code %d",
              sampling);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int rv_jpeg_quant_tables(int quality, uint16_t* luma, uint16_t* chroma) {
  RV_CHECK_ARG(luma != nullptr && chroma != nullptr, "null pointer");
  RV_CHECK_ARG(quality >= 1 && quality <= 100, "JPEG quality %d not in 1..100", quality);
  rvjpeg::quant_tables(quality, luma, chroma);
  return RV_OK;
}

extern "C" int rv_jpeg_write_header(int W, int H, int sampling, int quality,
                                    int restart_interval_mcus, uint8_t* out, size_t cap,
                                    size_t* n) {
  RV_CHECK_ARG(out != nullptr && n != nullptr, "null pointer");
  RV_CHECK_ARG(quality >= 1 && quality <= 100, "JPEG quality %d not in 1..100", quality);
  uint16_t luma[64], chroma[64];
  rvjpeg::quant_tables(quality, luma, chroma);
  if (rvjpeg::write_header(W, H, sampling, luma, chroma, restart_interval_mcus, out, cap, n,
                           g_enc_err) != rvjpeg::kOk) {
    set_error("%s", g_enc_err);
    return RV_EINVAL;
  }
  return RV_OK;
}

extern "C" int rv_jpeg_encode_coef(const uint8_t* record, size_t record_bytes,
                                   int restart_interval_mcus, uint8_t* out, size_t cap,
                                   size_t* n) {
  RV_CHECK_ARG(record != nullptr && out != nullptr && n != nullptr, "null pointer");
  if (rvjpeg::encode(record, record_bytes, restart_interval_mcus, out, cap, n, g_enc_err) !=
      rvjpeg::kOk) {
    set_error("%s", g_enc_err);
    return RV_EINVAL;
  }
  return RV_OK;
}

extern "C" size_t rv_jpeg_stream_bound(int W, int H, int sampling) {
  if (sampling < RV_JPEG_444 || sampling > RV_JPEG_420) return 0;
  const size_t b = rvjpeg::image_bound(W, H, sampling);
  return b ? (kStreamHeader + b + 15) / 16 * 16 : 0;
}

extern "C" int rv_jpeg_bgr_to_coef_u8(const uint8_t* bgr, int S, int H, int W, int sampling,
                                      int quality, uint8_t* records, size_t record_stride,
                                      void* stream) {
  RV_CHECK_ARG(bgr != nullptr && records != nullptr, "null pointer");
  if (!check_geometry(S, W, H, sampling)) return RV_EINVAL;
  RV_CHECK_ARG(quality >= 1 && quality <= 100, "JPEG quality %d not in 1..100", quality);
  const EncGeom g(W, H, sampling);
  RV_CHECK_ARG(record_stride % 16 == 0 && (uintptr_t)records % 16 == 0,
               "records and their stride must be 16-byte aligned");
  RV_CHECK_ARG(record_stride >= record_bytes_of(g), "record stride %zu too small for %dx%d",
               record_stride, W, H);
  if (S == 0) return RV_OK;
  QuantArg qa;
  rvjpeg::quant_tables(quality, qa.q[0], qa.q[1]);
  const int per_row = g.grid_w(0) * g.fv + 2 * g.mx;
  const dim3 grid(ceil_div(per_row, kBlocksPerPass), g.my, S);
  jpeg_bgr_to_coef_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(bgr, records, record_stride, W,
                                                                    H, sampling, qa);
  return launch_status("rv_jpeg_bgr_to_coef_u8");
}

extern "C" size_t rv_jpeg_stream_ws_bytes(int S, int W, int H, int sampling) {
  if (S < 0 || S > 65535 || W < 1 || H < 1 || W > 65535 || H > 65535 || sampling < RV_JPEG_444 ||
      sampling > RV_JPEG_420)
    return 0;
  const EncGeom g(W, H, sampling);
  return seg_table_bytes(g, S) + (size_t)S * g.my * seg_ws_bytes(g);
}

extern "C" int rv_jpeg_coef_to_stream(const uint8_t* records, size_t record_stride, int S, int W,
                                      int H, int sampling, const uint8_t* header,
                                      size_t header_bytes, uint8_t* ws, size_t ws_bytes,
                                      uint8_t* streams, size_t stream_stride, size_t capacity,
                                      void* stream) {
  RV_CHECK_ARG(records != nullptr && header != nullptr && ws != nullptr && streams != nullptr,
               "null pointer");
  if (!check_geometry(S, W, H, sampling)) return RV_EINVAL;
  RV_CHECK_ARG(record_stride % 16 == 0 && (uintptr_t)records % 16 == 0,
               "records and their stride must be 16-byte aligned");
  RV_CHECK_ARG((uintptr_t)ws % 16 == 0, "the workspace must be 16-byte aligned");
  RV_CHECK_ARG(header_bytes >= 2 && header_bytes <= (size_t)rvjpeg::kFileHeaderMax,
               "JPEG header prefix of %zu bytes (at most %d)", header_bytes,
               rvjpeg::kFileHeaderMax);
  RV_CHECK_ARG(ws_bytes >= rv_jpeg_stream_ws_bytes(S, W, H, sampling),
               "workspace of %zu bytes, %zu needed", ws_bytes,
               rv_jpeg_stream_ws_bytes(S, W, H, sampling));
  RV_CHECK_ARG(stream_stride % 4 == 0 && (uintptr_t)streams % 4 == 0 &&
                   capacity >= (size_t)kStreamHeader && capacity <= stream_stride,
               "streams must be 4-byte aligned, %d <= capacity (%zu) <= stride (%zu)",
               kStreamHeader, capacity, stream_stride);
  if (S == 0) return RV_OK;
  const EncGeom g(W, H, sampling);
  FileHeader fh;
  memset(&fh, 0, sizeof(fh));
  memcpy(fh.w, header, header_bytes);
  fh.n = (int)header_bytes;
  const dim3 grid(g.my, S);
  jpeg_entropy_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(records, record_stride, W, H,
                                                                sampling, ws, S);
  jpeg_compact_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(
      records, record_stride, W, H, sampling, ws, S, streams, stream_stride, capacity, fh);
  return launch_status("rv_jpeg_coef_to_stream");
}

extern "C" size_t rv_jpeg_encode_ws_bytes(int S, int W, int H, int sampling) {
  const size_t e = rv_jpeg_stream_ws_bytes(S, W, H, sampling);
  if (!e) return 0;
  return e + (size_t)S * record_bytes_of(EncGeom(W, H, sampling));
}

extern "C" int rv_jpeg_encode_bgr_u8(const uint8_t* bgr, int S, int H, int W, int sampling,
                                     int quality, uint8_t* ws, size_t ws_bytes, uint8_t* streams,
                                     size_t stream_stride, size_t capacity, void* stream) {
  RV_CHECK_ARG(ws != nullptr, "null pointer");
  if (!check_geometry(S, W, H, sampling)) return RV_EINVAL;
  RV_CHECK_ARG(quality >= 1 && quality <= 100, "JPEG quality %d not in 1..100", quality);
  RV_CHECK_ARG((uintptr_t)ws % 16 == 0, "the workspace must be 16-byte aligned");
  RV_CHECK_ARG(ws_bytes >= rv_jpeg_encode_ws_bytes(S, W, H, sampling),
               "workspace of %zu bytes, %zu needed", ws_bytes,
               rv_jpeg_encode_ws_bytes(S, W, H, sampling));
  const EncGeom g(W, H, sampling);
  uint8_t header[rvjpeg::kFileHeaderMax];
  size_t hn = 0;
  // one restart segment per MCU row
  int rc = rv_jpeg_write_header(W, H, sampling, quality, g.mx, header, sizeof(header), &hn);
  if (rc != RV_OK) return rc;
  const size_t ews = rv_jpeg_stream_ws_bytes(S, W, H, sampling);  // a multiple of 16
  uint8_t* records = ws + ews;
  const size_t rstride = record_bytes_of(g);
  rc = rv_jpeg_bgr_to_coef_u8(bgr, S, H, W, sampling, quality, records, rstride, stream);
  if (rc != RV_OK) return rc;
  return rv_jpeg_coef_to_stream(records, rstride, S, W, H, sampling, header, hn, ws, ews, streams,
                                stream_stride, capacity, stream);
}

}  // namespace rv
