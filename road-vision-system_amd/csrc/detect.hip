// Detect head decode kernel for gfx950 (decode_segments /
// launch_detect_decode of conv.h).
#include "conv.h"
#include "conv_common.h"
#include "head.h"

namespace rv {

// ---------------------------------------------------------------------------
// Detect head decode: DFL softmax-expectation, dist2bbox (xywh) * stride,
// class sigmoid; Ultralytics non_max_suppression candidate filter.
// ---------------------------------------------------------------------------
// One 256-thread workgroup per 64 consecutive anchors of one level: their
// (64 x cs) f32 head logits are one contiguous span, staged into LDS with
// coalesced 16-B loads at a padded row stride (cs + 4 floats: rows 20 banks
// apart at 80 classes, conflict-free fragment reads).  cs is 4 REG + nc
// rounded up to a multiple of 4: the (at most 3) padding logits of a row are
// zeros, and nc stays exact in the class scan and in raw.  Four lanes share
// an anchor: lane
// part p takes the DFL side p (softmax expectation over REG bins) and the
// classes p, p+4, ...; the quad then combines the four sides and the
// first-max class with lane shuffles.
//
// FUSED: the head's last 1x1 convs (cv2.i.2: 4*REG box logits, cv3.i.2: nc
// class logits, no activation) run here on MFMA from the level's bf16
// features (L.feat, [box feats | class feats]) straight into the LDS logits
// tile, so the f32 logits never touch HBM (L.logits, when non-null, still
// receives them: the parity tests read it).  Wave w computes anchors
// 16w..16w+15 of the block: box fragments m = 0..REG/4-1, class fragments
// after them; B fragments are 16-B loads of one anchor's 8 channels, A
// fragments 16-B loads of the packed [cout][cin_pad32] weights (L2-resident).
// Class score: exp + one v_rcp_f32 (no IEEE division sequence).  The raw
// output and the candidate filter use this same function, so the scores NMS
// sees are the scores in `raw`.
//
// CLASS-ONLY (BOX = false, the fixed head of a sparse forward): the class
// branch, the candidate filter and the segment counts exactly as above, but no
// box features, box MFMAs, logits tile or DFL; a candidate row's box stays
// zero until head_box.hip's kernel, next on the stream, fills it in.
__device__ __forceinline__ float head_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}

// The fused head's MFMA section with compile-time trip counts (KB box /
// KC class 32-channel k-steps, NCF class fragments: YOLOv8n's 80-class head
// is KB = 2, KC = 3, NCF = 5; with nc <= 64 classes its class branch is 64
// wide: KC = 2, NCF = ceil(nc / 16) in 1..4, the last fragment's classes
// beyond nc masked out of the scan; the packed weights and bias are padded to
// 16 couts, so every fragment row exists): every A / B fragment load of the
// wave is issued
// before the first MFMA, so the wave waits out one L2 latency instead of
// one per (fragment, k-step) -- the runtime-bound loops compiled to a
// load / s_waitcnt vmcnt(0) / MFMA chain.  Same k order and sums as the
// generic loops (bit-identical logits).  The weight fragments (23 x 16 B
// per lane) are loaded by head_weights once per level and stay in VGPRs
// while the block walks its anchor tiles: per 16-anchor wave tile they were
// 4.6x the feature bytes, all of it L2 -> CU traffic.
// BOX = false (the class-only decode): no box weights, features or MFMAs.
template <int REG, int KB, int KC, int NCF, bool BOX>
__device__ __forceinline__ void head_weights(const HeadLevel& L, uint4 (&Ab)[KB][REG / 4],
                                             uint4 (&Ac)[KC][NCF]) {
  constexpr int MB = REG / 4;
  const int lane = threadIdx.x & 63, col = lane & 15, quad = lane >> 4;
  constexpr int cinb = KB * 32, cinc = KC * 32;
  if constexpr (BOX) {
#pragma unroll
    for (int k = 0; k < KB; ++k)
#pragma unroll
      for (int m = 0; m < MB; ++m)
        Ab[k][m] = *(const uint4*)(L.w_box + (size_t)(m * 16 + col) * cinb + k * 32 + quad * 8);
  }
#pragma unroll
  for (int k = 0; k < KC; ++k)
#pragma unroll
    for (int m = 0; m < NCF; ++m)
      Ac[k][m] = *(const uint4*)(L.w_cls + (size_t)(m * 16 + col) * cinc + k * 32 + quad * 8);
}

// one 16-anchor wave tile's feature fragments (B operands): box channels,
// then class channels of anchor r0 + 16 wave + col
template <int REG, int KB, int KC, bool BOX>
__device__ __forceinline__ void head_feats(const HeadLevel& L, int b, int HW, int r0, int na,
                                           uint4 (&Bb)[KB], uint4 (&Bc)[KC]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int an0 = wave * 16 + col;
  const bool ok = an0 < na;
  const bf16_t* fp = L.feat + ((size_t)b * HW + r0 + (ok ? an0 : 0)) * L.feat_cs + quad * 8;
  if constexpr (BOX) {
#pragma unroll
    for (int k = 0; k < KB; ++k)
      Bb[k] = ok && k * 32 + quad * 8 < L.cin_b ? *(const uint4*)(fp + k * 32) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < KC; ++k)
    Bc[k] = ok && k * 32 + quad * 8 < L.cin_c ? *(const uint4*)(fp + 4 * REG + k * 32)
                                              : make_uint4(0, 0, 0, 0);
}

template <int REG, int KB, int KC, int NCF, bool BOX>
__device__ __forceinline__ void head_mfma_fixed(const HeadLevel& L, const uint4 (&Ab)[KB][REG / 4],
                                                const uint4 (&Ac)[KC][NCF], const uint4 (&Bb)[KB],
                                                const uint4 (&Bc)[KC], float* lg, int nc,
                                                float& best_out, int& bc_out) {
  constexpr int MB = REG / 4;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, col = lane & 15, quad = lane >> 4;
  float* row = lg + (size_t)(wave * 16 + col) * (L.cs + 4);
  if constexpr (BOX) {
    f32x4 acc[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KB; ++k)
#pragma unroll
      for (int m = 0; m < MB; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, Ab[k][m]),
                                                         __builtin_bit_cast(bf16x8, Bb[k]), acc[m], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      const int co = m * 16 + quad * 4;
      *(f32x4*)(row + co) = acc[m] + *(const f32x4*)(L.b_box + co);
    }
  }
  {
    f32x4 acc[NCF];
#pragma unroll
    for (int m = 0; m < NCF; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int m = 0; m < NCF; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, Ac[k][m]),
                                                         __builtin_bit_cast(bf16x8, Bc[k]), acc[m], 0, 0, 0);
    // the class scores never go to LDS: lane quad q holds classes
    // m * 16 + 4 q + i of its anchor (ascending in (m, i)), so a scan keeps
    // the lane's first maximum and two cross-quad steps (larger score, then
    // smaller class) give the anchor's first maximum -- the (score, class)
    // of a scan over all nc in order.  Same value per class as the LDS path
    // (acc + bias, then head_sigmoid).
    float best = -1.f;
    int bc = 0;
#pragma unroll
    for (int m = 0; m < NCF; ++m) {
      const int co = m * 16 + quad * 4;
      const f32x4 v = acc[m] + *(const f32x4*)(L.b_cls + co);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float sg = head_sigmoid(v[i]);
        if (co + i < nc && sg > best) {
          best = sg;
          bc = co + i;
        }
      }
    }
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const float ob = __shfl_xor(best, off);
      const int oc = __shfl_xor(bc, off);
      if (ob > best || (ob == best && oc < bc)) {
        best = ob;
        bc = oc;
      }
    }
    best_out = best;
    bc_out = bc;
  }
}


template <int REG, bool FUSED, int KB = 0, int KC = 0, int NCF = 0, int NCT = 0, bool BOX = true>
__global__ __launch_bounds__(256) void detect_decode_kernel(HeadLevels h, int B, int nc,
                                                            float conf, float* __restrict__ raw,
                                                            Cand* __restrict__ cand, int cap,
                                                            int* __restrict__ seg_n, int nblk,
                                                            int tpb) {
  extern __shared__ __attribute__((aligned(16))) float lg[];  // [64][cs + 4]
  __shared__ int wcnt[4];
  const int b = blockIdx.y;
  constexpr bool kFixed = FUSED && KC > 0;
  uint4 Ab[kFixed ? KB : 1][REG / 4], Ac[kFixed ? KC : 1][kFixed ? NCF : 1];
  uint4 Bb[kFixed ? KB : 1], Bc[kFixed ? KC : 1];  // the current tile's features
  int wl = -1;       // level whose head weights are in Ab / Ac
  bool pre = false;  // Bb / Bc already hold this tile's features
  float hbest = -1.f;  // fixed head: the lane's anchor's best class score / class
  int hbc = 0;
  // The block walks anchor tiles blockIdx.x * tpb .. + tpb - 1 (64 anchors
  // each; tpb > 1 only for the fixed fused head, whose weight fragments then
  // stay in registers).  Every lg read of a tile precedes the block barrier
  // before its candidate write-out, and a wave writes only its own 16 rows,
  // so the next tile's MFMA section may overwrite the tile in place.
  for (int t = 0; t < tpb; ++t) {
    // block -> (level, first anchor in level).  Only compile-time indices
    // into the by-value argument: a dynamic index would copy it to scratch.
    const int blk = blockIdx.x * tpb + t;
    if (blk >= nblk) break;  // block-uniform
    int l = 0, A = h.start[1], lstart = 0, lblk = 0;
    HeadLevel L = h.lv[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      if (i < h.nlv) A = h.start[i + 1];
      if (i < h.nlv && blk >= h.blk[i]) {
        l = i;
        L = h.lv[i];
        lstart = h.start[i];
        lblk = h.blk[i];
      }
    }
    const int HW = L.H * L.W;
    const int r0 = (blk - lblk) * 64;
    const int na = min(64, HW - r0);
    const int tid = threadIdx.x;
    const int cs4 = L.cs / 4, ls4 = cs4 + 1;  // row length / LDS row stride in float4
    if constexpr (kFixed) {
      if (l != wl) {
        head_weights<REG, KB, KC, NCF, BOX>(L, Ab, Ac);
        wl = l;
      }
      if (!pre) head_feats<REG, KB, KC, BOX>(L, b, HW, r0, na, Bb, Bc);
      head_mfma_fixed<REG, KB, KC, NCF, BOX>(L, Ab, Ac, Bb, Bc, lg, nc, hbest, hbc);
      // the next tile's features stream in under this tile's decode (same
      // level only; a level change loads them at the top of its iteration)
      pre = t + 1 < tpb && blk + 1 < nblk && r0 + 64 < HW;
      if (pre) head_feats<REG, KB, KC, BOX>(L, b, HW, r0 + 64, min(64, HW - r0 - 64), Bb, Bc);
      __syncthreads();
    } else if constexpr (FUSED) {
      constexpr int MB = REG / 4;  // box fragments (4*REG couts)
      const int wave = tid >> 6, lane = tid & 63, col = lane & 15, quad = lane >> 4;
      const int an0 = wave * 16 + col;  // this lane's anchor (B column / D column)
      const bool ok = an0 < na;
      const bf16_t* fp = L.feat + ((size_t)b * HW + r0 + (ok ? an0 : 0)) * L.feat_cs + quad * 8;
      const int ncf = (nc + 15) / 16;  // class fragments
      float* lrow = lg + (size_t)an0 * (L.cs + 4);
      // box: K = cin_b (multiple of 32)
      {
        f32x4 acc[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int cinp = (L.cin_b + 31) & ~31;
        for (int k = 0; k < cinp; k += 32) {
          const bool kv = ok && k + quad * 8 < L.cin_b;
          const uint4 bv = kv ? *(const uint4*)(fp + k) : make_uint4(0, 0, 0, 0);
          const bf16x8 Bf = __builtin_bit_cast(bf16x8, bv);
#pragma unroll
          for (int m = 0; m < MB; ++m) {
            const bf16x8 Af = __builtin_bit_cast(
                bf16x8, *(const uint4*)(L.w_box + (size_t)(m * 16 + col) * cinp + k + quad * 8));
            acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Af, Bf, acc[m], 0, 0, 0);
          }
        }
        // lane holds couts m*16 + quad*4 + i of anchor `col` of this wave
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          const int co = m * 16 + quad * 4;
          const f32x4 bb = *(const f32x4*)(L.b_box + co);
          *(f32x4*)(lg + (size_t)(wave * 16 + col) * (L.cs + 4) + co) = acc[m] + bb;
        }
      }
      // classes: K = cin_c, couts nc (padded to 16)
      {
        const int cinp = (L.cin_c + 31) & ~31;
        for (int m0 = 0; m0 < ncf; m0 += 5) {  // up to 5 fragments (80 classes) per pass
          f32x4 acc[5];
#pragma unroll
          for (int m = 0; m < 5; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int k = 0; k < cinp; k += 32) {
            const bool kv = ok && k + quad * 8 < L.cin_c;
            // the class features follow the box branch's cin_b channels in a
            // feature row (80 in YOLOv8x; 4 * REG = 64 in the other variants)
            const uint4 bv = kv ? *(const uint4*)(fp + L.cin_b + k) : make_uint4(0, 0, 0, 0);
            const bf16x8 Bf = __builtin_bit_cast(bf16x8, bv);
#pragma unroll
            for (int m = 0; m < 5; ++m) {
              if (m0 + m >= ncf) break;
              const bf16x8 Af = __builtin_bit_cast(
                  bf16x8,
                  *(const uint4*)(L.w_cls + (size_t)((m0 + m) * 16 + col) * cinp + k + quad * 8));
              acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Af, Bf, acc[m], 0, 0, 0);
            }
          }
#pragma unroll
          for (int m = 0; m < 5; ++m) {
            if (m0 + m >= ncf) break;
            const int co = (m0 + m) * 16 + quad * 4;  // class index (bias padded to 16)
            const f32x4 bb = *(const f32x4*)(L.b_cls + co);
            float* d = lg + (size_t)(wave * 16 + col) * (L.cs + 4) + 4 * REG + co;
            const f32x4 v = acc[m] + bb;
            // the last fragment may run past nc: zeros in the row's padding
            // (classes nc .. cs - 4 REG - 1, fewer than 4), nothing beyond the row
            if (co + 3 < nc) {
              *(f32x4*)d = v;
            } else {
              const int ncp = L.cs - 4 * REG;
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (co + i < ncp) d[i] = co + i < nc ? v[i] : 0.f;
            }
          }
        }
      }
      (void)lrow;
      __syncthreads();
      if (L.logits_out) {  // parity/debug copy of the logits (coalesced rows)
        f32x4* dst = (f32x4*)(L.logits_out + ((size_t)b * HW + r0) * L.cs);
        for (int i = tid; i < na * cs4; i += 256) {
          const int row = i / cs4, c4 = i - (i / cs4) * cs4;
          dst[i] = ((const f32x4*)lg)[row * ls4 + c4];
        }
      }
    } else {
      const f32x4* src = (const f32x4*)(L.logits + ((size_t)b * HW + r0) * L.cs);
      // 8 loads in flight per thread before any LDS store (a plain copy loop
      // would wait out one HBM latency per element)
      for (int i0 = tid; i0 < na * cs4; i0 += 8 * 256) {
        f32x4 v[8];  // native vectors (a float4 struct array would live in scratch)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + u * 256;
          v[u] = i < na * cs4 ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + u * 256;
          if (i < na * cs4) {
            const int row = i / cs4, c4 = i - (i / cs4) * cs4;
            ((f32x4*)lg)[row * ls4 + c4] = v[u];
          }
        }
      }
      __syncthreads();
    }
    const int an = tid >> 2, part = tid & 3;
    const bool live = an < na;
    const float* px = lg + (live ? an : 0) * (L.cs + 4);
    // DFL side `part` (the class-only form leaves the boxes to head_box.hip)
    float d = 0.f;
    if constexpr (BOX) d = dfl_side<REG>(px + part * REG);
    // first maximum of the sigmoid scores.  The fixed head (NCT > 0) found
    // it in registers (head_mfma_fixed: lane (col, quad) of the MFMA layout
    // holds anchor col's result); otherwise lane part scans classes part,
    // part + 4, ... in LDS and the quad reduction picks the larger score,
    // then the smaller class.
    const float* pc = px + 4 * REG;
    float best = -1.f;
    int bc = 0;
    if constexpr (NCT > 0) {
      best = __shfl(hbest, (tid & 63) >> 2);
      bc = __shfl(hbc, (tid & 63) >> 2);
    } else {
      for (int c = part; c < nc; c += 4) {
        const float sg = head_sigmoid(pc[c]);
        if (sg > best) {
          best = sg;
          bc = c;
        }
      }
#pragma unroll
      for (int off = 1; off < 4; off <<= 1) {
        const float ob = __shfl_xor(best, off);
        const int oc = __shfl_xor(bc, off);
        if (ob > best || (ob == best && oc < bc)) {
          best = ob;
          bc = oc;
        }
      }
    }
    const int base = tid & ~3;
    const float d0 = __shfl(d, base), d1 = __shfl(d, base + 1), d2 = __shfl(d, base + 2),
                d3 = __shfl(d, base + 3);
    const int r = r0 + (live ? an : 0);
    const int a = lstart + r;
    const int y = r / L.W, x = r - (r / L.W) * L.W;
    const BoxXYWH bx = dist2bbox(d0, d1, d2, d3, x, y, L.stride);
    if (NCT == 0 && raw && live) {  // (the fixed head runs without raw / logits_out)
      for (int c = part; c < nc; c += 4)
        raw[((size_t)b * (4 + nc) + 4 + c) * A + a] = head_sigmoid(pc[c]);
      const float bxv = part == 0 ? bx.cx : (part == 1 ? bx.cy : (part == 2 ? bx.w : bx.h));
      raw[((size_t)b * (4 + nc) + part) * A + a] = bxv;
    }
    // Candidates go to this block's own 64-slot segment of the image's list
    // (slot = segment * 64 + rank, ranks in anchor order) and the segment's
    // count to seg_n: no cross-block atomics (same-address device atomics
    // from thousands of waves serialise for ~100 us).
    const bool pass = live && part == 0 && cand && best > conf;
    const unsigned long long m = __ballot(pass);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (!cand) continue;
    int base0 = blk * 64;
    for (int w2 = 0; w2 < wave; ++w2) base0 += wcnt[w2];
    if (tid == 0) seg_n[(size_t)b * nblk + blk] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (pass) {
      const int i = base0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (i < cap) {
        const f32x4 xy = BOX ? xywh2xyxy(bx) : f32x4{0.f, 0.f, 0.f, 0.f};
        Cand c;
        c.x1 = xy[0];
        c.y1 = xy[1];
        c.x2 = xy[2];
        c.y2 = xy[3];
        c.score = best;
        c.cls = bc;
        c.anchor = a;
        c.pad = 0;
        cand[(size_t)b * cap + i] = c;
      }
    }
  }
}

int decode_segments(const HeadLevel* lv, int nlv) {
  int n = 0;
  for (int i = 0; i < nlv; ++i) n += ceil_div(lv[i].H * lv[i].W, 64);
  return n;
}

int launch_detect_decode(const HeadLevel* lv, int nlv, int B, int nc, int reg_max, float conf,
                         float* raw, Cand* cand, int cand_cap, int* cand_n, hipStream_t s,
                         int* form, bool cls_only) {
  HeadLevels h;
  if (!head_levels(lv, nlv, reg_max, h)) return RV_EINVAL;
  const int cs = lv[0].cs;
  // the rows hold 4 * reg_max + nc logits (then padding): every class read
  // stays inside the row and the (64 x cs) tile inside 64 KB of LDS
  if (nc < 1 || nc > 128 || cs < 4 * reg_max + nc) {
    set_error("detect decode: nc=%d outside 1..128 or beyond the logits row (cs %d)", nc, cs);
    return RV_EINVAL;
  }
  const size_t smem = (size_t)64 * (cs + 4) * 4;
  const bool fused = lv[0].feat != nullptr;
  // YOLOv8n's fused head (every level: box 64 -> 64, class 80 -> 80): the
  // compile-time MFMA section
  // (it keeps the class scores in registers: no raw output, no logits copy)
  // -- and the same head with at most 64 classes (class 64 -> nc: two class
  // k-steps, ceil(nc / 16) <= 4 class fragments)
  const int cin_c_fixed = nc == 80 ? 80 : 64;
  bool fixed = fused && (nc == 80 || nc <= 64) && raw == nullptr;
  for (int i = 0; i < nlv && fixed; ++i)
    fixed = lv[i].cin_b == 64 && lv[i].cin_c == cin_c_fixed && lv[i].logits_out == nullptr;
  if (cls_only && !(fixed && cand)) {
    set_error("detect decode: the class-only form needs the fixed fused head and a candidate list");
    return RV_EINVAL;
  }
  if (form) *form = !fused ? 0 : (fixed ? (cls_only ? 3 : 2) : 1);
  if (smem > 64 * 1024) {  // only raise the cap when the head needs it (large nc)
    // best effort: a failure surfaces as the launch error reported below
    (void)hipFuncSetAttribute(fused ? (const void*)detect_decode_kernel<16, true>
                              : (const void*)detect_decode_kernel<16, false>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipGetLastError();
  }
  const int nblk = h.blk[nlv];
  if (cand && cand_cap < nblk * 64) {
    set_error("detect decode: cand_cap %d < %d segments x 64", cand_cap, h.blk[nlv]);
    return RV_EINVAL;
  }
  if (fused) {
    for (int i = 0; i < nlv; ++i)
      if (lv[i].cs != ((4 * reg_max + nc + 3) & ~3) || lv[i].cin_b % 8 || lv[i].cin_c % 8 ||
          lv[i].feat_cs % 8) {
        set_error("fused head: bad level %d geometry", i);
        return RV_EINVAL;
      }
    if (fixed) {
      // anchor tiles per block: enough blocks to fill the chip several times
      int tpb = 4;
      while (tpb > 1 && (long)ceil_div(nblk, tpb) * B < 4L * num_cus()) --tpb;
      const dim3 grid(ceil_div(nblk, tpb), B);
      // (the class-only form keeps no logits tile)
#define RV_FIXED_HEAD(KC_, NCF_)                                                           \
  if (cls_only)                                                                            \
    detect_decode_kernel<16, true, 2, KC_, NCF_, 16 * NCF_, false><<<grid, 256, 0, s>>>(   \
        h, B, nc, conf, raw, cand, cand_cap, cand_n, nblk, tpb);                           \
  else                                                                                     \
    detect_decode_kernel<16, true, 2, KC_, NCF_, 16 * NCF_><<<grid, 256, smem, s>>>(       \
        h, B, nc, conf, raw, cand, cand_cap, cand_n, nblk, tpb)
      switch (nc == 80 ? 5 : ceil_div(nc, 16)) {
        case 5: RV_FIXED_HEAD(3, 5); break;
        case 4: RV_FIXED_HEAD(2, 4); break;
        case 3: RV_FIXED_HEAD(2, 3); break;
        case 2: RV_FIXED_HEAD(2, 2); break;
        default: RV_FIXED_HEAD(2, 1); break;
      }
#undef RV_FIXED_HEAD
    } else {
      detect_decode_kernel<16, true><<<dim3(nblk, B), 256, smem, s>>>(h, B, nc, conf, raw, cand,
                                                                      cand_cap, cand_n, nblk, 1);
    }
  } else {
    detect_decode_kernel<16, false><<<dim3(nblk, B), 256, smem, s>>>(h, B, nc, conf, raw, cand,
                                                                     cand_cap, cand_n, nblk, 1);
  }
  return launch_status("detect_decode");
}

}  // namespace rv
