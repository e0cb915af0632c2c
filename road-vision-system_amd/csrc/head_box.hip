// Sparse Detect box branch for gfx950 (launch_head_box of conv.h): the box
// convs behind cv2.i.0 evaluated at the candidates only.
//
// Ultralytics' non_max_suppression reads the box of an anchor only when its
// best class score passes conf -- a few percent of the anchors of a road
// scene -- so after the class-only decode (detect.hip, BOX = false) has
// listed those anchors, this kernel computes per candidate
//   u   = bf16(SiLU(cv2.i.1 over the 3x3 neighbourhood of cv2.i.0's map + bias))
//   box = dist2bbox(DFL(cv2.i.2 u + bias)) * stride
// and writes x1, y1, x2, y2 into the candidate row in place.
//
// Bit-identity with the dense launches: 16 candidates are the 16 columns of
// a v_mfma_f32_16x16x32_bf16 fragment (weights the A operand, lane quad q
// supplying channels 8q .. 8q+7 of a chunk), summed in the dense kernels'
// k order -- 32-channel chunks ascending, taps (ky, kx) ascending within a
// chunk, taps outside the map zero -- followed by their epilogue (acc +
// bias, silu4, pack_bf16x2) and by the decode's own cv2.i.2 / DFL code
// (head.h).  A fragment column never depends on its neighbours, so each
// candidate gets the dense result.
//
// Work: gridDim.z 256-thread workgroups per (level, image).  Per chunk of 64
// of the level's segments, wave 0 prefix-sums the segment counts, the block
// lists the occupied candidate slots in LDS, and the waves of the item's
// workgroups walk the list in groups of 16.  The kernel is latency-bound (a
// few groups per image), so a group costs three dependent memory round
// trips, not one per k-step: the anchors; then all 18 neighbourhood
// fragments at once; cv2.i.1's weights come from LDS (staged once per
// workgroup, their load issued beside the segment counts') and cv2.i.2's
// live in registers.  Every count is clamped to 0..64 and every anchor to
// its level's range before an address is formed, and loop bounds derive
// from the clamped values only: a stale or garbage list costs time, never a
// fault.
#include "conv.h"
#include "conv_common.h"
#include "head.h"

namespace rv {

struct HeadBoxLevels {
  HeadBoxLevel lv[4];
};

constexpr int kBoxC = 64;          // channels of cv2.i.0 / .1 / .2 (4 * reg_max)
constexpr int kURow = kBoxC + 8;   // u row stride in bf16 (144 B: 16-B aligned, rows 4 banks apart)
// cv2.i.1's weights in LDS: [64 couts][9 taps][64 ch] bf16 rows padded to
// 1168 B, so the 16 rows of an A fragment read fall on distinct banks
constexpr int kWRowB = 9 * kBoxC * 2 + 16;
constexpr int kWUnits = 9 * kBoxC * 2 / 16;       // 16-B units per weight row
constexpr int kWPerThread = kBoxC * kWUnits / 256;  // 18

template <int REG>
__global__ __launch_bounds__(256) void head_box_kernel(HeadLevels h, HeadBoxLevels hb, int B,
                                                       Cand* __restrict__ cand, int cap,
                                                       const int* __restrict__ seg_n, int nblk) {
  static_assert(4 * REG == kBoxC, "box branch width");
  static_assert(kBoxC * kWUnits % 256 == 0, "weight staging: whole units per thread");
  constexpr int MB = kBoxC / 16, KB = kBoxC / 32;
  extern __shared__ __attribute__((aligned(16))) uint8_t wlds[];  // [64][kWRowB]
  __shared__ int soff[65];                 // slot offsets of the chunk's segments in `list`
  __shared__ uint16_t list[64 * 64];       // occupied slots of the chunk: segment * 64 + rank
  __shared__ __attribute__((aligned(16))) bf16_t ub[4][16 * kURow];     // per wave: u, [cand][ch]
  __shared__ __attribute__((aligned(16))) float lgb[4][16 * (kBoxC + 4)];  // per wave: box logits
  const int b = blockIdx.y, z = blockIdx.z, nz = gridDim.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, quad = lane >> 4;
  // level of this block; only compile-time indices into the by-value arguments
  HeadLevel L = h.lv[0];
  HeadBoxLevel X = hb.lv[0];
  int lstart = 0, blk0 = 0, nsegl = h.blk[1];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (i == (int)blockIdx.x) {
      L = h.lv[i];
      X = hb.lv[i];
      lstart = h.start[i];
      blk0 = h.blk[i];
      nsegl = h.blk[i + 1] - h.blk[i];
    }
  const int H = L.H, W = L.W, HW = H * W;
  const bf16_t* tmap = X.t + (size_t)b * HW * X.t_cs;
  bf16_t* uw = ub[wave];
  float* lw = lgb[wave];
  // cv2.i.2's fragments and every bias this lane adds
  uint4 Aw[KB][MB];
  f32x4 b1v[MB], b2v[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) {
#pragma unroll
    for (int k = 0; k < KB; ++k)
      Aw[k][m] = *(const uint4*)(L.w_box + (size_t)(m * 16 + col) * kBoxC + k * 32 + quad * 8);
    b1v[m] = *(const f32x4*)(X.b1 + m * 16 + quad * 4);
    b2v[m] = *(const f32x4*)(L.b_box + m * 16 + quad * 4);
  }
  // the first chunk's counts are asked for before the weight rows, which
  // then stream into LDS under the same memory round trip
  int n0 = wave == 0 && lane < nsegl ? seg_n[(size_t)b * nblk + blk0 + lane] : 0;
  {
    uint4 wr[kWPerThread];
#pragma unroll
    for (int j = 0; j < kWPerThread; ++j)  // unit tid + 256 j of the [64][kWUnits] packed rows
      wr[j] = *(const uint4*)(X.w1 + (size_t)(tid + j * 256) * 8);
#pragma unroll
    for (int j = 0; j < kWPerThread; ++j) {
      const int u = tid + j * 256;
      *(uint4*)(wlds + (u / kWUnits) * kWRowB + (u % kWUnits) * 16) = wr[j];
    }
  }
  for (int c0 = 0; c0 < nsegl; c0 += 64) {
    if (wave == 0) {
      const int sgi = c0 + lane;
      int n = c0 == 0 ? n0 : (sgi < nsegl ? seg_n[(size_t)b * nblk + blk0 + sgi] : 0);
      n = min(max(n, 0), 64);
      // a segment's rows beyond the list's capacity were never written
      n = min(n, max(cap - (blk0 + sgi) * 64, 0));
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(n, off);
        if (lane >= off) n += o;
      }
      soff[lane + 1] = n;
      if (lane == 0) soff[0] = 0;
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
      const int o = soff[e >> 6];
      if ((e & 63) < soff[(e >> 6) + 1] - o) list[o + (e & 63)] = (uint16_t)e;
    }
    __syncthreads();
    const int total = soff[64];  // <= 4096
    Cand* const cbase = cand + (size_t)b * cap + (size_t)(blk0 + c0) * 64;
    for (int g0 = z * 4; g0 * 16 < total; g0 += 4 * nz) {  // block-uniform trip count
      const int g = g0 + wave;
      const bool active = g * 16 < total;  // wave-uniform
      int x = 0, y = 0, slot = 0;
      uint4 Bf[KB * 9];  // the candidate's 3x3 neighbourhood: [chunk][tap] fragments
      if (active) {
        const int ci = g * 16 + col;
        slot = list[ci < total ? ci : g * 16];  // idle columns repeat the group's first candidate
        int r = cbase[slot].anchor - lstart;
        r = min(max(r, 0), HW - 1);
        y = r / W;
        x = r - y * W;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
          const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
          const bf16_t* p = tmap + (size_t)(in ? yy * W + xx : 0) * X.t_cs + quad * 8;
#pragma unroll
          for (int k = 0; k < KB; ++k)
            Bf[k * 9 + t] = in ? *(const uint4*)(p + k * 32) : make_uint4(0, 0, 0, 0);
        }
      }
      if (active) {
        // cv2.i.1 (weights in wlds, staged before the list's barriers): chunks
        // ascending, taps ascending within a chunk
        f32x4 acc[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KB; ++k)
#pragma unroll
          for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int m = 0; m < MB; ++m) {
              const uint4 Af = *(const uint4*)(wlds + (m * 16 + col) * kWRowB +
                                               ((t * kBoxC + k * 32 + quad * 8) * 2));
              acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  __builtin_bit_cast(bf16x8, Af), __builtin_bit_cast(bf16x8, Bf[k * 9 + t]), acc[m],
                  0, 0, 0);
            }
        // the conv epilogue; lane holds channels m * 16 + quad * 4 + i of
        // candidate `col`: re-laid through LDS to the B layout
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = acc[m][i] + b1v[m][i];
          silu4(v);
          *(uint2*)(uw + col * kURow + m * 16 + quad * 4) =
              make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
        }
      }
      __syncthreads();
      if (active) {
        // cv2.i.2 (the decode's box MFMAs: head_mfma_fixed)
        f32x4 acc[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const uint4 Bu = *(const uint4*)(uw + col * kURow + k * 32 + quad * 8);
#pragma unroll
          for (int m = 0; m < MB; ++m)
            acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, Aw[k][m]),
                                                             __builtin_bit_cast(bf16x8, Bu), acc[m],
                                                             0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < MB; ++m)
          *(f32x4*)(lw + col * (kBoxC + 4) + m * 16 + quad * 4) = acc[m] + b2v[m];
      }
      __syncthreads();
      if (active) {
        // four lanes per candidate: lane part takes DFL side part
        const int an = lane >> 2, part = lane & 3;
        const float d = dfl_side<REG>(lw + an * (kBoxC + 4) + part * REG);
        const int base = lane & ~3;
        const float d0 = __shfl(d, base), d1 = __shfl(d, base + 1), d2 = __shfl(d, base + 2),
                    d3 = __shfl(d, base + 3);
        // candidate `an`'s position and slot live in lane an (quad 0, col an)
        const int xa = __shfl(x, an), ya = __shfl(y, an), sa = __shfl(slot, an);
        if (part == 0 && g * 16 + an < total)
          *(f32x4*)&cbase[sa].x1 = xywh2xyxy(dist2bbox(d0, d1, d2, d3, xa, ya, L.stride));
      }
    }
    __syncthreads();  // the next chunk rewrites soff / list
  }
}

int launch_head_box(const HeadLevel* lv, const HeadBoxLevel* bx, int nlv, int B, int reg_max,
                    Cand* cand, int cand_cap, const int* seg_n, hipStream_t s) {
  HeadLevels h;
  if (!head_levels(lv, nlv, reg_max, h)) return RV_EINVAL;
  HeadBoxLevels hb = {};
  for (int i = 0; i < nlv; ++i) {
    if (!lv[i].w_box || !lv[i].b_box || lv[i].cin_b != kBoxC || !bx[i].t || !bx[i].w1 ||
        !bx[i].b1 || bx[i].t_cs % 8 || (uintptr_t)bx[i].t % 16 || (uintptr_t)bx[i].w1 % 16 ||
        (uintptr_t)bx[i].b1 % 16) {
      set_error("sparse box branch: bad level %d (box width %d)", i, lv[i].cin_b);
      return RV_EINVAL;
    }
    hb.lv[i] = bx[i];
  }
  const int nblk = h.blk[nlv];
  if (!cand || !seg_n || B < 1 || cand_cap < 1 || (uintptr_t)cand % 16) {
    set_error("sparse box branch: candidate buffers incomplete");
    return RV_EINVAL;
  }
  constexpr int smem = kBoxC * kWRowB;  // 74752 B: above the 64 KB default cap
  static const bool raised =
      hipFuncSetAttribute((const void*)head_box_kernel<16>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, smem) == hipSuccess;
  if (!raised) {
    (void)hipGetLastError();
    set_error("sparse box branch: cannot raise the dynamic LDS limit to %d bytes", smem);
    return RV_EINVAL;
  }
  // workgroups per (level, image): a scene's few 16-candidate groups side by
  // side (each workgroup runs 4 at a time) while the grid stays near the
  // chip's size
  int nz = 4;
  while (nz > 1 && (long)nlv * B * nz > 2L * num_cus()) nz >>= 1;
  head_box_kernel<16><<<dim3(nlv, B, nz), 256, smem, s>>>(h, hb, B, cand, cand_cap, seg_n, nblk);
  return launch_status("head_box");
}

}  // namespace rv
