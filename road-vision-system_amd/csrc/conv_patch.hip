// The LDS-staged patch conv kernel and its launcher (conv.hip: the kernels' order).
#include "conv_kernels.h"

namespace rv {

// ---------------------------------------------------------------------------
// conv_patch_kernel: LDS-staged implicit GEMM for k in {1,3}, s in {1,2}.
//
// A workgroup owns an R x C tile of output pixels of one image (flattened
// into 64*NR pixel slots, 16*NR per wave) and 16*MR output channels.  The K
// loop walks the input channels in 32-channel chunks; per chunk the input
// halo patch ((R-1)*S+K rows x (C-1)*S+K cols x 32 ch) and the chunk's
// weights (16*MR rows x K*K taps x 32 ch) are DMA'd HBM/L2 -> LDS with
// global_load_lds_dwordx4 (no VGPR round trip), double-buffered so chunk c+1
// streams in while chunk c's K*K taps run on MFMA from LDS.  Every input
// pixel is fetched once per chunk and reused K*K times from LDS.
// LDS images are lane-linear per DMA instruction (16 B per lane); bank
// conflicts on the 16-B fragment reads are removed by an XOR swizzle of the
// 16-B quarter inside each 64-B pixel/tap row, applied on the DMA source
// address and on the read address (the same involution on both sides).
// Out-of-image pixels and channels >= Cin DMA from a zero block.
// ---------------------------------------------------------------------------
#ifdef RV_PHASE_PROF
// Timing build (-DRV_PHASE_PROF): s_memtime cycles per phase of
// conv_patch_kernel summed over every wave of every launch: 0 prologue
// (resident weights + first stage + barrier), 1 next-step DMA issue (incl.
// the tile's offset prep), 2 compute, 3 epilogue, 4 end-of-step barrier
// (incl. the vmcnt wait for the next stage), 5 steps, 6 waves.
__device__ unsigned long long g_conv_phase[8];
#define RV_PH_T() __builtin_amdgcn_s_memtime()
#endif

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, void* lds, uint32_t voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16,
                                           (int)voff, soff, 0, 0);
}

// The patch kernel's form of epilogue_fast, split in two: epi_pack computes
// the tile's packed bf16 outputs and their store offsets into registers
// (the same values and store layout as epilogue_fast; invalid pixels and
// fragments beyond Cout get the dropped offset, so every lane issues every
// store), epi_store issues the stores.  The patch kernel packs before its
// end-of-step barrier and stores after it, so the stores drain under the
// next step's MFMAs instead of being waited for at that barrier
// (s_waitcnt vmcnt(0) counts stores too: tools/conv_phase.py put 26 % of the
// patch kernel's wave time in that wait).
template <int MR, int NR>
struct EpiPend {
  v4u32 pk[MR / 2 > 0 ? MR / 2 : 1][NR];
  uint32_t off[MR / 2 > 0 ? MR / 2 : 1][NR];
  v2u32 pk1[NR];
  uint32_t off1[NR];
};

template <int MR, int NR>
__device__ __forceinline__ void epi_pack(const ConvArgs& a, f32x4 (&acc)[MR][NR], int cout0,
                                         const bool (&pv)[NR], const uint32_t (&opx)[NR], int quad,
                                         const f32x4 (&bias)[MR], EpiPend<MR, NR>& ep) {
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, 0x7FFFFFFF, kRsrcFlags);
  const int cq = cout0 + quad * 4;
  constexpr uint32_t kDrop = 0x80000000u;
  // residual: every fragment's 8-B load issued up front, one wait for all
  // (a load then wait per fragment paid a full memory latency each, behind
  // the next stage's DMA in the same in-order counter)
  uint2 rq[MR][NR];
  if (a.res) {
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const uint32_t vr = (__umul24(opx[n], (uint32_t)a.res_cs) + a.res_co + cq) * 2;
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        // invalid pixels (past the map's end on the last image's bottom
        // tile row) and fragments beyond Cout read the dropped offset
        const uint32_t roff = pv[n] && cout0 + m * 16 < a.Cout ? vr + m * 32 : kDrop;
        rq[m][n] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rr, (int)roff, 0, 0));
      }
    }
  }
  auto value = [&](int m, int n, uint32_t vr, uint32_t& lo, uint32_t& hi) {
    (void)vr;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = acc[m][n][i] + bias[m][i];
    if (a.act) silu4(v);
    if (a.res) {
      const uint2 q = rq[m][n];
      v[0] += bf2f(q.x & 0xFFFF);
      v[1] += bf2f(q.x >> 16);
      v[2] += bf2f(q.y & 0xFFFF);
      v[3] += bf2f(q.y >> 16);
    }
    lo = pack_bf16x2(v[0], v[1]);
    hi = pack_bf16x2(v[2], v[3]);
  };
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    const uint32_t vo = (__umul24(opx[n], (uint32_t)a.out0_cs) + a.out0_co + cq) * 2;
    const uint32_t vr = a.res ? (__umul24(opx[n], (uint32_t)a.res_cs) + a.res_co + cq) * 2 : 0u;
    const uint32_t vo16 = vo + (16 * (quad & 1) + 8 * (quad >> 1) - 4 * quad) * 2;
#pragma unroll
    for (int m = 0; m + 1 < MR; m += 2) {
      uint32_t a0, a1, b0, b1;
      value(m, n, vr, a0, a1);
      value(m + 1, n, vr, b0, b1);
      const auto x0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
      const auto x1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
      const bool ok = pv[n] && cout0 + (m + (quad & 1)) * 16 < a.Cout;
      ep.off[m / 2][n] = ok ? vo16 + m * 32 : kDrop;
      ep.pk[m / 2][n] = v4u32{x0[0], x1[0], x0[1], x1[1]};
    }
    if constexpr (MR & 1) {
      constexpr int m = MR - 1;
      uint32_t lo, hi;
      value(m, n, vr, lo, hi);
      ep.off1[n] = pv[n] && cout0 + m * 16 < a.Cout ? vo + m * 32 : kDrop;
      ep.pk1[n] = v2u32{lo, hi};
    }
  }
}

template <int MR, int NR>
__device__ __forceinline__ void epi_store(const ConvArgs& a, const EpiPend<MR, NR>& ep) {
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out0, 0, 0x7FFFFFFF, kRsrcFlags);
#pragma unroll
  for (int n = 0; n < NR; ++n) {
#pragma unroll
    for (int m = 0; m + 1 < MR; m += 2)
      __builtin_amdgcn_raw_buffer_store_b128(ep.pk[m / 2][n], ro, (int)ep.off[m / 2][n], 0, 0);
    if constexpr (MR & 1) __builtin_amdgcn_raw_buffer_store_b64(ep.pk1[n], ro, (int)ep.off1[n], 0, 0);
  }
}

// Patch layout in LDS.  Stride-1 convs: pixel pp of the halo patch owns 64
// bytes at pp * 64 (its 32 channels = 4 x 16-B quarters); LDS slot quarter
// q of a pixel in patch column px holds source quarter q ^ swzq(px), so the
// 16 consecutive pixels of a B fragment (one patch row) are conflict-free
// in every ds_read_b128 lane group.  The swizzle depends on the column only, so a
// kernel-row step (ky) moves every address by the same PW * 64 and the
// per-lane tap addresses are precomputed once per block (NR x K values).
// Stride-2 convs store the patch columns de-interleaved (even columns, then
// odd ones: stored column sc of column px = px/2 or HE + px/2, HE = the even
// count), so the 16 output pixels of a fragment -- patch columns two apart --
// read 16 consecutive stored columns at every tap (kx = 0: sc = c, 1: HE + c,
// 2: c + 1) and the same swizzle, on the stored column, keeps them
// conflict-free.  The DMA stays lane-linear: lane l of DMA instruction j
// fills slot L = 64 j + l, i.e. stored pixel L / 4, slot quarter L % 4.
template <int S>
constexpr int patch_pixb() {
  return 64;
}
// stored column of patch column px (S = 2: de-interleaved)
template <int S>
__device__ __forceinline__ int patch_scol(int px, int PW) {
  return S == 1 ? px : ((px & 1) ? (PW + 1) / 2 + (px >> 1) : (px >> 1));
}

// Per-lane DMA source offsets of one patch (elements from the image base,
// -1 = zero block), at most patch_maxit(NR, S) DMA instructions per wave.
template <int NR, int S>
constexpr int patch_maxit() {
  return (S == 2 ? 6 : 2) * NR + 2;
}

template <int MR, int NR>
__device__ __forceinline__ void epilogue8(const ConvArgs& a, f32x4 (&acc)[MR][NR], int cout0,
                                          const bool (&pv)[NR], const int (&pb)[NR],
                                          const int (&py)[NR], const int (&px)[NR], int quad,
                                          const f32x4 (&bias)[MR], const f32x4 (&dq)[MR]) {
  const float inv0 = 1.0f / a.s_out0, inv1 = 1.0f / a.s_out1;
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    if (!pv[n]) continue;
    const int b = pb[n], oy = py[n], ox = px[n];
    const size_t opix = ((size_t)b * a.Ho + oy) * a.Wo + ox;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int co = cout0 + m * 16 + quad * 4;
      if (co >= a.Cout) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = acc[m][n][i] * dq[m][i] + bias[m][i];
      if (a.act) {
        silu4(v);
      }
      if (a.res) {
        const uint32_t rr = *(const uint32_t*)((const uint8_t*)a.res + opix * a.res_cs + a.res_co + co);
        v[0] += __builtin_amdgcn_cvt_f32_fp8((int)rr, 0) * a.s_res;
        v[1] += __builtin_amdgcn_cvt_f32_fp8((int)rr, 1) * a.s_res;
        v[2] += __builtin_amdgcn_cvt_f32_fp8((int)rr, 2) * a.s_res;
        v[3] += __builtin_amdgcn_cvt_f32_fp8((int)rr, 3) * a.s_res;
      }
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        void* outp = d == 0 ? a.out0 : a.out1;
        if (!outp) continue;
        const int cs_ = d == 0 ? a.out0_cs : a.out1_cs;
        const int co_ = (d == 0 ? a.out0_co : a.out1_co) + co;
        const int up = d == 0 ? a.out0_up : a.out1_up;
        const int o8 = d == 0 ? a.out0_8 : a.out1_8;
        const int ny = up ? 2 : 1;
        for (int dy = 0; dy < ny; ++dy)
          for (int dx = 0; dx < ny; ++dx) {
            const size_t q = up ? ((size_t)(b * 2 * a.Ho + 2 * oy + dy) * (2 * a.Wo) + 2 * ox + dx) : opix;
            if (o8) {
              *(uint32_t*)((uint8_t*)outp + q * cs_ + co_) = f8_encode4(v, d == 0 ? inv0 : inv1);
            } else if (a.out_f32) {
              *(float4*)((float*)outp + q * cs_ + co_) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
              *(uint2*)((uint16_t*)outp + q * cs_ + co_) =
                  make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
            }
          }
      }
    }
  }
}

// Persistent, software-pipelined form: the block owns cout tile blockIdx.y
// and walks pixel tiles blockIdx.x, +gridDim.x, ...  A step is (tile, group
// of G input-channel chunks); the DMA of step s+1 -- the next group or the
// next tile's first group -- streams in while step s runs on MFMA and while
// the previous tile's epilogue stores drain.  G > 1 cuts the number of
// dependent DMA round trips per tile (a deep-K layer with few tiles is a
// chain of nch / G latencies, not nch).  RESW: the block's whole weight slab
// (nch chunks) is DMA'd into LDS once at kernel start and stays resident, so
// a step only moves its input patch.  Per-lane DMA offsets are computed once
// per tile (no integer division in the chunk loop).
//
// Grouped form (ConvArgs::g2_*): cout tiles at or above g2_cout0 read their
// own input channel slice / weights / bias (a block-diagonal conv: the
// Detect head's cv2 and cv3 branches in one launch).  The host keeps every
// tile inside one group.
// F8 = true: fp8 e4m3 inputs / weights (ConvArgs::in8).  A pipeline chunk
// is 64 channels (64 B per pixel slot, the same LDS image as the bf16
// kernel's 32-channel chunk); each tap runs two v_mfma_f32_16x16x32_fp8_fp8
// per chunk (channels 0-31 and 32-63), each lane reading 8 of its 16-B
// quarter pair (logical quarter 2h + quad/2, byte (quad & 1) * 8).
// NW = 8 (kind 2): one 512-thread workgroup per CU instead of two of 256,
// so a resident weight slab (or a staged chunk of weights) is shared by 8
// waves and the pixel tile is twice as large -- half the LDS-DMA bytes per
// MFMA of the 4-wave form at the same occupancy (2 waves per SIMD).
// CH (ConvArgs::ch_w): a chained 1x1 conv Cout -> Cout on the tile's output
// in LDS (bf16, one cout tile covering Cout) -- a C2f cv1 (SiLU, stored):
// see chain_tile.
template <int MR, int NR, int K, int S, bool RESW, bool F8, int NW = 4, bool CH = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void conv_patch_kernel(ConvArgs a, PatchGeo g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int T2 = K * K;
  constexpr int BC = 16 * MR;
  constexpr int W_BYTES = BC * T2 * 64;
  constexpr int MAXP = patch_maxit<NR, S>();
  static_assert(MAXP <= 32, "tail mask is 32 bits");
  constexpr int WJ = BC * T2 / 16;            // weight DMA instructions per chunk
  constexpr int MAXW = (WJ + NW - 1) / NW;
  constexpr int EB = F8 ? 1 : 2;              // bytes per element
  constexpr int CC = F8 ? 64 : 32;            // channels per chunk (64 B per pixel)
  const int tid = threadIdx.x;
  // the wave index as a scalar: every per-wave DMA test below is then a
  // scalar branch, not an exec-mask region inside the MFMA stream
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int col = lane & 15, quad = lane >> 4;
  const int cout0 = blockIdx.y * BC;  // first output channel of the tile (output numbering)
  // the tile's group: its input slice, weights, bias and weight row base wc0
  int wc0 = cout0, gcout = a.g2_cout0 > 0 ? a.g2_cout0 : a.Cout;
  int in_co = a.in_co, Cin = a.Cin;
  const uint8_t* wts = (const uint8_t*)a.w;
  const float* bias_p = a.bias;
  const float* wsc_p = a.wscale;
  if (a.g2_cout0 > 0 && cout0 >= a.g2_cout0) {
    wc0 = cout0 - a.g2_cout0;
    gcout = a.Cout - a.g2_cout0;
    in_co = a.g2_in_co;
    Cin = a.g2_Cin;
    wts = (const uint8_t*)a.g2_w;
    bias_p = a.g2_bias;
    wsc_p = a.g2_wscale;
  }
  const int wcout_pad = (gcout + 15) & ~15;
  const int cin_pad = (Cin + CC - 1) & ~(CC - 1);
  const int Kp = T2 * cin_pad;                // weight row length (elements)
  const int nch = cin_pad / CC;
  const int G = g.G < nch ? g.G : nch;
  const int ngrp = (nch + G - 1) / G;
  const int chunk_bytes = g.p_bytes + (RESW ? 0 : W_BYTES);
  const int stage_bytes = G * chunk_bytes;
  uint8_t* const stages = smem + (RESW ? nch * W_BYTES : 0);
  constexpr int pad = K / 2;
  const int tiles_img = g.tiles_x * g.tiles_y;
  const int ntiles = a.B * tiles_img;
  const TileWalk walk = tile_walk(ntiles);
  const int nsteps = walk.count() * ngrp;
  const int npp = g.PH * g.PW;
  const float inv_pw = 1.0f / (float)g.PW;

  // block-constant: output slots -> (r, cc) of the tile, patch byte base
  constexpr int PB = patch_pixb<S>(), SL = PB / 16;
  // fp8: lane quad reads channel half 0 at logical quarter quad / 2; half 1
  // (quarter + 2) is the same address XOR 32 (the swizzle XORs the quarter)
  int orow[NR], ocol[NR], boff[NR][K];
  bool oin[NR];
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    const int q = wave * (NR * 16) + n * 16 + col;
    orow[n] = q / g.C;
    ocol[n] = q - orow[n] * g.C;
    oin[n] = q < g.R * g.C;
    // per-lane LDS byte address of tap (0, kx) for output slot n
    const int pr = oin[n] ? orow[n] * S : 0, pc = oin[n] ? ocol[n] * S : 0;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int sc = patch_scol<S>(pc + kx, g.PW);
      const int lq = F8 ? quad >> 1 : quad;
      if constexpr (F8 && K == 3)  // tap-pair path: pixel slot base | swizzle (low bits)
        boff[n][kx] = (pr * g.PW + sc) * 64 + swzq<true>(sc);
      else
        boff[n][kx] = (pr * g.PW + sc) * 64 + ((lq ^ swzq<F8>(sc)) << 4) + (F8 ? (quad & 1) * 8 : 0);
    }
  }
  // fp8 3x3 convs run v_mfma_scale_f32_16x16x128_f8f6f4 (unit scales) on tap
  // pairs: k-slots 32q .. 32q+31 of lane quad q = channels 32 (q & 1) ..
  // +31 of tap t + (q >> 1) -- two 16-B quarters of that tap's 64-B slot.
  // aoff: this lane's two weight-quarter offsets within a (row, tap) slot
  // pair, per m (row = m*16 + col; the swizzle of the row picks the order)
  int aoff[F8 && K == 3 ? MR : 1][2];
  if constexpr (F8 && K == 3) {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int row = m * 16 + col, sw = swzq<true>(row);
      const int base = (row * T2 + (quad >> 1)) * 64;
      aoff[m][0] = base + (((2 * (quad & 1)) ^ sw) << 4);
      aoff[m][1] = base + (((2 * (quad & 1) + 1) ^ sw) << 4);
    }
  }
  // bf16: the block's bias lives in LDS (BC floats after the two stages;
  // patch_geo sizes it) and is read back per tile in the epilogue, so its
  // 4 * MR registers are free during the MFMA loop.  fp8 keeps bias and
  // dequantisation scales in registers.
  float* const bias_lds = (float*)(stages + 2 * stage_bytes);
  f32x4 bias[F8 ? MR : 1], dq[F8 ? MR : 1];
  if constexpr (F8) {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int co = wc0 + m * 16 + quad * 4;  // bias is padded to Cout_pad16
      bias[m] = co < wcout_pad ? *(const f32x4*)(bias_p + co) : f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 ws = co < wcout_pad ? *(const f32x4*)(wsc_p + co) : f32x4{0.f, 0.f, 0.f, 0.f};
      dq[m] = ws * a.s_in;
    }
  } else {
    for (int i = tid; i < BC; i += 64 * NW) bias_lds[i] = wc0 + i < wcout_pad ? bias_p[wc0 + i] : 0.f;
  }
  auto bias_tile = [&](f32x4 (&bl)[MR]) {
#pragma unroll
    for (int m = 0; m < MR; ++m) bl[m] = *(const f32x4*)(bias_lds + m * 16 + quad * 4);
  };
  // CH: the chained 1x1's weights (chunk-major [c][row][64 B], the quarter
  // swizzle of conv1x1_direct_kernel), its bias, and one x tile per wave
  // (the wave's 16 NR pixels x Cout channels of the producer's bf16 output,
  // chunk-major [c][pixel][64 B], quarter swizzle by pixel)
  constexpr int CHN = (MR + 1) / 2;                 // 32-channel chunks of the chained input
  uint8_t* const ch_w_lds = (uint8_t*)(bias_lds + BC);
  float* const ch_b_lds = (float*)(ch_w_lds + (CH ? CHN * BC * 64 : 0));
  uint8_t* const ch_x_lds = (uint8_t*)(ch_b_lds + (CH ? BC : 0)) + wave * (CH ? CHN * NR * 16 * 64 : 0);
  if constexpr (CH) {
    static_assert(!F8 && K == 3 && MR % 2 == 0, "chained 1x1: bf16 behind a 3x3 conv, fragment pairs");
    // BC / 16 DMA instructions per chunk (16 rows x 64 B each); the packed
    // 1x1 rows are CHN * 32 channels long (zero beyond Cout)
    for (int j = wave; j < CHN * (BC / 16); j += NW) {
      const int c = j / (BC / 16), jr = j - c * (BC / 16);
      const int row = jr * 16 + (lane >> 2);
      const int q = (lane & 3) ^ swzq<false>(row);
      __builtin_amdgcn_global_load_lds((const void*)(a.ch_w + (size_t)row * (CHN * 32) + c * 32 + q * 8),
                                       (void*)(ch_w_lds + c * BC * 64 + jr * 1024), 16, 0, 0);
    }
    for (int i = tid; i < BC; i += 64 * NW) ch_b_lds[i] = a.ch_b[i];
  }
  // Patch and weight DMA through buffer resources (buffer_load ... lds):
  // every DMA instruction's per-lane byte offset is computed once -- per
  // tile for the patch, per kernel for the weights --, the chunk offset
  // rides in the scalar soffset, and out-of-image pixels / rows beyond Cout
  // read zeros from the range check (voffset kOOB).  So a chunk step issues
  // its DMA with no address VALU; the tile-invariant lane geometry (patch
  // row, column, source quarter of every slot) is computed once per kernel.
  uint32_t tailbad = 0;  // bit it: this lane's quarter is >= Cin in the last chunk
  // slot it's patch row / column / source quarter: py | px << 12 | sq << 24;
  // a slot beyond the patch gets row 4095, which no map reaches (range check)
  int lgeo[MAXP];
#pragma unroll
  for (int it = 0; it < MAXP; ++it) {
    const int L = 64 * (wave + NW * it) + lane;
    const int pix = L / SL, q = L - SL * pix;
    const int py = (int)(((float)pix + 0.5f) * inv_pw);
    const int sc = pix - py * g.PW;  // stored column
    const int he = (g.PW + 1) >> 1;
    const int px = S == 1 ? sc : (sc < he ? 2 * sc : 2 * (sc - he) + 1);
    const int sq = q ^ swzq<F8>(sc);  // source quarter of slot q
    lgeo[it] = (pix < npp ? py : 4095) | (px << 12) | (sq << 24);
    if ((nch - 1) * CC + sq * (16 / EB) >= Cin) tailbad |= 1u << it;
  }
  const bool has_tail = Cin % CC != 0;
  uint32_t voff[MAXP];
  __amdgpu_buffer_rsrc_t img_rsrc;
  const int pix_bytes = a.in_cs * EB;
  auto prep_tile = [&](int ti) {
    const int b = ti / tiles_img;
    const int r = ti - b * tiles_img;
    const int ty = r / g.tiles_x, tx = r - (r / g.tiles_x) * g.tiles_x;
    const int iy0 = ty * g.R * S - pad, ix0 = tx * g.C * S - pad;
    const uint8_t* base = (const uint8_t*)a.in + ((size_t)b * a.Hin * a.Win * a.in_cs + in_co) * EB;
    img_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0,
                                                 (a.Hin * a.Win * a.in_cs - in_co) * EB, kRsrcFlags);
#pragma unroll
    for (int it = 0; it < MAXP; ++it) {
      const int gg = lgeo[it];
      const int iy = iy0 + (gg & 4095), ix = ix0 + ((gg >> 12) & 4095);
      const bool ok = (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
      // branchless select: an out-of-image slot reads zeros (kOOB)
      // 24-bit multiplies (full rate): a map pixel index and the pixel
      // stride are < 2^24 and the in-image byte offset < 2^31, so the low 32
      // bits are the product (an out-of-image slot's garbage is masked)
      const uint32_t off = __umul24((uint32_t)(__umul24(iy, a.Win) + ix), (uint32_t)pix_bytes) +
                           ((gg >> 24) & 3) * 16;
      const uint32_t m = ok ? 0u : 0xFFFFFFFFu;
      voff[it] = (off & ~m) | (kOOB & m);
    }
  };
  // weight DMA: instruction j moves (row, tap) pairs 16 j .. 16 j + 15, a
  // 16-B quarter of chunk c per lane
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(wts + (size_t)wc0 * Kp * EB), 0, (wcout_pad - wc0) * Kp * EB, kRsrcFlags);
  uint32_t wvoff[MAXW];
#pragma unroll
  for (int it = 0; it < MAXW; ++it) {
    const int j = wave + NW * it;
    const int pr = j * 16 + (lane >> 2);
    const int row = pr / T2, tap = pr - (pr / T2) * T2;
    const int q = (lane & 3) ^ swzq<F8>(row);
    wvoff[it] = wc0 + row < wcout_pad ? (uint32_t)((row * Kp + tap * cin_pad) * EB + q * 16) : kOOB;
  }
  auto dma_weights = [&](int c, uint8_t* Wl) {
#pragma unroll
    for (int it = 0; it < MAXW; ++it) {
      const int j = wave + NW * it;
      if (j < WJ) dma16(w_rsrc, Wl + j * 1024, wvoff[it], c * 64);
    }
  };
  auto stage = [&](int grp, int buf) {
    for (int gi = 0; gi < G; ++gi) {
      const int c = grp * G + gi;
      if (c >= nch) break;
      uint8_t* P = stages + buf * stage_bytes + gi * chunk_bytes;
      const bool tail = has_tail && c == nch - 1;  // block-uniform
      // Two paths: a select feeding every DMA (tail chunk only) made the
      // compiler route all of them through ONE address VGPR, and each
      // v_cndmask into it then waited for the previous buffer_load to read
      // its operand (a VMEM-read / VALU-write interlock per DMA); the common
      // path issues straight from the per-slot offset registers.
      if (tail) {
#pragma unroll
        for (int it = 0; it < MAXP; ++it) {
          const int j = wave + NW * it;
          if (j < g.pinst)
            dma16(img_rsrc, P + j * 1024, tail && ((tailbad >> it) & 1) ? kOOB : voff[it], c * 64);
        }
      } else {
#pragma unroll
        for (int it = 0; it < MAXP; ++it) {
          const int j = wave + NW * it;
          if (j < g.pinst) dma16(img_rsrc, P + j * 1024, voff[it], c * 64);
        }
      }
      if constexpr (!RESW) dma_weights(c, P + g.p_bytes);
    }
  };
  f32x4 acc[MR][NR];
  auto compute = [&](int grp, int buf) {
    for (int gi = 0; gi < G; ++gi) {
      const int c = grp * G + gi;
      if (c >= nch) break;
      const uint8_t* P = stages + buf * stage_bytes + gi * chunk_bytes;
      const uint8_t* Wl = RESW ? smem + c * W_BYTES : P + g.p_bytes;
      if constexpr (F8 && K == 3) {
        const int rowb = g.PW * PB;
#pragma unroll
        for (int t = 0; t < 9; t += 2) {
          const bool odd = t + 1 >= 9;  // the last tap pairs with zeros
          const int ky0 = t / 3, kx0 = t % 3;
          const int ky1 = odd ? ky0 : (t + 1) / 3, kx1 = odd ? kx0 : (t + 1) % 3;
          const bool hi = (quad >> 1) != 0;
          i32x8 A[MR], Bv[NR];
#pragma unroll
          for (int m = 0; m < MR; ++m) {
            const uint4 lo = *(const uint4*)(Wl + aoff[m][0] + t * 64);
            const uint4 up = *(const uint4*)(Wl + aoff[m][1] + t * 64);
            A[m] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                         (int)up.x, (int)up.y, (int)up.z, (int)up.w};
            if (odd && hi) A[m] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
          }
#pragma unroll
          for (int n = 0; n < NR; ++n) {
            const int v = hi ? boff[n][kx1] + ky1 * rowb : boff[n][kx0] + ky0 * rowb;
            const int sw = v & 3, base = v & ~63;
            const uint4 lo = *(const uint4*)(P + base + (((2 * (quad & 1)) ^ sw) << 4));
            const uint4 up = *(const uint4*)(P + base + (((2 * (quad & 1) + 1) ^ sw) << 4));
            Bv[n] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                          (int)up.x, (int)up.y, (int)up.z, (int)up.w};
          }
#pragma unroll
          for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int n = 0; n < NR; ++n)
              acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                  A[m], Bv[n], acc[m][n], 0, 0, 0, 127, 0, 127);
        }
        continue;
      }
      if constexpr (!F8 && MR * NR < 16) {
        // bf16: the taps' fragment reads are software-pipelined one tap
        // ahead -- tap t + 1's A / B fragments are read into the other
        // register set before tap t's MFMAs issue, so the MFMAs of a tap
        // never wait on the LDS reads issued right before them
        bf16x8 Af[2][MR], Bq[2][NR];
        auto ld = [&](int tap, int sl) {
          const int ky = tap / K, kx = tap - (tap / K) * K;
#pragma unroll
          for (int m = 0; m < MR; ++m) {
            const int row = m * 16 + col;
            Af[sl][m] = __builtin_bit_cast(
                bf16x8, *(const uint4*)(Wl + (row * T2 + tap) * 64 + ((quad ^ swzq<false>(row)) << 4)));
          }
#pragma unroll
          for (int n = 0; n < NR; ++n)
            Bq[sl][n] = __builtin_bit_cast(bf16x8, *(const uint4*)(P + ky * g.PW * PB + boff[n][kx]));
        };
        ld(0, 0);
#pragma unroll
        for (int t = 0; t < T2; ++t) {
          // hard fences pin the order (the scheduler otherwise sinks each
          // read next to its first use): tap t + 1's reads, then tap t's
          // MFMAs, which wait only for the reads issued one tap earlier
          if (t + 1 < T2) ld(t + 1, (t + 1) & 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int n = 0; n < NR; ++n)
              acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Af[t & 1][m], Bq[t & 1][n],
                                                                  acc[m][n], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        continue;
      }
      // (fp8, and the largest bf16 tiles, whose fragments of all taps in
      // flight would exceed the register file: kernel rows not unrolled)
#pragma unroll(F8 || MR * NR >= 16 ? 1 : K)
      for (int ky = 0; ky < K; ++ky) {
        const uint8_t* Prow = P + ky * g.PW * PB;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int tap = ky * K + kx;
          if constexpr (F8) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
              long A[MR], Bf[NR];
#pragma unroll
              for (int m = 0; m < MR; ++m) {
                const int row = m * 16 + col;
                A[m] = *(const long*)(Wl + (((row * T2 + tap) * 64 +
                                             (((quad >> 1) ^ swzq<true>(row)) << 4) + (quad & 1) * 8) ^
                                            (hh << 5)));
              }
#pragma unroll
              for (int n = 0; n < NR; ++n) Bf[n] = *(const long*)(Prow + (boff[n][kx] ^ (hh << 5)));
              // every read of the tap issued before its MFMAs (left alone,
              // the scheduler waits for each A fragment right before its
              // MFMAs: one LDS round trip per m)
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int n = 0; n < NR; ++n)
                  acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(A[m], Bf[n], acc[m][n], 0, 0, 0);
            }
          } else {
            bf16x8 A[MR], Bf[NR];
#pragma unroll
            for (int m = 0; m < MR; ++m) {
              const int row = m * 16 + col;
              A[m] = __builtin_bit_cast(
                  bf16x8, *(const uint4*)(Wl + (row * T2 + tap) * 64 + ((quad ^ swzq<false>(row)) << 4)));
            }
#pragma unroll
            for (int n = 0; n < NR; ++n)
              Bf[n] = __builtin_bit_cast(bf16x8, *(const uint4*)(Prow + boff[n][kx]));
            // every read of the tap issued before its MFMAs (left alone, the
            // scheduler waits for each A fragment right before its MFMAs:
            // one LDS round trip per m)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
              for (int n = 0; n < NR; ++n)
                acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[m], Bf[n], acc[m][n], 0, 0, 0);
          }
        }
      }
    }
  };

  if (nsteps == 0) return;
#ifdef RV_PHASE_PROF
  unsigned long long ph[5] = {0, 0, 0, 0, 0}, t_ph = RV_PH_T();
#define RV_PH(i)                             \
  {                                          \
    const unsigned long long t_ = RV_PH_T(); \
    ph[i] += t_ - t_ph;                      \
    t_ph = t_;                               \
  }
#else
#define RV_PH(i)
#endif
  int ti = walk.t0;  // tile of the current step
  int grp = 0;       // chunk group of the current step
  constexpr bool kDefer = !F8 && !CH && MR * NR <= 10;
  // epilogue of tile `tile` from acc (kDefer tiles on the fast path: packed
  // only, into ep; epi_store issues the stores after the barrier)
  // CH: the finished tile's producer values (bias, SiLU, bf16 -- what the
  // unfused conv stores) go to this wave's x tile instead of HBM, then the
  // chained 1x1 runs on them: per 32-channel chunk c ascending, A = its
  // weights, B = the wave's pixels (the k order of conv1x1_direct_kernel and
  // of the patch kernel's 1x1 form: bit-identical to the unfused launch),
  // and its epilogue (bias, SiLU) stores the output views.  Each wave reads
  // only the pixels it wrote (in-order LDS, no barrier).
  auto chain_tile = [&](const bool (&pv)[NR], const uint32_t (&opx)[NR]) {
    if constexpr (CH) {
      f32x4 bl[MR];
      bias_tile(bl);
#pragma unroll
      for (int n = 0; n < NR; ++n) {
        const int px = n * 16 + col;
#pragma unroll
        for (int m = 0; m < MR; m += 2) {
          uint32_t v0[2], v1[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = acc[m + h][n][i] + bl[m + h][i];
            if (a.act) silu4(v);
            v0[h] = pack_bf16x2(v[0], v[1]);
            v1[h] = pack_bf16x2(v[2], v[3]);
          }
          // quad q: channels 16 (q & 1) + 8 (q >> 1) .. +7 of chunk m / 2
          const auto x0 = __builtin_amdgcn_permlane16_swap(v0[0], v0[1], false, false);
          const auto x1 = __builtin_amdgcn_permlane16_swap(v1[0], v1[1], false, false);
          const int qq = 2 * (quad & 1) + (quad >> 1);
          *(v4u32*)(ch_x_lds + ((m / 2) * NR * 16 + px) * 64 + ((qq ^ swzq<false>(px)) << 4)) =
              v4u32{x0[0], x1[0], x0[1], x1[1]};
        }
      }
      f32x4 acc2[MR][NR];
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < NR; ++n) acc2[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CHN; ++c) {
        bf16x8 A2[MR], B2[NR];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          const int row = m * 16 + col;
          A2[m] = __builtin_bit_cast(
              bf16x8, *(const uint4*)(ch_w_lds + c * BC * 64 + row * 64 + ((quad ^ swzq<false>(row)) << 4)));
        }
#pragma unroll
        for (int n = 0; n < NR; ++n) {
          const int px = n * 16 + col;
          B2[n] = __builtin_bit_cast(
              bf16x8, *(const uint4*)(ch_x_lds + (c * NR * 16 + px) * 64 + ((quad ^ swzq<false>(px)) << 4)));
        }
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int n = 0; n < NR; ++n)
            acc2[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A2[m], B2[n], acc2[m][n], 0, 0, 0);
      }
      f32x4 bl2[MR];
#pragma unroll
      for (int m = 0; m < MR; ++m) bl2[m] = *(const f32x4*)(ch_b_lds + m * 16 + quad * 4);
      ConvArgs a2 = a;
      a2.act = 1;
      a2.res = nullptr;
      epilogue_fast<MR, NR>(a2, acc2, 0, pv, opx, quad, bl2);
    }
  };
  auto finish = [&](int tile, EpiPend<MR, NR>& ep) {
    const int b = tile / tiles_img;
    const int r = tile - b * tiles_img;
    const int ty = r / g.tiles_x, tx = r - (r / g.tiles_x) * g.tiles_x;
    bool pv[NR];
    int pb[NR], py[NR], px[NR];
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      pb[n] = b;
      py[n] = ty * g.R + orow[n];
      px[n] = tx * g.C + ocol[n];
      pv[n] = oin[n] && py[n] < a.Ho && px[n] < a.Wo;
    }
    if constexpr (F8) {
      epilogue8<MR, NR>(a, acc, cout0, pv, pb, py, px, quad, bias, dq);
    } else if constexpr (CH) {
      uint32_t opx[NR];
#pragma unroll
      for (int n = 0; n < NR; ++n) opx[n] = (uint32_t)((b * a.Ho + py[n]) * a.Wo + px[n]);
      chain_tile(pv, opx);
    } else if (g.fast) {
      uint32_t opx[NR];  // < 2^23 (epi_fast): 24-bit multiplies
#pragma unroll
      for (int n = 0; n < NR; ++n) opx[n] = __umul24((uint32_t)(b * a.Ho + py[n]), (uint32_t)a.Wo) + px[n];
      f32x4 bl[MR];
      bias_tile(bl);
      if constexpr (kDefer)
        epi_pack<MR, NR>(a, acc, cout0, pv, opx, quad, bl, ep);
      else
        epilogue_fast<MR, NR>(a, acc, cout0, pv, opx, quad, bl);
    } else {
      f32x4 bl[MR];
      bias_tile(bl);
      epilogue<MR, NR>(a, acc, cout0, pv, pb, py, px, quad, bl);
    }
  };
  if constexpr (RESW)
    for (int c = 0; c < nch; ++c) dma_weights(c, smem + c * W_BYTES);
  prep_tile(ti);
  stage(0, 0);
  __syncthreads();
  RV_PH(0);
  for (int s = 0; s < nsteps; ++s) {
    EpiPend<MR, NR> ep;
    if (grp == 0) {
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < NR; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // issue step s+1
    const bool last = grp + 1 == ngrp;
    if (s + 1 < nsteps) {
      if (last) prep_tile(ti + walk.step);
      stage(last ? 0 : grp + 1, (s + 1) & 1);
    }
    RV_PH(1);
    compute(grp, s & 1);
    RV_PH(2);
    // a finished tile's packed outputs, stored after the barrier (tiles whose
    // pack registers fit beside the compute registers without spills)
    if (last) {
      finish(ti, ep);
      ti += walk.step;
      grp = 0;
      RV_PH(3);
    } else {
      ++grp;
    }
    __syncthreads();
    if constexpr (kDefer) {
      if (last && g.fast) epi_store<MR, NR>(a, ep);  // the finished tile's stores (epi_pack)
    }
    RV_PH(4);
  }
#ifdef RV_PHASE_PROF
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) atomicAdd(&g_conv_phase[i], ph[i]);
    atomicAdd(&g_conv_phase[5], (unsigned long long)nsteps);
    atomicAdd(&g_conv_phase[6], 1ull);
  }
#endif
#undef RV_PH
}

// Input-channel chunks (32 channels) of the larger group.
int conv_nch(const ConvArgs& a) {
  int cin = a.Cin;
  if (a.g2_cout0 > 0 && a.g2_Cin > cin) cin = a.g2_Cin;
  const int cc = a.in8 ? 64 : 32;  // channels per chunk (64 B per pixel either way)
  return (cin + cc - 1) / cc;
}

bool patch_geo(const ConvArgs& a, const ConvCfg& c, PatchGeo& g, size_t& smem) {
  if (!((a.k == 1 || a.k == 3) && (a.stride == 1 || a.stride == 2) && a.pad == a.k / 2)) return false;
  // the kernel's patch offsets use 24-bit multiplies (prep_tile)
  if ((size_t)a.Hin * a.Win >= (1u << 24) || (size_t)a.in_cs * 2 >= (1u << 24)) return false;
  const int NR = c.nr, MR = c.mr;
  const int NW = c.kind == 2 ? 8 : 4;  // waves per workgroup
  const int P = 16 * NR * NW;
  // tile width: the fewest halo-patch pixels DMA'd over the whole layer
  // (tiles x PH x PW, edge tiles included); at least 16 columns, so a B
  // fragment's 16 pixels mostly share one patch row (conflict-free reads)
  // (the search runs up to ~300 candidates with four divisions each; a plan
  // asks for the same few shapes on every forward, so the answers are kept:
  // host time per launch matters at batch 1, where the kernels are ~5 us)
  struct TileKey {
    int wo, ho, s, k, p, c;
  };
  static thread_local TileKey memo[64];
  static thread_local int memo_n = 0, memo_w = 0;
  int C = 0;
  for (int i = 0; i < memo_n && !C; ++i)
    if (memo[i].wo == a.Wo && memo[i].ho == a.Ho && memo[i].s == a.stride && memo[i].k == a.k &&
        memo[i].p == P)
      C = memo[i].c;
  if (!C) {
    long best = -1;
    for (int c = std::min(a.Wo, P); c >= std::min(16, a.Wo); --c) {
      const int r = P / c;
      const long cost = (long)ceil_div(a.Wo, c) * ceil_div(a.Ho, r) * ((r - 1) * a.stride + a.k) *
                        ((c - 1) * a.stride + a.k);
      if (best < 0 || cost < best) {
        best = cost;
        C = c;
      }
    }
    memo[memo_w++ & 63] = TileKey{a.Wo, a.Ho, a.stride, a.k, P, C};
    memo_n = std::min(memo_n + 1, 64);
  }
  g.C = C;
  g.R = P / C;
  if (g.R < 1) return false;
  g.PH = (g.R - 1) * a.stride + a.k;
  g.PW = (g.C - 1) * a.stride + a.k;
  g.pinst = ceil_div(g.PH * g.PW * 4, 64);  // 4 16-B slots per pixel (patch_pixb)
  g.p_bytes = g.pinst * 1024;
  g.tiles_x = ceil_div(a.Wo, g.C);
  g.tiles_y = ceil_div(a.Ho, g.R);
  const int nch = conv_nch(a);
  g.G = std::max(1, std::min(c.G, nch));
  g.fast = epi_fast(a) ? 1 : 0;
  // per-lane offset registers of the kernel (patch_maxit)
  const int maxit = (a.stride == 2 ? 6 : 2) * NR + 2;
  if (ceil_div(g.pinst, NW) > maxit) return false;
  const size_t wb = (size_t)16 * MR * a.k * a.k * 64;
  // two stages: the next (tile, chunk group) streams in during the current one
  smem = (c.resw ? nch * wb : 0) + 2 * (size_t)g.G * (g.p_bytes + (c.resw ? 0 : wb)) +
         (a.in8 ? 0 : (size_t)16 * MR * 4);  // bf16: the block's bias
  if (a.ch_w) {  // chained 1x1: its weights and bias, one x tile per wave
    const size_t chn = (MR + 1) / 2;
    smem += chn * 16 * MR * 64 + (size_t)16 * MR * 4 + (size_t)NW * chn * NR * 16 * 64;
  }
  return smem <= 160 * 1024;
}

template <int MR, int NR, int K, int S, bool RESW, bool F8, int NW, bool CH>
static int launch_patch_t(const ConvArgs& a, const PatchGeo& g, size_t smem, int persist,
                          hipStream_t s) {
  static ConvLaunchState st;
  auto fn = conv_patch_kernel<MR, NR, K, S, RESW, F8, NW, CH>;
  const int ytiles = ceil_div((a.Cout + 15) / 16, MR);
  const int ntiles = a.B * g.tiles_x * g.tiles_y;
  const int gx = conv_grid_x(st, (const void*)fn, 64 * NW, smem, ytiles, ntiles, persist);
  if (gx < 0) return gx;
  dim3 grid(gx, ytiles);
  fn<<<grid, 64 * NW, smem, s>>>(a, g);
  return launch_status("conv_patch");
}

// The instantiating switch: every (K, S, RESW) of a (tile, NW, F8, CH) form
// that patch_built names, and nothing else.
template <int MR, int NR, int NW, bool F8, bool CH>
static int launch_patch_ks(const ConvArgs& a, const ConvCfg& c, const PatchGeo& g, size_t smem,
                           hipStream_t s) {
#define RV_KS(K_, S_, R_)                                          \
  if constexpr (patch_built(NW, F8, CH, MR, NR, K_, S_, R_))       \
    if (a.k == K_ && a.stride == S_ && (c.resw != 0) == R_)        \
      return launch_patch_t<MR, NR, K_, S_, R_, F8, NW, CH>(a, g, smem, c.persist, s);
  RV_KS(3, 1, true) RV_KS(1, 1, true) RV_KS(3, 2, true)
  RV_KS(3, 1, false) RV_KS(1, 1, false) RV_KS(3, 2, false)
#undef RV_KS
  set_error("conv_patch (%d waves, fp8 %d, chained %d): no variant MR=%d NR=%d k=%d s=%d resw=%d", NW,
            F8, CH, MR, NR, a.k, a.stride, c.resw);
  return RV_EINVAL;
}

int launch_conv_patch(const ConvArgs& a, const ConvCfg& c, const PatchGeo& g, size_t smem, hipStream_t s) {
#define RV_PATCH(M_, N_)                                                                \
  if (c.mr == M_ && c.nr == N_)                                                         \
    return c.kind == 2 ? (a.ch_w ? launch_patch_ks<M_, N_, 8, false, true>(a, c, g, smem, s)   \
                                 : launch_patch_ks<M_, N_, 8, false, false>(a, c, g, smem, s)) \
           : a.ch_w    ? launch_patch_ks<M_, N_, 4, false, true>(a, c, g, smem, s)    \
           : a.in8     ? launch_patch_ks<M_, N_, 4, true, false>(a, c, g, smem, s)    \
                       : launch_patch_ks<M_, N_, 4, false, false>(a, c, g, smem, s);
  RV_TILES(RV_PATCH)
#undef RV_PATCH
  set_error("no conv_patch tile MR=%d NR=%d", c.mr, c.nr);
  return RV_EINVAL;
}

}  // namespace rv

#ifdef RV_PHASE_PROF
// Timing build only (not in include/rvhip.h): read (and with reset != 0
// clear) the conv_patch_kernel phase sums, 8 x u64.
extern "C" int rv_conv_phase_read(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rv::g_conv_phase), 8 * sizeof(unsigned long long)) != hipSuccess)
    return -1;
  if (reset) {
    static const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(rv::g_conv_phase), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
