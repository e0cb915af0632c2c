// The generic conv kernel and its launcher (conv.hip: the kernels' order).
#include "conv_kernels.h"

namespace rv {

// conv_mfma_kernel, the generic fallback: an implicit GEMM
// D[cout][pixel] = W[cout][k] * X[k][pixel] on v_mfma_f32_16x16x32_bf16 with
// no LDS.  The accumulator layout puts 4 consecutive output channels of one
// pixel in each lane, so the epilogue (bias, SiLU, residual add, bf16 pack)
// stores 8 contiguous bytes per lane into each destination view (concat
// slice and/or nearest-2x upsampled copy).
// Wave tile: MR x NR fragments of 16x16 (16*MR output channels x 16*NR
// pixels).  A workgroup is 4 waves arranged WP (pixel groups) x WC (channel
// groups); every wave streams its own A (weights, L1/L2-resident, shared by
// the WP waves of a channel group) and B (input pixels: 16 B per lane, lane l
// reads 8 channels of pixel l&15) fragments straight from HBM/L2
// into VGPRs, double-buffered one k-step ahead, so there is no LDS and no
// barrier in the K loop: the loads of k-step s+1 are in flight while the
// MFMAs of k-step s issue.
template <int MR, int NR, int WC>
__global__ __launch_bounds__(256, 2) void conv_mfma_kernel(ConvArgs a) {
  constexpr int WP = 4 / WC;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, quad = lane >> 4;
  const int wp = wave % WP, wc = wave / WP;
  const int cout_pad = (a.Cout + 15) & ~15;
  const int cout0 = (blockIdx.y * WC + wc) * (16 * MR);
  const int HWo = a.Ho * a.Wo;
  const int M = a.B * HWo;
  const int pix0 = (blockIdx.x * WP + wp) * (16 * NR);
  if (cout0 >= cout_pad || pix0 >= M) return;  // whole-wave early exit (no barriers below)

  const int cin_pad = (a.Cin + 31) & ~31;
  const int kspt = cin_pad >> 5;  // k-steps per tap
  const int Kp = a.k * a.k * cin_pad;
  const int nks = a.k * kspt;     // k-steps per kernel row
  const int total = a.k * nks;

  const bf16_t* wrow[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    int r = cout0 + m * 16 + col;
    r = r < cout_pad ? r : cout_pad - 1;
    wrow[m] = a.w + (size_t)r * Kp + quad * 8;
  }
  int iy0[NR], ix0[NR], pb[NR];
  bool pv[NR];
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    const int p = pix0 + n * 16 + col;
    pv[n] = p < M;
    const int pp = pv[n] ? p : 0;
    const int b = pp / HWo;
    const int r = pp - b * HWo;
    const int oy = r / a.Wo;
    const int ox = r - oy * a.Wo;
    iy0[n] = oy * a.stride - a.pad;
    ix0[n] = ox * a.stride - a.pad;
    pb[n] = b * a.Hin * a.Win * a.in_cs + a.in_co + quad * 8;
  }

  f32x4 acc[MR][NR];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  // k-step s <-> (ky, kx, cs); weights column = s*32
  auto load = [&](int s, bf16x8 (&A)[MR], bf16x8 (&Bf)[NR]) {
    const int ky = s / nks;
    const int r = s - ky * nks;
    const int kx = r / kspt;
    const int cs = r - kx * kspt;
    const int kcol = s * 32;
#pragma unroll
    for (int m = 0; m < MR; ++m) A[m] = __builtin_bit_cast(bf16x8, *(const uint4*)(wrow[m] + kcol));
    const bool cvalid = cs * 32 + quad * 8 < a.Cin;
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const int iy = iy0[n] + ky, ix = ix0[n] + kx;
      const bool ok = pv[n] && cvalid && (unsigned)iy < (unsigned)a.Hin &&
                      (unsigned)ix < (unsigned)a.Win;
      uint4 v = zero4;
      if (ok)
        v = *(const uint4*)(a.in + (size_t)pb[n] + ((size_t)iy * a.Win + ix) * a.in_cs + cs * 32);
      Bf[n] = __builtin_bit_cast(bf16x8, v);
    }
  };
  auto mma = [&](const bf16x8 (&A)[MR], const bf16x8 (&Bf)[NR]) {
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int n = 0; n < NR; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[m], Bf[n], acc[m][n], 0, 0, 0);
  };
  bf16x8 A0[MR], B0[NR], A1[MR], B1[NR];
  load(0, A0, B0);
  for (int s = 0; s < total; s += 2) {
    if (s + 1 < total) load(s + 1, A1, B1);
    mma(A0, B0);
    if (s + 1 >= total) break;
    if (s + 2 < total) load(s + 2, A0, B0);
    mma(A1, B1);
  }

  // epilogue: lane holds couts cout0 + m*16 + quad*4 + i of pixel pix0 + n*16 + col
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    if (!pv[n]) continue;
    const int p = pix0 + n * 16 + col;
    const int b = p / HWo;
    const int r = p - b * HWo;
    const int oy = r / a.Wo;
    const int ox = r - oy * a.Wo;
    const size_t opix = (size_t)p;  // == (b*Ho + oy)*Wo + ox
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int co = cout0 + m * 16 + quad * 4;
      if (co >= a.Cout) continue;
      float v[4];
      const float4 bb = *(const float4*)(a.bias + co);
      v[0] = acc[m][n][0] + bb.x;
      v[1] = acc[m][n][1] + bb.y;
      v[2] = acc[m][n][2] + bb.z;
      v[3] = acc[m][n][3] + bb.w;
      if (a.act) {
        silu4(v);
      }
      if (a.res) {
        const uint2 rr = *(const uint2*)(a.res + opix * a.res_cs + a.res_co + co);
        v[0] += bf2f(rr.x & 0xFFFF);
        v[1] += bf2f(rr.x >> 16);
        v[2] += bf2f(rr.y & 0xFFFF);
        v[3] += bf2f(rr.y >> 16);
      }
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        void* outp = d == 0 ? a.out0 : a.out1;
        if (!outp) continue;
        const int cs_ = d == 0 ? a.out0_cs : a.out1_cs;
        const int co_ = (d == 0 ? a.out0_co : a.out1_co) + co;
        const int up = d == 0 ? a.out0_up : a.out1_up;
        if (a.out_f32) {
          float* o = (float*)outp;
          const float4 pk = make_float4(v[0], v[1], v[2], v[3]);
          if (!up) {
            *(float4*)(o + opix * cs_ + co_) = pk;
          } else {
            for (int dy = 0; dy < 2; ++dy)
              for (int dx = 0; dx < 2; ++dx) {
                const size_t q = ((size_t)(b * 2 * a.Ho + 2 * oy + dy) * (2 * a.Wo) + 2 * ox + dx);
                *(float4*)(o + q * cs_ + co_) = pk;
              }
          }
        } else {
          uint16_t* o = (uint16_t*)outp;
          const uint2 pk = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
          if (!up) {
            *(uint2*)(o + opix * cs_ + co_) = pk;
          } else {
            for (int dy = 0; dy < 2; ++dy)
              for (int dx = 0; dx < 2; ++dx) {
                const size_t q = ((size_t)(b * 2 * a.Ho + 2 * oy + dy) * (2 * a.Wo) + 2 * ox + dx);
                *(uint2*)(o + q * cs_ + co_) = pk;
              }
          }
        }
      }
    }
  }
}

template <int MR, int NR, int WC>
static void launch_t(const ConvArgs& a, hipStream_t s) {
  constexpr int WP = 4 / WC;
  const int M = a.B * a.Ho * a.Wo;
  const int T = (a.Cout + 15) / 16;
  dim3 grid(ceil_div(M, 16 * NR * WP), ceil_div(T, MR * WC));
  conv_mfma_kernel<MR, NR, WC><<<grid, 256, 0, s>>>(a);
}

// Tile choice: the largest wave tile (MR*NR fragments, i.e. MFMAs per
// k-step) that leaves >= ~2048 busy waves (8 per CU), with no more than one
// padded 16-channel tile; the 4 waves of a workgroup split channels first
// (WC) when the layer has few pixels.
int launch_conv_generic(const ConvArgs& a, hipStream_t s) {
  const int T = (a.Cout + 15) / 16;
  const long M = (long)a.B * a.Ho * a.Wo;
  struct Cand {
    int mr, nr;
  };
  static const Cand cands[] = {{4, 4}, {2, 8}, {4, 2}, {2, 4}, {1, 8}, {4, 1}, {2, 2},
                               {1, 4}, {2, 1}, {1, 2}, {1, 1}};
  int MR = 1, NR = 1;
  for (const Cand& c : cands) {
    if (c.mr > T) continue;
    const int waste = ceil_div(T, c.mr) * c.mr - T;
    if (waste > 1 && c.mr > 1) continue;
    const long waves = (long)ceil_div((int)((M + 16 * c.nr - 1) / (16 * c.nr)), 1) * ceil_div(T, c.mr);
    MR = c.mr;
    NR = c.nr;
    if (waves >= 2048) break;
  }
  const int groups_c = ceil_div(T, MR);
  const int WC = groups_c >= 4 ? 4 : (groups_c >= 2 ? 2 : 1);
#define RV_CONV_WC(mr, nr)                                           \
  if (MR == mr && NR == nr) {                                        \
    if (WC == 4) launch_t<mr, nr, 4>(a, s);                          \
    else if (WC == 2) launch_t<mr, nr, 2>(a, s);                     \
    else launch_t<mr, nr, 1>(a, s);                                  \
    return launch_status("conv_mfma");                               \
  }
  RV_CONV_WC(4, 4) RV_CONV_WC(2, 8) RV_CONV_WC(4, 2) RV_CONV_WC(2, 4) RV_CONV_WC(1, 8)
  RV_CONV_WC(4, 1) RV_CONV_WC(2, 2) RV_CONV_WC(1, 4) RV_CONV_WC(2, 1) RV_CONV_WC(1, 2)
  RV_CONV_WC(1, 1)
#undef RV_CONV_WC
  set_error("no conv variant for MR=%d NR=%d", MR, NR);
  return RV_EINVAL;
}

}  // namespace rv
