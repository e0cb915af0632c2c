// The direct 1x1 conv kernel and its launcher (conv.hip: the kernels' order).
#include "conv_kernels.h"

namespace rv {

// the zero block invalid pixels / channels load from
__device__ __attribute__((aligned(64))) uint4 g_zero16[4];

// ---------------------------------------------------------------------------
// conv1x1_direct_kernel: 1x1 stride-1 convs without LDS staging of the
// pixels.  A 1x1 conv has no halo, so an input pixel feeds exactly one B
// fragment column: each lane loads its 16-B fragment slice straight from
// HBM/L2 into VGPRs (global_load_dwordx4), and chunk c+1's loads are in
// flight while chunk c runs on MFMA -- no LDS round trip and no barrier in
// the K loop.  The block's weights (16*MR couts x Cin) are DMA'd into LDS
// once (same per-chunk layout and quarter swizzle as the patch kernel) and
// stay resident while a persistent block walks its pixel tiles (64*NR
// consecutive NHWC pixels of the flattened B x H x W range).  The k order
// (chunks ascending, 32 channels per MFMA) equals the patch kernel's, so the
// two are bit-identical.
// ---------------------------------------------------------------------------
template <int MR, int NR>
__global__ __launch_bounds__(256, 2) void conv1x1_direct_kernel(ConvArgs a, int fast) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int BC = 16 * MR;
  constexpr int W_BYTES = BC * 64;  // one 32-channel chunk of the block's weights
  constexpr int WJ = BC / 16;       // its DMA instructions (16 rows x 64 B each)
  constexpr int MAXW = (WJ + 3) / 4;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, quad = lane >> 4;
  const int cout0 = blockIdx.y * BC;
  const int wcout_pad = (a.Cout + 15) & ~15;
  const int cin_pad = (a.Cin + 31) & ~31;
  const int nch = cin_pad >> 5;
  const int HW = a.Ho * a.Wo;
  const int npix = a.B * HW;
  const int ntiles = (npix + 64 * NR - 1) / (64 * NR);
  for (int c = 0; c < nch; ++c) {
#pragma unroll
    for (int it = 0; it < MAXW; ++it) {
      const int j = wave + 4 * it;
      if (j < WJ) {
        const int row = j * 16 + (lane >> 2);
        const int q = (lane & 3) ^ swzq<false>(row);
        const int co = cout0 + row;
        const void* src = co < wcout_pad ? (const void*)(a.w + (size_t)co * cin_pad + q * 8 + c * 32)
                                         : (const void*)g_zero16;
        __builtin_amdgcn_global_load_lds(src, (void*)(smem + c * W_BYTES + j * 1024), 16, 0, 0);
      }
    }
  }
  __syncthreads();
  f32x4 bias[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    const int co = cout0 + m * 16 + quad * 4;  // bias is padded to Cout_pad16
    bias[m] = co < wcout_pad ? *(const f32x4*)(a.bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // per-lane A fragment offsets within a chunk
  int aoff[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    const int row = m * 16 + col;
    aoff[m] = row * 64 + ((quad ^ swzq<false>(row)) << 4);
  }
  // (b, y, x) of a pixel only where it is used: the upsampled view and the
  // generic epilogue (integer divisions are long VALU sequences)
  const bool need_geo = a.in_up || !fast;
  const TileWalk walk = tile_walk(ntiles);
  // a tile's lane pixels: source pointers of both input views and validity
  struct Geo {
    const bf16_t* src[NR];
    const bf16_t* src2[NR];
    bool pv[NR];
    int pb[NR], py[NR], px[NR];
  };
  auto geo = [&](int t, Geo& G) {
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const int p = t * 64 * NR + wave * 16 * NR + n * 16 + col;
      G.pv[n] = t < walk.end && p < npix;
      const int pp = G.pv[n] ? p : 0;
      G.pb[n] = G.py[n] = G.px[n] = 0;
      if (need_geo) {
        G.pb[n] = pp / HW;
        const int r = pp - G.pb[n] * HW;
        G.py[n] = r / a.Wo;
        G.px[n] = r - G.py[n] * a.Wo;
      }
      // the `in` view's pixel: itself, or (y/2, x/2) of the half-resolution map
      const size_t ps = a.in_up ? ((size_t)G.pb[n] * (a.Ho >> 1) + (G.py[n] >> 1)) * (a.Wo >> 1) +
                                      (G.px[n] >> 1)
                                : (size_t)pp;
      G.src[n] = a.in + ps * a.in_cs + a.in_co + quad * 8;
      // the in2 view, addressed by logical channel (chunks at or above split)
      G.src2[n] = a.in2 + (size_t)pp * a.in2_cs + a.in2_co + quad * 8 - a.split;
    }
  };
  // the B fragments of chunk c of tile G (unconditional loads: invalid
  // pixels / channels read the zero block; a branch around a load would make
  // the compiler drain vmcnt to 0 before the MFMAs, i.e. wait for the
  // prefetched chunks as well)
  auto load = [&](const Geo& G, int c, uint4 (&B)[NR]) {
    const bool kin = c * 32 + quad * 8 < a.Cin;
    const bool second = a.split > 0 && c * 32 >= a.split;
#pragma unroll
    for (int n = 0; n < NR; ++n)
      B[n] = *(const uint4*)((G.pv[n] && kin) ? (const void*)((second ? G.src2[n] : G.src[n]) + c * 32)
                                              : (const void*)g_zero16);
  };
  auto mma = [&](int c, const uint4 (&B)[NR], f32x4 (&acc)[MR][NR]) {
    const uint8_t* Wl = smem + c * W_BYTES;
    bf16x8 A[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) A[m] = __builtin_bit_cast(bf16x8, *(const uint4*)(Wl + aoff[m]));
    // all MR weight reads in flight before the first MFMA (left alone, the
    // scheduler waits for each A fragment right before its MFMAs)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int n = 0; n < NR; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[m], __builtin_bit_cast(bf16x8, B[n]),
                                                            acc[m][n], 0, 0, 0);
  };
  auto finish = [&](int t, const Geo& G, f32x4 (&acc)[MR][NR]) {
    if (fast) {
      uint32_t opx[NR];
#pragma unroll
      for (int n = 0; n < NR; ++n) opx[n] = (uint32_t)(t * 64 * NR + wave * 16 * NR + n * 16 + col);
      epilogue_fast<MR, NR>(a, acc, cout0, G.pv, opx, quad, bias);
    } else {
      epilogue<MR, NR>(a, acc, cout0, G.pv, G.pb, G.py, G.px, quad, bias);
    }
  };
  // A stream of (tile, chunk) positions with two chunk loads always in
  // flight ACROSS tile boundaries: the last chunks' MFMAs and the epilogue of
  // tile t run while tile t + step's first two chunks load (G1), so a
  // persistent block never restarts its pipeline from an empty queue, and no
  // chunk is loaded twice.  A tile spans P = nch rounded up to even positions
  // (an odd count's last position reads the zero block: the k-order and sums
  // are unchanged).
  const int P = (nch + 1) & ~1;
  uint4 B0[NR], B1[NR];
  Geo G0, G1;
  int t = walk.t0;
  geo(t, G0);
  geo(t + walk.step, G1);
  // (the last pair of positions is peeled: no branch around a load, which
  // made the compiler wait for every outstanding load at the join)
  load(G0, 0, B0);
  load(G0, 1, B1);
  for (; t < walk.end; t += walk.step) {
    f32x4 acc[MR][NR];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int n = 0; n < NR; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < P - 2; c += 2) {  // B0: chunk c, B1: chunk c + 1 (< nch here)
      mma(c, B0, acc);
      __builtin_amdgcn_sched_barrier(0);
      load(G0, c + 2, B0);
      __builtin_amdgcn_sched_barrier(0);
      mma(c + 1, B1, acc);
      __builtin_amdgcn_sched_barrier(0);
      load(G0, c + 3, B1);
      __builtin_amdgcn_sched_barrier(0);
    }
    mma(P - 2, B0, acc);
    __builtin_amdgcn_sched_barrier(0);
    load(G1, 0, B0);
    __builtin_amdgcn_sched_barrier(0);
    if (P - 1 < nch) mma(P - 1, B1, acc);  // odd nch: position P - 1 is padding
    __builtin_amdgcn_sched_barrier(0);
    load(G1, 1, B1);
    __builtin_amdgcn_sched_barrier(0);
    finish(t, G0, acc);
    G0 = G1;
    geo(t + 2 * walk.step, G1);
  }
}

// 1x1 direct kernel: LDS = the block's resident weights
static size_t direct_smem(const ConvArgs& a, int MR) {
  return (size_t)((a.Cin + 31) / 32) * 16 * MR * 64;
}

template <int MR, int NR>
static int launch_direct_t(const ConvArgs& a, int persist, hipStream_t s) {
  static ConvLaunchState st;
  auto fn = conv1x1_direct_kernel<MR, NR>;
  const size_t smem = direct_smem(a, MR);
  const int ytiles = ceil_div((a.Cout + 15) / 16, MR);
  const int ntiles = ceil_div(a.B * a.Ho * a.Wo, 64 * NR);
  const int gx = conv_grid_x(st, (const void*)fn, 256, smem, ytiles, ntiles, persist);
  if (gx < 0) return gx;
  fn<<<dim3(gx, ytiles), 256, smem, s>>>(a, epi_fast(a) ? 1 : 0);
  return launch_status("conv1x1_direct");
}

bool direct_ok(const ConvArgs& a, const ConvCfg& c) {
  const int T = (a.Cout + 15) / 16;
  const bool vcat_ok = (a.split == 0 && !a.in_up) ||
                       (a.split % 32 == 0 && a.split <= a.Cin && (!a.in_up || (a.Ho % 2 == 0 && a.Wo % 2 == 0)) &&
                        (a.split == a.Cin || (a.in2 && a.in2_cs % 8 == 0 && a.in2_co % 8 == 0)));
  return a.k == 1 && a.stride == 1 && a.pad == 0 && a.g2_cout0 <= 0 && a.Hin == a.Ho &&
         a.Win == a.Wo && (c.mr <= T || c.mr == 1) && a.in_cs % 8 == 0 && a.in_co % 8 == 0 &&
         !a.in8 && vcat_ok && direct_smem(a, c.mr) <= 160 * 1024;
}

int launch_conv_direct(const ConvArgs& a, const ConvCfg& c, hipStream_t s) {
#define RV_DIRECT(M_, N_) \
  if (c.mr == M_ && c.nr == N_) return launch_direct_t<M_, N_>(a, c.persist, s);
  RV_TILES(RV_DIRECT)
#undef RV_DIRECT
  set_error("no conv1x1_direct tile MR=%d NR=%d", c.mr, c.nr);
  return RV_EINVAL;
}

}  // namespace rv
