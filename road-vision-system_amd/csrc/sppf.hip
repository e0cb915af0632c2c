// SPPF pooling kernel for gfx950 (launch_sppf_pool / launch_sppf_pool_fp8 of
// conv.h).
#include "conv.h"
#include "conv_common.h"

namespace rv {

// ---------------------------------------------------------------------------
// SPPF: three chained MaxPool2d(5, 1, 2) == clipped 5/9/13 windows.
// One thread per (pixel, 8-channel group).
// ---------------------------------------------------------------------------
// One workgroup per (image, 8-channel group).  The clipped k x k max is
// separable (the clipped window is a rectangle), so a horizontal pass writes
// the row maxima for k = 5/9/13 to LDS and a vertical pass finishes them;
// one thread per pixel, 8 channels (one 16-B vector) each.  bf16 max is
// exact, so values stay bf16 throughout.
constexpr int kSppfLds = 160 * 1024;

__device__ __forceinline__ void bf8_to_f(const uint4 v, float (&f)[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(w[j] << 16);
    f[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
  }
}
__device__ __forceinline__ uint4 f_to_bf8(const float (&f)[8]) {
  // inputs are bf16 values: truncation is exact
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    w[j] = (__float_as_uint(f[2 * j]) >> 16) | (__float_as_uint(f[2 * j + 1]) & 0xFFFF0000u);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// 16-B vector <-> its lanes as f32: 8 bf16 values, or 16 fp8 codes (one
// buffer scale, so the max over codes' values re-encodes exactly).
template <bool F8>
struct SppfVec {
  static constexpr int N = F8 ? 16 : 8;
  __device__ static void dec(const uint4 v, float (&f)[N]) {
    if constexpr (F8) {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f[4 * j] = __builtin_amdgcn_cvt_f32_fp8((int)w[j], 0);
        f[4 * j + 1] = __builtin_amdgcn_cvt_f32_fp8((int)w[j], 1);
        f[4 * j + 2] = __builtin_amdgcn_cvt_f32_fp8((int)w[j], 2);
        f[4 * j + 3] = __builtin_amdgcn_cvt_f32_fp8((int)w[j], 3);
      }
    } else {
      bf8_to_f(v, f);
    }
  }
  __device__ static uint4 enc(const float (&f)[N]) {
    if constexpr (F8) {
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float q[4] = {f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]};
        w[j] = f8_encode4(q, 1.f);
      }
      return make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      return f_to_bf8(f);
    }
  }
};

template <bool F8>
__global__ __launch_bounds__(256) void sppf_pool_kernel(uint8_t* __restrict__ buf, int B, int H,
                                                        int W, int c) {
  using V = SppfVec<F8>;
  constexpr int NV = V::N, EB = F8 ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) uint4 sp[];  // x, h5, h9, h13: [H*W] uint4 each
  const int groups = c / NV;
  const int b = blockIdx.x / groups, g = blockIdx.x - (blockIdx.x / groups) * groups;
  const int cs = 4 * c * EB;  // pixel stride, bytes
  const int HW = H * W;
  uint4* xs = sp;
  uint4* h5 = sp + HW;
  uint4* h9 = sp + 2 * HW;
  uint4* h13 = sp + 3 * HW;
  uint8_t* img = buf + (size_t)b * HW * cs + g * 16;
  for (int p = threadIdx.x; p < HW; p += 256) xs[p] = *(const uint4*)(img + (size_t)p * cs);
  __syncthreads();
  for (int p = threadIdx.x; p < HW; p += 256) {
    const int y = p / W, x = p - (p / W) * W;
    float a5[NV], a9[NV], a13[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) a5[j] = a9[j] = a13[j] = -INFINITY;
    // the taps' LDS reads issued in two groups (7 + 6) ahead of their max
    // chains (a branch around each read made every one a separate LDS round
    // trip; all 13 at once doubled the VGPRs, which cost more beside the
    // forward's other kernels than the round trips saved); out-of-map taps
    // read the edge pixel instead, which the window always holds, so the
    // max (the -inf padding of MaxPool2d) is unchanged
#pragma unroll
    for (int d0 = -6; d0 <= 6; d0 += 7) {
      uint4 raw[7];
#pragma unroll
      for (int d = d0; d < d0 + 7 && d <= 6; ++d) raw[d - d0] = xs[y * W + min(max(x + d, 0), W - 1)];
#pragma unroll
      for (int d = d0; d < d0 + 7 && d <= 6; ++d) {
        float f[NV];
        V::dec(raw[d - d0], f);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          a13[j] = fmaxf(a13[j], f[j]);
          if (d >= -4 && d <= 4) a9[j] = fmaxf(a9[j], f[j]);
          if (d >= -2 && d <= 2) a5[j] = fmaxf(a5[j], f[j]);
        }
      }
    }
    h5[p] = V::enc(a5);
    h9[p] = V::enc(a9);
    h13[p] = V::enc(a13);
  }
  __syncthreads();
  for (int p = threadIdx.x; p < HW; p += 256) {
    const int y = p / W, x = p - (p / W) * W;
    float a5[NV], a9[NV], a13[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) a5[j] = a9[j] = a13[j] = -INFINITY;
    // column pass, the same way: each map's taps read first, edge rows
    // standing in for the out-of-map ones
    auto col_max = [&](const uint4* hm, int r, float (&acc)[NV]) {
#pragma unroll
      for (int d0 = -r; d0 <= r; d0 += 7) {
        uint4 rv[7];
#pragma unroll
        for (int d = d0; d < d0 + 7 && d <= r; ++d) rv[d - d0] = hm[min(max(y + d, 0), H - 1) * W + x];
#pragma unroll
        for (int d = d0; d < d0 + 7 && d <= r; ++d) {
          float f[NV];
          V::dec(rv[d - d0], f);
#pragma unroll
          for (int j = 0; j < NV; ++j) acc[j] = fmaxf(acc[j], f[j]);
        }
      }
    };
    col_max(h13, 6, a13);
    col_max(h9, 4, a9);
    col_max(h5, 2, a5);
    uint8_t* o = img + (size_t)p * cs;
    *(uint4*)(o + c * EB) = V::enc(a5);
    *(uint4*)(o + 2 * c * EB) = V::enc(a9);
    *(uint4*)(o + 3 * c * EB) = V::enc(a13);
  }
}

template <bool F8>
static int launch_sppf_t(uint8_t* buf, int B, int H, int W, int c, hipStream_t s) {
  const size_t smem = (size_t)H * W * 64;  // 4 x 16 B per pixel
  const int nv = F8 ? 16 : 8;
  if (c % nv != 0 || smem > kSppfLds) {
    set_error("sppf: c=%d / map %dx%d unsupported by the LDS pool", c, H, W);
    return RV_EINVAL;
  }
  static bool attr = false;
  if (!attr && smem > 64 * 1024) {  // only raise the cap when a map needs it
    // best effort: a failure surfaces as the launch error reported below
    (void)hipFuncSetAttribute((const void*)sppf_pool_kernel<F8>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, kSppfLds);
    (void)hipGetLastError();
    attr = true;
  }
  sppf_pool_kernel<F8><<<B * (c / nv), 256, smem, s>>>(buf, B, H, W, c);
  return launch_status("sppf_pool");
}

int launch_sppf_pool(bf16_t* buf, int B, int H, int W, int c, hipStream_t s) {
  return launch_sppf_t<false>((uint8_t*)buf, B, H, W, c, s);
}

int launch_sppf_pool_fp8(uint8_t* buf, int B, int H, int W, int c, hipStream_t s) {
  return launch_sppf_t<true>(buf, B, H, W, c, s);
}

}  // namespace rv
