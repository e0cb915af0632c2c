// Depthwise 3x3 conv (stride 1, zero pad 1) on NHWC bf16 maps: YOLO11's
// Detect class branch (DWConv 3x3 + SiLU) and the positional conv `pe` of its
// PSA attention (no activation, `o` as the residual).  torch Conv2d with
// groups = C: out[y][x][c] = bias[c] + sum_{ky,kx} w[c][ky][kx] in[y+ky-1][x+kx-1][c].
//
// A bandwidth kernel.  One thread owns 8 channels (one 16-byte vector) of one
// output column and walks down a strip of kRows output rows: input row r is
// loaded once per strip (the pixel and its two x neighbours, whose vectors
// lie in the cache lines the neighbouring threads fetch) and added into the
// three output rows it feeds (r + 1 with tap row 0, r with 1, r - 1 with 2),
// whose f32 sums roll through registers.  Every output element therefore sums
// its taps in the order bias, ky 0, 1, 2 (kx 0, 1, 2 inside), whatever the
// strip.  Consecutive threads own consecutive channel groups, so loads and
// stores of a wave are contiguous runs of the pixel's channels.
#include "conv.h"
#include "conv_common.h"

namespace rv {

struct DwArgs {
  const bf16_t* in;
  int in_cs, in_co, in_gw, in_gs;  // group form: channel c at in_co + (c / gw) gs + c % gw
  const bf16_t* w;                 // [9][C] bf16, tap ky * 3 + kx
  const float* bias;               // [C]
  int B, H, W, C, act;
  const bf16_t* res;
  int res_cs, res_co;
  bf16_t* out;
  int out_cs, out_co;
};

constexpr int kDwRows = 8;       // output rows per strip
constexpr int kDwThreads = 256;

__device__ __forceinline__ void dw_unpack(const v4u32 v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(v[i] << 16);
    f[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u);
  }
}

__global__ __launch_bounds__(kDwThreads) void dwconv3x3_kernel(const DwArgs a) {
  const int CG = a.C >> 3;
  const int t = blockIdx.x * kDwThreads + threadIdx.x;  // (x, channel group) of this thread
  if (t >= a.W * CG) return;
  const int x = t / CG, c0 = (t - x * CG) << 3;
  const int b = blockIdx.z, y0 = blockIdx.y * kDwRows;
  const int y1 = min(y0 + kDwRows, a.H);  // output rows [y0, y1)
  const int cin = a.in_co + (c0 / a.in_gw) * a.in_gs + c0 % a.in_gw;

  v4u32 wv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wv[k] = *(const v4u32*)(a.w + (size_t)k * a.C + c0);
  float bias[8];
  {
    const f32x4 b0 = *(const f32x4*)(a.bias + c0), b1 = *(const f32x4*)(a.bias + c0 + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) bias[i] = b0[i], bias[4 + i] = b1[i];
  }

  // acc[0]: output row r - 1 (taps ky 0, 1 in), acc[1]: row r (ky 0 in),
  // acc[2]: row r + 1 (bias only) before input row r is added
  float acc[3][8];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = bias[i];

  const size_t img = (size_t)b * a.H * a.W;
  for (int r = y0 - 1; r <= y1; ++r) {
    if (r >= 0 && r < a.H) {
      const bf16_t* row = a.in + (img + (size_t)r * a.W) * a.in_cs + cin;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = x + kx - 1;
        if (xx < 0 || xx >= a.W) continue;
        float v[8], w[8];
        dw_unpack(*(const v4u32*)(row + (size_t)xx * a.in_cs), v);
        // input row r is tap row ky of output row r + 1 - ky: acc[2 - ky]
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          dw_unpack(wv[ky * 3 + kx], w);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[2 - ky][i] += v[i] * w[i];
        }
      }
    }
    // output row r - 1 is complete
    const int yo = r - 1;
    if (yo >= y0 && yo < y1) {
      float o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = acc[0][i];
      if (a.act) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = silu(o[i]);
      }
      const size_t px = img + (size_t)yo * a.W + x;
      if (a.res) {
        float rv[8];
        dw_unpack(*(const v4u32*)(a.res + px * a.res_cs + a.res_co + c0), rv);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] += rv[i];
      }
      v4u32 pk;
#pragma unroll
      for (int i = 0; i < 4; ++i) pk[i] = pack_bf16x2(o[2 * i], o[2 * i + 1]);
      *(v4u32*)(a.out + px * a.out_cs + a.out_co + c0) = pk;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc[0][i] = acc[1][i];
      acc[1][i] = acc[2][i];
      acc[2][i] = bias[i];
    }
  }
}

int launch_dwconv3x3(const bf16_t* in, int in_cs, int in_co, int in_gw, int in_gs, const bf16_t* w,
                     const float* bias, int B, int H, int W, int C, int act, const bf16_t* res,
                     int res_cs, int res_co, bf16_t* out, int out_cs, int out_co, hipStream_t s) {
  DwArgs a{in,  in_cs, in_co, in_gw > 0 ? in_gw : C, in_gw > 0 ? in_gs : 0, w,   bias,   B,     H,
           W,   C,     act,   res,                   res_cs,                res_co, out, out_cs, out_co};
  const dim3 grid(ceil_div(W * (C / 8), kDwThreads), ceil_div(H, kDwRows), B);
  hipLaunchKernelGGL(dwconv3x3_kernel, grid, dim3(kDwThreads), 0, s, a);
  return launch_status("dwconv3x3");
}

}  // namespace rv

extern "C" int rv_dwconv3x3_bf16(const void* in, int B, int H, int W, int C, int in_cs, int in_co,
                                 int in_gw, int in_gs, const void* w, const float* bias, void* out,
                                 int out_cs, int out_co, const void* res, int res_cs, int res_co,
                                 int act, void* stream) {
  using namespace rv;
  RV_CHECK_ARG(in && w && bias && out, "null pointer");
  RV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0,
               "bad shape B=%d %dx%d C=%d (C a positive multiple of 8)", B, H, W, C);
  RV_CHECK_ARG(B <= 65535 && (H + kDwRows - 1) / kDwRows <= 65535, "B=%d / H=%d exceed the grid", B, H);
  RV_CHECK_ARG(in_co >= 0 && out_co >= 0 && (!res || res_co >= 0), "negative channel offset");
  if (in_gw > 0) {
    RV_CHECK_ARG(in_gw % 8 == 0 && C % in_gw == 0 && in_gs >= in_gw && in_gs % 8 == 0,
                 "input groups: width %d must be a multiple of 8 dividing C=%d, stride %d a multiple "
                 "of 8 no smaller", in_gw, C, in_gs);
    RV_CHECK_ARG((long long)in_co + (long long)(C / in_gw - 1) * in_gs + in_gw <= in_cs,
                 "input groups (%d of width %d every %d from %d) exceed the channel stride %d",
                 C / in_gw, in_gw, in_gs, in_co, in_cs);
  } else {
    RV_CHECK_ARG(in_gw == 0 && in_gs == 0, "input groups: width %d, stride %d", in_gw, in_gs);
    RV_CHECK_ARG((long long)in_co + C <= in_cs, "input channels [%d, %d) exceed the channel stride %d",
                 in_co, in_co + C, in_cs);
  }
  RV_CHECK_ARG((long long)out_co + C <= out_cs && (!res || (long long)res_co + C <= res_cs),
               "output / residual channels exceed their channel stride");
  // 16-byte loads and stores of 8 channels
  RV_CHECK_ARG(in_cs % 8 == 0 && in_co % 8 == 0 && (uintptr_t)in % 16 == 0,
               "input: in_cs %d and in_co %d must be multiples of 8, in 16-byte aligned", in_cs, in_co);
  RV_CHECK_ARG(out_cs % 8 == 0 && out_co % 8 == 0 && (uintptr_t)out % 16 == 0,
               "output: out_cs %d and out_co %d must be multiples of 8, out 16-byte aligned", out_cs,
               out_co);
  RV_CHECK_ARG(!res || (res_cs % 8 == 0 && res_co % 8 == 0 && (uintptr_t)res % 16 == 0),
               "residual: res_cs %d and res_co %d must be multiples of 8, res 16-byte aligned", res_cs,
               res_co);
  RV_CHECK_ARG((uintptr_t)w % 16 == 0 && (uintptr_t)bias % 16 == 0,
               "w and bias must be 16-byte aligned");
  RV_CHECK_ARG((double)W * (C / 8) < 2147483648.0, "row of %d pixels x %d channels too wide", W, C);
  return launch_dwconv3x3((const bf16_t*)in, in_cs, in_co, in_gw, in_gs, (const bf16_t*)w, bias, B, H,
                          W, C, act ? 1 : 0, (const bf16_t*)res, res_cs, res_co, (bf16_t*)out, out_cs,
                          out_co, (hipStream_t)stream);
}
