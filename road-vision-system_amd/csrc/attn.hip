// Multi-head self-attention of YOLO11's PSA block (Ultralytics Attention:
// key_dim 32, head_dim 64) over the N = H * W positions of one image, on
// v_mfma_f32_16x16x32_bf16.
//
// qkv is an NHWC bf16 view: position p of image b at row b * N + p, head h in
// channels [128 h, 128 h + 128) of the view = q (32) | k (32) | v (64).
// Per image and head: S = q^T k * 32^-1/2 (f32, the scale applied to the f32
// scores), P = softmax over the keys, o = P v, written as bf16 to channel
// 64 h + d of the output view.
//
// One wave owns 16 queries of one (image, head) and walks the keys in tiles
// of 32 with online rescaling -- one code path for every N, tail keys masked:
//   S^T tile = K Q^T: two MFMAs (A = 16 keys x 32 key_dim, B = Q^T, K = 32
//     is exactly key_dim), so a lane holds, for ITS query (lane & 15), the
//     scores of keys 4 g + r and 16 + 4 g + r (g = lane >> 4, r = 0..3);
//   row maximum / sum: 8 registers, then the 4 lanes of the query (xor 16, 32);
//   O^T += V^T P^T: four MFMAs (one per 16 output channels) whose B operand
//     is the lane's own 8 probabilities rounded to bf16 -- k slot 8 g + j of the
//     MFMA stands for key kappa(g, j) = 4 g + j (j < 4) or 16 + 4 g + j - 4, a
//     bijection on the tile's 32 keys -- and whose A operand gathers v of
//     those keys.  The accumulators (16 f32) again belong to the lane's query,
//     so the rescale factor needs no lane movement.
// The denominator sums the unrounded f32 probabilities.  Nothing is staged in
// LDS and no wave waits on another; every address is formed from a key /
// query index clamped to [0, N), so nothing outside the view's B * N rows
// and its heads' channels is read.
#include "conv.h"
#include "conv_common.h"

namespace rv {

struct AttnArgs {
  const bf16_t* qkv;
  int B, N, heads, qkv_cs, qkv_co;
  bf16_t* out;
  int out_cs, out_co;
};

constexpr int kAttnWaves = 4;  // waves (query tiles) per workgroup

__global__ __launch_bounds__(64 * kAttnWaves) void psa_attention_kernel(const AttnArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = (blockIdx.x * kAttnWaves + wave) * 16;
  if (q0 >= a.N) return;  // wave-uniform
  const int h = blockIdx.y, b = blockIdx.z;
  const int c = lane & 15, g = lane >> 4;
  const int N = a.N;
  const bf16_t* base = a.qkv + (size_t)b * N * a.qkv_cs + a.qkv_co + 128 * h;
  const int qi = q0 + c;  // this lane's query
  // B operand of K Q^T: Q^T[k = 8 g + j][query c]
  const bf16x8 qf = *(const bf16x8*)(base + (size_t)min(qi, N - 1) * a.qkv_cs + 8 * g);

  const float scale = 0.17677669529663687f;  // 32^-1/2
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < N; k0 += 32) {
    // scores of this lane's query against keys k0 + 16 t + 4 g + r
    float s[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kr = min(k0 + 16 * t + c, N - 1);  // A operand row: key c of the half tile
      const bf16x8 kf = *(const bf16x8*)(base + (size_t)kr * a.qkv_cs + 32 + 8 * g);
      const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        s[4 * t + r] = k0 + 16 * t + 4 * g + r < N ? acc[r] * scale : -INFINITY;
    }
    float tm = s[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) tm = fmaxf(tm, s[i]);
    tm = fmaxf(tm, __shfl_xor(tm, 16));
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    // key k0 is always valid, so tm and m_new are finite for finite scores
    const float m_new = fmaxf(m, tm);
    const float alpha = __expf(m - m_new);  // 0 on the first tile (m = -inf)
    m = m_new;
    float p[8], ps = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      p[i] = __expf(s[i] - m_new);  // masked keys: exp(-inf) = 0
      ps += p[i];
    }
    l = l * alpha + ps;
    bf16x8 pf;
#pragma unroll
    for (int i = 0; i < 8; ++i) pf[i] = (__bf16)p[i];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      // A operand of V^T P^T: V^T[channel 16 d + c][k slot 8 g + j] = v of key kappa(g, j)
      bf16x8 vf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = k0 + (j < 4 ? 4 * g + j : 16 + 4 * g + j - 4);
        const bf16_t raw = base[(size_t)min(key, N - 1) * a.qkv_cs + 64 + 16 * d + c];
        vf[j] = __builtin_bit_cast(__bf16, key < N ? raw : (bf16_t)0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) o[d][r] *= alpha;
      o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[d], 0, 0, 0);
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qi >= N) return;
  const float inv = 1.0f / l;
  bf16_t* orow = a.out + ((size_t)b * N + qi) * a.out_cs + a.out_co + 64 * h;
  // o[d][r]: channel 16 d + 4 g + r of this lane's query
#pragma unroll
  for (int d = 0; d < 4; ++d)
    *(v2u32*)(orow + 16 * d + 4 * g) =
        v2u32{pack_bf16x2(o[d][0] * inv, o[d][1] * inv), pack_bf16x2(o[d][2] * inv, o[d][3] * inv)};
}

int launch_psa_attention(const bf16_t* qkv, int B, int N, int heads, int qkv_cs, int qkv_co,
                         bf16_t* out, int out_cs, int out_co, hipStream_t s) {
  const AttnArgs a{qkv, B, N, heads, qkv_cs, qkv_co, out, out_cs, out_co};
  const dim3 grid(ceil_div(ceil_div(N, 16), kAttnWaves), heads, B);
  hipLaunchKernelGGL(psa_attention_kernel, grid, dim3(64 * kAttnWaves), 0, s, a);
  return launch_status("psa_attention");
}

}  // namespace rv

extern "C" int rv_psa_attention_bf16(const void* qkv, int B, int N, int heads, int qkv_cs, int qkv_co,
                                     void* out, int out_cs, int out_co, void* stream) {
  using namespace rv;
  RV_CHECK_ARG(qkv && out, "null pointer");
  RV_CHECK_ARG(B >= 1 && N >= 1 && heads >= 1, "bad shape B=%d N=%d heads=%d", B, N, heads);
  RV_CHECK_ARG(B <= 65535 && heads <= 65535, "B=%d / heads=%d exceed the grid", B, heads);
  RV_CHECK_ARG(qkv_co >= 0 && out_co >= 0, "negative channel offset");
  RV_CHECK_ARG((long long)qkv_co + 128LL * heads <= qkv_cs,
               "qkv: %d heads of 128 channels from %d exceed the channel stride %d", heads, qkv_co,
               qkv_cs);
  RV_CHECK_ARG((long long)out_co + 64LL * heads <= out_cs,
               "out: %d heads of 64 channels from %d exceed the channel stride %d", heads, out_co,
               out_cs);
  // 16-byte q / k loads of 8 channels, 8-byte output stores of 4
  RV_CHECK_ARG(qkv_cs % 8 == 0 && qkv_co % 8 == 0 && (uintptr_t)qkv % 16 == 0,
               "qkv: qkv_cs %d and qkv_co %d must be multiples of 8, qkv 16-byte aligned", qkv_cs,
               qkv_co);
  RV_CHECK_ARG(out_cs % 4 == 0 && out_co % 4 == 0 && (uintptr_t)out % 8 == 0,
               "out: out_cs %d and out_co %d must be multiples of 4, out 8-byte aligned", out_cs,
               out_co);
  return launch_psa_attention((const bf16_t*)qkv, B, N, heads, qkv_cs, qkv_co, (bf16_t*)out, out_cs,
                              out_co, (hipStream_t)stream);
}
