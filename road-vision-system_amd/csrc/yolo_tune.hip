// Per-layer autotuning of the YOLOv8 conv launches: rv_yolo_autotune and the
// entries that read, install and list kernel configurations.
#include <algorithm>
#include <cstdlib>
#include "yolo_model.h"

namespace rv {

// Bytes of the buffer an output view lives in (the view's base pointer is
// the buffer start): B x (2x upsampled) rows x channel stride x element.
static size_t out_bytes(const ConvArgs& a, int d) {
  const void* p = d == 0 ? a.out0 : a.out1;
  if (!p) return 0;
  const int up = d == 0 ? a.out0_up : a.out1_up;
  const int cs = d == 0 ? a.out0_cs : a.out1_cs;
  const int o8 = d == 0 ? a.out0_8 : a.out1_8;
  return (size_t)a.B * a.Ho * a.Wo * (up ? 4 : 1) * cs * (a.out_f32 ? 4 : (o8 ? 1 : 2));
}

__global__ void count_diff_kernel(const uint32_t* __restrict__ x, const uint32_t* __restrict__ y,
                                  size_t n, unsigned* __restrict__ cnt) {
  unsigned c = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    c += x[i] != y[i];
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(cnt, c);
}

// cfg6 = {MR, NR, G, resw, persist, kind}: a ConvCfg across the C ABI
static void to6(const ConvCfg& c, int* cfg6) {
  const int v[6] = {c.mr, c.nr, c.G, c.resw, c.persist, c.kind};
  std::copy(v, v + 6, cfg6);
}
static ConvCfg from6(const int* cfg6) {
  return ConvCfg{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5]};
}

}  // namespace rv

using namespace rv;

// Time every valid kernel configuration of every conv launch of a forward on
// this input (the activations of one default forward, so every launch sees
// its real operands) and keep the fastest per launch index for later
// forwards of this handle.  Synchronous; not capturable.  verify != 0 also
// compares each configuration's output buffers with the default's (all
// configurations accumulate in the same k order, so they must be bit-equal);
// *n_bad = configurations that differed.
extern "C" int rv_yolo_autotune(void* h, const uint8_t* lb, int B, void* ws, size_t ws_bytes,
                                int reps, int verify, int* n_bad, void* stream) {
  RV_CHECK_ARG(h && lb && ws, "null pointer");
  Model* M = (Model*)h;
  hipStream_t s = as_stream(stream);
  reps = reps < 1 ? 1 : reps;
  M->tuned.clear();
  int st = rv_yolo_forward(h, lb, B, ws, ws_bytes, nullptr, 1.0f, nullptr, 0, nullptr, stream);
  if (st) return st;
  const std::vector<ConvArgs> L = M->launches;
  std::vector<ConvCfg> best(L.size(), ConvCfg{0, 0, 0, 0, 0});
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    set_error("hipEventCreate failed");
    return RV_EINVAL;
  }
  size_t maxb = 0;
  for (const ConvArgs& a : L) maxb = std::max(maxb, std::max(out_bytes(a, 0), out_bytes(a, 1)));
  uint8_t* ref = nullptr;
  unsigned* cnt = nullptr;
  if (verify && (hipMalloc((void**)&ref, 2 * maxb) != hipSuccess ||
                 hipMalloc((void**)&cnt, sizeof(unsigned)) != hipSuccess)) {
    set_error("autotune: hipMalloc of %zu verification bytes failed", 2 * maxb);
    st = RV_EINVAL;
  }
  int bad = 0;
  static const int dbg = getenv("RV_CONV_DEBUG") ? atoi(getenv("RV_CONV_DEBUG")) : 0;
  std::vector<ConvCfg> cands(512);
  for (size_t i = 0; i < L.size() && !st; ++i) {
    const ConvArgs& a = L[i];
    // fused C2f chains have one kernel configuration (and a sparse-head
    // placeholder none: the autotuner's own forward is dense)
    if (a.fused != 0) continue;
    if (verify)
      for (int d = 0; d < 2; ++d)
        if (out_bytes(a, d))
          if (!st)
            st = hip_check(hipMemcpyAsync(ref + d * maxb, d == 0 ? a.out0 : a.out1,
                                          out_bytes(a, d), hipMemcpyDeviceToDevice, s),
                           "autotune reference copy");
    auto time_cfg = [&](const ConvCfg* c) -> float {
      int r = c ? launch_conv_cfg(a, *c, s) : launch_conv(a, s);  // warm-up launch
      if (!r) r = hip_check(hipEventRecord(e0, s), "autotune hipEventRecord");
      for (int k = 0; k < reps && !r; ++k) r = c ? launch_conv_cfg(a, *c, s) : launch_conv(a, s);
      if (!r) r = hip_check(hipEventRecord(e1, s), "autotune hipEventRecord");
      if (r || hipEventSynchronize(e1) != hipSuccess) {
        if (!st) st = r ? r : RV_EINVAL;
        return 1e30f;
      }
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return 1e30f;  // never chosen
      return ms / reps;
    };
    const float t0 = time_cfg(nullptr);
    float tbest = t0;
    const int n = std::min(conv_candidates(a, cands.data(), (int)cands.size()), (int)cands.size());
    for (int j = 0; j < n && !st; ++j) {
      const float t = time_cfg(&cands[j]);
      if (dbg >= 2)
        fprintf(stderr, "[autotune]   launch %2zu cand MR=%d NR=%d G=%d resw=%d persist=%d kind=%d %7.1f us\n",
                i, cands[j].mr, cands[j].nr, cands[j].G, cands[j].resw, cands[j].persist,
                cands[j].kind, t * 1e3);
      if (verify) {
        unsigned diff = 0;
        for (int d = 0; d < 2; ++d) {
          const size_t nb = out_bytes(a, d);
          if (!nb) continue;
          int vs = hip_check(hipMemsetAsync(cnt, 0, sizeof(unsigned), s), "autotune verify");
          count_diff_kernel<<<1024, 256, 0, s>>>((const uint32_t*)(ref + d * maxb),
                                                 (const uint32_t*)(d == 0 ? a.out0 : a.out1),
                                                 nb / 4, cnt);
          unsigned h_cnt = 0;
          if (!vs)
            vs = hip_check(hipMemcpyAsync(&h_cnt, cnt, sizeof(unsigned), hipMemcpyDeviceToHost, s),
                           "autotune verify");
          if (!vs) vs = hip_check(hipStreamSynchronize(s), "autotune verify");
          if (vs && !st) st = vs;
          diff += h_cnt;
        }
        if (diff) ++bad;
      }
      if (t < tbest) {
        tbest = t;
        best[i] = cands[j];
      }
    }
    if (dbg)
      fprintf(stderr, "[autotune] launch %2zu %3dx%-3d k%d s%d %4d->%-4d default %7.1f us best %7.1f us"
                      " MR=%d NR=%d G=%d resw=%d persist=%d kind=%d (%d cfgs)\n",
              i, a.Ho, a.Wo, a.k, a.stride, a.Cin, a.Cout, t0 * 1e3, tbest * 1e3, best[i].mr,
              best[i].nr, best[i].G, best[i].resw, best[i].persist, best[i].kind, n);
  }
  // teardown of the autotuner's private buffers: nothing to report
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (ref) (void)hipFree(ref);
  if (cnt) (void)hipFree(cnt);
  if (n_bad) *n_bad = bad;
  if (!st) M->tuned = best;
  return st;
}

// The autotuned configuration of conv launch `idx` (cfg6; MR = 0: the
// default heuristic).  Returns the number of launches.
extern "C" int rv_yolo_tuned_config(void* h, int idx, int* cfg6) {
  if (!h) return RV_EINVAL;
  Model* M = (Model*)h;
  if (cfg6 && idx >= 0 && idx < (int)M->tuned.size()) to6(M->tuned[idx], cfg6);
  return (int)M->tuned.size();
}

// Install a configuration for conv launch idx (saved from rv_yolo_tuned_config
// of an earlier autotune of the same plan): n = number of launches of the
// plan (resizes the table; entries not set keep the default heuristic).
// Invalid configurations fall back to the default at launch (conv_cfg_ok).
extern "C" int rv_yolo_set_tuned(void* h, int n, int idx, const int* cfg6) {
  RV_CHECK_ARG(h && cfg6 && n > 0 && idx >= 0 && idx < n, "bad args");
  Model* M = (Model*)h;
  if ((int)M->tuned.size() != n) M->tuned.assign(n, ConvCfg{0, 0, 0, 0, 0});
  M->tuned[idx] = from6(cfg6);
  return RV_OK;
}

// The valid kernel configurations of conv launch idx of the last whole
// forward (the autotuner's search space for it; fused C2f launches have
// none): writes up to cap entries of cfg6 and returns the count.  A caller
// that times configurations in its own schedule (bench.py's in-pipeline
// tuning) installs them with rv_yolo_set_tuned.
extern "C" int rv_yolo_conv_candidates(void* h, int idx, int* cfg6, int cap) {
  RV_CHECK_ARG(h, "null handle");
  Model* M = (Model*)h;
  RV_CHECK_ARG(idx >= 0 && idx < (int)M->launches.size(),
               "launch %d not in the last forward (%d launches)", idx, (int)M->launches.size());
  const ConvArgs& a = M->launches[idx];
  if (a.fused != 0) return 0;
  std::vector<ConvCfg> c(512);
  const int n = std::min(conv_candidates(a, c.data(), (int)c.size()), (int)c.size());
  for (int i = 0; i < n && i < cap && cfg6; ++i) to6(c[i], cfg6 + 6 * i);
  return n;
}
