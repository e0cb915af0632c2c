// The preprocess entry points of include/rvhip.h: the per-op calls and
// rv_preprocess_chain_u8 (any chain of the built-in ops + the low-contrast
// gate + the detector's LetterBox).  Every entry checks its arguments and
// hands one ChainPass to the pass runner (launch_pass) or the fused runner
// (launch_fused) below; the kernels are clahe.hip's, median.hip's and
// dehaze.hip's.  Here: the gate's gray-span kernels and the frame copy.
//
// HBM layout: frames are B x H x pitch bytes (interleaved BGR).
#include "clahe.h"
#include "dehaze.h"
#include "derain.h"

namespace rv {

// Gray span for the low-contrast gate (pipeline.py:24-30).  A thread takes
// 4-pixel groups (12 bytes): three dword loads when `vec` (pitch and base
// 4-byte aligned) and the group lies inside the row, else its pixels one by
// one (the ragged right edge, unaligned frames).
__global__ __launch_bounds__(256) void gray_span_kernel(const uint8_t* __restrict__ in, int H,
                                                        int W, int pitch, int vec,
                                                        int* __restrict__ mn_mx) {
  const int b = blockIdx.y;
  const uint8_t* frame = in + (size_t)b * H * pitch;
  int mn = 255, mx = 0;
  const int groups = (W + 3) >> 2;
  const int total = H * groups;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int y = i / groups, x = (i - y * groups) * 4;
    const uint8_t* p = frame + (size_t)y * pitch + x * 3;
    if (vec && x + 3 < W) {
      const uint32_t w0 = ((const uint32_t*)p)[0], w1 = ((const uint32_t*)p)[1],
                     w2 = ((const uint32_t*)p)[2];
      // bytes little-endian: w0 = b0 g0 r0 b1 | w1 = g1 r1 b2 g2 | w2 = r2 b3 g3 r3
      const int v0 = bgr_to_y(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255);
      const int v1 = bgr_to_y(w0 >> 24, w1 & 255, (w1 >> 8) & 255);
      const int v2 = bgr_to_y((w1 >> 16) & 255, w1 >> 24, w2 & 255);
      const int v3 = bgr_to_y((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24);
      mn = min(mn, min(min(v0, v1), min(v2, v3)));
      mx = max(mx, max(max(v0, v1), max(v2, v3)));
    } else {
      const int n = min(4, W - x);
      for (int j = 0; j < n; ++j) {
        const int v = bgr_to_y(p[3 * j], p[3 * j + 1], p[3 * j + 2]);
        mn = min(mn, v);
        mx = max(mx, v);
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    mn = min(mn, __shfl_xor(mn, off));
    mx = max(mx, __shfl_xor(mx, off));
  }
  // one atomic pair per block: the 2 B words share a few cache lines, and
  // the atomics of every wave of 256 blocks per frame serialised on them
  // (0.45 ms per 32 x 1080p, ten times the read)
  __shared__ int smn[4], smx[4];
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = mn;
    smx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMin(&mn_mx[2 * b], min(min(smn[0], smn[1]), min(smn[2], smn[3])));
    atomicMax(&mn_mx[2 * b + 1], max(max(smx[0], smx[1]), max(smx[2], smx[3])));
  }
}
__global__ void gray_span_init(int* mn_mx, int B) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) {
    mn_mx[2 * i] = 255;
    mn_mx[2 * i + 1] = 0;
  }
}
__global__ void gray_span_finish(const int* mn_mx, int* span, int B) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) span[i] = mn_mx[2 * i + 1] - mn_mx[2 * i];
}

// The gate of rv_preprocess_chain_u8: flags[b] = 1 for a low-contrast frame
// (pipeline.py:28-29: span < contrast_thresh, compared in double as Python
// compares int < float), 0 for a frame that passes through unchanged.
__global__ void gray_span_gate(const int* mn_mx, int* flags, int B, double thresh) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) flags[i] = (double)(mn_mx[2 * i + 1] - mn_mx[2 * i]) < thresh ? 1 : 0;
}

// in -> out for every frame (flags == nullptr) or for the frames the gate
// passed through (flags[b] == 0).  16 bytes per thread, rows by blockIdx.y.
__global__ __launch_bounds__(256) void copy_frames_kernel(const uint8_t* __restrict__ in,
                                                          uint8_t* __restrict__ out, int H,
                                                          int rowbytes, int pitch, int vec,
                                                          const int* __restrict__ flags) {
  const int b = blockIdx.z;
  if (flags != nullptr && flags[b] != 0) return;
  const int i = (blockIdx.x * 256 + threadIdx.x) * 16;
  if (i >= rowbytes) return;
  for (int y = blockIdx.y; y < H; y += gridDim.y) {
    const size_t off = ((size_t)b * H + y) * pitch + i;
    if (vec && i + 16 <= rowbytes) {
      *(uint4*)(out + off) = *(const uint4*)(in + off);
    } else {
      const int n = min(16, rowbytes - i);
      for (int j = 0; j < n; ++j) out[off + j] = in[off + j];
    }
  }
}

static void launch_copy_frames(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                               const int* flags, hipStream_t s) {
  const int vec = (pitch % 16 == 0) && (((uintptr_t)in) % 16 == 0) && (((uintptr_t)out) % 16 == 0);
  const dim3 grid(ceil_div(W * 3, 256 * 16), min(H, 65535), B);
  copy_frames_kernel<<<grid, 256, 0, s>>>(in, out, H, W * 3, pitch, vec, flags);
}

static void launch_gray_span(const uint8_t* in, int B, int H, int W, int pitch, int* mn_mx,
                             hipStream_t s) {
  const int vec = (pitch % 4 == 0) && (((uintptr_t)in) % 4 == 0);
  const int blocks = min(64, ceil_div(H * ((W + 3) / 4), 256));
  gray_span_init<<<ceil_div(B, 256), 256, 0, s>>>(mn_mx, B);
  gray_span_kernel<<<dim3(blocks, B), 256, 0, s>>>(in, H, W, pitch, vec, mn_mx);
}

}  // namespace rv

using namespace rv;

static int check_frames(const uint8_t* in, const void* out, int B, int H, int W, int pitch) {
  RV_CHECK_ARG(in != nullptr && out != nullptr, "null frame pointer");
  RV_CHECK_ARG(B >= 0 && H > 0 && W > 0, "bad frame shape B=%d H=%d W=%d", B, H, W);
  RV_CHECK_ARG(pitch >= 3 * W, "pitch %d < 3*W", pitch);
  RV_CHECK_ARG((const void*)in != out, "in and out must not alias");
  return RV_OK;
}

// ---------------------------------------------------------------------------
// The two runners: the only code that picks a CLAHE / median / DCP / streak
// launch.
// ---------------------------------------------------------------------------
namespace {

static_assert(kYCrCb == RV_CHAIN_YCRCB && kLab == RV_CHAIN_LAB, "ChainPass::space");

enum PassKind {
  kPassClahe = 0,
  kPassMedian = 1,
  kPassClaheMedian = 2,
  kPassDcp = 3,
  kPassStreak = 4
};

// kPassClaheMedian: CLAHE(YCrCb) + median where clahe_median_fuses.
struct ChainPass {
  int kind, space, tiles, k;
  double clip;
  DcpParams dcp;  // kPassDcp only
  StreakParams streak;  // kPassStreak only
};

// One pass src -> dst (flags: nullptr, or the gate's per-frame flags: frames
// it passed through are skipped).  op_ws: the workspace of a DCP or streak pass.
void launch_pass(const ChainPass& q, const uint8_t* src, uint8_t* dst, uint8_t* lut, void* op_ws,
                 int B, int H, int W, int pitch, const int* flags, hipStream_t s) {
  if (q.kind == kPassDcp) {
    launch_dcp(src, dst, B, H, W, pitch, q.dcp, op_ws, nullptr, nullptr, flags, s);
    return;
  }
  if (q.kind == kPassStreak) {
    launch_streak(src, dst, B, H, W, pitch, q.streak, op_ws, nullptr, flags, s);
    return;
  }
  if (q.kind == kPassMedian) {
    const ClaheGeo g{};
    if (q.k == 3)
      launch_med3(false, src, dst, nullptr, B, H, W, pitch, g, nullptr, nullptr, flags, 0, s);
    else
      dispatch_median<false>(q.k, src, dst, nullptr, B, H, W, pitch, g, s, flags);
    return;
  }
  const ClaheGeo g = make_geo(H, W, q.tiles, q.clip);
  launch_clahe_lut(q.space, src, lut, B, H, W, pitch, g, flags, s);
  if (q.kind == kPassClahe)
    launch_clahe_apply(q.space, src, dst, lut, B, H, W, pitch, g, flags, s);
  else if (q.k == 3 && med3_cells_fit(g))
    launch_med3(true, src, dst, lut, B, H, W, pitch, g, nullptr, nullptr, flags, 0, s);
  else
    dispatch_median<true>(q.k, src, dst, lut, B, H, W, pitch, g, s, flags);
}

// The 128 x 32 pass of [CLAHE(YCrCb), median 3] with the letterbox from its
// tile (G, lb_out: nullable), for a geometry where med3_cells_fit and
// med3_lb_fits.  With flags the frames the gate passed through are copied to
// `out` and letterboxed raw by the same launch.
int launch_fused(const ChainPass& q, const uint8_t* in, uint8_t* out, uint8_t* lut, int B, int H,
                 int W, int pitch, const LbGeo* G, uint8_t* lb_out, const int* flags,
                 hipStream_t s) {
  const ClaheGeo g = make_geo(H, W, q.tiles, q.clip);
  if (G != nullptr) {
    const int st = launch_letterbox_pad(lb_out, B, *G, s);
    if (st) return st;
  }
  launch_clahe_lut(kYCrCb, in, lut, B, H, W, pitch, g, flags, s);
  launch_med3(true, in, out, lut, B, H, W, pitch, g, G, lb_out, flags, 1, s);
  return RV_OK;
}

}  // namespace

// B x tiles^2 LUTs of 256 bytes
extern "C" size_t rv_clahe_ws_bytes(int B, int tiles) {
  if (B <= 0 || tiles <= 0) return 0;
  return lut_bytes(B, tiles);
}

extern "C" int rv_clahe_ycrcb_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                                 int tiles, double clip, void* ws, size_t ws_bytes, void* stream) {
  int st = check_frames(in, out, B, H, W, pitch);
  if (st) return st;
  RV_CHECK_ARG(tiles >= 1 && tiles <= 64, "tiles %d out of range", tiles);
  RV_CHECK_ARG(ws != nullptr && ws_bytes >= rv_clahe_ws_bytes(B, tiles), "workspace too small");
  if (B == 0) return RV_OK;
  const ChainPass q{kPassClahe, kYCrCb, tiles, 0, clip, DcpParams{}};
  launch_pass(q, in, out, (uint8_t*)ws, nullptr, B, H, W, pitch, nullptr, as_stream(stream));
  return launch_status("rv_clahe_ycrcb_u8");
}

extern "C" int rv_median_u8c3(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                              int k, void* stream) {
  int st = check_frames(in, out, B, H, W, pitch);
  if (st) return st;
  RV_CHECK_ARG(k == 3 || k == 5 || k == 7 || k == 9, "median k=%d must be 3,5,7,9", k);
  if (B == 0) return RV_OK;
  const ChainPass q{kPassMedian, 0, 0, k, 0.0, DcpParams{}};
  launch_pass(q, in, out, nullptr, nullptr, B, H, W, pitch, nullptr, as_stream(stream));
  return launch_status("rv_median_u8c3");
}

extern "C" int rv_clahe_lab_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                               int tiles, double clip, void* ws, size_t ws_bytes, void* stream) {
  int st = check_frames(in, out, B, H, W, pitch);
  if (st) return st;
  RV_CHECK_ARG(tiles >= 1 && tiles <= 64, "tiles %d out of range", tiles);
  RV_CHECK_ARG(ws != nullptr && ws_bytes >= rv_clahe_ws_bytes(B, tiles), "workspace too small");
  st = ensure_lab_tables();
  if (st) return st;
  if (B == 0) return RV_OK;
  const ChainPass q{kPassClahe, kLab, tiles, 0, clip, DcpParams{}};
  launch_pass(q, in, out, (uint8_t*)ws, nullptr, B, H, W, pitch, nullptr, as_stream(stream));
  return launch_status("rv_clahe_lab_u8");
}

extern "C" int rv_clahe_median_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                                  int tiles, double clip, int k, void* ws, size_t ws_bytes,
                                  void* stream) {
  int st = check_frames(in, out, B, H, W, pitch);
  if (st) return st;
  RV_CHECK_ARG(tiles >= 1 && tiles <= 64, "tiles %d out of range", tiles);
  RV_CHECK_ARG(k == 3 || k == 5 || k == 7 || k == 9, "median k=%d must be 3,5,7,9", k);
  RV_CHECK_ARG(ws != nullptr && ws_bytes >= rv_clahe_ws_bytes(B, tiles), "workspace too small");
  if (B == 0) return RV_OK;
  const ClaheGeo g = make_geo(H, W, tiles, clip);
  RV_CHECK_ARG(clahe_median_fuses(g, k),
               "LUT window too large for the fused pass (tiles=%d, tile %dx%d); "
               "use rv_clahe_ycrcb_u8 + rv_median_u8c3",
               tiles, g.tw, g.th);
  const ChainPass q{kPassClaheMedian, kYCrCb, tiles, k, clip, DcpParams{}};
  launch_pass(q, in, out, (uint8_t*)ws, nullptr, B, H, W, pitch, nullptr, as_stream(stream));
  return launch_status("rv_clahe_median_u8");
}

extern "C" int rv_clahe_median_fits(int H, int W, int tiles, int k) {
  if (H <= 0 || W <= 0 || tiles < 1 || tiles > 64) return 0;
  return clahe_median_fuses(make_geo(H, W, tiles, 0.0), k) ? 1 : 0;
}

extern "C" int rv_clahe_median_letterbox_fits(int H, int W, int tiles, int k, const int* geo) {
  if (H <= 0 || W <= 0 || tiles < 1 || tiles > 64 || k != 3 || geo == nullptr) return 0;
  LbGeo G;
  if (!lbgeo_from(geo, H, W, G)) return 0;
  return med3_cells_fit(make_geo(H, W, tiles, 0.0)) && med3_lb_fits(G, H, W) ? 1 : 0;
}

extern "C" int rv_clahe_median_letterbox_u8(const uint8_t* in, uint8_t* out, int B, int H, int W,
                                            int pitch, int tiles, double clip, int k, void* ws,
                                            size_t ws_bytes, uint8_t* lb_out, const int* geo,
                                            void* stream) {
  int st = check_frames(in, out, B, H, W, pitch);
  if (st) return st;
  RV_CHECK_ARG(tiles >= 1 && tiles <= 64, "tiles %d out of range", tiles);
  RV_CHECK_ARG(ws != nullptr && ws_bytes >= rv_clahe_ws_bytes(B, tiles), "workspace too small");
  RV_CHECK_ARG(lb_out != nullptr && geo != nullptr, "null letterbox pointer");
  RV_CHECK_ARG(rv_clahe_median_letterbox_fits(H, W, tiles, k, geo),
               "geometry not supported by the fused pass (k=%d, %dx%d, tiles=%d); use "
               "rv_clahe_median_u8 + rv_letterbox_u8", k, W, H, tiles);
  if (B == 0) return RV_OK;
  LbGeo G;
  lbgeo_from(geo, H, W, G);
  const ChainPass q{kPassClaheMedian, kYCrCb, tiles, k, clip, DcpParams{}};
  st = launch_fused(q, in, out, (uint8_t*)ws, B, H, W, pitch, &G, lb_out, nullptr,
                    as_stream(stream));
  if (st) return st;
  return launch_status("rv_clahe_median_letterbox_u8");
}

extern "C" int rv_gray_span_u8(const uint8_t* in, int B, int H, int W, int pitch, int* ws,
                               int* span_out, void* stream) {
  RV_CHECK_ARG(in != nullptr && ws != nullptr && span_out != nullptr, "null pointer");
  RV_CHECK_ARG(B >= 0 && H > 0 && W > 0 && pitch >= 3 * W, "bad frame shape");
  if (B == 0) return RV_OK;
  hipStream_t s = as_stream(stream);
  launch_gray_span(in, B, H, W, pitch, ws, s);
  gray_span_finish<<<ceil_div(B, 256), 256, 0, s>>>(ws, span_out, B);
  return launch_status("rv_gray_span_u8");
}

// ---------------------------------------------------------------------------
// rv_preprocess_chain_u8: any chain of the built-in ops + the low-contrast
// gate + the detector's LetterBox as stream-ordered launches (rvhip.h).
// ---------------------------------------------------------------------------
static_assert(sizeof(rv_chain_desc) == RV_CHAIN_DESC_BYTES, "rv_chain_desc layout");

namespace {

// How a descriptor runs on an H x W frame: the passes (adjacent CLAHE(YCrCb)
// + median fused where rv_clahe_median_u8 would), the route and the
// workspace layout [gate ints | LUTs | scratch batch | DCP workspace | streak
// workspace].
struct ChainPlan {
  bool identity;  // disabled or empty chain: proc = raw
  bool gate, lab;
  int n;
  ChainPass pass[RV_CHAIN_MAX_OPS];
  int route;
  int lut_tiles;  // largest CLAHE grid (0: no CLAHE)
  int dcp_radius;  // largest refine radius of a DCP pass (-1: no DCP)
  int streak_max_len;  // largest max_len of a streak pass (-1: no streak pass)
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int check_desc(const rv_chain_desc* d) {
  RV_CHECK_ARG(d != nullptr, "null chain descriptor");
  RV_CHECK_ARG((d->enabled == 0 || d->enabled == 1) && (d->gate_on == 0 || d->gate_on == 1),
               "chain descriptor: enabled=%d gate_on=%d must be 0 or 1", d->enabled, d->gate_on);
  RV_CHECK_ARG(d->n_ops >= 0 && d->n_ops <= RV_CHAIN_MAX_OPS, "chain descriptor: n_ops=%d not in 0..%d",
               d->n_ops, RV_CHAIN_MAX_OPS);
  RV_CHECK_ARG(d->contrast_thresh == d->contrast_thresh, "chain descriptor: contrast_thresh is NaN");
  for (int i = 0; i < d->n_ops; ++i) {
    const rv_chain_op& o = d->ops[i];
    if (o.kind == RV_CHAIN_CLAHE) {
      RV_CHECK_ARG(o.space == RV_CHAIN_YCRCB || o.space == RV_CHAIN_LAB,
                   "chain op %d: CLAHE space %d", i, o.space);
      RV_CHECK_ARG(o.tiles >= 2 && o.tiles <= 64, "chain op %d: CLAHE tiles %d not in 2..64", i,
                   o.tiles);
      RV_CHECK_ARG(o.clip == o.clip, "chain op %d: CLAHE clip is NaN", i);
    } else if (o.kind == RV_CHAIN_MEDIAN) {
      RV_CHECK_ARG(o.k == 3 || o.k == 5 || o.k == 7 || o.k == 9,
                   "chain op %d: median k=%d must be 3,5,7,9", i, o.k);
    } else if (o.kind == RV_CHAIN_DCP) {
      char what[32];
      snprintf(what, sizeof(what), "chain op %d: DCP", i);
      const int st = dcp_check(DcpParams{o.patch, o.wq, o.tq, o.radius, o.eq}, 0, 0, what);
      if (st) return st;
    } else if (o.kind == RV_CHAIN_STREAK) {
      char what[32];
      snprintf(what, sizeof(what), "chain op %d: streak", i);
      const int st = streak_check(StreakParams{o.width, o.min_len, o.max_len, o.slant, o.thr}, what);
      if (st) return st;
    } else {
      RV_CHECK_ARG(false, "chain op %d: unknown kind %d", i, o.kind);
    }
  }
  return RV_OK;
}

// G: the letterbox wanted (nullptr: none).  The descriptor is already checked.
void make_plan(const rv_chain_desc& d, int H, int W, const LbGeo* G, ChainPlan& p) {
  p.identity = !d.enabled || d.n_ops == 0;
  p.gate = !p.identity && d.gate_on;
  p.lab = false;
  p.n = 0;
  p.lut_tiles = 0;
  p.dcp_radius = -1;
  p.streak_max_len = -1;
  p.route = RV_CHAIN_ROUTE_OPS;
  if (p.identity) return;
  for (int i = 0; i < d.n_ops;) {
    const rv_chain_op& o = d.ops[i];
    ChainPass& q = p.pass[p.n++];
    if (o.kind == RV_CHAIN_DCP) {  // a pass of its own: never fused with a neighbour
      q = ChainPass{kPassDcp, 0, 0, 0, 0.0, DcpParams{o.patch, o.wq, o.tq, o.radius, o.eq}};
      p.dcp_radius = max(p.dcp_radius, o.radius);
      ++i;
      continue;
    }
    if (o.kind == RV_CHAIN_STREAK) {  // likewise a pass of its own
      q = ChainPass{kPassStreak, 0, 0, 0, 0.0, DcpParams{},
                    StreakParams{o.width, o.min_len, o.max_len, o.slant, o.thr}};
      p.streak_max_len = max(p.streak_max_len, o.max_len);
      ++i;
      continue;
    }
    q = ChainPass{o.kind == RV_CHAIN_CLAHE ? kPassClahe : kPassMedian, o.space, o.tiles, o.k, o.clip,
                  DcpParams{}};
    if (o.kind == RV_CHAIN_CLAHE) {
      p.lut_tiles = max(p.lut_tiles, o.tiles);
      p.lab = p.lab || o.space == RV_CHAIN_LAB;
      if (o.space == RV_CHAIN_YCRCB && i + 1 < d.n_ops && d.ops[i + 1].kind == RV_CHAIN_MEDIAN &&
          clahe_median_fuses(make_geo(H, W, o.tiles, 0.0), d.ops[i + 1].k)) {
        q.kind = kPassClaheMedian;
        q.k = d.ops[i + 1].k;
        i += 2;
        continue;
      }
    }
    ++i;
  }
  // the single 128 x 32 pass of the default chain (+ the letterbox from its tile)
  if (p.n == 1 && p.pass[0].kind == kPassClaheMedian && p.pass[0].k == 3 &&
      med3_cells_fit(make_geo(H, W, p.pass[0].tiles, 0.0)) &&
      (G == nullptr || med3_lb_fits(*G, H, W)))
    p.route = p.gate ? RV_CHAIN_ROUTE_FUSED_GATED : RV_CHAIN_ROUTE_FUSED;
}

struct ChainWs {
  size_t gate, lut, scratch, dcp, streak;  // byte sizes, in this order
  size_t total() const { return gate + lut + scratch + dcp + streak; }
};

ChainWs plan_ws(const ChainPlan& p, int B, int H, int W, int pitch) {
  ChainWs w;
  w.gate = p.gate ? align256((size_t)3 * B * sizeof(int)) : 0;
  w.lut = p.lut_tiles ? align256(lut_bytes(B, p.lut_tiles)) : 0;
  w.scratch = p.n >= 2 ? align256((size_t)B * H * pitch) : 0;
  w.dcp = p.dcp_radius >= 0 && B > 0 ? align256(dcp_ws_bytes(B, H, W, p.dcp_radius)) : 0;
  w.streak =
      p.streak_max_len >= 0 && B > 0 ? align256(streak_ws_bytes(B, H, W, p.streak_max_len)) : 0;
  return w;
}

}  // namespace

extern "C" int rv_preprocess_chain_route(const rv_chain_desc* desc, int H, int W, const int* geo) {
  int st = check_desc(desc);
  if (st) return st;
  RV_CHECK_ARG(H > 0 && W > 0, "bad frame shape H=%d W=%d", H, W);
  LbGeo G;
  if (geo != nullptr) RV_CHECK_ARG(lbgeo_from(geo, H, W, G), "inconsistent letterbox geometry");
  ChainPlan p;
  make_plan(*desc, H, W, geo ? &G : nullptr, p);
  return p.route;
}

extern "C" size_t rv_preprocess_chain_ws_bytes(const rv_chain_desc* desc, int B, int H, int W,
                                               int pitch) {
  if (check_desc(desc) != RV_OK || B <= 0 || H <= 0 || W <= 0 || pitch < 3 * W) return 0;
  ChainPlan p;
  make_plan(*desc, H, W, nullptr, p);  // the layout does not depend on the letterbox
  if (p.dcp_radius >= 0 && (int64_t)H * W > (1 << 24)) return 0;
  return plan_ws(p, B, H, W, pitch).total();
}

extern "C" int rv_preprocess_chain_u8(const uint8_t* in, uint8_t* out, int B, int H, int W,
                                      int pitch, const rv_chain_desc* desc, void* ws,
                                      size_t ws_bytes, uint8_t* lb_out, const int* geo,
                                      void* stream) {
  int st = check_desc(desc);
  if (st) return st;
  // out == nullptr: "proc is the input", for a disabled or empty chain only
  const bool no_out = out == nullptr && (!desc->enabled || desc->n_ops == 0);
  st = check_frames(in, no_out ? (const void*)lb_out : (const void*)out, B, H, W, pitch);
  if (st) return st;
  RV_CHECK_ARG((lb_out != nullptr) == (geo != nullptr),
               "lb_out and geo must be given together (lb_out %s, geo %s)",
               lb_out ? "set" : "null", geo ? "set" : "null");
  LbGeo G;
  if (geo != nullptr) RV_CHECK_ARG(lbgeo_from(geo, H, W, G), "inconsistent letterbox geometry");
  ChainPlan p;
  make_plan(*desc, H, W, geo ? &G : nullptr, p);
  if (p.dcp_radius >= 0)
    RV_CHECK_ARG((int64_t)H * W <= (1 << 24) && B <= 65535,
                 "a DCP op takes at most 65535 frames of 2^24 pixels (B=%d, %d x %d)", B, W, H);
  if (p.streak_max_len >= 0)
    RV_CHECK_ARG(B <= 65535, "a streak op takes at most 65535 frames (B=%d)", B);
  const ChainWs w = plan_ws(p, B, H, W, pitch);
  RV_CHECK_ARG(w.total() == 0 || (ws != nullptr && ws_bytes >= w.total()),
               "workspace too small: %zu bytes, rv_preprocess_chain_ws_bytes says %zu", ws_bytes,
               w.total());
  RV_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  if (w.total()) {
    const uint8_t* w0 = (const uint8_t*)ws;
    const size_t fb = (size_t)B * H * pitch;
    RV_CHECK_ARG((w0 + w.total() <= in || in + fb <= w0) &&
                     (out == nullptr || w0 + w.total() <= out || out + fb <= w0),
                 "the workspace overlaps the frames");
  }
  if (B == 0) return RV_OK;
  if (p.lab) {
    st = ensure_lab_tables();
    if (st) return st;
  }
  hipStream_t s = as_stream(stream);
  int* gate = (int*)ws;  // mn_mx[2 B], then flags[B]
  const int* flags = p.gate ? gate + 2 * B : nullptr;
  uint8_t* lut = (uint8_t*)ws + w.gate;
  uint8_t* scratch = (uint8_t*)ws + w.gate + w.lut;
  if (p.gate) {
    launch_gray_span(in, B, H, W, pitch, gate, s);
    gray_span_gate<<<ceil_div(B, 256), 256, 0, s>>>(gate, gate + 2 * B, B, desc->contrast_thresh);
  }
  if (p.route != RV_CHAIN_ROUTE_OPS) {
    st = launch_fused(p.pass[0], in, out, lut, B, H, W, pitch, geo ? &G : nullptr, lb_out, flags, s);
    if (st) return st;
    return launch_status("rv_preprocess_chain_u8");
  }
  if (p.identity) {
    if (out != nullptr) launch_copy_frames(in, out, B, H, W, pitch, nullptr, s);
  } else {
    // the last pass writes `out`; the ones before alternate with the scratch batch
    const uint8_t* src = in;
    for (int i = 0; i < p.n; ++i) {
      uint8_t* dst = ((p.n - 1 - i) & 1) ? scratch : out;
      uint8_t* op_ws = scratch + w.scratch + (p.pass[i].kind == kPassStreak ? w.dcp : 0);
      launch_pass(p.pass[i], src, dst, lut, op_ws, B, H, W, pitch, flags, s);
      src = dst;
    }
    if (p.gate) launch_copy_frames(in, out, B, H, W, pitch, flags, s);
  }
  if (lb_out != nullptr) launch_letterbox(out ? out : in, lb_out, B, H, W, pitch, G, s);
  return launch_status("rv_preprocess_chain_u8");
}
