// Detection overlays and the compare canvas (include/rvhip.h, "Detection
// overlays"): the reference's draw_detections (src/vis/draw.py:25-102) and
// make_canvas (main_preview.py:12-34) for frames that stay on the device.
//
// rv_overlay_layout turns one step's device results into a display list per
// stream -- the reference's layout arithmetic and f-strings, one thread per
// detection slot, an ordered block scan so that a skipped detection leaves no
// gap.  rv_overlay_raster composes base image + display list: one workgroup
// per 128 x 64 tile of one stream culls the list against its tile into LDS,
// 256 primitives at a time from the end of the list, and every thread resolves
// its 32 pixels against the culled entries (the first hit wins, which is the
// last primitive in painter's order).  Pixels nothing covers are a copy of the
// base, so the kernel reads and writes every pixel once.
#include "common.h"
#include "overlay_font.h"

namespace rv {

namespace {

// Tile shape and row mapping as measured at 32 x 1080p with 100 detections a
// stream (tools/time_overlay.py): 128 x 64 with a thread's rows 8 apart, 0.28
// ms; the same tile with 8 consecutive rows a thread, 0.40 ms; 256 x 32 with a
// wave per tile row, 0.38 ms.
constexpr int kTileW = 128, kTileH = 64, kThreads = 256;
constexpr int kCols = kTileW / 4;           // threads across a tile: 32
constexpr int kRowStep = kThreads / kCols;  // a thread's rows are this far apart: 8
constexpr int kRows = kTileH / kRowStep;    // rows per thread: 8
constexpr int kHdr = RV_OVERLAY_LIST_HEADER_BYTES, kPrim = RV_OVERLAY_PRIM_BYTES;
constexpr int kCoordMax = 1 << 28;  // coordinates are clamped here: no overflow in a +- t
constexpr uint32_t kNone = 0xffffffffu;
// a record's bytes 16..95 as words, and where its text starts in them
constexpr int kTextWords = (RV_OVERLAY_PRIM_BYTES - 16) / 4;
constexpr int kTextAt = (int)offsetof(rv_overlay_prim, text) - 16;

__constant__ uint8_t kFont[RV_OVERLAY_FONT_GLYPHS * RV_OVERLAY_FONT_ROWS] = {RV_OVERLAY_FONT_TABLE};

static_assert(sizeof(rv_overlay_prim) == RV_OVERLAY_PRIM_BYTES, "record layout");

__host__ __device__ inline size_t list_stride(int dmax) {
  return (size_t)kHdr + (size_t)(5 * dmax + 8) * kPrim;
}

// ---------------------------------------------------------------- layout ----

// draw.py:11-22
__constant__ uint8_t kColors[10][3] = {{255, 128, 64}, {0, 255, 255}, {80, 175, 76}, {255, 0, 255},
                                       {0, 128, 255},  {255, 64, 64}, {64, 255, 64}, {128, 128, 255},
                                       {255, 200, 0},  {0, 255, 128}};

// The text of one record, written in place; bytes past the end stay 0.
struct Text {
  uint8_t* p;
  int n;
  __device__ void put(char c) {
    if (n < RV_OVERLAY_TEXT_BYTES) p[n++] = (uint8_t)c;
  }
  __device__ void put(const char* s) {
    while (*s) put(*s++);
  }
  __device__ void put_uint(unsigned long long v) {
    char d[20];
    int k = 0;
    do {
      d[k++] = (char)('0' + (int)(v % 10));
      v /= 10;
    } while (v);
    while (k) put(d[--k]);
  }
  __device__ void put_int(long long v) {
    if (v < 0) put('-');
    put_uint(v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v);
  }
  // n hundredths / tenths -> "i.ff" / "i.f"
  __device__ void put_scaled(unsigned long long n, int digits) {
    const unsigned long long den = digits == 2 ? 100 : 10;
    put_uint(n / den);
    put('.');
    const int f = (int)(n % den);
    if (digits == 2) put((char)('0' + f / 10));
    put((char)('0' + f % 10));
  }
  // f"{conf:.2f}" of an f32 widened to f64: conf * 100 is exact in f64 (24 + 7
  // bits), so rint (half to even) decides on the exact value.
  __device__ void put_conf(float conf) {
    const double x = (double)conf;
    if (!(fabs(x) < 1e9)) {  // no confidence is: NaN, infinite or huge
      put("---");
      return;
    }
    if (signbit(x)) put('-');
    put_scaled((unsigned long long)rint(fabs(x) * 100.0), 2);
  }
  // f"{x:.1f}", correctly rounded: |x| * 10 = p + e exactly (e from the fma),
  // p = n + frac with n = floor(p), so the value's distance from the tie is
  // (frac - 0.5) + e, whose floating-point sum has the exact sum's sign.
  __device__ void put_metric(double x) {
    if (!(fabs(x) < 1e9)) {  // 1e9 and above, infinite: no digits, no sign
      put("---");
      return;
    }
    if (signbit(x)) put('-');
    const double a = fabs(x);
    const double p = a * 10.0;
    const double e = fma(a, 10.0, -p);
    const double fl = floor(p);
    unsigned long long n = (unsigned long long)fl;
    const double t = ((p - fl) - 0.5) + e;
    if (t > 0.0 || (t == 0.0 && (n & 1))) ++n;
    put_scaled(n, 1);
  }
};

__device__ inline int trunc_coord(float v) {
  if (!(v == v)) return 0;
  if (v >= (float)kCoordMax) return kCoordMax;
  if (v <= -(float)kCoordMax) return -kCoordMax;
  return (int)v;  // toward zero, Python's int()
}

__device__ inline rv_overlay_prim* begin_prim(uint8_t* list, int i, int kind, int x0, int y0, int x1,
                                              int y1, const uint8_t* bgr, int thickness, int scale) {
  uint32_t* w = reinterpret_cast<uint32_t*>(list + kHdr + (size_t)i * kPrim);
  for (int k = 0; k < kPrim / 4; ++k) w[k] = 0;
  rv_overlay_prim* r = reinterpret_cast<rv_overlay_prim*>(w);
  r->kind = kind;
  r->x0 = x0;
  r->y0 = y0;
  r->x1 = x1;
  r->y1 = y1;
  r->b = bgr[0];
  r->g = bgr[1];
  r->r = bgr[2];
  r->thickness = (uint8_t)thickness;
  r->scale = (uint8_t)scale;
  return r;
}

__global__ __launch_bounds__(kThreads) void overlay_layout_kernel(
    const float* __restrict__ dets, const int* __restrict__ det_n, const int* __restrict__ track_id,
    const double* __restrict__ distance_m, const double* __restrict__ speed_kmh, int dmax, int H,
    const uint8_t* __restrict__ names, int nc, int thickness, int scale, uint8_t* __restrict__ lists) {
  __shared__ int wcnt[kThreads / 64];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint8_t* list = lists + (size_t)s * list_stride(dmax);
  int n = det_n[s];
  n = n < 0 ? 0 : (n > dmax ? dmax : n);
  const int th = 9 * scale, bl = 2 * scale, pad = 2;
  const int tt = thickness - 1 > 1 ? thickness - 1 : 1;
  const uint8_t white[3] = {255, 255, 255};
  int running = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + tid;
    int cnt = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    double dist = 0.0, spd = 0.0;
    bool has_d = false, has_v = false;
    const size_t di = (size_t)s * dmax + (i < n ? i : 0);
    if (i < n) {
      const float* d = dets + di * 6;
      x1 = trunc_coord(d[0]);
      y1 = trunc_coord(d[1]);
      x2 = trunc_coord(d[2]);
      y2 = trunc_coord(d[3]);
      if (x2 > x1 && y2 > y1) {
        dist = distance_m[di];
        spd = speed_kmh[di];
        has_d = dist == dist;
        has_v = spd == spd;
        cnt = has_d || has_v ? 5 : 3;
      }
    }
    // ordered exclusive scan of cnt over the block
    int incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wcnt[wave] = incl;
    __syncthreads();
    int off = running + incl - cnt, total = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
      if (w < wave) off += wcnt[w];
      total += wcnt[w];
    }
    running += total;
    __syncthreads();
    if (cnt == 0) continue;

    const float* d = dets + di * 6;
    const float clsf = d[5];
    const long long cls = clsf == clsf ? (long long)clsf : 0;
    const uint8_t* color = kColors[(int)(((cls % 10) + 10) % 10)];
    begin_prim(list, off, RV_OVERLAY_OUTLINE, x1, y1, x2, y2, color, thickness, 0);

    // _draw_label_top (draw.py:59-79) at (x1, y1)
    {
      const int x = x1 > 0 ? x1 : 0, y = y1 > 0 ? y1 : 0;
      rv_overlay_prim* tp = begin_prim(list, off + 2, RV_OVERLAY_TEXT, 0, 0, 0, 0, white, tt, scale);
      Text t{tp->text, 0};
      const int id = track_id[di];
      if (id >= 0) {
        t.put("ID ");
        t.put_uint((unsigned long long)id);
        t.put(" | ");
      }
      const uint8_t* name = (cls >= 0 && cls < nc) ? names + (size_t)cls * RV_OVERLAY_NAME_BYTES : nullptr;
      if (name != nullptr && name[0] != 0) {
        for (int k = 0; k < RV_OVERLAY_NAME_BYTES - 1 && name[k] != 0; ++k) t.put((char)name[k]);
      } else {
        t.put_int(cls);
      }
      t.put(' ');
      t.put_conf(d[4]);
      tp->len = (uint8_t)t.n;
      const int tw = 6 * scale * t.n;
      int box_top = y - th - bl - pad * 2;
      box_top = box_top > 0 ? box_top : 0;
      begin_prim(list, off + 1, RV_OVERLAY_FILL, x, box_top, x + tw + pad * 2, y, color, 0, 0);
      tp->x0 = x + pad;
      tp->y0 = box_top + th > pad + th ? box_top + th : pad + th;
    }
    if (cnt == 5) {
      // _draw_label_bottom (draw.py:82-102) at (x1, y2 + 4)
      const int x = x1 > 0 ? x1 : 0, y = y2 + 4 > 0 ? y2 + 4 : 0;
      rv_overlay_prim* tp = begin_prim(list, off + 4, RV_OVERLAY_TEXT, 0, 0, 0, 0, white, tt, scale);
      Text t{tp->text, 0};
      if (has_d) {
        t.put_metric(dist);
        t.put(" m");
      }
      if (has_v) {
        if (has_d) t.put(" / ");
        t.put_metric(spd);
        t.put(" km/h");
      }
      tp->len = (uint8_t)t.n;
      const int tw = 6 * scale * t.n;
      const int lim = H - th - bl - pad * 2;
      const int box_top = y < lim ? y : lim;
      const int bb = box_top + th + bl + pad * 2;
      const int box_bottom = H < bb ? H : bb;
      begin_prim(list, off + 3, RV_OVERLAY_FILL, x, box_top, x + tw + pad * 2, box_bottom, color, 0, 0);
      tp->x0 = x + pad;
      tp->y0 = H - bl - 1 < box_top + th + bl ? H - bl - 1 : box_top + th + bl;
    }
  }
  if (tid == 0) {
    int* hdr = reinterpret_cast<int*>(list);
    hdr[0] = running;
    hdr[1] = hdr[2] = hdr[3] = 0;
  }
}

// ---------------------------------------------------------------- raster ----

struct RasterArgs {
  const uint8_t* proc;
  const uint8_t* raw;
  const uint8_t* lists;
  const uint8_t* canvas;
  uint8_t* out;
  int H, W, OH, OW;  // pane and output sizes
  int px, py;        // the PROC pane's offset in the output
  int mode, divider, cap;
  size_t stride;  // bytes between two streams' lists
};

// A primitive that touches the tile: bbox (output coordinates, clipped), and
// outline: the hole; text: a = left, b = top of the glyph cells, c = bytes, d
// = the reciprocal of 6k (recip20).
struct Cull {
  int x0, y0, x1, y1;
  int a, b, c, d;
  uint32_t color;  // b | g << 8 | r << 16 | kind << 24
  uint32_t tk;     // text: thickness | scale << 6 | recip20(scale) << 10
};

__device__ inline uint32_t recip20(int d) { return ((1u << 20) + (uint32_t)d - 1u) / (uint32_t)d; }

__device__ inline int clampc(int v) { return v < -kCoordMax ? -kCoordMax : (v > kCoordMax ? kCoordMax : v); }

__device__ inline const uint8_t* prim_ptr(const RasterArgs& p, int s, int i, int n_det) {
  return i < n_det ? p.lists + (size_t)s * p.stride + kHdr + (size_t)i * kPrim
                   : p.canvas + kHdr + (size_t)(i - n_det) * kPrim;
}

// Primitive i of the concatenated list (stream list, then canvas list) against
// the tile (tx0..tx1, ty0..ty1): false when it draws nothing there.
__device__ inline bool cull_prim(const RasterArgs& p, int s, int i, int n_det, int tx0, int ty0,
                                 int tx1, int ty1, Cull& c) {
  // every field but the text is in the record's first 28 bytes: two 16-byte
  // loads, instead of ten narrow ones a record (96 bytes) apart
  const uint4* rp = reinterpret_cast<const uint4*>(prim_ptr(p, s, i, n_det));
  const uint4 r0 = rp[0], r1 = rp[1];
  const int kind = (int)r0.x, rx0 = (int)r0.y, ry0 = (int)r0.z, rx1 = (int)r0.w, ry1 = (int)r1.x;
  const uint32_t bgr = r1.y & 0xffffffu;
  const bool pane = i < n_det;
  const int ox = pane ? p.px : 0, oy = pane ? p.py : 0;
  // clip: the pane for a stream's primitives, the whole output for the canvas's
  int cx0 = ox, cy0 = oy, cx1 = pane ? ox + p.W - 1 : p.OW - 1, cy1 = pane ? oy + p.H - 1 : p.OH - 1;
  cx0 = cx0 > tx0 ? cx0 : tx0;
  cy0 = cy0 > ty0 ? cy0 : ty0;
  cx1 = cx1 < tx1 ? cx1 : tx1;
  cy1 = cy1 < ty1 ? cy1 : ty1;
  int t = (int)(r1.y >> 24);
  int bx0, by0, bx1, by1;
  c.a = c.b = c.c = c.d = 0;
  c.tk = 0;
  if (kind == RV_OVERLAY_FILL || kind == RV_OVERLAY_OUTLINE) {
    const int x0 = clampc(rx0) + ox, y0 = clampc(ry0) + oy, x1 = clampc(rx1) + ox,
              y1 = clampc(ry1) + oy;
    bx0 = x0 < x1 ? x0 : x1;
    bx1 = x0 < x1 ? x1 : x0;
    by0 = y0 < y1 ? y0 : y1;
    by1 = y0 < y1 ? y1 : y0;
    if (kind == RV_OVERLAY_OUTLINE) {
      t = t < 1 ? 1 : t;
      const int a = t / 2, b = (t - 1) / 2;
      c.a = bx0 + b + 1;
      c.b = by0 + b + 1;
      c.c = bx1 - a - 1;
      c.d = by1 - a - 1;
      bx0 -= a;
      by0 -= a;
      bx1 += b;
      by1 += b;
    }
  } else if (kind == RV_OVERLAY_TEXT) {
    t = t < 1 ? 1 : (t > 32 ? 32 : t);
    int k = (int)(r1.z & 255u);
    k = k < 1 ? 1 : (k > 8 ? 8 : k);
    int len = (int)((r1.z >> 8) & 255u);
    len = len > RV_OVERLAY_TEXT_BYTES ? RV_OVERLAY_TEXT_BYTES : len;
    if (len == 0) return false;
    const int lo = (t - 1) / 2, hi = t / 2;
    c.a = clampc(rx0) + ox;
    c.b = clampc(ry0) + oy - 9 * k + 1;
    c.c = len;
    // n / d as (n * ceil(2^20 / d)) >> 20: exact while n * d < 2^20, and here
    // n < 6 * 8 * 64 and d <= 48; a label's pixels all pay for these divisions
    c.d = (int)recip20(6 * k);
    c.tk = (uint32_t)t | (uint32_t)k << 6 | recip20(k) << 10;
    bx0 = c.a - lo;
    by0 = c.b - lo;
    bx1 = c.a + 6 * k * len - 1 + hi;
    by1 = c.b + 11 * k - 1 + hi;
  } else {
    return false;
  }
  c.x0 = bx0 > cx0 ? bx0 : cx0;
  c.y0 = by0 > cy0 ? by0 : cy0;
  c.x1 = bx1 < cx1 ? bx1 : cx1;
  c.y1 = by1 < cy1 ? by1 : cy1;
  c.color = bgr | (uint32_t)kind << 24;
  if (c.x0 > c.x1 || c.y0 > c.y1) return false;
  // an outline whose hole holds the whole tile paints nothing here: most tiles
  // under a box are such
  return !(kind == RV_OVERLAY_OUTLINE && c.x0 >= c.a && c.x1 <= c.c && c.y0 >= c.b && c.y1 <= c.d);
}

// Does the text of culled entry c paint pixel (x, y)?  (x, y) is in its bbox.
// `text` and `font` are in LDS: a label's pixels all come here, and a thread
// walks its pixels one after the other.  Not inlined: the walk is unrolled over
// a thread's 32 pixels, and 32 copies of this push the kernel past the
// instruction cache.
struct TextCell {
  int a, b, c;  // Cull's: left, top, bytes
  uint32_t m6k, tk;
};
__device__ __noinline__ bool text_covers(TextCell c, const uint8_t* text, const uint8_t* font,
                                         int x, int y) {
  const int t = (int)(c.tk & 63u), k = (int)((c.tk >> 6) & 15u);
  const uint32_t mk = c.tk >> 10, m6k = c.m6k;
  const int lo = (t - 1) / 2, hi = t / 2;
  const int gx1 = c.a + 6 * k * c.c - 1, gy1 = c.b + 11 * k - 1;
  // the glyph pixels (u, v) whose shift by some dx, dy in [-lo, hi] lands on (x, y)
  const int u0 = x - hi > c.a ? x - hi : c.a, u1 = x + lo < gx1 ? x + lo : gx1;
  const int v0 = y - hi > c.b ? y - hi : c.b, v1 = y + lo < gy1 ? y + lo : gy1;
  for (int u = u0; u <= u1; ++u) {
    const int cx = u - c.a, ci = (int)(((uint32_t)cx * m6k) >> 20),
              col = (int)(((uint32_t)(cx - ci * 6 * k) * mk) >> 20);
    int ch = text[ci];
    if (ch < RV_OVERLAY_FONT_FIRST || ch >= RV_OVERLAY_FONT_FIRST + RV_OVERLAY_FONT_GLYPHS) ch = '?';
    const uint8_t* g = font + (ch - RV_OVERLAY_FONT_FIRST) * RV_OVERLAY_FONT_ROWS;
    for (int v = v0; v <= v1; ++v)
      if ((g[((uint32_t)(v - c.b) * mk) >> 20] >> (5 - col)) & 1) return true;
  }
  return false;
}

// The base image's pixel run starting at output (x, y): its address, or null
// inside the divider.  A run never crosses a region (the caller's job).
__device__ inline const uint8_t* base_ptr(const RasterArgs& p, int s, int x, int y) {
  const size_t frame = (size_t)p.H * p.W * 3;
  if (p.mode == RV_OVERLAY_ANNOTATE) return p.proc + s * frame + ((size_t)y * p.W + x) * 3;
  if (p.mode == RV_OVERLAY_COMPARE_H) {
    if (x < p.W) return p.raw + s * frame + ((size_t)y * p.W + x) * 3;
    if (x < p.px) return nullptr;
    return p.proc + s * frame + ((size_t)y * p.W + (x - p.px)) * 3;
  }
  if (y < p.H) return p.raw + s * frame + ((size_t)y * p.W + x) * 3;
  if (y < p.py) return nullptr;
  return p.proc + s * frame + ((size_t)(y - p.py) * p.W + x) * 3;
}

struct __attribute__((aligned(4))) Px4 {
  uint32_t w[3];  // four BGR pixels
};

// VEC: W, the pane offset and the output width are multiples of 4 pixels and
// the images 4-byte aligned, so a thread's four pixels are three aligned
// dwords of one region.  Otherwise every byte is moved on its own.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void overlay_raster_kernel(RasterArgs p) {
  __shared__ Cull cull[kThreads];
  __shared__ uint32_t ctext[kThreads][kTextWords];  // a culled text's bytes 16..95 of its record
  __shared__ uint32_t font[(sizeof(kFont) + 3) / 4];
  __shared__ int wcnt[kThreads / 64];
  const int s = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int tx1 = min(tx0 + kTileW, p.OW) - 1, ty1 = min(ty0 + kTileH, p.OH) - 1;
  const int gx = tx0 + (tid % kCols) * 4, gy = ty0 + tid / kCols;  // rows gy, gy + 8, ...

  int n_det = 0, n_can = 0;
  if (p.lists != nullptr) {
    n_det = *reinterpret_cast<const int*>(p.lists + (size_t)s * p.stride);
    n_det = n_det < 0 ? 0 : (n_det > p.cap ? p.cap : n_det);
  }
  if (p.canvas != nullptr) {
    n_can = *reinterpret_cast<const int*>(p.canvas);
    n_can = n_can < 0 ? 0 : (n_can > RV_OVERLAY_CANVAS_PRIMS ? RV_OVERLAY_CANVAS_PRIMS : n_can);
  }

  uint32_t col[kRows][4];
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) col[r][q] = kNone;
  if (n_det + n_can > 0) {
    for (int k = tid; k < (int)(sizeof(font) / 4); k += kThreads) {
      uint32_t w = 0;
      for (int b = 0; b < 4; ++b)
        if (4 * k + b < (int)sizeof(kFont)) w |= (uint32_t)kFont[4 * k + b] << (8 * b);
      font[k] = w;
    }
  }  // visible after the first chunk's barriers

  for (int hi = n_det + n_can; hi > 0; hi -= kThreads) {
    // thread 0 takes the last primitive: the culled entries are in reverse
    // painter's order, so the first hit of a walk from entry 0 wins
    const int idx = hi - 1 - tid;
    Cull c;
    const bool hit = idx >= 0 && cull_prim(p, s, idx, n_det, tx0, ty0, tx1, ty1, c);
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = __popcll(bal & ((1ull << lane) - 1ull)), m = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
      if (w < wave) off += wcnt[w];
      m += wcnt[w];
    }
    if (hit) {
      cull[off] = c;
      if ((c.color >> 24) == RV_OVERLAY_TEXT) {
        const uint4* rp = reinterpret_cast<const uint4*>(prim_ptr(p, s, idx, n_det));
#pragma unroll
        for (int k = 0; k < kTextWords / 4; ++k) {
          const uint4 v = rp[1 + k];
          ctext[off][4 * k] = v.x;
          ctext[off][4 * k + 1] = v.y;
          ctext[off][4 * k + 2] = v.z;
          ctext[off][4 * k + 3] = v.w;
        }
      }
    }
    __syncthreads();
    if (m > 0) {
      // entries outside, the thread's pixels inside: an entry that misses the
      // thread's four columns or its rows costs one LDS read and a compare
      for (int j = 0; j < m; ++j) {
        const Cull e = cull[j];
        if (gx + 3 < e.x0 || gx > e.x1 || gy > e.y1 || gy + (kRows - 1) * kRowStep < e.y0)
          continue;
        const uint32_t kind = e.color >> 24;
        // under a box most threads have all four columns inside the hole
        const bool cols_in_hole = kind == RV_OVERLAY_OUTLINE && gx >= e.a && gx + 3 <= e.c;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const int y = gy + r * kRowStep;
          if (y < e.y0 || y > e.y1 || (cols_in_hole && y >= e.b && y <= e.d)) continue;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int x = gx + q;
            if (col[r][q] != kNone || x < e.x0 || x > e.x1) continue;
            if (kind == RV_OVERLAY_OUTLINE && x >= e.a && x <= e.c && y >= e.b && y <= e.d) continue;
            if (kind == RV_OVERLAY_TEXT &&
                !text_covers(TextCell{e.a, e.b, e.c, (uint32_t)e.d, e.tk}, reinterpret_cast<const uint8_t*>(ctext[j]) + kTextAt,
                             reinterpret_cast<const uint8_t*>(font), x, y))
              continue;
            col[r][q] = e.color & 0xffffffu;
          }
        }
      }
      __syncthreads();  // the next chunk overwrites cull[]
    }
  }

  const size_t out_frame = (size_t)p.OH * p.OW * 3;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = gy + r * kRowStep;
    if (y > ty1 || gx > tx1) continue;
    uint8_t* o = p.out + s * out_frame + ((size_t)y * p.OW + gx) * 3;
    if (VEC) {
      const uint8_t* b = base_ptr(p, s, gx, y);
      Px4 v;
      if (b != nullptr) {
        v = *reinterpret_cast<const Px4*>(b);
      } else {
        v.w[0] = v.w[1] = v.w[2] = 0x28282828u;
      }
      // pixel q's bytes are 3q .. 3q + 2 of the 12
      if (col[r][0] != kNone) v.w[0] = (v.w[0] & 0xff000000u) | col[r][0];
      if (col[r][1] != kNone) {
        v.w[0] = (v.w[0] & 0x00ffffffu) | (col[r][1] << 24);
        v.w[1] = (v.w[1] & 0xffff0000u) | (col[r][1] >> 8);
      }
      if (col[r][2] != kNone) {
        v.w[1] = (v.w[1] & 0x0000ffffu) | (col[r][2] << 16);
        v.w[2] = (v.w[2] & 0xffffff00u) | (col[r][2] >> 16);
      }
      if (col[r][3] != kNone) v.w[2] = (v.w[2] & 0x000000ffu) | (col[r][3] << 8);
      *reinterpret_cast<Px4*>(o) = v;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (gx + q > tx1) continue;
        uint32_t c = col[r][q];
        if (c == kNone) {
          const uint8_t* b = base_ptr(p, s, gx + q, y);
          c = b != nullptr ? (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 : 0x282828u;
        }
        o[3 * q] = (uint8_t)c;
        o[3 * q + 1] = (uint8_t)(c >> 8);
        o[3 * q + 2] = (uint8_t)(c >> 16);
      }
    }
  }
}

bool overlaps(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
  return a < b + nb && b < a + na;
}

}  // namespace

extern "C" size_t rv_overlay_ws_bytes(int S, int dmax) {
  if (S < 1 || S > 4096 || dmax < 1 || dmax > 65536) return 0;
  return (size_t)S * list_stride(dmax);
}

extern "C" int rv_overlay_layout(const float* dets, const int* det_n, const int* track_id,
                                 const double* distance_m, const double* speed_kmh, int S, int dmax,
                                 int H, int W, const uint8_t* names, int nc, int thickness,
                                 int scale, uint8_t* lists, size_t lists_bytes, void* stream) {
  RV_CHECK_ARG(dets && det_n && track_id && distance_m && speed_kmh && lists, "null pointer");
  RV_CHECK_ARG(rv_overlay_ws_bytes(S, dmax) != 0, "S %d / dmax %d out of range", S, dmax);
  RV_CHECK_ARG(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "frame %d x %d", W, H);
  RV_CHECK_ARG(nc >= 0 && nc <= 65536 && (nc == 0 || names != nullptr), "class names: nc %d", nc);
  RV_CHECK_ARG(thickness <= 255, "thickness %d above 255", thickness);
  RV_CHECK_ARG(scale >= 1 && scale <= 8, "glyph scale %d not in 1..8", scale);
  RV_CHECK_ARG(lists_bytes >= rv_overlay_ws_bytes(S, dmax) && ((uintptr_t)lists & 15) == 0,
               "display lists: %zu bytes (need %zu), 16-byte aligned", lists_bytes,
               rv_overlay_ws_bytes(S, dmax));
  hipLaunchKernelGGL(overlay_layout_kernel, dim3(S), dim3(kThreads), 0, as_stream(stream), dets,
                     det_n, track_id, distance_m, speed_kmh, dmax, H, names, nc,
                     thickness < 1 ? 1 : thickness, scale, lists);
  return launch_status("rv_overlay_layout");
}

extern "C" int rv_overlay_raster(const uint8_t* proc, const uint8_t* raw, int S, int H, int W,
                                 int mode, int divider_px, const uint8_t* lists, int dmax,
                                 const uint8_t* canvas_list, uint8_t* out, void* stream) {
  RV_CHECK_ARG(proc != nullptr && out != nullptr, "null pointer");
  RV_CHECK_ARG(mode == RV_OVERLAY_ANNOTATE || mode == RV_OVERLAY_COMPARE_H ||
                   mode == RV_OVERLAY_COMPARE_V, "mode %d", mode);
  RV_CHECK_ARG(mode == RV_OVERLAY_ANNOTATE || raw != nullptr, "a compare canvas needs raw frames");
  RV_CHECK_ARG(S >= 1 && S <= 4096 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768,
               "S %d, frame %d x %d", S, W, H);
  RV_CHECK_ARG(divider_px >= 0 && divider_px <= 4096, "divider_px %d", divider_px);
  RV_CHECK_ARG(lists == nullptr || rv_overlay_ws_bytes(S, dmax) != 0, "dmax %d out of range", dmax);
  RV_CHECK_ARG(((uintptr_t)lists & 15) == 0 && ((uintptr_t)canvas_list & 15) == 0,
               "display lists must be 16-byte aligned");
  RasterArgs p{};
  p.proc = proc;
  p.raw = raw;
  p.lists = lists;
  p.canvas = canvas_list;
  p.out = out;
  p.H = H;
  p.W = W;
  p.mode = mode;
  p.divider = mode == RV_OVERLAY_ANNOTATE ? 0 : divider_px;
  p.OH = mode == RV_OVERLAY_COMPARE_V ? 2 * H + p.divider : H;
  p.OW = mode == RV_OVERLAY_COMPARE_H ? 2 * W + p.divider : W;
  p.px = mode == RV_OVERLAY_COMPARE_H ? W + p.divider : 0;
  p.py = mode == RV_OVERLAY_COMPARE_V ? H + p.divider : 0;
  p.cap = lists != nullptr ? 5 * dmax + 8 : 0;
  p.stride = lists != nullptr ? list_stride(dmax) : 0;
  const size_t in_bytes = (size_t)S * H * W * 3, out_bytes = (size_t)S * p.OH * p.OW * 3;
  RV_CHECK_ARG(!overlaps(out, out_bytes, proc, in_bytes) &&
                   (mode == RV_OVERLAY_ANNOTATE || !overlaps(out, out_bytes, raw, in_bytes)),
               "out overlaps an input image");
  const bool vec = W % 4 == 0 && p.px % 4 == 0 && (((uintptr_t)proc | (uintptr_t)out) & 3) == 0 &&
                   (mode == RV_OVERLAY_ANNOTATE || ((uintptr_t)raw & 3) == 0);
  const dim3 grid(ceil_div(p.OW, kTileW), ceil_div(p.OH, kTileH), S);
  if (vec)
    hipLaunchKernelGGL(overlay_raster_kernel<true>, grid, dim3(kThreads), 0, as_stream(stream), p);
  else
    hipLaunchKernelGGL(overlay_raster_kernel<false>, grid, dim3(kThreads), 0, as_stream(stream), p);
  return launch_status("rv_overlay_raster");
}

}  // namespace rv
