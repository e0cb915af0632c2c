// libjpeg's default forward path, one 8-sample row at a time: 16-bit
// fixed-point RGB -> YCbCr (jccolor.c), edge replication and h2v1 / h2v2
// downsampling (jcprepct.c, jcsample.c), the "islow" forward DCT
// (jfdctint.c) and the quantiser (jcdctmgr.c).  Plain integer C++, shared by
// the device encoder (jpeg_enc.hip) and host programs that check it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RVJ_HD __host__ __device__ __forceinline__
#else
#define RVJ_HD inline
#endif

namespace rvjpeg {

// Block grids of a W x H image with sampling code 0..2 (three components).
struct EncGeom {
  int W, H, fh, fv;  // fh, fv: luma samples per chroma sample
  int mx, my;        // MCUs across / down
  RVJ_HD EncGeom(int W_, int H_, int samp) : W(W_), H(H_) {
    fh = samp == 1 || samp == 2 ? 2 : 1;
    fv = samp == 2 ? 2 : 1;
    mx = (W + 8 * fh - 1) / (8 * fh);
    my = (H + 8 * fv - 1) / (8 * fv);
  }
  // blocks of the MCU-padded grid the record stores
  RVJ_HD int grid_w(int c) const { return c == 0 ? mx * fh : mx; }
  RVJ_HD int grid_h(int c) const { return c == 0 ? my * fv : my; }
  // blocks that hold image samples (libjpeg's width_in_blocks / height_in_blocks)
  RVJ_HD int real_w(int c) const { return c == 0 ? (W + 7) / 8 : ((W + fh - 1) / fh + 7) / 8; }
  RVJ_HD int real_h(int c) const { return c == 0 ? (H + 7) / 8 : ((H + fv - 1) / fv + 7) / 8; }
  RVJ_HD int blocks_per_mcu() const { return fh * fv + 2; }
  // The block whose DCT block (bx, by) of component c takes.  A block that
  // only pads the component to the MCU grid is a dummy: all-zero AC and the
  // DC of the block before it in MCU order, which is the block to its left,
  // or for a dummy row the last block of the MCU's row above.
  RVJ_HD bool source(int c, int bx, int by, int& sbx, int& sby) const {
    const int rw = real_w(c), rh = real_h(c);
    sbx = bx;
    sby = by;
    if (by >= rh) {
      sby = by - 1;
      sbx = bx / fh * fh + fh - 1;
    }
    if (sbx >= rw) sbx -= 1;
    return bx >= rw || by >= rh;
  }
};

RVJ_HD int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
RVJ_HD int ycc_cb(int r, int g, int b) {
  return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
RVJ_HD int ycc_cr(int r, int g, int b) {
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Component c (0 Y, 1 Cb, 2 Cr) of the BGR pixel (x, y) of a W-wide frame.
RVJ_HD int ycc_at(const uint8_t* bgr, int W, int c, int x, int y) {
  const uint8_t* p = bgr + ((size_t)y * W + x) * 3;
  const int b = p[0], g = p[1], r = p[2];
  return c == 0 ? ycc_y(r, g, b) : (c == 1 ? ycc_cb(r, g, b) : ycc_cr(r, g, b));
}

// Row t of block (sbx, sby) of component c, level-shifted.  The right edge
// replicates the last input column; the bottom edge pads the input to a whole
// row group, downsamples, and then repeats the last downsampled row: a
// replicated input row pair is never downsampled on its own.
RVJ_HD void sample_row(const uint8_t* bgr, const EncGeom& g, int c, int sbx, int sby, int t,
                       int (&x)[8]) {
  const int W = g.W, H = g.H;
  const int y = sby * 8 + t;
  if (c == 0 || (g.fh == 1 && g.fv == 1)) {
    const int yy = y < H ? y : H - 1;
    for (int u = 0; u < 8; ++u) {
      const int xx = sbx * 8 + u;
      x[u] = ycc_at(bgr, W, c, xx < W ? xx : W - 1, yy) - 128;
    }
    return;
  }
  const int rows = (H + g.fv - 1) / g.fv;
  const int yc = y < rows ? y : rows - 1;
  const int r0 = yc * g.fv, r1 = r0 + g.fv - 1 < H ? r0 + g.fv - 1 : H - 1;
  for (int u = 0; u < 8; ++u) {
    const int xc = sbx * 8 + u;
    const int c0 = 2 * xc < W ? 2 * xc : W - 1, c1 = 2 * xc + 1 < W ? 2 * xc + 1 : W - 1;
    int v;
    if (g.fv == 1)
      v = (ycc_at(bgr, W, c, c0, r0) + ycc_at(bgr, W, c, c1, r0) + (xc & 1)) >> 1;
    else
      v = (ycc_at(bgr, W, c, c0, r0) + ycc_at(bgr, W, c, c1, r0) + ycc_at(bgr, W, c, c0, r1) +
           ycc_at(bgr, W, c, c1, r1) + 1 + (xc & 1)) >> 2;
    x[u] = v - 128;
  }
}

RVJ_HD int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// jfdctint.c on eight values: PASS 1 along a row (results scaled up by 4),
// PASS 2 down a column (that scaling removed; the output stays scaled by 8).
template <int PASS>
RVJ_HD void fdct8(int (&d)[8]) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int S = PASS == 1 ? 13 - 2 : 13 + 2;
  if (PASS == 1) {
    d[0] = (t10 + t11) * 4;
    d[4] = (t10 - t11) * 4;
  } else {
    d[0] = descale(t10 + t11, 2);
    d[4] = descale(t10 - t11, 2);
  }
  int z1 = (t12 + t13) * 4433;
  d[2] = descale(z1 + t13 * 6270, S);
  d[6] = descale(z1 - t12 * 15137, S);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = descale(a4 + z1 + z3, S);
  d[5] = descale(a5 + z2 + z4, S);
  d[3] = descale(a6 + z2 + z3, S);
  d[1] = descale(a7 + z1 + z4, S);
}

// DCT output (scaled by 8) / table entry q, rounded half away from zero.
RVJ_HD int quantise(int c, int q) {
  const int d = 8 * q;
  const int a = ((c < 0 ? -c : c) + (d >> 1)) / d;
  return c < 0 ? -a : a;
}

}  // namespace rvjpeg
