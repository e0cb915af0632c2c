// Baseline JPEG marker parser, Huffman decoder and Huffman coder: see jpeg_host.h.
#include "jpeg_host.h"
#include "jpeg_tables.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace rvjpeg {

namespace {

int fail(char* err, int code, const char* fmt, ...) {
  if (err) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, kErrLen, fmt, ap);
    va_end(ap);
  }
  return code;
}

int truncated(char* err) { return fail(err, kTruncated, "JPEG: input ends inside the image"); }

constexpr int kLook = 9;  // bits resolved by one table look-up

struct Huff {
  bool defined = false;
  int nsym = 0;
  uint16_t lut[1 << kLook];  // length << 8 | symbol for codes of <= kLook bits, else 0
  int32_t maxcode[17];       // largest code of each length, -1 when there is none
  int32_t valoff[17];        // symbol index of a code = valoff[length] + code
  uint8_t sym[256];
};

bool build_huff(Huff* h, const uint8_t* counts, const uint8_t* syms, int nsym) {
  memset(h->lut, 0, sizeof(h->lut));
  memcpy(h->sym, syms, (size_t)nsym);
  h->nsym = nsym;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int c = counts[l - 1];
    h->valoff[l] = k - code;
    h->maxcode[l] = c ? code + c - 1 : -1;
    if (code + c > (1 << l)) return false;  // more codes than this length holds
    for (int i = 0; i < c; ++i, ++code, ++k) {
      if (l > kLook) continue;
      const int lo = code << (kLook - l);
      for (int j = 0; j < (1 << (kLook - l)); ++j)
        h->lut[lo + j] = (uint16_t)((l << 8) | syms[k]);
    }
    code <<= 1;
  }
  h->defined = true;
  return true;
}

// Entropy-coded bytes as a bit queue.  Past a marker or the end of the input
// the queue is fed zero bits, counted in `fake`; a decode step that consumed
// any of them ran past the data (checked once per block: nbits < fake).
struct Bits {
  const uint8_t* d;
  size_t n, pos;
  uint64_t acc = 0;
  int nbits = 0, fake = 0;
  int stop = 0;  // 0 reading, 1 pos is at a marker's 0xFF, 2 end of input

  inline void refill() {
    while (nbits <= 56) {
      unsigned b = 0;
      if (stop == 0) {
        if (pos >= n) {
          stop = 2;
        } else if (d[pos] != 0xFF) {
          b = d[pos++];
        } else if (pos + 1 >= n) {
          stop = 2;
        } else if (d[pos + 1] == 0) {
          b = 0xFF;
          pos += 2;
        } else {
          stop = 1;
        }
      }
      if (stop) fake += 8;
      acc = (acc << 8) | b;
      nbits += 8;
    }
  }
  inline unsigned peek16() { return (unsigned)(acc >> (nbits - 16)) & 0xFFFFu; }
  inline int get(int k) {  // k in 1..16, after a refill
    nbits -= k;
    return (int)((acc >> nbits) & ((1u << k) - 1));
  }
  inline bool overran() const { return nbits < fake; }
};

// One Huffman symbol, or -1 for a code that is not in the table.
inline int symbol(Bits& b, const Huff& h) {
  const unsigned p = b.peek16();
  const unsigned e = h.lut[p >> (16 - kLook)];
  if (e) {
    b.nbits -= (int)(e >> 8);
    return (int)(e & 255);
  }
  for (int l = kLook + 1; l <= 16; ++l) {
    const int code = (int)(p >> (16 - l));
    if (code <= h.maxcode[l]) {
      const int i = h.valoff[l] + code;
      if (i < 0 || i >= h.nsym) return -1;
      b.nbits -= l;
      return h.sym[i];
    }
  }
  return -1;
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

struct Comp {
  int id, h, v, tq, td, ta;
};

struct Frame {
  Info info = {0, 0, 0, 0};
  Comp comp[3];
  uint16_t qt[4][64];
  bool qt_defined[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  int restart = 0;
  bool have_sof = false;
  size_t scan_start = 0;  // first entropy-coded byte
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

const char* sof_name(int m) {
  switch (m) {
    case 0xC1: return "extended sequential (SOF1)";
    case 0xC2: return "progressive (SOF2)";
    case 0xC3: return "lossless (SOF3)";
    case 0xC5: case 0xC6: case 0xC7: return "hierarchical (SOF5-7)";
    case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
      return "arithmetic coding (SOF9-15)";
    default: return "unknown frame type";
  }
}

int parse_sof(Frame* f, const uint8_t* p, int len, char* err) {
  if (f->have_sof) return fail(err, kInvalid, "JPEG: second SOF in one image");
  if (len < 6) return fail(err, kInvalid, "JPEG: SOF0 segment too short");
  if (p[0] != 8)
    return fail(err, kInvalid, "JPEG: %d-bit samples not supported (8-bit only)", p[0]);
  const int H = be16(p + 1), W = be16(p + 3), nc = p[5];
  if (nc == 4) return fail(err, kInvalid, "JPEG: 4 components (CMYK / YCCK) not supported");
  if (nc != 1 && nc != 3) return fail(err, kInvalid, "JPEG: %d components not supported", nc);
  if (W <= 0 || H <= 0) return fail(err, kInvalid, "JPEG: size %dx%d not supported", W, H);
  if (len != 6 + 3 * nc) return fail(err, kInvalid, "JPEG: SOF0 length does not match");
  for (int i = 0; i < nc; ++i) {
    Comp& c = f->comp[i];
    c.id = p[6 + 3 * i];
    c.h = p[7 + 3 * i] >> 4;
    c.v = p[7 + 3 * i] & 15;
    c.tq = p[8 + 3 * i];
    if (c.tq > 3) return fail(err, kInvalid, "JPEG: quant table index %d", c.tq);
    if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4)
      return fail(err, kInvalid, "JPEG: sampling factor %dx%d", c.h, c.v);
  }
  int sampling = 3;
  if (nc == 3) {
    const Comp* c = f->comp;
    const bool chroma11 = c[1].h == 1 && c[1].v == 1 && c[2].h == 1 && c[2].v == 1;
    if (chroma11 && c[0].h == 1 && c[0].v == 1) sampling = 0;
    else if (chroma11 && c[0].h == 2 && c[0].v == 1) sampling = 1;
    else if (chroma11 && c[0].h == 2 && c[0].v == 2) sampling = 2;
    else
      return fail(err, kInvalid,
                  "JPEG: sampling factors %dx%d,%dx%d,%dx%d not supported "
                  "(4:4:4, 4:2:2 and 4:2:0 only)",
                  c[0].h, c[0].v, c[1].h, c[1].v, c[2].h, c[2].v);
  } else {
    f->comp[0].h = f->comp[0].v = 1;  // a one-component scan is not interleaved
  }
  f->info = {W, H, sampling, nc};
  f->have_sof = true;
  return kOk;
}

int parse_dqt(Frame* f, const uint8_t* p, int len, char* err) {
  while (len > 0) {
    const int pq = p[0] >> 4, tq = p[0] & 15;
    if (pq != 0) return fail(err, kInvalid, "JPEG: 16-bit quant tables not supported");
    if (tq > 3) return fail(err, kInvalid, "JPEG: quant table index %d", tq);
    if (len < 65) return fail(err, kInvalid, "JPEG: DQT segment too short");
    for (int i = 0; i < 64; ++i) f->qt[tq][kZigzag[i]] = p[1 + i];
    f->qt_defined[tq] = true;
    p += 65;
    len -= 65;
  }
  return kOk;
}

int parse_dht(Frame* f, const uint8_t* p, int len, char* err) {
  while (len > 0) {
    if (len < 17) return fail(err, kInvalid, "JPEG: DHT segment too short");
    const int tc = p[0] >> 4, th = p[0] & 15;
    if (tc > 1 || th > 3) return fail(err, kInvalid, "JPEG: DHT class %d index %d", tc, th);
    int ns = 0;
    for (int i = 0; i < 16; ++i) ns += p[1 + i];
    if (ns > 256 || len < 17 + ns) return fail(err, kInvalid, "JPEG: DHT symbol count %d", ns);
    if (!build_huff(tc ? &f->ac[th] : &f->dc[th], p + 1, p + 17, ns))
      return fail(err, kInvalid, "JPEG: DHT code lengths are not a prefix code");
    p += 17 + ns;
    len -= 17 + ns;
  }
  return kOk;
}

int parse_sos(Frame* f, const uint8_t* p, int len, char* err) {
  if (!f->have_sof) return fail(err, kInvalid, "JPEG: SOS before SOF");
  if (len < 1) return fail(err, kInvalid, "JPEG: SOS segment too short");
  const int ns = p[0], nc = f->info.ncomp;
  if (ns != nc)
    return fail(err, kInvalid,
                "JPEG: multi-scan image not supported (scan has %d of %d components)", ns, nc);
  if (len != 4 + 2 * ns) return fail(err, kInvalid, "JPEG: SOS length does not match");
  for (int i = 0; i < ns; ++i) {
    Comp& c = f->comp[i];
    if (p[1 + 2 * i] != c.id) return fail(err, kInvalid, "JPEG: scan component order");
    c.td = p[2 + 2 * i] >> 4;
    c.ta = p[2 + 2 * i] & 15;
    if (c.td > 3 || c.ta > 3 || !f->dc[c.td].defined || !f->ac[c.ta].defined)
      return fail(err, kInvalid, "JPEG: Huffman table %d/%d not defined", c.td, c.ta);
    if (!f->qt_defined[c.tq]) return fail(err, kInvalid, "JPEG: quant table %d not defined", c.tq);
  }
  const uint8_t* q = p + 1 + 2 * ns;
  if (q[0] != 0 || q[1] != 63 || q[2] != 0)
    return fail(err, kInvalid, "JPEG: spectral selection / approximation in a baseline scan");
  return kOk;
}

// Header segments from data[0] (SOI) up to the SOF (sof_only) or the SOS.
int parse_headers(Frame* f, const uint8_t* d, size_t n, bool sof_only, char* err) {
  if (n < 2) return truncated(err);
  if (d[0] != 0xFF || d[1] != 0xD8) return fail(err, kInvalid, "JPEG: no SOI marker");
  build_huff(&f->dc[0], kDcLumaBits, kDcVals, 12);
  build_huff(&f->dc[1], kDcChromaBits, kDcVals, 12);
  build_huff(&f->ac[0], kAcLumaBits, kAcLumaVals, 162);
  build_huff(&f->ac[1], kAcChromaBits, kAcChromaVals, 162);
  size_t p = 2;
  for (;;) {
    if (p + 2 > n) return truncated(err);
    if (d[p] != 0xFF) return fail(err, kInvalid, "JPEG: expected a marker at byte %zu", p);
    if (d[p + 1] == 0xFF) {  // fill byte
      ++p;
      continue;
    }
    const int m = d[p + 1];
    if (m == 0xD9) return fail(err, kInvalid, "JPEG: EOI before any scan");
    if (m == 0xD8 || m == 0x01 || m == 0 || (m >= 0xD0 && m <= 0xD7))
      return fail(err, kInvalid, "JPEG: marker 0x%02X in the header", m);
    if (p + 4 > n) return truncated(err);
    const int len = be16(d + p + 2);
    if (len < 2) return fail(err, kInvalid, "JPEG: segment length %d", len);
    if (p + 2 + (size_t)len > n) {
      // the announced segment runs past the input: truncation, unless there
      // is no room for it even in a complete file of this size
      return truncated(err);
    }
    const uint8_t* body = d + p + 4;
    const int blen = len - 2;
    int rc = kOk;
    if (m == 0xC0) {
      rc = parse_sof(f, body, blen, err);
      if (rc == kOk && sof_only) return kOk;
    } else if (m == 0xC4) {
      rc = parse_dht(f, body, blen, err);
    } else if (m == 0xDB) {
      rc = parse_dqt(f, body, blen, err);
    } else if (m == 0xDD) {
      if (blen != 2) return fail(err, kInvalid, "JPEG: DRI length");
      f->restart = be16(body);
    } else if (m == 0xDA) {
      rc = parse_sos(f, body, blen, err);
      if (rc == kOk) f->scan_start = p + 2 + (size_t)len;
      return rc;
    } else if (m == 0xCC) {
      return fail(err, kInvalid, "JPEG: arithmetic coding not supported");
    } else if (m >= 0xC1 && m <= 0xCF) {
      return fail(err, kInvalid, "JPEG: %s not supported (baseline SOF0 only)", sof_name(m));
    } else if (m == 0xDC) {
      return fail(err, kInvalid, "JPEG: DNL not supported");
    }  // APPn, COM and the rest: skipped by length
    if (rc != kOk) return rc;
    p += 2 + (size_t)len;
  }
}

// Byte-align after an entropy-coded segment and consume the marker that must
// follow it; returns the marker, or an error code (< 0).
int next_marker(Bits& b, char* err) {
  if (b.nbits - b.fake >= 8)
    return fail(err, kInvalid, "JPEG: entropy data left over before a marker (missing RSTn?)");
  b.acc = 0;
  b.nbits = b.fake = 0;
  if (b.stop == 2) return truncated(err);
  b.stop = 0;
  if (b.pos >= b.n) return truncated(err);
  if (b.d[b.pos] != 0xFF)
    return fail(err, kInvalid, "JPEG: expected a marker at byte %zu (missing RSTn?)", b.pos);
  while (b.pos < b.n && b.d[b.pos] == 0xFF) ++b.pos;
  if (b.pos >= b.n) return truncated(err);
  return b.d[b.pos++];
}

}  // namespace

int layout(int W, int H, int sampling, Layout* out) {
  if (!out || W < 1 || H < 1 || W > 65535 || H > 65535 || sampling < 0 || sampling > 3)
    return kInvalid;
  const int hs = sampling == 1 || sampling == 2 ? 2 : 1, vs = sampling == 2 ? 2 : 1;
  const int mx = (W + 8 * hs - 1) / (8 * hs), my = (H + 8 * vs - 1) / (8 * vs);
  Layout l;
  memset(&l, 0, sizeof(l));
  l.ncomp = sampling == 3 ? 1 : 3;
  l.qt_off = kHeaderBytes;
  size_t off = l.qt_off + (size_t)l.ncomp * 128;
  for (int c = 0; c < l.ncomp; ++c) {
    l.blocks_w[c] = c == 0 ? mx * hs : mx;
    l.blocks_h[c] = c == 0 ? my * vs : my;
    l.coef_off[c] = off;
    off += (size_t)l.blocks_w[c] * l.blocks_h[c] * 128;
  }
  l.record_bytes = off;
  *out = l;
  return kOk;
}

int frame_extent(const uint8_t* d, size_t n, size_t* begin, size_t* end, char* err) {
  size_t p = 0;
  while (p + 1 < n && !(d[p] == 0xFF && d[p + 1] == 0xD8)) ++p;
  if (p + 1 >= n) {
    *begin = n > 0 && d[n - 1] == 0xFF ? n - 1 : n;
    return truncated(err);
  }
  *begin = p;
  p += 2;
  bool in_scan = false;
  for (;;) {
    if (in_scan) {  // entropy-coded bytes run to the next marker
      while (p < n && d[p] != 0xFF) ++p;
    }
    if (p + 2 > n) return truncated(err);
    if (d[p] != 0xFF)
      return fail(err, kInvalid, "JPEG: expected a marker at byte %zu of the image", p - *begin);
    const int m = d[p + 1];
    if (m == 0xFF) {
      ++p;
      continue;
    }
    if (in_scan && (m == 0 || (m >= 0xD0 && m <= 0xD7))) {
      p += 2;
      continue;
    }
    if (m == 0xD9) {
      *end = p + 2;
      return kOk;
    }
    if (m == 0xD8 || m == 0 || m == 0x01 || (m >= 0xD0 && m <= 0xD7))
      return fail(err, kInvalid, "JPEG: marker 0x%02X in the header", m);
    if (p + 4 > n) return truncated(err);
    const int len = be16(d + p + 2);
    if (len < 2) return fail(err, kInvalid, "JPEG: segment length %d", len);
    if (p + 2 + (size_t)len > n) return truncated(err);
    p += 2 + (size_t)len;
    in_scan = m == 0xDA;
  }
}

int probe(const uint8_t* data, size_t n, Info* info, char* err) {
  if (!data || !info) return fail(err, kInvalid, "JPEG: null pointer");
  Frame* f = new Frame();
  const int rc = parse_headers(f, data, n, true, err);
  if (rc == kOk) *info = f->info;
  delete f;
  return rc;
}

namespace {

int decode_scan(const Frame& f, const uint8_t* data, size_t n, uint8_t* record, const Layout& lay,
                char* err) {
  const int nc = f.info.ncomp;
  Bits b;
  b.d = data;
  b.n = n;
  b.pos = f.scan_start;
  int pred[3] = {0, 0, 0};
  const int mx = lay.blocks_w[0] / f.comp[0].h, my = lay.blocks_h[0] / f.comp[0].v;
  const long total = (long)mx * my;
  long mcu = 0;
  int rst = 0;
  for (int yy = 0; yy < my; ++yy) {
    for (int xx = 0; xx < mx; ++xx, ++mcu) {
      if (f.restart && mcu && mcu % f.restart == 0) {
        const int m = next_marker(b, err);
        if (m < 0) return m;
        if (m != 0xD0 + (rst & 7))
          return fail(err, kInvalid, "JPEG: missing RST%d (found marker 0x%02X)", rst & 7, m);
        ++rst;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < nc; ++c) {
        const Comp& cp = f.comp[c];
        const Huff& hd = f.dc[cp.td];
        const Huff& ha = f.ac[cp.ta];
        int16_t* plane = reinterpret_cast<int16_t*>(record + lay.coef_off[c]);
        for (int j = 0; j < cp.h * cp.v; ++j) {
          const size_t bi = (size_t)(yy * cp.v + j / cp.h) * lay.blocks_w[c] + xx * cp.h + j % cp.h;
          int16_t* blk = plane + bi * 64;
          b.refill();
          int s = symbol(b, hd);
          if (s < 0) return fail(err, kInvalid, "JPEG: Huffman code not in the DC table");
          if (s > 15) return fail(err, kInvalid, "JPEG: DC size %d", s);
          if (s) {
            b.refill();
            pred[c] += extend(b.get(s), s);
          }
          if (pred[c] < -32768 || pred[c] > 32767)
            return fail(err, kInvalid, "JPEG: DC coefficient out of range");
          blk[0] = (int16_t)pred[c];
          int k = 1;
          while (k < 64) {
            b.refill();  // >= 57 bits: one symbol (<= 16) and its value (<= 15)
            const int rs = symbol(b, ha);
            if (rs < 0) return fail(err, kInvalid, "JPEG: Huffman code not in the AC table");
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;  // end of block
              k += 16;
              continue;
            }
            k += r;
            if (k > 63) return fail(err, kInvalid, "JPEG: run past coefficient 63");
            blk[kZigzag[k]] = (int16_t)extend(b.get(s), s);
            ++k;
          }
          if (k > 64) return fail(err, kInvalid, "JPEG: run past coefficient 63");
          if (b.overran())
            return b.stop == 2 ? truncated(err)
                               : fail(err, kInvalid, "JPEG: entropy data ends before MCU %ld of %ld",
                                      mcu, total);
        }
      }
    }
  }
  const int m = next_marker(b, err);
  if (m < 0) return m;
  if (m == 0xDA || m == 0xC4 || m == 0xDB)
    return fail(err, kInvalid, "JPEG: multi-scan image not supported");
  if (m != 0xD9) return fail(err, kInvalid, "JPEG: expected EOI, found marker 0x%02X", m);
  return kOk;
}

}  // namespace

int decode(const uint8_t* data, size_t n, uint8_t* record, size_t cap, const Info* expect,
           char* err) {
  if (!data || !record) return fail(err, kInvalid, "JPEG: null pointer");
  Frame* f = new Frame();
  int rc = parse_headers(f, data, n, false, err);
  Layout lay;
  if (rc == kOk && layout(f->info.W, f->info.H, f->info.sampling, &lay) != kOk)
    rc = fail(err, kInvalid, "JPEG: size %dx%d", f->info.W, f->info.H);
  if (rc == kOk && expect &&
      (expect->W != f->info.W || expect->H != f->info.H || expect->sampling != f->info.sampling))
    rc = fail(err, kInvalid, "JPEG: size or sampling changed: %dx%d code %d, expected %dx%d code %d",
              f->info.W, f->info.H, f->info.sampling, expect->W, expect->H, expect->sampling);
  if (rc == kOk && cap < lay.record_bytes)
    rc = fail(err, kInvalid, "JPEG: record needs %zu bytes, %zu given", lay.record_bytes, cap);
  if (rc == kOk) {
    memset(record, 0, lay.record_bytes);
    int32_t hdr[8] = {(int32_t)kMagic, f->info.W, f->info.H, f->info.sampling, f->info.ncomp,
                      0, 0, 0};
    memcpy(record, hdr, sizeof(hdr));
    for (int c = 0; c < f->info.ncomp; ++c)
      memcpy(record + lay.qt_off + (size_t)c * 128, f->qt[f->comp[c].tq], 128);
    rc = decode_scan(*f, data, n, record, lay, err);
  }
  delete f;
  return rc;
}

// ---- encoder half ---------------------------------------------------------

void quant_tables(int quality, uint16_t luma[64], uint16_t chroma[64]) {
  const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  for (int i = 0; i < 64; ++i) {
    const int l = (kQuantLuma[i] * scale + 50) / 100, c = (kQuantChroma[i] * scale + 50) / 100;
    luma[i] = (uint16_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
    chroma[i] = (uint16_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
  }
}

size_t image_bound(int W, int H, int sampling) {
  Layout l;
  if (layout(W, H, sampling, &l) != kOk) return 0;
  size_t blocks = 0;
  for (int c = 0; c < l.ncomp; ++c) blocks += (size_t)l.blocks_w[c] * l.blocks_h[c];
  return (size_t)kFileHeaderMax + blocks * (2 * ((kBlockBitsMax + 7) / 8)) +
         (size_t)l.blocks_h[l.ncomp - 1] * 4 + 2;
}

namespace {

constexpr HuffEnc kHuffEnc = make_huff_enc();

// Bounded byte sink: counts every byte, stores those that fit.
struct Out {
  uint8_t* o;
  size_t cap, n = 0;
  inline void byte(unsigned b) {
    if (n < cap) o[n] = (uint8_t)b;
    ++n;
  }
  inline void be16(unsigned v) {
    byte(v >> 8);
    byte(v & 255);
  }
  inline void marker(unsigned m, unsigned len) {
    byte(0xFF);
    byte(m);
    be16(len);
  }
};

// Entropy-coded bits, MSB first, 0x00 stuffed after every 0xFF byte.
struct PutBits {
  Out* out;
  uint64_t acc = 0;
  int cnt = 0;
  inline void put(uint32_t v, int k) {  // k <= 32, v < 2^k
    acc = (acc << k) | v;
    cnt += k;
    while (cnt >= 8) {
      const unsigned b = (unsigned)(acc >> (cnt - 8)) & 255;
      out->byte(b);
      if (b == 0xFF) out->byte(0);
      cnt -= 8;
    }
  }
  inline void align() {  // pad the last byte with 1-bits
    if (cnt) put((1u << (8 - cnt)) - 1, 8 - cnt);
  }
};

inline int category(int a) {  // bits of |v|
  int s = 0;
  while (a) {
    ++s;
    a >>= 1;
  }
  return s;
}

void write_dht(Out& o, int tc_th, const uint8_t* counts, const uint8_t* syms, int nsym) {
  o.marker(0xC4, 2 + 1 + 16 + nsym);
  o.byte(tc_th);
  for (int i = 0; i < 16; ++i) o.byte(counts[i]);
  for (int i = 0; i < nsym; ++i) o.byte(syms[i]);
}

}  // namespace

int write_header(int W, int H, int sampling, const uint16_t* luma, const uint16_t* chroma,
                 int restart_interval_mcus, uint8_t* out, size_t cap, size_t* n, char* err) {
  Layout lay;
  if (!out || !n || !luma || (sampling != 3 && !chroma))
    return fail(err, kInvalid, "JPEG: null pointer");
  if (layout(W, H, sampling, &lay) != kOk)
    return fail(err, kInvalid, "JPEG: size %dx%d, sampling code %d", W, H, sampling);
  if (restart_interval_mcus < 0 || restart_interval_mcus > 65535)
    return fail(err, kInvalid, "JPEG: restart interval %d", restart_interval_mcus);
  const int nc = lay.ncomp;
  for (int t = 0; t < (nc == 1 ? 1 : 2); ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = (t ? chroma : luma)[i];
      if (v < 1 || v > 255)
        return fail(err, kInvalid, "JPEG: quant table entry %d is not baseline (1..255)", v);
    }
  Out o{out, cap};
  o.byte(0xFF);
  o.byte(0xD8);
  o.marker(0xE0, 16);  // JFIF 1.01, no units, density 1 x 1, no thumbnail
  const uint8_t jfif[12] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1};
  for (int i = 0; i < 12; ++i) o.byte(jfif[i]);
  o.byte(0);
  o.byte(0);
  for (int t = 0; t < (nc == 1 ? 1 : 2); ++t) {
    o.marker(0xDB, 67);
    o.byte(t);
    for (int i = 0; i < 64; ++i) o.byte((t ? chroma : luma)[kZigzag[i]]);
  }
  o.marker(0xC0, 8 + 3 * nc);
  o.byte(8);
  o.be16(H);
  o.be16(W);
  o.byte(nc);
  const int hs = sampling == 1 || sampling == 2 ? 2 : 1, vs = sampling == 2 ? 2 : 1;
  for (int c = 0; c < nc; ++c) {
    o.byte(c + 1);
    o.byte(c == 0 ? (hs << 4) | vs : 0x11);
    o.byte(c == 0 ? 0 : 1);
  }
  write_dht(o, 0x00, kDcLumaBits, kDcVals, 12);
  write_dht(o, 0x10, kAcLumaBits, kAcLumaVals, 162);
  if (nc == 3) {
    write_dht(o, 0x01, kDcChromaBits, kDcVals, 12);
    write_dht(o, 0x11, kAcChromaBits, kAcChromaVals, 162);
  }
  if (restart_interval_mcus) {
    o.marker(0xDD, 4);
    o.be16(restart_interval_mcus);
  }
  o.marker(0xDA, 6 + 2 * nc);
  o.byte(nc);
  for (int c = 0; c < nc; ++c) {
    o.byte(c + 1);
    o.byte(c == 0 ? 0x00 : 0x11);
  }
  o.byte(0);
  o.byte(63);
  o.byte(0);
  *n = o.n;
  if (o.n > cap) return fail(err, kInvalid, "JPEG: header needs %zu bytes, %zu given", o.n, cap);
  return kOk;
}

int encode(const uint8_t* record, size_t record_bytes, int restart_interval_mcus, uint8_t* out,
           size_t cap, size_t* n, char* err) {
  if (!record || !out || !n) return fail(err, kInvalid, "JPEG: null pointer");
  if (record_bytes < (size_t)kHeaderBytes) return fail(err, kInvalid, "JPEG: record too short");
  int32_t hdr[8];
  memcpy(hdr, record, sizeof(hdr));
  Layout lay;
  if ((uint32_t)hdr[0] != kMagic || layout(hdr[1], hdr[2], hdr[3], &lay) != kOk ||
      hdr[4] != lay.ncomp)
    return fail(err, kInvalid, "JPEG: not a coefficient record");
  if (record_bytes < lay.record_bytes)
    return fail(err, kInvalid, "JPEG: record needs %zu bytes, %zu given", lay.record_bytes,
                record_bytes);
  const int nc = lay.ncomp, sampling = hdr[3];
  uint16_t qt[3][64];
  memcpy(qt, record + lay.qt_off, (size_t)nc * 128);
  if (nc == 3 && memcmp(qt[1], qt[2], 128) != 0)
    return fail(err, kInvalid, "JPEG: Cb and Cr use different quant tables");
  size_t hn = 0;
  int rc = write_header(hdr[1], hdr[2], sampling, qt[0], qt[nc == 3 ? 1 : 0],
                        restart_interval_mcus, out, cap, &hn, err);
  if (rc != kOk) return rc;
  Out o{out, cap};
  o.n = hn;
  PutBits pb{&o};
  const int hs = sampling == 1 || sampling == 2 ? 2 : 1, vs = sampling == 2 ? 2 : 1;
  const int mx = lay.blocks_w[0] / hs, my = lay.blocks_h[0] / vs;
  int pred[3] = {0, 0, 0};
  long mcu = 0;
  int rst = 0;
  for (int yy = 0; yy < my; ++yy) {
    for (int xx = 0; xx < mx; ++xx, ++mcu) {
      if (restart_interval_mcus && mcu && mcu % restart_interval_mcus == 0) {
        pb.align();
        o.byte(0xFF);
        o.byte(0xD0 + (rst++ & 7));
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < nc; ++c) {
        const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1, t = c == 0 ? 0 : 1;
        for (int j = 0; j < ch * cv; ++j) {
          const size_t bi = (size_t)(yy * cv + j / ch) * lay.blocks_w[c] + xx * ch + j % ch;
          int16_t blk[64];
          memcpy(blk, record + lay.coef_off[c] + bi * 128, 128);
          const int diff = blk[0] - pred[c];
          pred[c] = blk[0];
          int s = category(diff < 0 ? -diff : diff);
          if (s > 11) return fail(err, kInvalid, "JPEG: DC difference %d has no baseline code", diff);
          uint32_t e = kHuffEnc.dc[t][s];
          pb.put(e & 0xFFFF, (int)(e >> 16));
          if (s) pb.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
          int run = 0;
          for (int k = 1; k < 64; ++k) {
            const int v = blk[kZigzag[k]];
            if (v == 0) {
              ++run;
              continue;
            }
            for (; run >= 16; run -= 16) {
              e = kHuffEnc.ac[t][0xF0];
              pb.put(e & 0xFFFF, (int)(e >> 16));
            }
            s = category(v < 0 ? -v : v);
            if (s > 10) return fail(err, kInvalid, "JPEG: coefficient %d has no baseline code", v);
            e = kHuffEnc.ac[t][(run << 4) | s];
            pb.put(e & 0xFFFF, (int)(e >> 16));
            pb.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
            run = 0;
          }
          if (run) {
            e = kHuffEnc.ac[t][0];
            pb.put(e & 0xFFFF, (int)(e >> 16));
          }
        }
      }
    }
  }
  pb.align();
  o.byte(0xFF);
  o.byte(0xD9);
  *n = o.n;
  if (o.n > cap) return fail(err, kInvalid, "JPEG: image needs %zu bytes, %zu given", o.n, cap);
  return kOk;
}

}  // namespace rvjpeg
