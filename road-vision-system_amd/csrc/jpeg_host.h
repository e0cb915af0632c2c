// Baseline JPEG on the host: marker parser and Huffman decoder (ITU-T T.81),
// and their inverse: quant tables, file header and Huffman coder.
// Host only -- no HIP, no Python -- so it also builds alone for the sanitizer
// program tools/jpeg_host_check.cpp.  The device halves are csrc/jpeg.hip
// (dequantise, IDCT, upsample, colour) and csrc/jpeg_enc.hip (colour,
// downsample, DCT, quantise, entropy coding); between host and device travels
// the coefficient record documented in include/rvhip.h (RV_JPEG_*).
//
// Supported: SOF0, 8-bit, Huffman, one interleaved scan; three components
// with Y 1x1 / 2x1 / 2x2 and Cb, Cr 1x1, or one component; DRI / RSTn;
// Annex K tables when a frame carries no DHT.  Everything else is an error
// with its cause in `err`.  Every read of the input is bounds-checked.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rvjpeg {

constexpr int kOk = 0;
constexpr int kInvalid = -1;    // corrupt or unsupported: cause in err
constexpr int kTruncated = -2;  // the input ended inside the image
constexpr int kErrLen = 200;

constexpr uint32_t kMagic = 0x46434a52u;  // "RJCF"
constexpr int kHeaderBytes = 32;          // int32[8]: magic, W, H, sampling, ncomp, 0, 0, 0

struct Info {
  int W, H, sampling, ncomp;  // sampling: RV_JPEG_444 / 422 / 420 / GRAY (0..3)
};

struct Layout {
  size_t record_bytes;
  int ncomp;
  size_t qt_off;       // u16[ncomp][64], natural order
  size_t coef_off[3];  // int16[blocks_h][blocks_w][64], natural order
  int blocks_w[3], blocks_h[3];
};

// Record layout of a W x H image: kInvalid for a bad size or sampling code.
int layout(int W, int H, int sampling, Layout* out);

// [*begin, *end) of the first image (SOI .. EOI inclusive) in data[0, n):
// kOk, kTruncated when more bytes are needed (*begin is then the SOI, or n
// when there is none), kInvalid for a broken segment.
int frame_extent(const uint8_t* data, size_t n, size_t* begin, size_t* end, char* err);

// Size and sampling of the image that starts at data[0] (SOI).
int probe(const uint8_t* data, size_t n, Info* info, char* err);

// Entropy-decode the image at data[0] into a coefficient record of at most
// `cap` bytes.  `expect`, when not null, is the size and sampling the image
// must have.  The record is complete only when kOk is returned.
int decode(const uint8_t* data, size_t n, uint8_t* record, size_t cap, const Info* expect,
           char* err);

// ---- The way back: what libjpeg writes with its default settings ---------
// (jpeg_set_quality with force_baseline, the Annex K Huffman tables, JFIF
// 1.01 APP0 with density 1x1 and no units).

constexpr int kFileHeaderMax = 640;  // SOI .. SOS of a three-component image is 629 bytes

// Annex K.1 / K.2 scaled as jpeg_quality_scaling does (quality 1..100, clamped
// to that range), entries clamped to 1..255; natural order.
void quant_tables(int quality, uint16_t luma[64], uint16_t chroma[64]);

// SOI, APP0, DQT (one per table), SOF0, DHT (one per table), DRI when
// restart_interval_mcus > 0, SOS: *n bytes into out[0, cap).  chroma is not
// read for RV_JPEG_GRAY.
int write_header(int W, int H, int sampling, const uint16_t* luma, const uint16_t* chroma,
                 int restart_interval_mcus, uint8_t* out, size_t cap, size_t* n, char* err);

// A coefficient record (as decode() fills it) -> a complete image, *n bytes
// into out[0, cap): the inverse of decode() for images that use the Annex K
// Huffman tables.  The quant tables come from the record (component 0's as
// table 0, component 1's as table 1; component 2 must use component 1's).
// restart_interval_mcus = 0 writes no DRI and no RSTn.  kInvalid for a record
// that is malformed, holds a value baseline JPEG has no code for, or does
// not fit `cap`.
int encode(const uint8_t* record, size_t record_bytes, int restart_interval_mcus, uint8_t* out,
           size_t cap, size_t* n, char* err);

// Most bytes the image of one W x H frame can take when every MCU row is its
// own restart segment (the device encoder's form), 0 for a bad size or code:
//   kFileHeaderMax
//   + blocks x 416   a block is at most kBlockBitsMax = 1660 bits (11-bit DC
//                    code + 11 value bits, 63 x (16-bit AC code + 10 value
//                    bits)), 208 bytes, each possibly 0xFF and then stuffed
//   + MCU rows x 4   the padded last byte of a segment, stuffed, and its RSTn
//   + 2              EOI
size_t image_bound(int W, int H, int sampling);

}  // namespace rvjpeg
