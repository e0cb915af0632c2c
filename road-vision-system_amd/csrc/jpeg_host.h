// Baseline JPEG on the host: marker parser and Huffman decoder (ITU-T T.81).
// Host only -- no HIP, no Python -- so it also builds alone for the sanitizer
// program tools/jpeg_host_check.cpp.  The device half (dequantise, IDCT,
// upsample, colour) is csrc/jpeg.hip; between the two travels the coefficient
// record documented in include/rvhip.h (RV_JPEG_*).
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

}  // namespace rvjpeg
