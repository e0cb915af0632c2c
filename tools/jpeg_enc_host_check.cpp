// The host JPEG coder (csrc/jpeg_host.cpp: decode, write_header, encode)
// under sanitizers.  Stand-alone: no HIP, no Python.  Every .jpg fixture of
// the given directories goes through decode -> encode with the file's own
// restart interval; a file that uses the Annex K Huffman tables must come
// back byte for byte ("_opt", "_nodht" and "reject_" files are only required
// to return).  The output buffer is an exact-size heap block, and is tried
// one byte short too, so AddressSanitizer sees any write past the capacity.
// Records with flipped bytes follow: encode must return, never crash.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I road-vision-system_amd/csrc tools/jpeg_enc_host_check.cpp \
//       road-vision-system_amd/csrc/jpeg_host.cpp -o /tmp/jpeg_enc_host_check
//   /tmp/jpeg_enc_host_check tests/golden/jpeg tests/golden/jpeg_enc
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "jpeg_host.h"

namespace {

// The DRI value of the image's header, 0 when it has none.
int restart_interval(const std::vector<uint8_t>& d) {
  size_t p = 2;
  while (p + 4 <= d.size() && d[p] == 0xFF) {
    const int m = d[p + 1], len = (d[p + 2] << 8) | d[p + 3];
    if (m == 0xDD && p + 6 <= d.size()) return (d[p + 4] << 8) | d[p + 5];
    if (m == 0xDA) break;
    p += 2 + (size_t)len;
  }
  return 0;
}

uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <directory of .jpg fixtures> ...\n", argv[0]);
    return 2;
  }
  int files = 0, equal = 0, bad = 0;
  long mutated = 0;
  for (int a = 1; a < argc; ++a) {
    DIR* dir = opendir(argv[a]);
    if (!dir) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<std::string> names;
    while (dirent* e = readdir(dir)) {
      const std::string s = e->d_name;
      if (s.size() > 4 && s.rfind(".jpg") == s.size() - 4) names.push_back(s);
    }
    closedir(dir);
    for (const std::string& name : names) {
      const std::string path = std::string(argv[a]) + "/" + name;
      FILE* f = fopen(path.c_str(), "rb");
      if (!f) return 2;
      std::vector<uint8_t> bytes;
      uint8_t chunk[4096];
      for (size_t got; (got = fread(chunk, 1, sizeof(chunk), f)) > 0;)
        bytes.insert(bytes.end(), chunk, chunk + got);
      fclose(f);
      ++files;
      char err[rvjpeg::kErrLen] = "";
      rvjpeg::Info info;
      rvjpeg::Layout lay;
      const bool must_match = name.find("_opt") == std::string::npos &&
                              name.find("_nodht") == std::string::npos &&
                              name.rfind("reject_", 0) != 0;
      if (rvjpeg::probe(bytes.data(), bytes.size(), &info, err) != rvjpeg::kOk ||
          rvjpeg::layout(info.W, info.H, info.sampling, &lay) != rvjpeg::kOk) {
        if (must_match) {
          fprintf(stderr, "%s: %s\n", name.c_str(), err);
          ++bad;
        }
        continue;
      }
      uint8_t* rec = (uint8_t*)malloc(lay.record_bytes);  // exact size: no slack
      if (rvjpeg::decode(bytes.data(), bytes.size(), rec, lay.record_bytes, nullptr, err) !=
          rvjpeg::kOk) {
        if (must_match) {
          fprintf(stderr, "%s: %s\n", name.c_str(), err);
          ++bad;
        }
        free(rec);
        continue;
      }
      const int ri = restart_interval(bytes);
      uint8_t* out = (uint8_t*)malloc(bytes.size());
      size_t n = 0;
      const int rc = rvjpeg::encode(rec, lay.record_bytes, ri, out, bytes.size(), &n, err);
      const bool same = rc == rvjpeg::kOk && n == bytes.size() && !memcmp(out, bytes.data(), n);
      if (same) ++equal;
      if (must_match && !same) {
        fprintf(stderr, "%s: encode(decode(file)) differs from the file (%zu / %zu bytes) %s\n",
                name.c_str(), n, bytes.size(), rc == rvjpeg::kOk ? "" : err);
        ++bad;
      }
      free(out);
      if (same) {  // one byte short: an error, and nothing written past the block
        out = (uint8_t*)malloc(bytes.size() - 1);
        if (rvjpeg::encode(rec, lay.record_bytes, ri, out, bytes.size() - 1, &n, err) !=
            rvjpeg::kInvalid) {
          fprintf(stderr, "%s: a short buffer was not refused\n", name.c_str());
          ++bad;
        }
        free(out);
        for (size_t cap : {(size_t)0, (size_t)1, (size_t)100, (size_t)640}) {
          out = (uint8_t*)malloc(cap ? cap : 1);
          (void)rvjpeg::encode(rec, lay.record_bytes, ri, out, cap, &n, err);
          free(out);
        }
      }
      // damaged records: any answer will do
      uint32_t seed = (uint32_t)bytes.size() * 2654435761u + 7u;
      out = (uint8_t*)malloc(rvjpeg::image_bound(info.W, info.H, info.sampling) + 1);
      const size_t cap = rvjpeg::image_bound(info.W, info.H, info.sampling);
      for (int i = 0; i < 200; ++i) {
        uint8_t* m = (uint8_t*)malloc(lay.record_bytes);
        memcpy(m, rec, lay.record_bytes);
        const int flips = 1 + (int)(lcg(seed) % 8);
        for (int k = 0; k < flips; ++k) {
          const size_t at = i < 40 ? lcg(seed) % (lay.qt_off + 128) : lcg(seed) % lay.record_bytes;
          m[at] = (uint8_t)(lcg(seed) >> 24);
        }
        (void)rvjpeg::encode(m, i % 5 == 4 ? lay.record_bytes - 1 : lay.record_bytes,
                             (int)(lcg(seed) % 3) * ri, out, cap, &n, err);
        free(m);
        ++mutated;
      }
      free(out);
      free(rec);
    }
  }
  printf("%d fixtures, %d equal after decode -> encode, %ld damaged records, %d unexpected\n",
         files, equal, mutated, bad);
  return bad ? 1 : 0;
}
