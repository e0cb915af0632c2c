// The conv launcher's accept set, as text: for a grid of layers, which of
// every ConvCfg rv::conv_cfg_ok accepts and what rv::conv_candidates lists.
// Two builds of the library accept the same configurations exactly when
// their outputs are byte-equal (profiles/r11/conv_split/accept_set.txt is the
// --digest output at the conv.hip split, with the SHA-256 of the full one;
// both equal the parent's).  Host arithmetic only: no HIP call is made, so it
// runs without a GPU.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 tools/conv_accept_set.cpp \
//       -L road-vision-system_amd/rvs_amd -lrvhip -o /tmp/conv_accept_set
//   LD_LIBRARY_PATH=road-vision-system_amd/rvs_amd /tmp/conv_accept_set --digest > accept_set.txt
//
// One line per layer: its description, the number of accepted configurations
// and an FNV-1a digest of the accept bits (mr 1..9 x nr 1..5 x G in {1, 2,
// nch, nch + 1} x resw x persist x kind -1..3, in that nesting), then the
// candidates as mr,nr,G,resw,persist,kind.  Then one line per patch-kernel
// variant (waves, fp8, chained, tile, k, s, weights) some layer accepted, with
// the number of accepting configurations: the variants the grid can reach.
// With --digest (the committed form) the layer lines are folded into one per
// kernel size, stride and map: layers, accepted configurations, candidates
// listed and a digest of the full lines; the variants are grouped by tile.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../road-vision-system_amd/csrc/conv.h"

using rv::ConvArgs;
using rv::ConvCfg;

namespace {

struct Fnv {
  unsigned long long h = 1469598103934665603ull;
  void add(unsigned v) {
    h = (h ^ (v & 0xFF)) * 1099511628211ull;
  }
};

alignas(64) char g_dummy[64];  // a non-null pointer no host code dereferences
bool g_digest = false;
long g_layers = 0, g_empty = 0;
std::map<std::string, long> g_variants;
struct Fold {  // --digest: the layer lines of one k, stride and map
  Fnv f;
  long layers = 0, accepted = 0, listed = 0;
} g_fold;

void layer_line(const char* tag, const ConvArgs& a) {
  const int cc = a.in8 ? 64 : 32;
  int cin = a.Cin;
  if (a.g2_cout0 > 0 && a.g2_Cin > cin) cin = a.g2_Cin;
  const int nch = (cin + cc - 1) / cc;
  const int Gs[4] = {1, 2, nch, nch + 1};
  Fnv f;
  long accepted = 0;
  for (int mr = 1; mr <= 9; ++mr)
    for (int nr = 1; nr <= 5; ++nr)
      for (int G : Gs)
        for (int resw = 0; resw <= 1; ++resw)
          for (int persist = 0; persist <= 1; ++persist)
            for (int kind = -1; kind <= 3; ++kind) {
              const bool ok = rv::conv_cfg_ok(a, ConvCfg{mr, nr, G, resw, persist, kind});
              f.add(ok ? 1 : 0);
              accepted += ok;
              if (ok && kind != 1) {
                char v[96];
                snprintf(v, sizeof(v), "%d waves %s%s MR=%d NR=%d k%d s%d %s", kind == 2 ? 8 : 4,
                         a.in8 ? "fp8" : "bf16", a.ch_w ? " chained" : "", mr, nr, a.k, a.stride,
                         resw ? "resident" : "staged");
                ++g_variants[v];
              }
            }
  static ConvCfg cand[1024];
  const int n = rv::conv_candidates(a, cand, 1024);
  ++g_layers;
  if (!accepted && !n) ++g_empty;
  char line[128];
  std::string full;
  snprintf(line, sizeof(line), "k%d s%d %dx%d %d->%d B%d cs%d %s: %ld %016llx | %d", a.k, a.stride, a.Hin,
           a.Win, a.Cin, a.Cout, a.B, a.out0_cs, tag, accepted, f.h, n);
  full = line;
  for (int i = 0; i < n && i < 1024; ++i) {
    snprintf(line, sizeof(line), " %d,%d,%d,%d,%d,%d", cand[i].mr, cand[i].nr, cand[i].G, cand[i].resw,
             cand[i].persist, cand[i].kind);
    full += line;
  }
  if (!g_digest) {
    printf("%s\n", full.c_str());
    return;
  }
  for (char ch : full) g_fold.f.add((unsigned char)ch);
  g_fold.f.add('\n');
  ++g_fold.layers;
  g_fold.accepted += accepted;
  g_fold.listed += n;
}

}  // namespace

int main(int argc, char** argv) {
  g_digest = argc > 1 && !strcmp(argv[1], "--digest");
  const int maps[][2] = {{1, 1}, {3, 5}, {7, 10}, {17, 6}, {80, 80}, {4097, 4096}};  // the last: >= 2^24 pixels
  const int chans[][2] = {{8, 16}, {16, 16}, {48, 80}, {64, 64}, {96, 640}, {1280, 64}, {64, 144}};
  const rv::bf16_t* p = (const rv::bf16_t*)g_dummy;
  for (int k : {1, 3})
    for (int stride : {1, 2})
      for (const auto& m : maps) {
        g_fold = Fold();
        for (const auto& ch : chans)
          for (int B : {1, 32})
            for (int wide : {0, 1}) {
              ConvArgs a;
              memset(&a, 0, sizeof(a));
              a.in = p;
              a.w = p;
              a.bias = (const float*)g_dummy;
              a.Hin = m[0];
              a.Win = m[1];
              a.Cin = ch[0];
              a.in_cs = 2 * ch[0];  // room for a second group's slice
              a.Cout = ch[1];
              a.k = k;
              a.stride = stride;
              a.pad = k / 2;
              a.Ho = (a.Hin + 2 * a.pad - k) / stride + 1;
              a.Wo = (a.Win + 2 * a.pad - k) / stride + 1;
              a.B = B;
              a.out0 = g_dummy;
              a.out0_cs = wide ? 2048 : a.Cout;
              a.act = 1;
              auto with_res = [&](ConvArgs& x) {
                x.res = p;
                x.res_cs = x.Cout;
              };
              auto with_out1 = [&](ConvArgs& x) {
                x.out1 = g_dummy;
                x.out1_cs = x.Cout;
              };
              auto with_in8 = [&](ConvArgs& x) {
                x.in8 = 1;
                x.s_in = x.s_res = x.s_out0 = x.s_out1 = 1.f;
                x.wscale = x.g2_wscale = (const float*)g_dummy;
              };
              auto with_g2 = [&](ConvArgs& x, int cout0) {
                x.g2_cout0 = cout0;
                x.g2_in_co = x.Cin;
                x.g2_Cin = x.Cin;
                x.g2_w = p;
                x.g2_bias = (const float*)g_dummy;
              };
              layer_line("plain", a);
              ConvArgs x = a;
              with_res(x);
              layer_line("res", x);
              x = a;
              with_out1(x);
              layer_line("out1", x);
              x = a;
              x.out0_up = 1;
              layer_line("up", x);
              x = a;
              with_res(x);
              with_out1(x);
              x.out0_up = 1;
              layer_line("res+out1+up", x);
              x = a;
              with_in8(x);
              layer_line("in8", x);
              with_res(x);
              x.out0_8 = 1;
              layer_line("in8+res+out8", x);
              for (int cout0 : {64, 80}) {
                x = a;
                with_g2(x, cout0);
                layer_line(cout0 == 64 ? "g2_64" : "g2_80", x);
                with_in8(x);
                layer_line(cout0 == 64 ? "g2_64+in8" : "g2_80+in8", x);
              }
              for (int cout : {52, 64, 68}) {  // chained 1x1 behind this conv
                x = a;
                x.Cout = cout;
                if (!wide) x.out0_cs = cout;
                x.ch_w = p;
                x.ch_b = (const float*)g_dummy;
                layer_line(cout == 52 ? "ch52" : cout == 64 ? "ch64" : "ch68", x);
                with_res(x);
                layer_line(cout == 52 ? "ch52+res" : cout == 64 ? "ch64+res" : "ch68+res", x);
              }
              x = a;  // virtual concat inputs of the direct 1x1 kernel
              x.in_up = 1;
              layer_line("in_up", x);
              x.split = x.Cin;
              layer_line("in_up+split=Cin", x);
              x = a;
              x.split = 32;
              layer_line("split32", x);
              x.in2 = p;
              x.in2_cs = x.Cin;
              layer_line("split32+in2", x);
              x.in_up = 1;
              layer_line("split32+in2+in_up", x);
            }
        if (g_digest)
          printf("k%d s%d %dx%d: layers %ld accepted %ld listed %ld digest %016llx\n", k, stride, m[0], m[1],
                 g_fold.layers, g_fold.accepted, g_fold.listed, g_fold.f.h);
      }
  printf("layers %ld, accepting and listing nothing %ld\n", g_layers, g_empty);
  if (!g_digest) {
    for (const auto& v : g_variants) printf("variant %s: %ld\n", v.first.c_str(), v.second);
    return 0;
  }
  std::map<std::string, std::string> by_kernel;  // "4 waves bf16 k3 s1 staged" -> " 1x1:n 2x1:n .."
  for (const auto& v : g_variants) {
    const size_t t = v.first.find(" MR="), e = v.first.find(" k", t);
    int mr = 0, nr = 0;
    sscanf(v.first.c_str() + t, " MR=%d NR=%d", &mr, &nr);
    char tile[48];
    snprintf(tile, sizeof(tile), " %dx%d:%ld", mr, nr, v.second);
    by_kernel[v.first.substr(0, t) + v.first.substr(e)] += tile;
  }
  for (const auto& v : by_kernel) printf("variants %s:%s\n", v.first.c_str(), v.second.c_str());
  return 0;
}
