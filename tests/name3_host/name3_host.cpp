// Host build of the two walks of pclean_amd/csrc/class_rules.h that decide the byte tables of the three-name FormatName
// (PCLEAN_CLASS_NAME_PREFIX / PCLEAN_CLASS_NAME_SUFFIX), driven the way class_kernels.hip drives them: the observed string
// front to back, in pieces, on folded symbols.  tests/test_name3_cpu.py holds them against the Python restatement.
#include <algorithm>
#include <cstdint>

#include "../../pclean_amd/csrc/class_rules.h"

extern "C" {
// o[0 .. l): folded observed string, v[0 .. s): folded latent string, sep: the folded separator; piece: symbols per piece
int n3h_prefix(const uint16_t* o, int l, const uint16_t* v, int s, uint16_t sep, int piece) {
  bool ok = name_affix_start(s, l);
  for (int p0 = 0; p0 < l; p0 += piece) {
    const int np = std::min(piece, l - p0);
    if (!ok || p0 > s) continue;
    for (int b = 0; b < np; ++b) ok = name_prefix_step(ok, p0 + b, s, o[p0 + b], sep, [&](int a) { return v[a]; });
  }
  return ok ? 1 : 0;
}
int n3h_suffix(const uint16_t* o, int l, const uint16_t* v, int s, uint16_t sep, int piece) {
  bool ok = name_affix_start(s, l);
  for (int p0 = 0; p0 < l; p0 += piece) {
    const int np = std::min(piece, l - p0);
    if (!ok || p0 + np <= l - s - 1) continue;
    for (int b = 0; b < np; ++b) ok = name_suffix_step(ok, p0 + b, s, l, o[p0 + b], sep, [&](int a) { return v[a]; });
  }
  return ok ? 1 : 0;
}
}
