// Class rules of the tabulated likelihood terms (PCLEAN_DENS_TABULATED), on FOLDED symbols (pclean_set_fold_table:
// equal fold ids = equal after `lowercase`).  One definition for the device kernels (class_kernels.hip) and for host
// programs that check them; both walk the observed string front to back, so a caller may feed it in pieces.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PCLEAN_HD __host__ __device__ inline
#else
#define PCLEAN_HD inline
#endif

// is_short_version(short, long) of expand_on_short_version.jl:6-19 as a resumable two-pointer walk: `a` symbols of the short
// (latent) string are matched so far, `cur` is its folded symbol number a (anything when a == s).
struct ShortWalk {
  int a;
  uint16_t cur;
};
// one symbol `lb` of the long (observed) string; next(a) returns the short string's folded symbol a (called for a < s only)
template <typename Next>
PCLEAN_HD void short_walk_step(ShortWalk& w, int s, uint16_t lb, Next next) {
  if (w.a < s && w.cur == lb) {
    ++w.a;
    w.cur = w.a < s ? next(w.a) : (uint16_t)0;
  }
}
PCLEAN_HD int short_walk_class(const ShortWalk& w, int s) { return w.a >= s ? 0 : 1; }

// FormatName, the one-name method (format_name.jl:47-54): 0 = equal ignoring case, 1 = observed is the name's initial + ".",
// 2 = neither.  eq: the first min(s, l) symbols agree; init: l == 2, s >= 1, observed[0] ~ name[0], observed[1] is the dot.
PCLEAN_HD int format_name_class_of(bool eq, bool init, int s, int l) { return (eq && s == l) ? 0 : (init ? 1 : 2); }

// FormatName, the three-name method (format_name.jl:14-26), needs two facts of (observed string of l symbols, latent string
// of s symbols): the observed one STARTS with the latent one followed by the separator (PCLEAN_CLASS_NAME_PREFIX), and it
// ENDS with the separator followed by the latent one (PCLEAN_CLASS_NAME_SUFFIX).  Both as a walk that is handed symbol p of
// the observed string, p = 0 .. l - 1; `ok` starts as name_affix_start(s, l) and is the answer after the last symbol.
// name(a) returns the latent string's folded symbol a and is called for 0 <= a < s only.
PCLEAN_HD bool name_affix_start(int s, int l) { return l >= s + 1; }
template <typename Name>
PCLEAN_HD bool name_prefix_step(bool ok, int p, int s, uint16_t lb, uint16_t sep, Name name) {
  if (!ok || p > s) return ok;
  return p < s ? lb == name(p) : lb == sep;
}
template <typename Name>
PCLEAN_HD bool name_suffix_step(bool ok, int p, int s, int l, uint16_t lb, uint16_t sep, Name name) {
  const int start = l - s - 1;  // (>= 0 while ok: where the separator stands)
  if (!ok || p < start) return ok;
  return p == start ? lb == sep : lb == name(p - start - 1);
}
