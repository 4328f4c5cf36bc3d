// Value sampled for a chosen ProposalDummyValue, scored inside the sweep (block_proposal.jl:58-60):
// random(StringPrior) draw (string_prior.jl:28-39, the draw order of random_kernels.hip) as pool symbols, and its
// Damerau-Levenshtein distance to an observed pool string in either flavour (add_typos.jl:56) — single-thread
// device code for a rare path: a particle draws the dummy with an observation below the node only when no
// proposal atom explains that observation.
#pragma once
#include "ctx.h"
#include "../../include/pclean_detmath.h"
#include "../../include/pclean_philox.h"

#define DUMMY_MAX_LEN 255  // StringPrior max_len and observed string length both fit a byte-wide pair table

// fixed-point inverse CDF over 28 probabilities (random_kernels.hip: draw28)
__device__ inline int dummy_draw28(const double* p, uint64_t r64) {
  uint64_t w[28];
  uint64_t total = 0;
  for (int j = 0; j < 28; ++j) {
    w[j] = (uint64_t)(p[j] * 1099511627776.0);
    total += w[j];
  }
  const uint64_t r = pclean_mulhi64(r64, total);
  uint64_t acc = 0;
  for (int j = 0; j < 28; ++j) {
    acc += w[j];
    if (acc > r) return j;
  }
  return 27;
}

// the string of (key, row): symbols into out[0 .. len), returns len (random_string_prior_at_kernel's draws, stream 0)
__device__ inline int dummy_draw_string(uint64_t key, uint32_t row, int min_len, int max_len, const double* init_p,
                                        const double* trans_p, const uint16_t* letter_sym, uint16_t* out) {
  uint32_t t = 0;
  const uint32_t site = PCLEAN_SITE_RANDOM(PCLEAN_RANDOM_STRING_PRIOR);
  const int len = min_len + (int)pclean_mulhi64(pclean_rand64(key, row, site, t++, 0u), (uint64_t)(max_len - min_len + 1));
  int prev = 0;
  for (int k = 0; k < len; ++k) {
    prev = dummy_draw28(k == 0 ? init_p : trans_p + (size_t)prev * 28, pclean_rand64(key, row, site, t++, 0u));
    out[k] = letter_sym[prev];
  }
  return len;
}

// distance between a[0..la) and b[0..lb) on the full matrix H [(la + 2)][(lb + 2)] (int16, caller's scratch):
// restricted (optimal string alignment) or unrestricted (Lowrance-Wagner; the "last row where this symbol occurred"
// table is replaced by a backward search, the strings are short)
__device__ inline int dummy_distance(int dist_mode, const uint16_t* a, int la, const uint16_t* b, int lb, int16_t* H) {
  const int W = lb + 2;
  const int maxdist = la + lb;
  H[0] = (int16_t)maxdist;
  for (int i = 0; i <= la; ++i) {
    H[(i + 1) * W + 0] = (int16_t)maxdist;
    H[(i + 1) * W + 1] = (int16_t)i;
  }
  for (int j = 0; j <= lb; ++j) {
    H[0 * W + (j + 1)] = (int16_t)maxdist;
    H[1 * W + (j + 1)] = (int16_t)j;
  }
  for (int i = 1; i <= la; ++i) {
    int db = 0;
    for (int j = 1; j <= lb; ++j) {
      const int cost = a[i - 1] == b[j - 1] ? 0 : 1;
      int v = H[i * W + j] + cost;
      v = min(v, H[(i + 1) * W + j] + 1);
      v = min(v, H[i * W + (j + 1)] + 1);
      if (dist_mode == PCLEAN_DIST_OSA) {
        if (i > 1 && j > 1 && a[i - 1] == b[j - 2] && a[i - 2] == b[j - 1]) v = min(v, H[(i - 1) * W + (j - 1)] + 1);
      } else {
        int k = 0;  // last row < i whose symbol equals b[j-1]
        for (int q = i - 1; q >= 1; --q)
          if (a[q - 1] == b[j - 1]) {
            k = q;
            break;
          }
        const int l = db;
        v = min(v, H[k * W + l] + (i - k - 1) + 1 + (j - l - 1));
        if (cost == 0) db = j;
      }
      H[(i + 1) * W + (j + 1)] = (int16_t)v;
    }
  }
  return H[(la + 1) * W + (lb + 1)];
}

#define DUMMY_TIME_LEN 10  // "12:59 a.m."

// random(TimePrior) of (key, row) (time_prior.jl:21-23; random_time_prior_at_kernel's three draws, stream 0) rendered
// "{h}:{m} a.m." / "{h}:{m} p.m." (minutes not zero-padded: sampling.random_time_prior) as pool symbols into
// out[0 .. len), returns len.  tsym: the symbols of 0 .. 9 : ' ' a p . m (pclean_set_time_symbols; 0xFFFF: not in the
// pool — the time then equals no pool string)
__device__ inline int dummy_draw_time(uint64_t key, uint32_t row, const uint16_t* tsym, uint16_t* out) {
  const uint32_t site = PCLEAN_SITE_RANDOM(PCLEAN_RANDOM_TIME_PRIOR);
  const int h = 1 + (int)pclean_mulhi64(pclean_rand64(key, row, site, 0u, 0u), (uint64_t)12);
  const int m = 1 + (int)pclean_mulhi64(pclean_rand64(key, row, site, 1u, 0u), (uint64_t)60);
  const bool am = (pclean_rand64(key, row, site, 2u, 0u) >> 63) != 0;
  int n = 0;
  if (h >= 10) out[n++] = tsym[h / 10];
  out[n++] = tsym[h % 10];
  out[n++] = tsym[10];
  if (m >= 10) out[n++] = tsym[m / 10];
  out[n++] = tsym[m % 10];
  out[n++] = tsym[11];
  out[n++] = tsym[am ? 12 : 13];
  out[n++] = tsym[14];
  out[n++] = tsym[15];
  out[n++] = tsym[14];
  return n;
}

// is pool string a[0 .. la) the string s[0 .. ls) (ls <= DUMMY_TIME_LEN)?  Every symbol is read (at a clamped index) before
// any is compared: one level of loads
__device__ inline bool dummy_same_string(const uint16_t* a, int la, const uint16_t* s, int ls) {
  bool same = la == ls;
  uint16_t x[DUMMY_TIME_LEN];
#pragma unroll
  for (int k = 0; k < DUMMY_TIME_LEN; ++k) x[k] = la > 0 ? a[min(k, la - 1)] : (uint16_t)0;  // (an empty string: nothing to read)
#pragma unroll
  for (int k = 0; k < DUMMY_TIME_LEN; ++k) same = same && (k >= ls || x[k] == s[k]);
  return same;
}
