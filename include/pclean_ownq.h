/* pclean_ownq.h — the fixed-point quantiser of pclean_own_gauss_stats (include/pclean_hip.h), for host and device.
 *
 * The sufficient statistic of a Gaussian mean parameter is a sum of backward-transformed numbers bx.  Summed in floating
 * point by atomics it would depend on scheduling; summed as integers  q = llrint(bx * 2^e)  it does not.  The exponent e
 * is fixed once per term from the data: with M the largest finite |bx| and n the number of loaded rows,
 *     ex = frexp's exponent of M   (M < 2^ex),      er = bit length of n   (n < 2^er),
 *     e  = min(PCLEAN_OWNQ_MAX_EXP, 62 - ex - er),  e = PCLEAN_OWNQ_MAX_EXP for M == 0,
 * so every |q| <= 2^(62 - er) and a sum of n of them stays below 2^62: it cannot leave int64.  The multiplication by a power
 * of two is exact (the products are normal numbers or zero-ward of 2^-1022 * 2^40), llrint rounds to nearest, ties to even:
 * the NumPy restatement is  np.rint(bx * 2.0 ** e).astype(np.int64).  |q / 2^e - bx| <= 2^(-e-1) per value.
 */
#ifndef PCLEAN_OWNQ_H
#define PCLEAN_OWNQ_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PCLEAN_OWNQ_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PCLEAN_OWNQ_HD static inline
#endif

#define PCLEAN_OWNQ_MAX_EXP 40

/* e of a term whose largest finite |bx| is max_abs over n_rows loaded rows */
PCLEAN_OWNQ_HD int pclean_ownq_exponent(double max_abs, int64_t n_rows) {
  if (!(max_abs > 0.0)) return PCLEAN_OWNQ_MAX_EXP;
  int ex = 0;
  (void)frexp(max_abs, &ex);
  int er = 0;
  for (uint64_t n = n_rows > 0 ? (uint64_t)n_rows : 0; n; n >>= 1) ++er;
  const int e = 62 - ex - er;
  return e < PCLEAN_OWNQ_MAX_EXP ? e : PCLEAN_OWNQ_MAX_EXP;
}

/* 2^e as a double, e in [-1022, 1023] */
PCLEAN_OWNQ_HD double pclean_ownq_scale(int e) {
  const uint64_t b = (uint64_t)(e + 1023) << 52;
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}

/* q = llrint(bx * 2^e); bx finite, |bx| <= the max_abs that fixed e */
PCLEAN_OWNQ_HD int64_t pclean_ownq(double bx, double scale) {
  return (int64_t)llrint(bx * scale);
}

#endif
