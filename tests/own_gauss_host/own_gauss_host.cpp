// The fixed-point quantiser of pclean_own_gauss_stats (include/pclean_ownq.h) on the host, under sanitizers: a program with
// its own main.  Without arguments it checks the exponent rule, the int64 bound, ties to even and the error bound, and
// prints "all cases passed".  With `quantise <e>` it reads doubles (hex bit patterns, one per line) from stdin and prints
// llrint(x * 2^e) per line: the test compares that with the NumPy restatement.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pclean_ownq.h"

static int fails = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      ++fails;                        \
      printf("FAIL %s: ", #cond);     \
      printf(__VA_ARGS__);            \
      printf("\n");                   \
    }                                 \
  } while (0)

static int bit_length(int64_t n) {
  int b = 0;
  for (; n > 0; n >>= 1) ++b;
  return b;
}

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "quantise") == 0) {
    const int e = atoi(argv[2]);
    const double scale = pclean_ownq_scale(e);
    unsigned long long bits;
    while (scanf("%llx", &bits) == 1) {
      double x;
      memcpy(&x, &bits, 8);
      printf("%" PRId64 "\n", pclean_ownq(x, scale));
    }
    return 0;
  }
  const int64_t rows[] = {1, (int64_t)1 << 20, ((int64_t)1 << 31) - 1};
  const double mags[] = {0.0, 1e-300, 1.0, 1e15};
  int cases = 0;
  for (int64_t n : rows)
    for (double M : mags) {
      const int e = pclean_ownq_exponent(M, n);
      int ex = 0;
      if (M > 0.0) (void)frexp(M, &ex);
      const int want = M == 0.0 ? 40 : (62 - ex - bit_length(n) < 40 ? 62 - ex - bit_length(n) : 40);
      CHECK(e == want, "n = %" PRId64 " M = %g: e = %d, want %d", n, M, e, want);
      CHECK(e <= PCLEAN_OWNQ_MAX_EXP, "e = %d", e);
      // no overflow at the bound: n values of magnitude M sum to less than 2^62 in __int128, so the int64 sum is exact
      const int64_t q = pclean_ownq(M, pclean_ownq_scale(e));
      const __int128 total = (__int128)q * n;
      CHECK(total < ((__int128)1 << 62), "n = %" PRId64 " M = %g e = %d: n * q leaves 2^62", n, M, e);
      CHECK(pclean_ownq(-M, pclean_ownq_scale(e)) == -q, "the quantiser is odd");
      // the scale is the exact power of two
      CHECK(pclean_ownq_scale(e) == ldexp(1.0, e), "scale(%d)", e);
      printf("ok n %" PRId64 " M %g e %d\n", n, M, e);
      ++cases;
    }
  CHECK(pclean_ownq_exponent(1.0, 1) == 40 && pclean_ownq_exponent(1.0, (int64_t)1 << 20) == 40, "a small table keeps 40 bits");
  CHECK(pclean_ownq_exponent(1e15, ((int64_t)1 << 31) - 1) == 62 - 50 - 31, "1e15 over 2^31 - 1 rows: e = -19");
  CHECK(pclean_ownq_exponent(NAN, 5) == 40 && pclean_ownq_exponent(-1.0, 5) == 40, "no finite magnitude: 40");
  // ties to even (e = 0 and e = 1)
  const double s0 = pclean_ownq_scale(0), s1 = pclean_ownq_scale(1);
  CHECK(pclean_ownq(0.5, s0) == 0 && pclean_ownq(1.5, s0) == 2 && pclean_ownq(2.5, s0) == 2 && pclean_ownq(-0.5, s0) == 0 &&
            pclean_ownq(-1.5, s0) == -2 && pclean_ownq(-2.5, s0) == -2,
        "ties to even at e = 0");
  CHECK(pclean_ownq(0.25, s1) == 0 && pclean_ownq(0.75, s1) == 2 && pclean_ownq(1.25, s1) == 2, "ties to even at e = 1");
  // |qsum / 2^e - sum bx| <= n * 2^(-e-1), sums in long double and __int128
  {
    uint64_t st = 88172645463325252ull;
    const int n = 10000;
    std::vector<double> xs(n);
    double M = 0.0;
    for (int i = 0; i < n; ++i) {
      st ^= st << 13;
      st ^= st >> 7;
      st ^= st << 17;
      xs[i] = ((double)(st >> 11) / 9007199254740992.0 - 0.5) * 6000.0;
      M = fmax(M, fabs(xs[i]));
    }
    const int e = pclean_ownq_exponent(M, n);
    __int128 qs = 0;
    long double sum = 0.0L;
    for (double x : xs) {
      qs += pclean_ownq(x, pclean_ownq_scale(e));
      sum += (long double)x;
    }
    const long double err = fabsl((long double)qs / ldexpl(1.0L, e) - sum);
    CHECK(err <= (long double)n * ldexpl(1.0L, -e - 1) + 1e-9L, "error %Lg beyond n 2^(-e-1)", err);
    printf("ok error bound e %d\n", e);
    ++cases;
  }
  printf("cases %d\n", cases);
  if (fails) return 1;
  printf("all cases passed\n");
  return 0;
}
