// The grid rule of pclean_link_own_star (pclean_amd/csrc/own_star_check.h) on the host, under sanitizers: a program with its
// own main.  It builds key-major grids of every small shape — 1 x n, n x 1 and grids below 4 options among them, which the
// grid test of pclean_set_options_cols does not recognise — and checks that each is accepted with the right K_j, that one
// wrong entry in either column, a length that is no multiple of K_a and every limit are refused, that the value check names
// the first value outside the latent domain, and the LDS formula.  Prints "all cases passed".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pclean_amd/csrc/own_star_check.h"

static int fails = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      ++fails;                    \
      printf("FAIL %s: ", #cond); \
      printf(__VA_ARGS__);        \
      printf("\n");               \
    }                             \
  } while (0)

struct Grid {
  std::vector<int32_t> head, c0, c1;
};

// head values 10 + 3 a (not the option index: the rule follows the VALUES), arm values 7 b + 1
static Grid make(int ka, int kj) {
  Grid g;
  for (int a = 0; a < ka; ++a) g.head.push_back(10 + 3 * a);
  for (int a = 0; a < ka; ++a)
    for (int b = 0; b < kj; ++b) {
      g.c0.push_back(10 + 3 * a);
      g.c1.push_back(7 * b + 1);
    }
  return g;
}

int main() {
  char msg[200];
  int cases = 0;
  for (int ka = 1; ka <= 9; ++ka)
    for (int kj = 1; kj <= 9; ++kj) {
      Grid g = make(ka, kj);
      int32_t got = -1;
      int rc = own_star_check_grid(ka, g.head.data(), (int64_t)ka * kj, g.c0.data(), g.c1.data(), &got, msg, sizeof msg);
      CHECK(rc == 0 && got == kj, "%d x %d: rc %d kj %d", ka, kj, rc, got);
      if (ka == 1 || kj == 1 || ka * kj < 4) printf("ok %dx%d\n", ka, kj);
      // one wrong entry, at every place of either column
      for (size_t k = 0; k < g.c0.size(); ++k) {
        Grid h = g;
        h.c0[k] += 1;
        rc = own_star_check_grid(ka, h.head.data(), (int64_t)ka * kj, h.c0.data(), h.c1.data(), &got, msg, sizeof msg);
        CHECK(rc == -5, "%d x %d: column 0 wrong at %zu: rc %d", ka, kj, k, rc);
        h = g;
        h.c1[k] += 1;
        rc = own_star_check_grid(ka, h.head.data(), (int64_t)ka * kj, h.c0.data(), h.c1.data(), &got, msg, sizeof msg);
        // (entry b of the first row IS the definition of b's value: changing it breaks the rows below, if there are any)
        CHECK(ka == 1 ? (k < (size_t)kj ? rc == 0 : rc == -6) : rc == -6, "%d x %d: column 1 wrong at %zu: rc %d", ka, kj, k, rc);
      }
      if (ka > 1) {  // a length that is no multiple of K_a (the arrays are only read when the length fits)
        rc = own_star_check_grid(ka, g.head.data(), (int64_t)ka * kj + 1, g.c0.data(), g.c1.data(), &got, msg, sizeof msg);
        CHECK(rc == -2, "%d x %d + 1: rc %d", ka, kj, rc);
      }
      ++cases;
    }
  {  // the limits
    Grid g = make(2, 2);
    int32_t got = 0;
    CHECK(own_star_check_grid(0, g.head.data(), 4, g.c0.data(), g.c1.data(), &got, msg, sizeof msg) == -1, "K_a = 0");
    CHECK(own_star_check_grid(OWN_STAR_MAX_K + 1, g.head.data(), 4, g.c0.data(), g.c1.data(), &got, msg, sizeof msg) == -1, "K_a beyond");
    CHECK(own_star_check_grid(2, nullptr, 4, g.c0.data(), g.c1.data(), &got, msg, sizeof msg) == -1, "no head values");
    CHECK(own_star_check_grid(2, g.head.data(), 0, g.c0.data(), g.c1.data(), &got, msg, sizeof msg) == -2, "no options");
    CHECK(own_star_check_grid(2, g.head.data(), 4, nullptr, g.c1.data(), &got, msg, sizeof msg) == -2, "no column");
    // (refused on the lengths alone: the arrays are never read)
    CHECK(own_star_check_grid(1, g.head.data(), OWN_STAR_MAX_K + 1, g.c0.data(), g.c1.data(), &got, msg, sizeof msg) == -3, "K_j beyond");
    Grid big = make(OWN_STAR_MAX_K, 65);
    CHECK(own_star_check_grid(OWN_STAR_MAX_K, big.head.data(), (int64_t)OWN_STAR_MAX_K * 65, big.c0.data(), big.c1.data(), &got, msg,
                              sizeof msg) == -4, "4096 x 65 beyond the grid limit");
    Grid full = make(OWN_STAR_MAX_K, 64);
    CHECK(own_star_check_grid(OWN_STAR_MAX_K, full.head.data(), (int64_t)OWN_STAR_MAX_K * 64, full.c0.data(), full.c1.data(), &got, msg,
                              sizeof msg) == 0 && got == 64, "4096 x 64 is the largest grid");
    CHECK(strlen(msg) < sizeof msg, "message");
    ++cases;
  }
  {  // the value check
    const int32_t v[] = {0, 3, 4, -1, 9};
    CHECK(own_star_check_values(2, v, 4) == 0, "inside");
    CHECK(own_star_check_values(3, v, 4) == 3, "4 is outside 0 .. 3");
    CHECK(own_star_check_values(5, v, 5) == 4, "-1 is outside");
    CHECK(own_star_check_values(0, v, 0) == 0, "nothing to check");
    ++cases;
  }
  {  // the LDS formula: (terms x values + K_a + K_a / 64 rounded up) * 8
    const int32_t kj[] = {50, 7}, tpn[] = {1, 2, 0};
    CHECK(own_star_lds_bytes(3657, 2, kj, tpn) == (size_t)(3657 + 100 + 3657 + 58) * 8, "hospital-like star");
    const int32_t k1[] = {1, 1}, t1[] = {0, 0, 0};
    CHECK(own_star_lds_bytes(1, 2, k1, t1) == 16, "1; 1, 1 without terms");
    ++cases;
  }
  printf("cases %d\n", cases);
  if (fails) return 1;
  printf("all cases passed\n");
  return 0;
}
