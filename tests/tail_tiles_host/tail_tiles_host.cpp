// Host check of the sweep tail's tile ranges (pclean_amd/csrc/tail_tiles.h): every n_tiles in 0..200 against every workgroup
// count in 1..n_tiles + 3.  Built under -fsanitize=address,undefined by tests/test_tail_tiles_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pclean_amd/csrc/tail_tiles.h"

static int fail(const char* what, int n_tiles, int n_wgs, int wg) {
  std::printf("FAIL %s: n_tiles=%d n_wgs=%d wg=%d\n", what, n_tiles, n_wgs, wg);
  return 1;
}

int main() {
  int cases = 0;
  for (int n_tiles = 0; n_tiles <= 200; ++n_tiles) {
    for (int n_wgs = 1; n_wgs <= n_tiles + 3; ++n_wgs) {
      std::vector<int> seen((size_t)n_tiles, 0);
      int at = 0, lo = 1 << 30, hi = 0, empty = 0;
      for (int wg = 0; wg < n_wgs; ++wg) {
        const TailTileRange r = tail_tile_range(n_tiles, n_wgs, wg);
        if (r.begin != at) return fail("ranges not contiguous and in order", n_tiles, n_wgs, wg);
        if (r.end < r.begin || r.end > n_tiles) return fail("range out of bounds", n_tiles, n_wgs, wg);
        for (int t = r.begin; t < r.end; ++t) ++seen[(size_t)t];
        const int len = r.end - r.begin;
        if (len == 0) ++empty;
        if (len < lo) lo = len;
        if (len > hi) hi = len;
        at = r.end;
      }
      if (at != n_tiles) return fail("tiles left over", n_tiles, n_wgs, -1);
      for (int t = 0; t < n_tiles; ++t)
        if (seen[(size_t)t] != 1) return fail("tile not covered exactly once", n_tiles, n_wgs, t);
      if (hi - lo > 1) return fail("sizes differ by more than one", n_tiles, n_wgs, -1);
      const int surplus = n_wgs > n_tiles ? n_wgs - n_tiles : 0;
      if (empty != surplus) return fail("surplus workgroups must get the empty ranges, nobody else", n_tiles, n_wgs, -1);
      // the empty ranges are the LAST workgroups'
      for (int wg = n_wgs - surplus; wg < n_wgs; ++wg) {
        const TailTileRange r = tail_tile_range(n_tiles, n_wgs, wg);
        if (r.begin != r.end) return fail("a surplus workgroup got tiles", n_tiles, n_wgs, wg);
      }
      // out-of-range workgroup indices and counts: empty
      if (tail_tile_range(n_tiles, n_wgs, -1).end != 0 || tail_tile_range(n_tiles, n_wgs, n_wgs).end != 0 ||
          tail_tile_range(n_tiles, 0, 0).end != 0)
        return fail("bad arguments must give an empty range", n_tiles, n_wgs, -1);
      // the launch's workgroup count: capped, never more than the tiles, at least one
      for (int cap = 1; cap <= 9; cap += 4) {
        const int n = tail_wg_count(n_tiles, cap, 0), f = tail_wg_count(n_tiles, cap, n_wgs);
        if (n < 1 || (n_tiles > 0 && n > n_tiles) || n > (cap > 1 ? cap : 1)) return fail("capped workgroup count", n_tiles, cap, n);
        if (f < 1 || (n_tiles > 0 && (f > n_tiles || f > n_wgs))) return fail("forced workgroup count", n_tiles, n_wgs, f);
      }
      ++cases;
    }
  }
  // the split the GPU test relies on: 47 tiles over 3 workgroups
  const TailTileRange a = tail_tile_range(47, 3, 0), b = tail_tile_range(47, 3, 1), c = tail_tile_range(47, 3, 2);
  if (a.end - a.begin != 16 || b.end - b.begin != 16 || c.end - c.begin != 15) return fail("47 tiles over 3", 47, 3, -1);
  std::printf("ok 47 tiles over 3 workgroups: 16 16 15\n");
  std::printf("cases %d\n", cases);
  std::printf("all cases passed\n");
  return 0;
}
