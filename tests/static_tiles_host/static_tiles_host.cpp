// Host program for the tile walk of the static tuple order (pclean_amd/csrc/static_tiles.h): planted and random segment
// lengths, every invariant of the walk checked on every case.  Built and run by tests/test_static_tiles_cpu.py (g++,
// -fsanitize=address,undefined).  Prints one line per case; exit status 1 at the first violated invariant.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../pclean_amd/csrc/static_tiles.h"

static const int LT = STATIC_TILE_LONG;
static const int WAVE = STATIC_TILE_WAVE;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      fprintf(stderr, "case %s: ", name.c_str());         \
      fprintf(stderr, __VA_ARGS__);                       \
      fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__);  \
      exit(1);                                            \
    }                                                     \
  } while (0)

// segment lengths -> tuple ids in the static order (ids need not ascend: neighbours only have to differ)
static std::vector<int32_t> tids_of(const std::vector<int>& lens) {
  std::vector<int32_t> tid;
  uint32_t id = 7;
  for (int len : lens) {
    id = id * 5u + 3u;  // (unsigned: wraps)
    if (!tid.empty() && tid.back() == (int32_t)(id & 0x7fffffffu)) ++id;
    tid.insert(tid.end(), (size_t)len, (int32_t)(id & 0x7fffffffu));
  }
  return tid;
}

static void check_case(const std::string& name, const std::vector<int>& lens, int lt = LT) {
  const std::vector<int32_t> tid = tids_of(lens);
  const int n = (int)tid.size();
  StaticTiles t;
  static_tiles_walk(tid.data(), n, lt, t);
  const int nt = t.n_tiles();
  CHECK(nt >= 1, "no tiles");
  // the tiles partition [0, n) in order
  CHECK(t.tile_off.front() == 0 && t.tile_off.back() == n, "tiles cover [%d, %d), not [0, %d)", t.tile_off.front(), t.tile_off.back(), n);
  for (int k = 0; k < nt; ++k) CHECK(t.tile_off[k] < t.tile_off[k + 1], "tile %d is empty or out of order", k);
  // every tile is in exactly one of the two lists, both ascending
  std::vector<int> is_long((size_t)nt, -1);
  for (size_t j = 0; j < t.wave_tiles.size(); ++j) {
    const int k = t.wave_tiles[j];
    CHECK(k >= 0 && k < nt && is_long[k] == -1, "wave tile list entry %zu", j);
    CHECK(j == 0 || t.wave_tiles[j - 1] < k, "wave tile list not ascending at %zu", j);
    is_long[k] = 0;
  }
  for (size_t j = 0; j < t.long_tiles.size(); ++j) {
    const int k = t.long_tiles[j];
    CHECK(k >= 0 && k < nt && is_long[k] == -1, "long tile list entry %zu", j);
    CHECK(j == 0 || t.long_tiles[j - 1] < k, "long tile list not ascending at %zu", j);
    is_long[k] = 1;
  }
  for (int k = 0; k < nt; ++k) CHECK(is_long[k] != -1, "tile %d is in neither list", k);
  // sizes; a long tile holds one tuple id
  for (int k = 0; k < nt; ++k) {
    const int b = t.tile_off[k], e = t.tile_off[k + 1];
    if (is_long[k]) {
      CHECK(e - b <= lt, "long tile %d has %d positions", k, e - b);
      for (int p = b; p < e; ++p) CHECK(tid[p] == tid[b], "long tile %d holds two tuple ids", k);
    } else {
      CHECK(e - b <= WAVE, "wave tile %d has %d positions", k, e - b);
    }
  }
  // segments
  std::vector<int> tile_of((size_t)n);
  for (int k = 0; k < nt; ++k)
    for (int p = t.tile_off[k]; p < t.tile_off[k + 1]; ++p) tile_of[p] = k;
  int sb = 0;
  for (int len : lens) {
    const int se = sb + len, k0 = tile_of[sb], k1 = tile_of[se - 1];
    if (len <= WAVE) {
      CHECK(k0 == k1, "segment [%d, %d) is split over tiles %d..%d", sb, se, k0, k1);
      CHECK(!is_long[k0], "segment [%d, %d) of %d positions lies in a long tile", sb, se, len);
    } else {
      const int want = (len + lt - 1) / lt;
      CHECK(k1 - k0 + 1 == want, "segment of %d positions has %d tiles, not %d", len, k1 - k0 + 1, want);
      CHECK(t.tile_off[k0] == sb && t.tile_off[k1 + 1] == se, "the tiles of segment [%d, %d) hold other positions", sb, se);
      int lo = len, hi = 0;
      for (int k = k0; k <= k1; ++k) {
        CHECK(is_long[k], "segment of %d positions lies in wave tile %d", len, k);
        const int l = t.tile_off[k + 1] - t.tile_off[k];
        lo = l < lo ? l : lo;
        hi = l > hi ? l : hi;
      }
      CHECK(hi - lo <= 1, "stretches of a segment of %d positions: %d..%d", len, lo, hi);
    }
    sb = se;
  }
  // chunks: every tile in pieces of at most 64 positions, in order, nothing else
  CHECK(t.chunk_tile.size() == t.chunk_off.size(), "chunk lists differ in length");
  size_t c = 0;
  for (int k = 0; k < nt; ++k)
    for (int p = t.tile_off[k]; p < t.tile_off[k + 1]; p += WAVE, ++c)
      CHECK(c < t.chunk_tile.size() && t.chunk_tile[c] == k && t.chunk_off[c] == p, "chunk %zu of tile %d", c, k);
  CHECK(c == t.chunk_tile.size(), "%zu chunks too many", t.chunk_tile.size() - c);
  printf("ok %-40s n=%d tiles=%d wave=%zu long=%zu chunks=%zu\n", name.c_str(), n, nt, t.wave_tiles.size(), t.long_tiles.size(),
         t.chunk_tile.size());
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

int main() {
  const int planted[] = {1, 63, 64, 65, LT - 1, LT, LT + 1, 3 * LT + 7};
  for (int len : planted) check_case("one segment of " + std::to_string(len), {len});
  for (int len : planted)  // ... between short neighbours that share an open tile
    check_case("3, 40, " + std::to_string(len) + ", 5, 60", {3, 40, len, 5, 60});
  check_case("all planted lengths in a row", std::vector<int>(planted, planted + 8));
  check_case("n = 1", {1});
  {
    std::vector<int> lens;
    for (int k = 0; k < 500; ++k) lens.push_back(1 + (int)(rnd() % 9));
    lens.push_back(2 * LT + 100);
    check_case("many short segments, then one long", lens);
    lens.insert(lens.begin(), LT + 1);
    check_case("one long, many short, one long", lens);
  }
  check_case("64 + 1 (two tiles)", {64, 1});
  check_case("33 x 2 (one tile) + 33", {33, 31, 33});
  check_case("a smaller LT: 65, 200, 129 with LT = 64", {65, 200, 129, 7}, 64);
  for (int rep = 0; rep < 200; ++rep) {
    std::vector<int> lens;
    const int ns = 1 + (int)(rnd() % 60);
    for (int k = 0; k < ns; ++k) {
      const uint32_t kind = rnd() % 10;
      lens.push_back(kind < 6 ? 1 + (int)(rnd() % 12) : kind < 8 ? 1 + (int)(rnd() % 130) : kind < 9 ? 60 + (int)(rnd() % 10) : 1 + (int)(rnd() % (4 * LT)));
    }
    check_case("random " + std::to_string(rep), lens, (rep & 1) ? LT : 64 + (int)(rnd() % 300));
  }
  printf("all cases passed\n");
  return 0;
}
