// The tile walk of the static tuple order (eval.hip: ensure_static_order), in plain C++ so that a host program can call it
// (tests/static_tiles_host).
//
// Input: the tuple ids of the window's rows in the static order — rows of one tuple are neighbours (a SEGMENT).  Output: the
// order cut into TILES, the unit one wavefront or one workgroup classes by the dynamic part of the key in every sweep:
//   * a segment of at most STATIC_TILE_WAVE positions is never split: such segments are packed, in order, into WAVE tiles of
//     at most STATIC_TILE_WAVE positions (one wavefront per tile, classes by ballots);
//   * a segment of more than STATIC_TILE_WAVE positions is cut into ceil(len / lt) LONG tiles of near-equal length, each at
//     most lt positions of that one segment (one workgroup per tile, classes through a table in LDS).  With lt >= the longest
//     segment nothing is ever cut: every group of the segment is found whole.
// For the streaming pass that follows the scan (sg_fill_kernel) every tile is also listed as chunks of at most
// STATIC_TILE_WAVE positions.
#pragma once
#include <cstdint>
#include <vector>

#define STATIC_TILE_WAVE 64
#define STATIC_TILE_LONG 1024

struct StaticTiles {
  std::vector<int32_t> tile_off;    // [n_tiles + 1] first position of every tile, then n
  std::vector<int32_t> wave_tiles;  // the tiles of at most STATIC_TILE_WAVE positions, ascending
  std::vector<int32_t> long_tiles;  // the long tiles, ascending
  std::vector<int32_t> chunk_tile;  // [n_chunks] tile of the chunk
  std::vector<int32_t> chunk_off;   // [n_chunks] first position of the chunk (it ends after 64 positions or with its tile)
  int n_tiles() const { return (int)tile_off.size() - 1; }
};

static inline void static_tiles_walk(const int32_t* tid, int n, int lt, StaticTiles& out) {
  out = StaticTiles();
  if (n <= 0 || lt < STATIC_TILE_WAVE) return;
  auto close = [&](int begin, int end, bool is_long) {
    const int tile = (int)out.tile_off.size();
    out.tile_off.push_back(begin);
    (is_long ? out.long_tiles : out.wave_tiles).push_back(tile);
    for (int c = begin; c < end; c += STATIC_TILE_WAVE) {
      out.chunk_tile.push_back(tile);
      out.chunk_off.push_back(c);
    }
  };
  int start = 0;  // first position of the open wave tile
  for (int sb = 0; sb < n;) {
    int se = sb + 1;
    while (se < n && tid[se] == tid[sb]) ++se;
    const int len = se - sb;
    if (len > STATIC_TILE_WAVE) {
      if (sb > start) close(start, sb, false);
      const int k = (len + lt - 1) / lt, base = len / k, rem = len % k;
      for (int j = 0, at = sb; j < k; ++j) {
        const int l = base + (j < rem ? 1 : 0);
        close(at, at + l, true);
        at += l;
      }
      start = se;
    } else if (se - start > STATIC_TILE_WAVE) {  // the segment does not fit the open tile
      close(start, sb, false);
      start = sb;
    }
    sb = se;
  }
  if (n > start) close(start, n, false);
  out.tile_off.push_back(n);
}
