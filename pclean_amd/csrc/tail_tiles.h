// The tile ranges of the sweep's tail (sweep.hip: finalize_tail_kernel), in plain C++ so that a host program can call them
// (tests/tail_tiles_host).
//
// The rows of the active window are cut into tiles of TAIL_TILE_ROWS rows; workgroup `wg` of `n_wgs` walks the contiguous
// tiles [begin, end): the ranges follow each other in workgroup order, cover every tile exactly once and differ in length by
// at most one (the first n_tiles % n_wgs workgroups take the longer ones).  With more workgroups than tiles the surplus
// workgroups get an empty range.
#pragma once

#define TAIL_TILE_ROWS 256

struct TailTileRange {
  int begin, end;
};

#if defined(__HIPCC__)
__host__ __device__
#endif
static inline TailTileRange tail_tile_range(int n_tiles, int n_wgs, int wg) {
  TailTileRange r{0, 0};
  if (n_tiles <= 0 || n_wgs <= 0 || wg < 0 || wg >= n_wgs) return r;
  const int base = n_tiles / n_wgs, rem = n_tiles % n_wgs;
  r.begin = wg * base + (wg < rem ? wg : rem);
  r.end = r.begin + base + (wg < rem ? 1 : 0);
  return r;
}

// workgroups of the launch: at most `cap` (a few per compute unit), never more than there are tiles; forced > 0 overrides the
// cap (PCLEAN_TAIL_WGS) but still never exceeds the tiles
static inline int tail_wg_count(int n_tiles, int cap, int forced) {
  if (n_tiles <= 0) return 1;
  int n = forced > 0 ? forced : cap;
  if (n < 1) n = 1;
  return n < n_tiles ? n : n_tiles;
}
