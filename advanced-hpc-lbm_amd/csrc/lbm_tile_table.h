// lbm_tile_table.h -- the one layout in which the register-tile kernels (lbm_regtile.hip.h) take "which cells of my tile
// matter": forces (kRegForce), probes and windows (kRegProbe), and the table of an observer that is not wanted.  Host code
// only, nothing of HIP: a host compiler builds it alone (tests/tile_table_check.cpp).
//   slot[ntx * nty]        in tile order, tile = (y / ty) * ntx + x / 64: -1 for a tile without a marked cell, else the
//                          tile's rank among the occupied tiles
//   words[nslots][ty][64]  one word per cell of an occupied tile, at ((slot * ty) + y % ty) * 64 + x % 64; 0: not marked
// What a word means is its caller's business (forces: mask | label << 8; probes: index + 1; windows: place + 1).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// A table on a slab's device, for tiles of ty rows (0: not built -- both pointers null).
struct TileTable { int* slot = nullptr; uint32_t* words = nullptr; int nslots = 0, ty = 0; };

// A marked cell: column, row of the slab, word.
struct TileCell { int x, y; uint32_t word; };

// The table of `cells` for ntx x nty tiles of ty rows; returns the occupied tiles (an empty list: the table of -1s alone).
static inline int tile_table_build(int ty, int ntx, int nty, const std::vector<TileCell>& cells, std::vector<int>& slot,
                                   std::vector<uint32_t>& words) {
  slot.assign((size_t)ntx * (size_t)nty, -1);
  for (const TileCell& q : cells) slot[(size_t)(q.y / ty) * ntx + q.x / 64] = 0;
  int n = 0;
  for (int& v : slot) if (v == 0) v = n++;
  words.assign((size_t)n * ty * 64, 0u);
  for (const TileCell& q : cells) words[((size_t)slot[(size_t)(q.y / ty) * ntx + q.x / 64] * ty + q.y % ty) * 64 + q.x % 64] = q.word;
  return n;
}
