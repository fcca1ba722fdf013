// tile_table_check.cpp -- lbm_tile_table.h on its own, for tests/test_tile_table.py: reads "ty ntx nty ncells" and ncells
// lines "x y word" on stdin, prints the slot table on one line and the words on the next.
#include <cstdio>

#include "lbm_tile_table.h"

int main() {
  int ty = 0, ntx = 0, nty = 0, n = 0;
  if (scanf("%d %d %d %d", &ty, &ntx, &nty, &n) != 4 || ty < 1 || ntx < 1 || nty < 1 || n < 0) return 2;
  std::vector<TileCell> cells((size_t)n);
  for (TileCell& q : cells)
    if (scanf("%d %d %u", &q.x, &q.y, &q.word) != 3 || q.x < 0 || q.x >= 64 * ntx || q.y < 0 || q.y >= ty * nty) return 2;
  std::vector<int> slot;
  std::vector<uint32_t> words;
  const int nslots = tile_table_build(ty, ntx, nty, cells, slot, words);
  if (words.size() != (size_t)nslots * ty * 64) return 3;
  for (int v : slot) printf("%d ", v);
  printf("\n");
  for (uint32_t v : words) printf("%u ", v);
  printf("\n");
  return 0;
}
