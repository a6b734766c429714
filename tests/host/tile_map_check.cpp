// Exhaustive check of the block maps of csrc/evae_tile_map.h and of their grid functions, on the CPU (plain C++, no HIP):
// every map is a bijection from the live blocks of its grid onto the work items, keeps what shares an operand on one XCD
// (block id & 7), and its grid function returns the smallest grid that covers the work.  Exit status 0 = all hold.
#include <cstdio>
#include <vector>

#include "evae_tile_map.h"

using namespace evae;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (++failures <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                           \
  } while (0)

// contiguous runs: ids 0 .. grid - 1 hit every tile exactly once; the tiles of each XCD form one contiguous range
static void check_runs(const int ntiles) {
  const int grid = tile_grid(ntiles);
  CHECK(grid == ntiles, "ntiles=%d grid=%d", ntiles, grid);        // a bijection onto ntiles tiles needs exactly ntiles blocks
  std::vector<int> hits(ntiles, 0), lo(8, ntiles), hi(8, -1), cnt(8, 0);
  for (int id = 0; id < grid; ++id) {
    const int t = tile_of_block(id, ntiles);
    CHECK(t == tile_of_block(block_place(id), ntiles), "ntiles=%d id=%d: the two forms differ", ntiles, id);
    CHECK(t >= 0 && t < ntiles, "ntiles=%d id=%d tile=%d", ntiles, id, t);
    if (t < 0 || t >= ntiles) continue;
    ++hits[t];
    const int x = id & 7;
    if (t < lo[x]) lo[x] = t;
    if (t > hi[x]) hi[x] = t;
    ++cnt[x];
  }
  for (int t = 0; t < ntiles; ++t) CHECK(hits[t] == 1, "ntiles=%d tile=%d hit %d times", ntiles, t, hits[t]);
  for (int x = 0; x < 8; ++x)
    if (cnt[x] > 0) CHECK(hi[x] - lo[x] + 1 == cnt[x], "ntiles=%d xcd=%d: %d tiles in [%d, %d]", ntiles, x, cnt[x], lo[x], hi[x]);
}

// units: every (unit, index) exactly once, all blocks of a unit on one XCD, the rest of the grid idle, the last block live
static void check_units(const int nunits, const int per) {
  const int grid = unit_grid(nunits, per);
  std::vector<int> hits((size_t)nunits * per, 0), xcd_of(nunits, -1);
  int idle = 0;
  for (int id = 0; id < grid; ++id) {
    const BlockPlace b = block_place(id);
    if (unit_block_idle(b, nunits, per)) { ++idle; continue; }
    const UnitSlot us = unit_of_block(b, nunits, per);
    const bool ok = us.unit >= 0 && us.unit < nunits && us.idx >= 0 && us.idx < per;
    CHECK(ok, "nunits=%d per=%d id=%d -> (%d, %d)", nunits, per, id, us.unit, us.idx);
    if (!ok) continue;
    ++hits[(size_t)us.unit * per + us.idx];
    if (xcd_of[us.unit] < 0) xcd_of[us.unit] = id & 7;
    CHECK(xcd_of[us.unit] == (id & 7), "nunits=%d per=%d unit=%d on XCDs %d and %d", nunits, per, us.unit, xcd_of[us.unit], id & 7);
  }
  for (size_t i = 0; i < hits.size(); ++i) CHECK(hits[i] == 1, "nunits=%d per=%d (unit %zu, index %zu) hit %d times", nunits, per, i / per, i % per, hits[i]);
  CHECK(idle == grid - nunits * per, "nunits=%d per=%d grid=%d idle=%d", nunits, per, grid, idle);
  // smallest: one block less would drop a live block
  CHECK(grid >= 1 && !unit_block_idle(block_place(grid - 1), nunits, per), "nunits=%d per=%d: the last block of grid %d is idle", nunits, per, grid);
}

// strided slices: every (slice, tile) exactly once, slice % 8 == XCD, idle exactly when the slice does not exist, the last block live
static void check_slices(const int nslices, const int ntiles) {
  const int grid = slice_grid(ntiles, nslices);
  std::vector<int> hits((size_t)nslices * ntiles, 0);
  for (int id = 0; id < grid; ++id) {
    const BlockPlace b = block_place(id);
    const SliceTile st = slice_of_block(b, ntiles);
    CHECK(st.slice >= 0 && (st.slice & 7) == (id & 7), "nslices=%d ntiles=%d id=%d slice=%d", nslices, ntiles, id, st.slice);
    CHECK(st.tile >= 0 && st.tile < ntiles, "nslices=%d ntiles=%d id=%d tile=%d", nslices, ntiles, id, st.tile);
    CHECK(slice_block_idle(b, ntiles, nslices) == (st.slice >= nslices), "nslices=%d ntiles=%d id=%d slice=%d: idle test", nslices, ntiles, id, st.slice);
    if (st.slice < 0 || st.slice >= nslices || st.tile < 0 || st.tile >= ntiles) continue;
    ++hits[(size_t)st.slice * ntiles + st.tile];
  }
  for (size_t i = 0; i < hits.size(); ++i) CHECK(hits[i] == 1, "nslices=%d ntiles=%d (slice %zu, tile %zu) hit %d times", nslices, ntiles, i / ntiles, i % ntiles, hits[i]);
  CHECK(grid >= 1 && !slice_block_idle(block_place(grid - 1), ntiles, nslices), "nslices=%d ntiles=%d: the last block of grid %d is idle", nslices, ntiles, grid);
}

int main() {
  for (int ntiles = 1; ntiles <= 800; ++ntiles) check_runs(ntiles);
  for (int nunits = 1; nunits <= 200; ++nunits)
    for (int per = 1; per <= 6; ++per) check_units(nunits, per);
  for (int nslices = 1; nslices <= 40; ++nslices)
    for (int ntiles = 1; ntiles <= 12; ++ntiles) check_slices(nslices, ntiles);
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("tile maps: all checks hold\n");
  return 0;
}
