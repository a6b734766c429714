// Block scheduling of the GEMM and window-convolution kernels: how a block of a 1-D grid finds its work, and -- the host half
// of each map -- the grid size the map's arithmetic relies on.  A kernel calls the map, its launcher the grid function next
// to it; nothing else in csrc/ turns a block id into a tile.
//
// All maps rest on one fact of the machine: the blocks of a grid are dealt to the eight XCDs (each with an L2 of its own) round
// robin, block id -> XCD id & 7, so ids 8 j + x, j = 0, 1, ... run on XCD x back to back.
//
// Self-contained (no HIP header): a plain C++ compiler can include it (tests/host/tile_map_check.cpp checks every map
// exhaustively on the CPU).
#pragma once

#ifdef __HIPCC__
#define EVAE_HD __host__ __device__
#else
#define EVAE_HD
#endif
#define EVAE_HD_INLINE EVAE_HD inline __attribute__((always_inline))

namespace evae {

// The maps take the block id decomposed (block_place), and the idle test of a map is a function of its own: a kernel with two
// maps decomposes the id at the head of each branch and returns from an idle block before it computes anything else -- written
// this way the compiler produces the instructions of the maps spelled out in place.
struct BlockPlace { int xcd, slot; };       // the XCD that runs a block, and the block's place in that XCD's queue
EVAE_HD_INLINE BlockPlace block_place(const int id) { return {id & 7, id >> 3}; }

// ---- contiguous runs: XCD x works on a contiguous run of tiles (bijective: ids 0 .. ntiles - 1 -> tiles 0 .. ntiles - 1).
// Neighbouring tiles share operand panels (the A row panel of a row of tiles, the halo rows of neighbouring windows), which
// then meet in one L2.
EVAE_HD_INLINE int tile_of_block(const BlockPlace b, const int ntiles) {
  const int qq = ntiles >> 3, rr = ntiles & 7;
  return (b.xcd < rr ? b.xcd * (qq + 1) : rr * (qq + 1) + (b.xcd - rr) * qq) + b.slot;
}
EVAE_HD_INLINE int tile_of_block(const int id, const int ntiles) { return tile_of_block(block_place(id), ntiles); }
inline int tile_grid(const int ntiles) { return ntiles; }

// ---- block height of the byte layer's copy-pipeline forward (u8p_gemm_kernel, evae_dense_u8.hip): rows per block, 128, 256 or
// 448, for M rows x tiles_n column tiles on cus CUs.  The 256- and 448-row blocks run one per CU, so a launch takes
// ceil(blocks / cus) rounds and its busiest CU works through rounds x height rows.  256 rows (half the weight-image bytes per row
// of 128) once those blocks still fill the machine; 448 where they get the busiest CU through fewer rounds AND fewer rows --
// 19 968 rows x 5 tiles on 256 CUs: 225 blocks, one round of 448 rows, against 390 blocks, two rounds = 512 rows; at 25 000 rows
// both heights take two rounds and the launch stays at 256.
inline int u8_fwd_rounds(const int M, const int tiles_n, const int cus, const int h) {
  const int blocks = ((M + h - 1) / h) * tiles_n;
  return (blocks + cus - 1) / cus;
}
inline int u8_fwd_block_rows(const int M, const int tiles_n, const int cus) {
  if (((M + 255) / 256) * tiles_n < cus) return 128;
  const int r256 = u8_fwd_rounds(M, tiles_n, cus, 256), r448 = u8_fwd_rounds(M, tiles_n, cus, 448);
  return (r448 < r256 && r448 * 448 < r256 * 256) ? 448 : 256;
}

// ---- units (the XCD-local split-K): a UNIT is a set of `per_unit` blocks that read the same heavy operand strip -- the tiles
// of one (contraction slice, row or column tile) along the other tile axis; the call site says which operand.  A unit sits on
// ONE XCD, dispatched back to back, so its blocks walk the slice in step and all but the first find every slab in that XCD's
// L2; units are dealt to the XCDs in contiguous runs, so with slice-major unit numbers the units of a slice (which share the
// other operand) mostly meet on one XCD as well.  An XCD whose run is one unit shorter than the longest leaves its last
// per_unit blocks idle (unit_block_idle): such a block returns at once.
// (r02, a split-K launch on a 3-D grid (tiles, 1, slices): the blocks of a slice scattered over all eight L2s -- 346 MB read
// against 91 MB of operands for the layer-2 weight gradient; the byte layer's weight gradient, every (row tile x column tile
// x slice) block streaming both operands past its L2: 710 MB per launch against 110 MB.)
struct UnitSlot { int unit, idx; };       // idx = the block's place within its unit
EVAE_HD_INLINE bool unit_block_idle(const BlockPlace b, const int nunits, const int per_unit) {
  const int qq = nunits >> 3, rr = nunits & 7;
  return b.slot / per_unit >= qq + (b.xcd < rr ? 1 : 0);
}
EVAE_HD_INLINE UnitSlot unit_of_block(const BlockPlace b, const int nunits, const int per_unit) {      // of a block that is not idle
  const int qq = nunits >> 3, rr = nunits & 7;
  const int ul = b.slot / per_unit;
  return {b.xcd * qq + (b.xcd < rr ? b.xcd : rr) + ul, b.slot - ul * per_unit};
}
// up to the last block of the last XCD that has a longest run
inline int unit_grid(const int nunits, const int per_unit) {
  const int longest = (nunits + 7) >> 3, last_xcd = (nunits - 1) & 7;
  return 8 * (per_unit * longest - 1) + last_xcd + 1;
}

// ---- strided slices (the pre-split bf16 kernel's split contraction, r04): XCD x runs ALL the tiles of slices x, x + 8, ...:
// the blocks that share a slice's operand strips sit on one L2 and walk the slice in step.  A block whose slice does not
// exist is idle (slice_block_idle) and returns at once.
// (PMC of the 3-D grid at 600 x 301 x 25 100: 478 MB per launch against 135 MB of operand images, 7.4 TB/s -- every XCD met
// every slice.)
struct SliceTile { int tile, slice; };
EVAE_HD_INLINE SliceTile slice_of_block(const BlockPlace b, const int ntiles) {
  const int j = b.slot / ntiles;
  return {b.slot - j * ntiles, b.xcd + 8 * j};
}
EVAE_HD_INLINE bool slice_block_idle(const BlockPlace b, const int ntiles, const int nslices) {
  return slice_of_block(b, ntiles).slice >= nslices;
}
// up to the last tile of the last slice
inline int slice_grid(const int ntiles, const int nslices) {
  const int last = nslices - 1;
  return 8 * ((last >> 3) * ntiles + ntiles - 1) + (last & 7) + 1;
}

}  // namespace evae
