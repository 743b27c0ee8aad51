// wino4_layout.h -- layout arithmetic of the producer pass of the F(4,3) bf16 kernel (conv_wino4.hip): where the DMA puts the raw
// halo (RAW), which item a lane of the pass owns, where it reads and where it stores.  Plain constexpr C++ so that a host program
// (tests/wino4_layout_check.cpp) can check exhaustively what the kernel relies on: bank conflicts of the RAW reads and the V stores,
// every (pixel, piece) of the halo requested exactly once, every V word of a chunk written exactly once.
#pragma once

namespace fdw4 {

constexpr int NTH = 512;                            // lanes of a workgroup
constexpr int HH = 18, HW = 18;                     // halo of a 16 x 16 tile
constexpr int RROW = 20;                            // RAW: one 64-byte slot per pixel, 20 slots per halo row (18 columns + 2 pad slots);
constexpr int RROW_BYTES = RROW * 64;               // a slot holds the four 16-byte pieces [chunk parity][half] of a chunk PAIR
constexpr int RAW_PASSES = 3;                       // 18 x 20 x 4 = 1440 pieces, padded to 3 DMA passes of 512 lanes
constexpr int RAW_BYTES = RAW_PASSES * NTH * 16;
constexpr int NPIECE = HH * RROW * 4;
constexpr int VXI = HH * 4 * 32;                    // one position plane of V: [18 halo rows][4 tiles][32 B]
static_assert(NPIECE <= RAW_PASSES * NTH && RROW_BYTES % 128 == 0, "RAW layout");

// ---- RAW.  Lane k = 0..2 of an item group reads the halo columns 6 k + j, j = 0..5, of one channel pair (32-bit word 0..7 of a
// 32-byte (slot, chunk parity) quarter of the 128-byte bank row).  Slot of column c: a pad slot behind every six columns, so that
// the six columns of a third are consecutive slots (one base address + immediates) and thirds 0 / 1 / 2 start on an even / odd /
// even slot; the two pieces of a chunk parity sit at piece q = 2 parity + half, position q ^ (2 raw_flip(c)), flipped in third 2.
// For read j the three lanes of a group then hit the quarters (j & 1, e), (~j & 1, e), (j & 1, ~e): three different ones.
constexpr int raw_slot(int c) { return c + c / 6; }
constexpr int raw_flip(int c) { return c >= 12 ? 1 : 0; }
constexpr int raw_col(int ps) { return (ps == 6 || ps == 13) ? -1 : ps - ps / 7; }   // column of slot position ps of a row (-1: padding)

// request side: DMA lane sl = t + 512 i fills LDS piece sl (16 bytes) of RAW; which pixel's which source piece belongs there
struct Req { int row, col, piece; };                // col < 0: padding (any in-bounds source will do)
constexpr Req raw_request(int sl) {
  const int slot = sl >> 2, hr = slot / RROW, ps = slot - hr * RROW;
  const int hc = hr >= HH ? -1 : raw_col(ps);
  return {hr, hc, (sl & 3) ^ (hc >= 0 ? 2 * raw_flip(hc) : 0)};
}
// byte of RAW that holds channel pair `word` (0..7) of chunk parity e of halo pixel (row, c)
constexpr int raw_addr(int row, int c, int e, int word) { return row * RROW_BYTES + raw_slot(c) * 64 + ((raw_flip(c) ^ e) * 32) + word * 4; }

// ---- items of the producer pass: (halo row, word, column third k) = 18 x 8 x 3 = 432 lanes, the three lanes of a (row, word) group
// adjacent and inside one 16-lane DPP row: five groups per DPP row (lane 15 idles), 18 groups per wave (lanes 57..63 idle), all
// eight waves one pass each.  Wave w: groups 0..7 = row 2 w (words 0..7), groups 10..17 = row 2 w + 1, groups 8, 9 = two of the
// sixteen (row 16 / 17, word) groups.  So lanes 32..63 hold ONE halo row (conflict-free reads and stores) and lanes 0..31 one row
// plus two left-over groups, whose six lanes share their banks with the row's lanes of the same word (2-way) -- 30 lanes in groups
// of three same-word lanes cannot do better: a word has four quarters.
struct Item { bool active; int row, word, k; };
constexpr Item item(int t) {
  const int lane = t & 63, wave = t >> 6, l16 = lane & 15, gq = l16 / 3;
  const int g = (lane >> 4) * 5 + gq, k = l16 - 3 * gq;
  if (l16 == 15 || g >= 18) return {false, 2 * wave + (lane >> 5), 0, 0};   // idle: reads what the first lane of its 32-lane group reads (a broadcast)
  if (g < 8) return {true, 2 * wave, g, k};
  if (g >= 10) return {true, 2 * wave + 1, g - 10, k};
  const int left = 2 * wave + (g - 8);
  return {true, 16 + (left >> 3), left & 7, k};
}
// V plane offset of (halo row, tile, word): [18 rows][4 tiles][32 B], the two 16-byte halves swizzled by bit 3 of the tile index
constexpr int v_addr(int row, int tile, int word) {
  const int tidx = row * 4 + tile;
  return tidx * 32 + (((word >> 2) ^ ((tidx >> 3) & 1)) * 16) + (word & 3) * 4;
}
// tile of a lane's FIRST transform (lane 0: tile 0, lane 1: tile 1, lane 2: tile 3); lane 1's second transform is tile 2 = + 32 bytes
constexpr int first_tile(int k) { return k == 2 ? 3 : k; }
static_assert(v_addr(5, 2, 6) == v_addr(5, 1, 6) + 32 && v_addr(17, 2, 1) == v_addr(17, 1, 1) + 32, "tile 2 follows tile 1 in the same swizzle phase");

}  // namespace fdw4
