// Host check of flowdec_amd/csrc/wino4_layout.h: what the producer pass of the F(4,3) bf16 kernel (conv_wino4.hip) relies on, exhaustively.
//   1. banks: in every 32-lane group of every RAW read (6 columns x 2 chunk parities) and of every V store (2 transforms), the lanes
//      of one halo row hit distinct banks; lanes 32..63 of a wave hit 32 distinct banks or broadcast; in lanes 0..31 only the six
//      lanes of the two left-over (row 16 / 17) groups share a bank, each with exactly one other lane;
//   2. every (halo pixel, 16-byte piece) is requested exactly once by the three DMA passes, and every read of the pass finds the
//      bytes of its (row, column, chunk parity, word) at the address it uses;
//   3. every V word of a chunk is written exactly once, from the six halo columns of its tile, and the lanes that exchange words
//      are neighbours inside one 16-lane DPP row.
// Stand-alone: c++ -std=c++17 -I flowdec_amd/csrc tests/wino4_layout_check.cpp (tests/test_wino4_layout.py runs it under ASan + UBSan).
#include <cstdio>
#include <cstring>
#include <vector>

#include "wino4_layout.h"

using namespace fdw4;

static int failures = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (++failures <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                         \
  } while (0)

struct Access { int addr; int row; bool leftover; };

// one LDS instruction of one 32-lane group: addresses of the participating lanes
static void check_banks(const std::vector<Access>& acc, bool upper_half, const char* what, int wave, int j, int e) {
  int count[32] = {0}, first_addr[32];
  int shared_banks = 0;
  std::vector<int> distinct;   // distinct dword addresses (equal addresses are one broadcast access)
  for (const Access& a : acc) {
    bool seen = false;
    for (int d : distinct) seen = seen || d == a.addr / 4;
    if (!seen) distinct.push_back(a.addr / 4);
  }
  for (int d : distinct) {
    const int bank = d % 32;
    if (count[bank]++ == 0) first_addr[bank] = d;
  }
  for (int bk = 0; bk < 32; ++bk) {
    CHECK(count[bk] <= 2, "%s wave %d j %d e %d: bank %d is hit by %d addresses", what, wave, j, e, bk, count[bk]);
    if (count[bk] == 2) ++shared_banks;
  }
  if (upper_half) CHECK(shared_banks == 0, "%s wave %d j %d e %d: lanes 32..63 have %d shared banks", what, wave, j, e, shared_banks);
  else CHECK(shared_banks <= 6, "%s wave %d j %d e %d: lanes 0..31 have %d shared banks (two left-over groups = at most 6)", what, wave, j, e, shared_banks);
  // the lanes of one halo row never share a bank, and a shared bank always involves a left-over lane
  for (size_t x = 0; x < acc.size(); ++x)
    for (size_t y = x + 1; y < acc.size(); ++y) {
      if (acc[x].addr / 4 == acc[y].addr / 4 || (acc[x].addr / 4) % 32 != (acc[y].addr / 4) % 32) continue;
      CHECK(acc[x].row != acc[y].row, "%s wave %d j %d e %d: two lanes of halo row %d share bank %d", what, wave, j, e, acc[x].row, (acc[x].addr / 4) % 32);
      CHECK(acc[x].leftover != acc[y].leftover, "%s wave %d j %d e %d: a conflict without exactly one left-over lane", what, wave, j, e);
    }
  (void)first_addr;
}

int main() {
  // ---- 2. request side ---------------------------------------------------------------------------------------------------
  {
    std::vector<int> req(HH * HW * 4, 0);
    for (int sl = 0; sl < RAW_PASSES * NTH; ++sl) {
      const Req r = raw_request(sl);
      if (r.col < 0) continue;
      CHECK(r.row >= 0 && r.row < HH && r.col < HW && r.piece >= 0 && r.piece < 4, "request %d out of range", sl);
      if (r.row >= 0 && r.row < HH && r.col < HW && r.piece >= 0 && r.piece < 4) ++req[(r.row * HW + r.col) * 4 + r.piece];
    }
    for (int i = 0; i < HH * HW * 4; ++i) CHECK(req[i] == 1, "pixel (%d, %d) piece %d is requested %d times", i / 4 / HW, i / 4 % HW, i % 4, req[i]);
    // a read of (row, c, e, word) lands in the LDS piece that the DMA filled with source piece 2 e + half of that pixel
    for (int row = 0; row < HH; ++row)
      for (int c = 0; c < HW; ++c)
        for (int e = 0; e < 2; ++e)
          for (int word = 0; word < 8; ++word) {
            const int byte = raw_addr(row, c, e, word);
            CHECK(byte >= 0 && byte + 4 <= RAW_BYTES && byte < 65536, "RAW address %d out of range", byte);
            const Req r = raw_request(byte / 16);
            CHECK(r.row == row && r.col == c && r.piece == 2 * e + (word >> 2) && byte % 16 == (word & 3) * 4,
                  "read of (%d, %d, parity %d, word %d) at byte %d finds (%d, %d, piece %d)", row, c, e, word, byte, r.row, r.col, r.piece);
          }
  }
  // ---- 3. items, exchange, V words ---------------------------------------------------------------------------------------------
  {
    std::vector<int> items(HH * 8 * 3, 0), vword(VXI / 4, 0);
    for (int t = 0; t < NTH; ++t) {
      const Item it = item(t);
      CHECK(it.row >= 0 && it.row < HH && it.word >= 0 && it.word < 8 && it.k >= 0 && it.k < 3, "item of lane %d out of range", t);
      if (!it.active) continue;
      ++items[(it.row * 8 + it.word) * 3 + it.k];
      // neighbours: lane - k .. lane - k + 2 are the group, inside one 16-lane row
      const int t0 = t - it.k;
      CHECK((t0 >> 4) == ((t0 + 2) >> 4), "group of lane %d straddles a 16-lane row", t);
      for (int k = 0; k < 3; ++k) {
        const Item n = item(t0 + k);
        CHECK(n.active && n.row == it.row && n.word == it.word && n.k == k, "lane %d is not lane %d of the group of lane %d", t0 + k, k, t);
      }
      // first transform: tile first_tile(k) from columns 4 tile .. 4 tile + 5
      const int tile = first_tile(it.k);
      int cols[6];
      for (int j = 0; j < 6; ++j) cols[j] = it.k == 1 ? (j < 2 ? 6 * 0 + 4 + j /* from lane 0: its words 4, 5 */ : 6 + (j - 2)) : 6 * it.k + j;
      for (int j = 0; j < 6; ++j) CHECK(cols[j] == 4 * tile + j, "lane %d: input %d of tile %d is column %d", t, j, tile, cols[j]);
      const int va = v_addr(it.row, tile, it.word);
      CHECK(va >= 0 && va + 4 <= VXI && va % 4 == 0, "V address %d out of range", va);
      if (va >= 0 && va + 4 <= VXI) ++vword[va / 4];
      if (it.k == 1) {   // second transform: tile 2 = own words 2 .. 5 (columns 8 .. 11), words 0, 1 of lane 2 (columns 12, 13), 32 bytes on
        for (int j = 0; j < 6; ++j) CHECK((j < 4 ? 6 + 2 + j : 12 + (j - 4)) == 4 * 2 + j, "lane %d: input %d of tile 2", t, j);
        CHECK(va + 32 == v_addr(it.row, 2, it.word), "lane %d: tile 2 is not 32 bytes behind tile 1", t);
        if (va + 36 <= VXI) ++vword[(va + 32) / 4];
      }
    }
    for (int i = 0; i < HH * 8 * 3; ++i) CHECK(items[i] == 1, "item (row %d, word %d, third %d) is owned by %d lanes", i / 24, i / 3 % 8, i % 3, items[i]);
    for (int i = 0; i < VXI / 4; ++i) CHECK(vword[i] == 1, "V word %d is written %d times", i, vword[i]);
    int per_wave[8] = {0};
    for (int t = 0; t < NTH; ++t) per_wave[t >> 6] += item(t).active ? 1 : 0;
    for (int w = 0; w < 8; ++w) CHECK(per_wave[w] == 54, "wave %d holds %d items", w, per_wave[w]);
  }
  // ---- 1. banks ------------------------------------------------------------------------------------------------------------
  for (int wave = 0; wave < 8; ++wave)
    for (int half = 0; half < 2; ++half) {
      const int tb = wave * 64 + half * 32;
      for (int e = 0; e < 2; ++e)
        for (int j = 0; j < 6; ++j) {   // every lane reads (idle lanes repeat an active lane's address)
          std::vector<Access> acc;
          for (int t = tb; t < tb + 32; ++t) {
            const Item it = item(t);
            acc.push_back({raw_addr(it.row, 6 * it.k + j, e, it.word), it.row, it.row >= 16});
          }
          check_banks(acc, half == 1, "RAW read", wave, j, e);
        }
      for (int second = 0; second < 2; ++second) {   // stores: active lanes (first transform), middle lanes (second)
        std::vector<Access> acc;
        for (int t = tb; t < tb + 32; ++t) {
          const Item it = item(t);
          if (!it.active || (second && it.k != 1)) continue;
          acc.push_back({v_addr(it.row, first_tile(it.k), it.word) + 32 * second, it.row, it.row >= 16});
        }
        check_banks(acc, half == 1, "V store", wave, second, 0);
      }
    }
  if (failures) {
    std::printf("wino4_layout_check: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("wino4_layout_check: OK\n");
  return 0;
}
