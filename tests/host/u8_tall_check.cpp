// Check of the byte layer's block-height rule (u8_fwd_block_rows, csrc/evae_tile_map.h) on the CPU (plain C++, no HIP), over
// M = 1 .. 30 000 in steps that hit every residue mod 64, 1 .. 20 column tiles and 64 / 228 / 256 / 304 CUs:
//   it returns 128, 256 or 448; 448 only where 448-row blocks take fewer rounds than 256-row blocks; everywhere else it is the
//   choice the launcher made before 448 existed (256 rows once those blocks fill the machine, else 128); and the two launches
//   the rule was written for come out as 448 (19 968 rows x 5 tiles on 256 CUs) and 256 (25 000 x 5 on 256).
// Exit status 0 = all hold.
#include <cstdio>

#include "evae_tile_map.h"

using namespace evae;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (++failures <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                           \
  } while (0)

static int cdiv(const int a, const int b) { return (a + b - 1) / b; }
static int rounds(const int M, const int tn, const int cus, const int h) { return cdiv(cdiv(M, h) * tn, cus); }
// the launcher's choice before the 448-row instance
static int before(const int M, const int tn, const int cus) { return cdiv(M, 256) * tn >= cus ? 256 : 128; }

int main() {
  const int cu_counts[4] = {64, 228, 256, 304};
  long n448 = 0, ncases = 0;
  bool residue[64] = {false};
  for (int M = 1; M <= 30000; M += (M < 1200 ? 1 : 63)) {      // 63 is coprime to 64: every residue, again and again
    residue[M & 63] = true;
    for (int tn = 1; tn <= 20; ++tn)
      for (int c = 0; c < 4; ++c) {
        const int cus = cu_counts[c];
        const int h = u8_fwd_block_rows(M, tn, cus);
        ++ncases;
        CHECK(h == 128 || h == 256 || h == 448, "M=%d tn=%d cus=%d -> %d", M, tn, cus, h);
        CHECK(u8_fwd_rounds(M, tn, cus, 256) == rounds(M, tn, cus, 256) && u8_fwd_rounds(M, tn, cus, 448) == rounds(M, tn, cus, 448),
              "M=%d tn=%d cus=%d: round count", M, tn, cus);
        if (h == 448) {
          ++n448;
          CHECK(rounds(M, tn, cus, 448) < rounds(M, tn, cus, 256), "M=%d tn=%d cus=%d: 448 with %d rounds against %d", M, tn, cus,
                rounds(M, tn, cus, 448), rounds(M, tn, cus, 256));
          CHECK(before(M, tn, cus) == 256, "M=%d tn=%d cus=%d: 448 for a launch that does not fill the machine", M, tn, cus);
        } else {
          CHECK(h == before(M, tn, cus), "M=%d tn=%d cus=%d -> %d, was %d", M, tn, cus, h, before(M, tn, cus));
        }
      }
  }
  for (int r = 0; r < 64; ++r) CHECK(residue[r], "residue %d of M mod 64 never visited", r);
  CHECK(n448 > 0, "448 never chosen in %ld cases", ncases);
  CHECK(u8_fwd_block_rows(19968, 5, 256) == 448, "c2 step: %d", u8_fwd_block_rows(19968, 5, 256));
  CHECK(u8_fwd_block_rows(25000, 5, 256) == 256, "25 000 rows: %d", u8_fwd_block_rows(25000, 5, 256));
  CHECK(u8_fwd_block_rows(4200, 16, 256) == 448, "4 200 rows x 16 tiles: %d", u8_fwd_block_rows(4200, 16, 256));
  if (failures) std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
