// arena_check.cpp -- random alloc / release histories on the workspace planner (flowdec_amd/csrc/arena.h), stand-alone and without a GPU.
// Deterministic (its own LCG), no input.  After EVERY operation: the offset handed out is a multiple of 256, the block overlaps no live
// block, and peak() is the largest end ever handed out; after releasing everything alloc(1) is 0 again.  Built plain and under
// -fsanitize=address,undefined by tests/test_model_host_cpu.py; any violation (or sanitizer report) is a non-zero exit status.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "arena.h"

namespace {

uint64_t lcg = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(lcg >> 33);
}

struct Live { size_t off, size; };   // size: the bytes asked for (the arena reserves at least that much)

struct History {
  fdm::Arena arena;
  std::vector<Live> live;
  size_t top = 0;   // the largest end handed out so far, ends taken at the arena's own granularity of 256 bytes
  long allocs = 0;

  bool fail(const char* what, size_t a, size_t b) const {
    fprintf(stderr, "arena_check: %s (%zu, %zu) with %zu live blocks after %ld allocations\n", what, a, b, live.size(), allocs);
    return false;
  }
  bool peak_ok() const { return arena.peak() == top ? true : fail("peak() != largest end handed out", arena.peak(), top); }
  bool alloc(size_t bytes) {
    const size_t off = arena.alloc(bytes);
    const size_t held = ((bytes ? bytes : 1) + 255) / 256 * 256;
    ++allocs;
    if (off % 256 != 0) return fail("offset is not a multiple of 256", off, bytes);
    for (const Live& l : live) {
      const size_t lheld = ((l.size ? l.size : 1) + 255) / 256 * 256;
      if (off < l.off + lheld && l.off < off + held) return fail("block overlaps a live block", off, l.off);
    }
    live.push_back(Live{off, bytes});
    if (off + held > top) top = off + held;
    return peak_ok();
  }
  bool release(size_t i) {
    arena.release(live[i].off);
    live.erase(live.begin() + i);
    return peak_ok();
  }
  bool empty_again() {
    const size_t off = arena.alloc(1);
    return off == 0 ? true : fail("alloc(1) after releasing everything is not 0", off, 0);
  }
};

size_t random_size() {
  switch (rnd() % 8) {
    case 0: return 0;
    case 1: return 1 + rnd() % 255;           // below one granule
    case 2: return 256 * (1 + rnd() % 64);    // whole granules
    default: return rnd() % 5000001;          // up to ~5 MB, mostly no multiple of 256
  }
}

bool random_history() {
  History h;
  for (int op = 0; op < 400; ++op) {
    if (h.live.empty() || rnd() % 100 < 55) {
      if (!h.alloc(random_size())) return false;
    } else if (!h.release(rnd() % h.live.size())) {
      return false;
    }
  }
  while (!h.live.empty())
    if (!h.release(rnd() % h.live.size())) return false;
  return h.empty_again();
}

bool ordered_history(bool reverse) {
  History h;
  for (int i = 0; i < 400; ++i)
    if (!h.alloc(random_size())) return false;
  while (!h.live.empty())
    if (!h.release(reverse ? h.live.size() - 1 : 0)) return false;
  return h.empty_again();
}

}  // namespace

int main() {
  for (int i = 0; i < 2000; ++i)
    if (!random_history()) return 1;
  if (!ordered_history(false) || !ordered_history(true)) return 1;
  printf("arena ok: 2000 random histories of 400 operations, one released in allocation order, one in reverse\n");
  return 0;
}
