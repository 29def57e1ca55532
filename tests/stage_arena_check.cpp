// stage_arena_check.cpp — StageArena (csrc/shc_stage.hpp) on the CPU: a stand-alone program, built with the host compiler and
// -fsanitize=address,undefined by tests/test_stage_arena.py.  The arena's bytes are a real heap block, and every take is written
// end to end, so a take that passed the capacity is also an AddressSanitizer report.  Exit status 0 and "ok" on success.
#define SHC_STAGE_ARENA_ONLY
#include "../syropod_highlevel_controller_amd/csrc/shc_stage.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

struct Take {
  size_t at, bytes;
};
static const size_t npos = StageArena::npos;

// a take that fits: aligned address, inside the capacity, apart from every live take; its bytes are written
static void check_take(StageArena &a, std::vector<Take> &live, size_t at, size_t bytes, size_t align) {
  CHECK(at != npos);
  if (at == npos) return;
  CHECK((reinterpret_cast<uintptr_t>(a.base) + at) % align == 0);
  CHECK(at <= a.capacity && bytes <= a.capacity - at);
  CHECK(a.cursor == at + bytes);
  for (const Take &t : live) CHECK(at + bytes <= t.at || t.at + t.bytes <= at || bytes == 0 || t.bytes == 0);
  std::memset(a.base + at, int(live.size() + 1), bytes);
  live.push_back(Take{at, bytes});
}

int main() {
  const size_t capacity = 1000; // no multiple of any alignment
  for (size_t skew = 0; skew < 16; ++skew) { // the base address itself at every offset from a 16-byte boundary
    char *block = static_cast<char *>(std::aligned_alloc(16, 1024));
    StageArena a{block + skew, capacity, 0};
    std::vector<Take> live;

    // alignment of every take for 4, 8 and 16 bytes, odd sizes in between, no overlap, nothing past the capacity
    const size_t sizes[] = {1, 4, 7, 24, 3, 40, 8, 17}, aligns[] = {4, 8, 16};
    for (size_t s : sizes)
      for (size_t al : aligns) check_take(a, live, a.take(s, al), s, al);

    // zero-size takes work: they fit, are aligned, and move the cursor by their padding at most
    const size_t before_zero = a.cursor;
    check_take(a, live, a.take(0, 16), 0, 16);
    CHECK(a.cursor - before_zero < 16);
    check_take(a, live, a.take(size_t(0), size_t(8), size_t(8)), 0, 8);

    // a take that does not fit says so and leaves the cursor where it was - by one byte, by far, and by its padding alone
    const size_t cursor = a.cursor, room = a.capacity - a.cursor;
    CHECK(a.take(room + 1, 1) == npos && a.cursor == cursor);
    CHECK(a.take(capacity * 2, 4) == npos && a.cursor == cursor);
    CHECK(a.take(npos, 1) == npos && a.cursor == cursor);
    CHECK(a.take(npos - 8, 16) == npos && a.cursor == cursor);
    // count * size overflow is refused (each product wraps to a small number that would fit)
    CHECK(a.take(npos / 8 + 2, 8, 8) == npos && a.cursor == cursor);
    CHECK(a.take(npos / 2 + 1, 2, 4) == npos && a.cursor == cursor);
    CHECK(a.take(size_t(1) << 62, 16, 16) == npos && a.cursor == cursor);
    CHECK(a.take(npos, 152, 16) == npos && a.cursor == cursor);
    // ... and what is left can still be taken to the last byte
    check_take(a, live, a.take(room, 1), room, 1);
    CHECK(a.cursor == capacity);
    CHECK(a.take(1, 1) == npos && a.cursor == capacity);
    check_take(a, live, a.take(0, 1), 0, 1);

    // release(mark) restores the cursor exactly under three levels of nesting; a take after a release reuses the bytes
    a.release(0);
    live.clear();
    check_take(a, live, a.take(13, 4), 13, 4);
    const size_t m1 = a.mark();
    check_take(a, live, a.take(5, 3, 8), 15, 8);
    const size_t m2 = a.mark();
    check_take(a, live, a.take(33, 16), 33, 16);
    const size_t m3 = a.mark();
    check_take(a, live, a.take(100, 4), 100, 4);
    const size_t inner = live.back().at;
    a.release(m3);
    live.pop_back();
    CHECK(a.cursor == m3 && a.mark() == m3);
    check_take(a, live, a.take(100, 4), 100, 4);
    CHECK(live.back().at == inner); // the same bytes again
    a.release(m3);
    live.pop_back();
    CHECK(a.take(capacity, 4) == npos && a.cursor == m3); // (a refusal inside a nested scope moves nothing either)
    a.release(m2);
    live.pop_back();
    CHECK(a.cursor == m2);
    check_take(a, live, a.take(64, 8), 64, 8); // over what the two inner levels held
    a.release(m2);
    live.pop_back();
    a.release(m1);
    live.pop_back();
    CHECK(a.cursor == m1 && m1 == 13 + live[0].at);
    check_take(a, live, a.take(capacity - m1, 1), capacity - m1, 1);
    a.release(0);
    CHECK(a.cursor == 0);

    std::free(block);
  }
  // an arena of no bytes (a call without an engine): only zero-size takes fit
  StageArena none{nullptr, 0, 0};
  CHECK(none.take(1, 1) == npos && none.take(8, 8, 16) == npos && none.cursor == 0);
  CHECK(none.take(0, 16) == 0 && none.cursor == 0);

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
