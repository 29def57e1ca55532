// fleet_order_check.cpp — pick and place of csrc/shc_fleet_order.hpp on the CPU: a stand-alone program, built with the host compiler and
// -fsanitize=address,undefined by tests/test_fleet_order.py.  Every source and destination is a heap block of exactly its size, so a word
// read or written outside it is an AddressSanitizer report; what lands inside is compared with three-line reference loops written here.
// Exit status 0 and "ok" on success.
#include "../syropod_highlevel_controller_amd/csrc/shc_fleet_order.hpp"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// a heap block of exactly n elements.  For n = 0 it is one byte: malloc(0) may return NULL, and a NULL pointer handed to memcpy or memset is
// undefined even for a length of zero; no element of that byte is ever addressed, so it hides nothing
template <class T>
static T *block(size_t n) {
  return static_cast<T *>(std::malloc(n ? n * sizeof(T) : 1));
}

// the ids of `count` rows among n: every robot, or every third from the second on
static std::vector<int64_t> ids_of(int64_t count, bool skipping) {
  std::vector<int64_t> ids;
  for (int64_t r = 0; r < count; ++r) ids.push_back(skipping ? 1 + 3 * r : r);
  return ids;
}

template <class Word>
static Word filler() {
  Word w;
  std::memset(&w, 0xAB, sizeof(Word));
  return w;
}

// PLACE: `count` rows of [legs][k] words into [n][dst_legs][dst_k], pad elsewhere in those rows, nothing in the others
template <class Word>
static void check_place(int64_t count, bool skipping, int legs, int k, int dst_legs, int dst_k) {
  const std::vector<int64_t> ids = ids_of(count, skipping);
  const int64_t n = count ? ids.back() + 2 : 3; // (a row behind the last named one)
  const size_t row = size_t(dst_legs) * dst_k, w = size_t(legs) * k;
  Word *part = block<Word>(size_t(count) * w), *dst = block<Word>(size_t(n) * row), *want = block<Word>(size_t(n) * row);
  const Word pad = Word(0x7E57), untouched = filler<Word>();
  for (size_t t = 0; t < size_t(count) * w; ++t) part[t] = Word(1000 + t);
  for (size_t t = 0; t < size_t(n) * row; ++t) dst[t] = want[t] = untouched;
  // the reference: every word of every named row
  for (int64_t r = 0; r < count; ++r)
    for (int l = 0; l < dst_legs; ++l)
      for (int j = 0; j < dst_k; ++j) want[size_t(ids[r]) * row + size_t(l) * dst_k + j] = l < legs && j < k ? part[(size_t(r) * legs + l) * k + j] : pad;
  fleet_place_host<Word>(dst, part, ids.data(), count, legs, k, dst_legs, dst_k, pad);
  size_t wrong = 0, unwritten = 0;
  for (size_t t = 0; t < size_t(n) * row; ++t) wrong += dst[t] != want[t];
  for (int64_t r = 0; r < count; ++r)
    for (size_t c = 0; c < row; ++c) unwritten += dst[size_t(ids[r]) * row + c] == untouched; // (neither a value nor the pad is 0xAB..AB)
  if (wrong || unwritten)
    std::printf("place<%zu bytes>: count %lld%s, (%d, %d) into (%d, %d): %zu words differ, %zu words of named rows unwritten\n", sizeof(Word), (long long)count,
                skipping ? " skipping" : "", legs, k, dst_legs, dst_k, wrong, unwritten);
  CHECK(wrong == 0 && unwritten == 0);
  std::free(part), std::free(dst), std::free(want);
}

// PICK: the part's (legs, k) entries of `count` rows out of a caller's array of src_robot doubles per robot
static void check_pick(int64_t count, bool skipping, const FleetRows &g) {
  const std::vector<int64_t> ids = ids_of(count, skipping);
  const int64_t n = count ? ids.back() + 1 : 0; // the caller's array ends with the last named row ...
  const size_t w = size_t(g.legs) * g.k;
  double *src = block<double>(size_t(n) * g.src_robot), *dst = block<double>(size_t(count) * w), *want = block<double>(size_t(count) * w);
  for (size_t t = 0; t < size_t(n) * g.src_robot; ++t) src[t] = double(t) + 0.5;
  std::memset(dst, 0xAB, count * w * 8);
  for (int64_t r = 0; r < count; ++r)
    for (int l = 0; l < g.legs; ++l)
      for (int j = 0; j < g.k; ++j) want[(size_t(r) * g.legs + l) * g.k + j] = src[size_t(ids[r]) * g.src_robot + size_t(l) * g.src_leg + j];
  fleet_pick_host(dst, src, ids.data(), count, g);
  const bool same = std::memcmp(dst, want, count * w * 8) == 0;
  if (!same) std::printf("pick: count %lld%s, (%d, %d) of rows of %d, leg stride %d\n", (long long)count, skipping ? " skipping" : "", g.legs, g.k, g.src_robot, g.src_leg);
  CHECK(same);
  std::free(src), std::free(dst), std::free(want);
}

int main() {
  // the row description, from a group's (per leg, width) at a part's and the fleet's geometry
  const FleetRows robot = fleet_rows(false, 4, 6, 3, 8, 5), force = fleet_rows(true, 3, 6, 3, 8, 5), effort = fleet_rows(true, 0, 6, 3, 8, 5);
  CHECK(robot.legs == 1 && robot.k == 4 && robot.src_robot == 4 && robot.src_leg == 0);
  CHECK(force.legs == 6 && force.k == 3 && force.src_robot == 24 && force.src_leg == 3);
  CHECK(effort.legs == 6 && effort.k == 3 && effort.src_robot == 40 && effort.src_leg == 5);

  // parts whose (legs, k) equal the destination's, with fewer legs, fewer joints, fewer of both - in a destination of (8, 5) rows of one word
  // and of records of 64, 42, 20 and 4 words; no row, one row, several; ids that name every row and ids that skip rows
  const int shapes[][4] = {{8, 5, 8, 5}, {6, 5, 8, 5}, {8, 3, 8, 5}, {6, 3, 8, 5}, {1, 1, 1, 1}, {8, 64, 8, 64}, {6, 64, 8, 64}, {8, 42, 8, 42},
                           {6, 42, 8, 42}, {1, 20, 1, 20}, {1, 4, 1, 4}, {3, 20, 4, 42}, {2, 4, 3, 64}};
  const int64_t counts[] = {0, 1, 7};
  for (const auto &s : shapes)
    for (int64_t count : counts)
      for (int skipping = 0; skipping < 2; ++skipping) {
        check_place<uint64_t>(count, skipping != 0, s[0], s[1], s[2], s[3]);
        check_place<uint32_t>(count, skipping != 0, s[0], s[1], s[2], s[3]);
      }

  // pick: per-robot groups of every width, the two per-leg groups for the same four kinds of part
  const int geometry[][2] = {{8, 5}, {6, 5}, {8, 3}, {6, 3}};
  for (int64_t count : counts)
    for (int skipping = 0; skipping < 2; ++skipping) {
      for (int width = 1; width <= 4; ++width) check_pick(count, skipping != 0, fleet_rows(false, width, 6, 3, 8, 5));
      for (const auto &g : geometry)
        for (int width : {3, 0}) check_pick(count, skipping != 0, fleet_rows(true, width, g[0], g[1], 8, 5));
    }

  // the scratch buffer: aligned, grows, keeps its address while it does not have to grow
  FleetScratch scratch;
  char *a = scratch.room(100);
  CHECK(reinterpret_cast<uintptr_t>(a) % 16 == 0);
  std::memset(a, 1, 100);
  CHECK(scratch.room(40) == a);
  char *b = scratch.room(100000);
  CHECK(reinterpret_cast<uintptr_t>(b) % 16 == 0);
  std::memset(b, 2, 100000);
  CHECK(scratch.room(0) == b);

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
