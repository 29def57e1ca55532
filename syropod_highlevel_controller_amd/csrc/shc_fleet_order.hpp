// shc_fleet_order.hpp — the translation between the caller's rows and a part's rows of a fleet, stated once.  Plain host C++, no HIP: included
// by shc_fleet.hpp, and on its own by tests/fleet_order_check.cpp.
//
// A fleet presents its robots in the caller's instance order, rows padded to (max_legs, max_dof); a part (one engine per morphology bin and
// device) holds its own robots densely, rows of its own (legs, dof), and knows the caller's instance of each as ids[r], ascending.  The parts'
// ids partition [0, n).  Every fleet call that moves per-robot data does one of two things:
//   PICK   the part's rows out of the caller's padded array (inputs; the padding is never read),
//   PLACE  the part's dense rows into the caller's padded array at ids[r], every word of the row written, `pad` where the part lacks the leg
//          or joint (outputs).
// The device route does both with a kernel on the part's stream (fleet_pack_inputs_kernel, fleet_place_kernel of shc_fleet_io.hpp), the host
// route with the two loops below - the same row description (FleetRows), the same contract.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// The rows of one input array: a part's robot takes legs x k doubles of the src_robot doubles the caller's array holds per robot, leg l starting
// src_leg doubles into them.
struct FleetRows {
  int32_t legs, k;   // per robot of the part
  int32_t src_robot; // doubles per robot in the caller's array
  int32_t src_leg;   // doubles per leg there (per-robot inputs: legs = 1)
};
// ... of an input group that is per leg or per robot and `width` doubles wide (0: the joints of the longest leg - an entry of the group table of
// shc_inputs.hpp), for a part of (legs, dof) in a fleet of (max_legs, max_dof)
constexpr FleetRows fleet_rows(bool per_leg, int width, int legs, int dof, int max_legs, int max_dof) {
  const int k = width ? width : dof, src_k = width ? width : max_dof;
  return per_leg ? FleetRows{legs, k, max_legs * src_k, src_k} : FleetRows{1, k, k, 0};
}

// PICK: dst[r][l][j] = src[ids[r] * src_robot + l * src_leg + j] for the `rows` robots of a part; one run per robot where the part's legs lie
// back to back in the caller's row, else one per leg.
inline void fleet_pick_host(double *dst, const double *src, const int64_t *ids, int64_t rows, const FleetRows &g) {
  const size_t w = size_t(g.legs) * g.k;
  for (int64_t r = 0; r < rows; ++r, dst += w) {
    const double *row = src + ids[r] * g.src_robot;
    if (g.legs == 1 || g.src_leg == g.k) {
      std::memcpy(dst, row, w * 8);
      continue;
    }
    for (int l = 0; l < g.legs; ++l) std::memcpy(dst + size_t(l) * g.k, row + size_t(l) * g.src_leg, size_t(g.k) * 8);
  }
}

// PLACE: `count` rows of a part ([count][legs][k] words, dense) into dst ([n][dst_legs][dst_k] words) at the rows ids[0 .. count) - the contract
// of fleet_place_kernel: every word of each of those rows is written, `pad` where the part has no such leg or joint.  One run for the part's
// legs where k == dst_k (the whole row when legs == dst_legs too), else one per leg.
template <class Word>
inline void fleet_place_host(Word *dst, const Word *part, const int64_t *ids, int64_t count, int legs, int k, int dst_legs, int dst_k, Word pad) {
  const size_t row = size_t(dst_legs) * dst_k, w = size_t(legs) * k;
  for (int64_t r = 0; r < count; ++r, part += w) {
    Word *out = dst + ids[r] * row;
    if (k == dst_k) {
      std::memcpy(out, part, w * sizeof(Word));
    } else {
      for (int l = 0; l < legs; ++l) {
        std::memcpy(out + size_t(l) * dst_k, part + size_t(l) * k, size_t(k) * sizeof(Word));
        std::fill(out + size_t(l) * dst_k + k, out + size_t(l + 1) * dst_k, pad);
      }
    }
    std::fill(out + size_t(legs) * dst_k, out + row, pad);
  }
}

// The host route's dense rows of one part: one byte buffer per fleet, grown on demand and never shrunk.  room() is 16-byte aligned, and so is
// every piece a walk cuts from it (records are multiples of 16 bytes).
struct FleetScratch {
  std::vector<char> bytes;
  char *room(size_t n) {
    if (bytes.size() < n + 15) bytes.resize(n + 15);
    return bytes.data() + (-reinterpret_cast<uintptr_t>(bytes.data()) & 15);
  }
};
