// Per-range arithmetic of the gather plan, shared by the device planner (gh_gather_plan.hip)
// and by CPU code (tests/sanitize/gather_device_fuzz.cpp): one text, compiled for both.
// It restates gh_gather_plan's loop (gh_core.cpp) in a form that needs no loop over a
// range's blocks: the first block, the piece count and the j-th piece of a range are each
// found in O(log nblocks).
//
// offsets[0 .. nblocks] are the index entries as aligned u64.  rank[0 .. nblocks] counts
// the blocks that hold a symbol: rank[k] = #{k' < k : offsets[k' + 1] > offsets[k']}.  The
// host loop skips a block without symbols (pa >= pb); with `rank` the planner skips them
// too and still finds a range's j-th piece without walking: in an index of a real stream
// every block but possibly the last holds a symbol, rank[k] = k, and the j-th piece of a
// range lies in block k0 + j (one lookup confirms it); otherwise a binary search over rank
// selects the block.
#pragma once
#include <stdint.h>

#include "gaphuff.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GH_HD __host__ __device__ inline
#else
#define GH_HD inline
#endif

namespace gh {

// The last block k with offsets[k] <= lo (entry 0 is 0 <= lo); nblocks >= 1.  The loop of
// gh_gather_plan.
GH_HD uint64_t gr_first_block(const uint64_t* offsets, uint64_t nblocks, uint64_t lo) {
  uint64_t a = 0, b = nblocks;  // offsets[a] <= lo; b == nblocks or offsets[b] > lo
  while (b - a > 1) {
    const uint64_t mid = a + (b - a) / 2;
    if (offsets[mid] <= lo) a = mid; else b = mid;
  }
  return a;
}

// The first entry m > k0 with offsets[m] >= hi (entry nblocks is N >= hi): the range's
// blocks are [k0, m).  Needs offsets[k0] < hi.
GH_HD uint64_t gr_end_entry(const uint64_t* offsets, uint64_t nblocks, uint64_t k0, uint64_t hi) {
  uint64_t a = k0, b = nblocks;  // offsets[a] < hi <= offsets[b]
  while (b - a > 1) {
    const uint64_t mid = a + (b - a) / 2;
    if (offsets[mid] < hi) a = mid; else b = mid;
  }
  return b;
}

// What the planner keeps of one range.
struct RangeLoc {
  uint32_t k0;     // its first block
  uint32_t count;  // its pieces; GR_BAD_RANGE: lo > hi or hi > N
  uint64_t len;    // hi - lo (0 for a bad range)
};
constexpr uint32_t GR_BAD_RANGE = 0xFFFFFFFFu;

// Locate: validation, first block and piece count of [lo, hi).  Every block of [k0, m)
// starts before hi and, k0 being the last block that starts at or before lo, ends after
// lo: it gives a piece unless it holds no symbol.  (nblocks < 2^32 - 1: a count never
// equals GR_BAD_RANGE.)
GH_HD RangeLoc gr_locate(const uint64_t* offsets, const uint32_t* rank, uint64_t nblocks, uint64_t n,
                         uint64_t lo, uint64_t hi) {
  if (lo > hi || hi > n) return RangeLoc{0u, GR_BAD_RANGE, 0u};
  if (lo == hi) return RangeLoc{0u, 0u, 0u};  // (a non-empty range has N > 0: nblocks >= 1)
  const uint64_t k0 = gr_first_block(offsets, nblocks, lo);
  const uint64_t m = gr_end_entry(offsets, nblocks, k0, hi);
  return RangeLoc{(uint32_t)k0, rank[m] - rank[k0], hi - lo};
}

// The block of a range's j-th piece (j < count): the j-th block from k0 that holds a
// symbol.
GH_HD uint64_t gr_piece_block(const uint32_t* rank, uint64_t nblocks, uint64_t k0, uint64_t j) {
  const uint32_t want = rank[k0] + (uint32_t)j + 1u;  // rank[block + 1] == want, and the first such block
  uint64_t k = k0 + j;
  if (rank[k + 1] == want) return k;  // blocks k0 .. k0 + j all hold a symbol
  uint64_t a = k, b = nblocks - 1;    // rank[a + 1] < want <= rank[b + 1]
  while (b - a > 1) {
    const uint64_t mid = a + (b - a) / 2;
    if (rank[mid + 1] < want) a = mid; else b = mid;
  }
  return b;
}

// The piece of range [lo, hi) in `block`, the range's bytes starting at dst0 of the output:
// gh_gather_plan's {dst, block, pa - o0, pb - o0, 0} with pa = max(lo, o0), pb = min(hi, o1).
// A range's pieces are contiguous in the output, so this one starts pa - lo bytes in.
GH_HD gh_gather_piece gr_piece(const uint64_t* offsets, uint64_t block, uint64_t lo, uint64_t hi, uint64_t dst0) {
  const uint64_t o0 = offsets[block], o1 = offsets[block + 1];
  const uint64_t pa = lo > o0 ? lo : o0, pb = hi < o1 ? hi : o1;
  return gh_gather_piece{dst0 + (pa - lo), (uint32_t)block, (uint32_t)(pa - o0), (uint32_t)(pb - o0), 0u};
}

// The range of piece slot q: the last i with slot[i] <= q, slot[] being the exclusive scan of
// the ranges' counts (slot[0] = 0 <= q).  The ranges after i that share its slot are empty
// ones, and i itself is not: slot[i + 1] > q.
GH_HD uint32_t gr_piece_range(const uint32_t* slot, uint32_t nranges, uint64_t q) {
  uint32_t a = 0, b = nranges;  // slot[a] <= q; b == nranges or slot[b] > q
  while (b - a > 1) {
    const uint32_t mid = a + (b - a) / 2;
    if (slot[mid] <= q) a = mid; else b = mid;
  }
  return a;
}

// rank[] from the entries (host: gh_ctx_set_index, the CPU programs).
inline void gr_rank(const uint64_t* offsets, uint64_t nblocks, uint32_t* rank) {
  uint32_t r = 0;
  for (uint64_t k = 0; k < nblocks; ++k) {
    rank[k] = r;
    r += offsets[k + 1] > offsets[k];
  }
  rank[nblocks] = r;
}

}  // namespace gh
