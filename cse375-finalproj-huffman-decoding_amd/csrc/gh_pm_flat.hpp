// The boundary package-merge in its level-by-level ("flat") form, shared by the batched
// encoder's code kernel (gh_ebatch.hip) and by CPU code (gh_package_merge_flat in gh_core.cpp,
// tests/sanitize/pm_flat_fuzz.cpp): one text, compiled for both.
//
// gh_package_merge (gh_core.cpp) restates the reference's lazily evaluated lists.  Its tie
// rule is uniform: at every level a pending package is taken when its weight is <= the next
// leaf, and the top selection takes the leaf only when the package is strictly heavier.  So
// its lengths are those of the textbook package-merge with "package first on ties" and every
// list cut to its first 2n - 2 items (tests/test_pm_flat.py compares the two).
//
// For n >= 2 counts c[0 .. n) sorted ascending, need = 2n - 2:
//   level 1      the leaves, m_1 = n items;
//   level l > 1  packages P[i] = prev[2i] + prev[2i + 1], i < floor(m_{l-1} / 2), merged with
//                the leaves: package i at position i + #{j : c[j] < P[i]}, leaf j at position
//                j + #{i : P[i] <= c[j]}; items at positions >= need are dropped, so
//                m_l = min(need, n + floor(m_{l-1} / 2)).  Both lists are sorted, so both
//                counts are binary searches and every item of a level is placed on its own.
//                A level keeps one bit per kept position: leaf or package;
//   trace        take = need at level 16; at each level nl = leaves among the first
//                min(take, m_l) items, every leaf j < nl gains one bit of length, and
//                take = 2 (items looked at - nl) for the level below.
//                len[j] = #{l : j < nl_l}.
// n = 1 gives length 1, n = 0 no code (the callers' business: pm_need is 0 for both and the
// functions below then place and count nothing).
//
// Weights are u64: a level-l package weighs at most 2^(l-1) times the largest count, so
// counts below 2^48 never wrap (a batch holds fewer than 2^41 bytes).
#pragma once
#include <stdint.h>

#include "gaphuff.h"

#ifndef GH_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GH_HD __host__ __device__ inline
#else
#define GH_HD inline
#endif
#endif

namespace gh {

constexpr uint32_t PM_LEVELS = GH_MAX_CODE_LEN;
constexpr uint32_t PM_MAX_ITEMS = 2 * GH_MAX_SYMBOLS - 2;  // 510: the longest list
constexpr uint32_t PM_MASK_WORDS = 16;                     // u32 words of a level's leaf mask
static_assert(PM_MAX_ITEMS <= 32 * PM_MASK_WORDS, "a level's mask holds every position");

// Items every list is cut to.
GH_HD uint32_t pm_need(uint32_t n) { return n >= 2 ? 2 * n - 2 : 0u; }

// Items of the level above one of m_prev items.
GH_HD uint32_t pm_next_items(uint32_t n, uint32_t m_prev) {
  const uint32_t m = n + m_prev / 2, need = pm_need(n);
  return m < need ? m : need;
}

// Package i of the level above `prev` (i < floor(m_prev / 2)).
GH_HD uint64_t pm_package(const uint64_t* prev, uint32_t i) { return prev[2 * i] + prev[2 * i + 1]; }

// #{j < n : c[j] < x}
GH_HD uint32_t pm_leaves_below(const uint64_t* c, uint32_t n, uint64_t x) {
  uint32_t a = 0, b = n;  // c[j] < x for j < a, c[j] >= x for j >= b
  while (a < b) {
    const uint32_t mid = (a + b) / 2;
    if (c[mid] < x) a = mid + 1; else b = mid;
  }
  return a;
}

// #{i < np : P[i] <= x}, the packages formed from `prev` as they are compared
GH_HD uint32_t pm_packages_upto(const uint64_t* prev, uint32_t np, uint64_t x) {
  uint32_t a = 0, b = np;  // P[i] <= x for i < a, P[i] > x for i >= b
  while (a < b) {
    const uint32_t mid = (a + b) / 2;
    if (pm_package(prev, mid) <= x) a = mid + 1; else b = mid;
  }
  return a;
}

// Position of leaf j in the level above `prev` (np packages): after the packages that are
// not heavier.
GH_HD uint32_t pm_leaf_pos(const uint64_t* c, const uint64_t* prev, uint32_t np, uint32_t j) {
  return j + pm_packages_upto(prev, np, c[j]);
}

// Position of a package of weight P, the i-th of its level: before the leaves of its weight.
GH_HD uint32_t pm_package_pos(const uint64_t* c, uint32_t n, uint32_t i, uint64_t P) {
  return i + pm_leaves_below(c, n, P);
}

// Leaves among the first k <= PM_MAX_ITEMS items of a level: mask = its PM_MASK_WORDS words
// (bit p: position p holds a leaf), pre[w] = bits set in the words before w.
GH_HD uint32_t pm_leaves_before(const uint32_t* mask, const uint32_t* pre, uint32_t k) {
  const uint32_t w = k >> 5, r = k & 31u;
  return pre[w] + (r ? (uint32_t)__builtin_popcount(mask[w] & ((1u << r) - 1u)) : 0u);
}

// pre[] of one level's mask.
GH_HD void pm_mask_prefix(const uint32_t* mask, uint32_t* pre) {
  uint32_t s = 0;
  for (uint32_t w = 0; w < PM_MASK_WORDS; ++w) {
    pre[w] = s;
    s += (uint32_t)__builtin_popcount(mask[w]);
  }
}

// The trace.  mask / pre: PM_LEVELS x PM_MASK_WORDS words, row l - 1 for level l (row 0 is
// not read: level 1 holds leaves only).  nl[l - 1] = leaves of level l that are active.
GH_HD void pm_trace(const uint32_t* mask, const uint32_t* pre, uint32_t n, uint32_t* nl) {
  uint32_t m[PM_LEVELS];
  m[0] = n >= 2 ? n : 0u;
  for (uint32_t l = 1; l < PM_LEVELS; ++l) m[l] = pm_next_items(n, m[l - 1]);
  uint32_t take = pm_need(n);
  for (uint32_t l = PM_LEVELS; l-- > 0;) {
    const uint32_t looked = take < m[l] ? take : m[l];
    const uint32_t k = l ? pm_leaves_before(mask + l * PM_MASK_WORDS, pre + l * PM_MASK_WORDS, looked) : looked;
    nl[l] = k;
    take = 2 * (looked - k);
  }
}

// Length of the leaf of sorted rank j (n >= 2).
GH_HD uint32_t pm_length(const uint32_t* nl, uint32_t j) {
  uint32_t len = 0;
  for (uint32_t l = 0; l < PM_LEVELS; ++l) len += j < nl[l];
  return len;
}

// The canonical code by length (build_canon's assignment, gh_core.cpp): cnt[l] symbols of
// length l, l = 1 .. 16 (cnt[0] is not read).  base[l]: the first code of length l, first[l]:
// the file position (most frequent first, lengths non-decreasing) of the symbol that gets it.
GH_HD void pm_canon_bases(const uint32_t* cnt, uint32_t* base, uint32_t* first) {
  uint32_t code = 0, at = 0;
  base[0] = first[0] = 0;
  for (uint32_t l = 1; l <= PM_LEVELS; ++l) {
    code <<= 1;
    base[l] = code;
    first[l] = at;
    code += cnt[l];
    at += cnt[l];
  }
}

// The encoder's table entry of the symbol at file position f with length l: the code
// left-aligned, code << (32 - l) | l; 0 for a length outside 1 .. 16 (never expected).
GH_HD uint32_t pm_canon_entry(const uint32_t* base, const uint32_t* first, uint32_t f, uint32_t l) {
  if (l < 1 || l > PM_LEVELS) return 0u;
  return ((base[l] + (f - first[l])) << (32u - l)) | l;
}

}  // namespace gh
