// Segment transition functions of a gap-less (raw) stream, shared by the batched raw load's
// kernels (gh_batch_raw.hip) and by CPU code (gh_batchraw_gaps_host in gh_core.cpp,
// tests/sanitize/batch_raw_fuzz.cpp): one text, compiled for both.
//
// A codeword has at most 16 bits, so the entry of segment j (its first codeword start at or
// after bit 128 j, minus 128 j) lies in 0..15, and a segment is a total function on 16 states:
//   T_j(x) = (the first position >= 128 (j + 1) reached by the walk that starts at bit
//            128 j + x) - 128 (j + 1),
// packed into one u64, nibble x holding T_j(x).  e_0 = 0 and e_{j+1} = T_j(e_j); composition
// is associative, so every entry comes from a prefix scan of composed functions.  Only T_j at
// the true entry ever reaches a result: walks that start inside a codeword need only
// terminate (every step advances 1..16 bits) and stay inside bits [128 j, 128 j + 160).
#pragma once
#include <stdint.h>

#ifndef GH_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GH_HD __host__ __device__ inline
#else
#define GH_HD inline
#endif
#endif

namespace gh {

constexpr uint32_t TRANS_SEG_BITS = 128;
constexpr unsigned long long TRANS_IDENTITY = 0xFEDCBA9876543210ull;  // nibble x holds x

GH_HD unsigned long long trans_identity() { return TRANS_IDENTITY; }

// f(x), x in 0..15.
GH_HD uint32_t trans_apply(unsigned long long f, uint32_t x) { return (uint32_t)(f >> (4u * (x & 15u))) & 15u; }

// `then` after `first`: nibble x = then(first(x)).  Not commutative.
GH_HD unsigned long long trans_compose(unsigned long long first, unsigned long long then) {
  unsigned long long r = 0;
  for (uint32_t x = 0; x < 16; ++x) r |= (unsigned long long)trans_apply(then, trans_apply(first, x)) << (4u * x);
  return r;
}

// T(x) of one segment.  next() returns the length (1..16) of the codeword at the walk's
// position and moves the walk past it; the walk starts x bits into the segment.  With
// lengths in 1..16 it ends after at most 128 steps, at most 15 bits past the segment; the
// step bound and the mask keep the loop finite and the result a nibble whatever next() gives.
template <class Next>
GH_HD uint32_t trans_walk(uint32_t x, Next&& next) {
  uint32_t pos = x & 15u;
  for (uint32_t it = 0; it < TRANS_SEG_BITS && pos < TRANS_SEG_BITS; ++it) pos += next();
  return (pos - TRANS_SEG_BITS) & 15u;
}

// x's nibble of a function: the 16 walks' results are ORed into one u64.
GH_HD unsigned long long trans_nibble(uint32_t x, uint32_t t) { return (unsigned long long)(t & 15u) << (4u * (x & 15u)); }

}  // namespace gh
