// Per-range arithmetic of the element gather (gh_pgather_*, gaphuff.h "element gather"), shared
// by the device kernels (gh_planes_gather.hip), the host plan (gh_pgather_plan, gh_core.cpp) and
// CPU code (tests/sanitize/planes_gather_fuzz.cpp): one text, compiled for all three.
//
// An element range (tensor, lo, hi) of a tensor with C coded planes out of E becomes C byte
// ranges (stream[p], lo, hi) of the batch, in plane order; the batched gather writes them one
// after another into a staging buffer, so coded plane c (the c-th set bit of the mask) of the
// range lies at stage_off + c * (hi - lo), stage_off being the prefix of (hi - lo) * C over the
// ranges before it: the dst0 the batched gather's own scan gives the range's first byte range.
// The range join then interleaves the staged planes with the stored planes' bytes [lo, hi) into
// (hi - lo) * E bytes at dst_off, the prefix of (hi - lo) * E.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (uint4: the device side's 16-byte accesses)
#endif
#include <stdint.h>

#include <cstring>

#include "gaphuff.h"
#include "gh_planes.hpp"

namespace gh {

// 8 byte ranges per element range at the most, and the batched gather takes GH_GATHER_MAX_RANGES.
constexpr uint32_t PG_MAX_RANGES = GH_GATHER_MAX_RANGES / PLANES_MAX_E;
static_assert(PG_MAX_RANGES == GH_PGATHER_MAX_RANGES, "the header states the limit");
// A tensor of the list holds fewer bytes than this, so that no sum over PG_MAX_RANGES ranges
// overflows 64 bits.
constexpr uint64_t PG_MAX_TENSOR_BYTES = 1ull << 40;

GH_HD uint32_t pg_popc(uint32_t m) {
  uint32_t c = 0;
  for (; m; m &= m - 1) ++c;
  return c;
}

// What one element range adds to the four prefixes.  count == PG_BAD: an invalid range.
constexpr uint32_t PG_BAD = 0xFFFFFFFFu;
struct PgLoc {
  uint64_t stage;    // (hi - lo) * C
  uint64_t dst;      // (hi - lo) * E
  uint64_t units;    // ceil((hi - lo) / 1024)
  uint32_t ncoded;   // C, or PG_BAD
  uint32_t flagged;  // valid, and a coded plane's stream has a non-zero status word
};

// tensor_of(t): the PlanesTensor of tensor t < ntensors; status_of(s): stream s's status word.
template <class TensorOf, class StatusOf>
GH_HD PgLoc pg_locate(TensorOf tensor_of, StatusOf status_of, uint32_t ntensors, const gh_erange& r) {
  if (r.tensor >= ntensors || r.lo > r.hi) return PgLoc{0, 0, 0, PG_BAD, 0};
  const PlanesTensor& d = tensor_of((uint32_t)r.tensor);
  if (r.hi > d.nelem) return PgLoc{0, 0, 0, PG_BAD, 0};
  const uint64_t len = r.hi - r.lo;
  const uint32_t c = pg_popc(d.mask);
  uint32_t st = 0;
  for (uint32_t q = 0; q < PLANES_MAX_E; ++q)
    if ((d.mask >> q) & 1u) st |= status_of(d.stream[q]);
  return PgLoc{len * c, len * d.elem, planes_units(len), c, st ? 1u : 0u};
}

// The range's byte ranges, C of them, in plane order.
GH_HD void pg_emit(const PlanesTensor& d, const gh_erange& r, gh_brange* out) {
  uint32_t c = 0;
  for (uint32_t q = 0; q < PLANES_MAX_E; ++q)
    if ((d.mask >> q) & 1u) out[c++] = gh_brange{d.stream[q], r.lo, r.hi};
}

// ---- the range join ---------------------------------------------------------------------
// One element range as the join sees it.  stage / stored / dst: the three buffers' bases.
struct PgView {
  const uint8_t* stage;
  const uint8_t* stored;
  uint8_t* dst;
  uint64_t lo, len, stage_off, dst_off;
  bool vec;
};

// The vector path's test for a whole range: every plane's first byte and the range's first
// destination byte are 16-byte aligned.  (stage, stored and every stored_off are; coded plane
// c starts c * len bytes after the range's staging offset.)
GH_HD bool pg_vec_ok(uint64_t stage_off, uint64_t lo, uint64_t len, uint64_t dst_addr, uint32_t ncoded) {
  return ((stage_off | lo | dst_addr) & 15u) == 0 && (ncoded <= 1 || (len & 15u) == 0);
}

// Elements of the lane that starts at element i0 of the range: 16, fewer at the range's end, 0 past it.
GH_HD uint32_t pg_lane_rem(uint64_t len, uint64_t i0) {
  return i0 >= len ? 0u : len - i0 >= PLANES_GROUP ? PLANES_GROUP : (uint32_t)(len - i0);
}

GH_HD void pg_load16(const uint8_t* p, uint32_t (&o)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 v = *(const uint4*)p;
  o[0] = v.x;
  o[1] = v.y;
  o[2] = v.z;
  o[3] = v.w;
#else
  std::memcpy(o, p, 16);
#endif
}

GH_HD void pg_store16(uint8_t* p, const uint32_t* w) {
#if defined(__HIP_DEVICE_COMPILE__)
  *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
#else
  std::memcpy(p, w, 16);
#endif
}

// Elements [i0, i0 + 16) of the range (i0 a multiple of 16): a whole lane of a range that passes
// pg_vec_ok moves 16 bytes per access; every other lane reads exactly its `rem` bytes of each
// plane and stores exactly rem * E bytes, one by one.
template <uint32_t E>
GH_HD void pg_join_lane(const PgView& v, const PlanesTensor& d, uint64_t i0) {
  const uint32_t rem = pg_lane_rem(v.len, i0);
  if (!rem) return;
  uint32_t w[4 * E], pl[E][4];
  uint8_t* dst = v.dst + v.dst_off + i0 * E;
  const bool whole = v.vec && rem == PLANES_GROUP;
  uint32_t c = 0;
  for (uint32_t q = 0; q < E; ++q) {
    const bool coded = (d.mask >> q) & 1u;
    const uint8_t* src = coded ? v.stage + v.stage_off + c * v.len + i0 : v.stored + d.off[q] + v.lo + i0;
    c += coded;
    if (whole) {
      pg_load16(src, pl[q]);
    } else {
      for (uint32_t k = 0; k < 4; ++k) pl[q][k] = 0;
      for (uint32_t k = 0; k < PLANES_GROUP; ++k)
        if (k < rem) pl[q][k / 4] |= (uint32_t)src[k] << (8 * (k % 4));
    }
  }
  planes_join16<E>(pl, w);
  if (whole) {
    for (uint32_t j = 0; j < E; ++j) pg_store16(dst + 16 * j, w + 4 * j);
  } else {
    const uint32_t nb = rem * E;
    for (uint32_t b = 0; b < 16 * E; ++b)
      if (b < nb) dst[b] = (uint8_t)(w[b / 4] >> (8 * (b % 4)));
  }
}

}  // namespace gh
