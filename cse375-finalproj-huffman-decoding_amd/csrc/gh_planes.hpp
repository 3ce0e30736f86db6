// Byte planes of typed tensors (gaphuff.h, "byte planes"), shared by the split and join
// kernels (gh_planes_split.hip, gh_planes_join.hip) and by CPU code (gh_planes_layout,
// gh_planes_split_host, gh_planes_join_host in gh_core.cpp, tests/sanitize/planes_fuzz.cpp):
// one text, compiled for both.
//
// An element is E bytes (1, 2, 4, 8); plane p of a tensor is the bytes src[i * E + p].  The
// scalar rule below is the truth.  The vector rule works on a group of 16 elements: 4 E dwords
// on the tensor side, 4 dwords per plane, moved by byte permutes (v_perm_b32 on the device,
// planes_perm's loop on the host, the same selectors).
#pragma once
#include <cstdint>

#ifndef GH_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GH_HD __host__ __device__ inline
#else
#define GH_HD inline
#endif
#endif

namespace gh {

constexpr uint32_t PLANES_MAX_E = 8;
constexpr uint32_t PLANES_UNIT_ELEMS = 1024;  // elements per work unit: 1 KiB per plane, E KiB of the tensor
constexpr uint32_t PLANES_GROUP = 16;         // elements per lane: one 16-byte access per plane
constexpr uint32_t PLANES_MAX_CODED = 1u << 24;
constexpr uint64_t PLANES_MAX_UNITS = 1ull << 31;  // tensor units of a list, exclusive

// ---- layout arithmetic ------------------------------------------------------------------
GH_HD bool planes_elem_ok(uint32_t e) { return e == 1 || e == 2 || e == 4 || e == 8; }
GH_HD bool planes_mask_ok(uint32_t e, uint32_t mask) { return mask < (1u << e); }
// a + b into *r; false when the sum overflows 64 bits
GH_HD bool planes_add(uint64_t a, uint64_t b, uint64_t* r) {
  *r = a + b;
  return *r >= a;
}
// round_up(nelem, 16): the bytes a stored plane owns; false when it overflows
GH_HD bool planes_padded(uint64_t nelem, uint64_t* r) {
  uint64_t t;
  if (!planes_add(nelem, 15, &t)) return false;
  *r = t & ~15ull;
  return true;
}
GH_HD uint64_t planes_units(uint64_t nelem) { return nelem / PLANES_UNIT_ELEMS + (nelem % PLANES_UNIT_ELEMS ? 1 : 0); }

// One tensor as the kernels see it (device memory, 128 bytes).  off[p]: where plane p's bytes
// are, in the arena its kind selects (coded: the batch's arena; stored: the stored arena).
struct PlanesTensor {
  uint8_t* data;              // nelem * elem bytes, any alignment
  unsigned long long nelem;
  unsigned long long off[PLANES_MAX_E];
  uint32_t stream[PLANES_MAX_E];  // a coded plane's stream (the join reads its status word)
  uint32_t elem, mask;
  unsigned long long pad;
};
static_assert(sizeof(PlanesTensor) == 128, "PlanesTensor layout");

// ---- the scalar byte rule ---------------------------------------------------------------
// Byte p of element i of a tensor of e-byte elements.
GH_HD uint64_t planes_src_index(uint64_t i, uint32_t e, uint32_t p) { return i * e + p; }

// ---- the permute selectors ----------------------------------------------------------------
// planes_perm(hi, lo, sel): byte k of the result is byte sel.k of the eight bytes {hi, lo}
// (0..3: lo, 4..7: hi), v_perm_b32's rule for selectors 0..7.
constexpr uint32_t SEL_EVEN = 0x06040200u;   // bytes 0, 2 of lo, then of hi: plane 0 of four 2-byte elements
constexpr uint32_t SEL_ODD = 0x07050301u;    // bytes 1, 3 of lo, then of hi: plane 1
constexpr uint32_t SEL_ZIP_LO = 0x05010400u; // lo.0 hi.0 lo.1 hi.1: interleave the low halves
constexpr uint32_t SEL_ZIP_HI = 0x07030602u; // lo.2 hi.2 lo.3 hi.3: interleave the high halves
constexpr uint32_t SEL_PAIR_LO = 0x05040100u; // lo.0 lo.1 hi.0 hi.1
constexpr uint32_t SEL_PAIR_HI = 0x07060302u; // lo.2 lo.3 hi.2 hi.3

GH_HD uint32_t planes_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t both = ((uint64_t)hi << 32) | lo;
  uint32_t r = 0;
  for (uint32_t k = 0; k < 4; ++k) r |= (uint32_t)((both >> (8u * ((sel >> (8u * k)) & 7u))) & 0xFFu) << (8u * k);
  return r;
#endif
}

// The 4 x 4 byte transpose of four dwords (its own inverse): byte r of o[c] = byte c of a[r].
GH_HD void planes_transpose4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t (&o)[4]) {
  const uint32_t t0 = planes_perm(a1, a0, SEL_ZIP_LO), t1 = planes_perm(a1, a0, SEL_ZIP_HI);
  const uint32_t t2 = planes_perm(a3, a2, SEL_ZIP_LO), t3 = planes_perm(a3, a2, SEL_ZIP_HI);
  o[0] = planes_perm(t2, t0, SEL_PAIR_LO);
  o[1] = planes_perm(t2, t0, SEL_PAIR_HI);
  o[2] = planes_perm(t3, t1, SEL_PAIR_LO);
  o[3] = planes_perm(t3, t1, SEL_PAIR_HI);
}

// A group of 16 elements: w[0 .. 4 E) are the tensor's dwords (little-endian), pl[p][0 .. 4)
// plane p's.
template <uint32_t E>
GH_HD void planes_split16(const uint32_t (&w)[4 * E], uint32_t (&pl)[E][4]) {
  if constexpr (E == 1) {
    for (uint32_t k = 0; k < 4; ++k) pl[0][k] = w[k];
  } else if constexpr (E == 2) {
    for (uint32_t k = 0; k < 4; ++k) {
      pl[0][k] = planes_perm(w[2 * k + 1], w[2 * k], SEL_EVEN);
      pl[E - 1][k] = planes_perm(w[2 * k + 1], w[2 * k], SEL_ODD);
    }
  } else {
    // E = 4: one transpose per four elements; E = 8: one of the elements' low dwords (planes
    // 0..3), one of their high dwords (planes 4..7)
    constexpr uint32_t D = E / 4;  // dwords per element
    for (uint32_t k = 0; k < 4; ++k)
      for (uint32_t h = 0; h < D; ++h) {
        uint32_t o[4];
        const uint32_t b = 4 * D * k + h;
        planes_transpose4(w[b], w[b + D], w[b + 2 * D], w[b + 3 * D], o);
        for (uint32_t c = 0; c < 4; ++c) pl[4 * h + c][k] = o[c];
      }
  }
}

template <uint32_t E>
GH_HD void planes_join16(const uint32_t (&pl)[E][4], uint32_t (&w)[4 * E]) {
  if constexpr (E == 1) {
    for (uint32_t k = 0; k < 4; ++k) w[k] = pl[0][k];
  } else if constexpr (E == 2) {
    for (uint32_t k = 0; k < 4; ++k) {
      w[2 * k] = planes_perm(pl[E - 1][k], pl[0][k], SEL_ZIP_LO);
      w[2 * k + 1] = planes_perm(pl[E - 1][k], pl[0][k], SEL_ZIP_HI);
    }
  } else {
    constexpr uint32_t D = E / 4;
    for (uint32_t k = 0; k < 4; ++k)
      for (uint32_t h = 0; h < D; ++h) {
        uint32_t o[4];
        planes_transpose4(pl[4 * h][k], pl[4 * h + 1][k], pl[4 * h + 2][k], pl[4 * h + 3][k], o);
        const uint32_t b = 4 * D * k + h;
        for (uint32_t c = 0; c < 4; ++c) w[b + c * D] = o[c];
      }
  }
}

}  // namespace gh
