// Plane choice (gaphuff.h, "plane choice"): which byte planes of a tensor are worth coding,
// shared by the decide kernel (gh_pmask.hip) and by CPU code (gh_pmask_from_counts in
// gh_core.cpp, tests/sanitize/pmask_fuzz.cpp): one text, compiled for both.
//
// The rule.  fb(t, p) is the size of the compressed.huff image of plane p of tensor t, what
// gh_encode_plan_from_counts(the plane's byte counts, 0).file_bytes gives.  The plane is coded
// iff fb(t, p) < nelem; a tie is stored; a tensor without elements gets mask 0.  A container
// aligns its planes to 8 bytes, and fb < nelem implies round_up8(fb) <= round_up8(nelem): the
// chosen mask gives a container no larger than any other mask's, and never one larger than the
// all-stored container.
//
// Candidate planes are numbered in tensor order, then plane order, over ALL E planes of every
// tensor: q = q0[t] + p, q0[t] the sum of E_j for j < t.
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

constexpr uint32_t PMASK_MAX_PLANES = 1u << 24;  // candidate planes of a list

// ---- the image's size ---------------------------------------------------------------------
// plan_sizes' arithmetic (gh_core.cpp) with no forced version: w payload words, g segments of
// 128 bits with eight 4-bit gaps per word, the v2 (64-bit) header when n, w or g reach 2^31.
GH_HD uint64_t pmask_file_bytes(uint64_t bits, uint32_t nsyms, uint64_t n) {
  const uint64_t w = bits / 32 + (bits % 32 ? 1 : 0), g = bits / 128 + (bits % 128 ? 1 : 0);
  const uint64_t lim = 1ull << 31;
  const bool v2 = n >= lim || w >= lim || g >= lim;
  const uint64_t hdr = (v2 ? 16u : 8u) + 2ull * nsyms + (v2 ? 24u : 12u);
  return hdr + 4 * (g / 8 + (g % 8 ? 1 : 0)) + 4 * w;
}

// ---- the decision -------------------------------------------------------------------------
GH_HD bool pmask_coded(uint64_t file_bytes, uint64_t nelem) { return nelem != 0 && file_bytes < nelem; }
// What the plane occupies under the rule's choice.
GH_HD uint64_t pmask_chosen_bytes(uint64_t file_bytes, uint64_t nelem) {
  return pmask_coded(file_bytes, nelem) ? file_bytes : nelem;
}

// ---- the numbering ------------------------------------------------------------------------
// q0 of the tensor after one of e-byte elements that starts at q0; false past PMASK_MAX_PLANES.
GH_HD bool pmask_next_q0(uint32_t q0, uint32_t e, uint32_t* next) {
  *next = q0 + e;  // (q0 <= 2^24, e <= 8)
  return *next <= PMASK_MAX_PLANES;
}
// The tensor of candidate q: the t with q0[t] <= q < q0[t + 1] (q0[0 .. ntensors] ascending,
// strictly: every tensor has a plane; q < q0[ntensors]).  At most 25 steps.
GH_HD uint32_t pmask_tensor_of(const uint32_t* q0, uint32_t ntensors, uint32_t q) {
  uint32_t a = 0, b = ntensors;  // q0[a] <= q; b == ntensors or q0[b] > q
  while (b - a > 1) {
    const uint32_t mid = a + (b - a) / 2;
    if (q0[mid] <= q) a = mid; else b = mid;
  }
  return a;
}

}  // namespace gh
