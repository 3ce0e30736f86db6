// Per-range arithmetic of the batched gather's plan (gh_batchdec_*), shared by the device
// planner (gh_batch_gather.hip), the host plan (gh_batchdec_plan, gh_core.cpp) and CPU code
// (tests/sanitize/batch_gather_fuzz.cpp): one text, compiled for all three.
//
// A decoded or indexed batch holds a seek index of stride 2^8 for every stream: unit_off[]
// is the exclusive scan of the codewords per 256-segment work unit over the whole batch and
// unit0[0 .. nstreams] the prefix of the streams' unit counts, so stream s's index entries
// are unit_off[unit0[s] + j] - unit_off[unit0[s]].  Instead of subtracting the stream's base
// from every entry, the range is moved by it: [lo + base, hi + base) against the entries
// unit_off + unit0[s], with gh_gather_range.hpp's searches as they are.  The terminal entry
// is the stream's counted total (+ base): at least n_s >= hi for an unflagged stream, which
// is all gr_end_entry needs.
//
// No rank array: a range's pieces are the units [k0, m), one each.  A unit without symbols
// inside a range gives a piece with a == b, for which the gather kernel writes nothing; in
// an unflagged real stream it cannot occur (a non-last unit spans more than 2 047 x 16 bits).
// A piece's `block` is the GLOBAL unit index.
#pragma once
#include <stdint.h>

#include "gaphuff.h"
#include "gh_gather_range.hpp"

namespace gh {

// Locate: validation, first unit (global) and piece count of range r.  *flagged is set when
// the range is valid but names a stream whose status word is non-zero: it keeps its bytes in
// the layout (len) and gets no pieces.  n_of(s) / status_of(s): stream s's output bytes and
// status word, asked only for s < nstreams (the kernels read them from their descriptors).
template <class NOf, class StatusOf>
GH_HD RangeLoc br_locate(const uint32_t* unit0, const uint64_t* unit_off, NOf n_of, StatusOf status_of,
                         uint32_t nstreams, const gh_brange& r, bool* flagged) {
  *flagged = false;
  if (r.stream >= nstreams || r.lo > r.hi || r.hi > n_of((uint32_t)r.stream)) return RangeLoc{0u, GR_BAD_RANGE, 0u};
  const uint32_t s = (uint32_t)r.stream;
  if (status_of(s)) {
    *flagged = true;
    return RangeLoc{0u, 0u, r.hi - r.lo};
  }
  if (r.lo == r.hi) return RangeLoc{0u, 0u, 0u};  // (a non-empty range has n_s > 0: the stream has a unit)
  const uint32_t u0 = unit0[s];
  const uint64_t nblocks = unit0[s + 1] - u0, base = unit_off[u0];
  const uint64_t k0 = gr_first_block(unit_off + u0, nblocks, r.lo + base);
  const uint64_t m = gr_end_entry(unit_off + u0, nblocks, k0, r.hi + base);
  return RangeLoc{u0 + (uint32_t)k0, (uint32_t)(m - k0), r.hi - r.lo};
}

// The j-th piece (j < loc.count) of range r, whose bytes start at dst0 of the output.
GH_HD gh_gather_piece br_piece(const uint32_t* unit0, const uint64_t* unit_off, const gh_brange& r,
                               const RangeLoc& loc, uint64_t j, uint64_t dst0) {
  const uint64_t base = unit_off[unit0[r.stream]];
  return gr_piece(unit_off, loc.k0 + j, r.lo + base, r.hi + base, dst0);
}

}  // namespace gh
