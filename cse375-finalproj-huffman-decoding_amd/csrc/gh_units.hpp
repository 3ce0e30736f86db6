// The unit walk of a batch (device), shared by the batched decode (gh_batch.hip) and the
// batched encode (gh_ebatch.hip).  A batch's work units are numbered across its streams;
// unit0[0 .. nstreams] is the prefix of the streams' unit counts.  A wave takes a contiguous
// run of units and keeps a cursor on the stream it is in, reloaded only when the run leaves
// the stream.  What a stream is (its descriptor, its tables) stays with each side.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gh {

// The stream of unit u: the last s with unit0[s] <= u (streams without units share their
// unit0 with their successor and are never found).  Wave-uniform; at most 25 steps.
__device__ __forceinline__ uint32_t unit_stream_of(const uint32_t* unit0, uint32_t nstreams, uint32_t u) {
  uint32_t a = 0, b = nstreams;  // unit0[a] <= u; b == nstreams or unit0[b] > u
  while (b - a > 1) {
    const uint32_t mid = a + (b - a) / 2;
    if (unit0[mid] <= u) a = mid; else b = mid;
  }
  return a;
}

// Where a wave is in the batch.
struct UnitCursor {
  uint32_t s = 0xFFFFFFFFu;  // stream (0xFFFFFFFF: none yet)
  uint32_t first = 0;        // the stream's first unit
  uint32_t end = 0;          // the stream's last unit + 1
  uint32_t blk = 0;          // unit of the stream
};

// Points c at unit u; returns true when the stream changed (the caller then loads what it
// keeps per stream).  The stream fields are wave-uniform.
__device__ __forceinline__ bool unit_enter(const uint32_t* unit0, uint32_t nstreams, uint32_t u, UnitCursor& c) {
  if (c.s != 0xFFFFFFFFu && u < c.end) {
    c.blk = u - c.first;
    return false;
  }
  const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)unit_stream_of(unit0, nstreams, u));
  c.s = s;
  c.first = (uint32_t)__builtin_amdgcn_readfirstlane((int)unit0[s]);
  c.end = (uint32_t)__builtin_amdgcn_readfirstlane((int)unit0[s + 1]);
  c.blk = u - c.first;
  return true;
}

// This wave's run of units: wave w of the grid's nw waves (WAVES per workgroup) takes
// [w nunits / nw, (w + 1) nunits / nw).
template <int WAVES>
__device__ __forceinline__ void unit_run(uint32_t nunits, uint32_t wid, uint32_t& u0, uint32_t& u1) {
  const unsigned long long nw = (unsigned long long)gridDim.x * WAVES, gw = (unsigned long long)blockIdx.x * WAVES + wid;
  u0 = (uint32_t)(gw * nunits / nw);
  u1 = (uint32_t)((gw + 1) * nunits / nw);
}

}  // namespace gh
