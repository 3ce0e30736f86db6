// Device primitives with no decoder types: wave scans, the wave-uniform 64-bit copy and the
// one-workgroup scan.  Needs only the HIP runtime header; included by gh_device.hpp (for
// gh_decode.hip) and by gh_encode.hip directly.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gh {

// Inclusive wave scan on the VALU with DPP: row_shr 1/2/4/8 scans each 16-lane row,
// row_bcast 15/31 carry the row totals forward (no LDS traffic, unlike
// ds_bpermute-based shuffles).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
  return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// Wave-uniform copy of a 64-bit value (lane 0's).  readfirstlane returns int: each half
// is taken as uint32_t before widening (an int low half with bit 31 set would
// sign-extend over the high half).
__device__ __forceinline__ unsigned long long rfl_u64(unsigned long long v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// Exclusive u64 scan of in[0 .. n) by one workgroup of TB threads: stores out[0 .. n) and
// returns the total to every thread.  A slice of ceil(n / TB) values per thread, a wave scan
// of the slice sums, the wave totals in s_w (TB / 64 words of LDS), then a second pass over
// the slice that stores.  Holds one __syncthreads(); ordering the stores before an epilogue
// that reads `out` is the caller's.
template <int TB, class T>
__device__ __forceinline__ unsigned long long block_excl_scan(const T* in, unsigned long long* out, uint32_t n,
                                                              unsigned long long* s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t per = (n + TB - 1) / TB;
  const uint32_t i0 = min((uint32_t)tid * per, n), i1 = min(i0 + per, n);
  unsigned long long s = 0;
  for (uint32_t i = i0; i < i1; ++i) s += in[i];
  unsigned long long incl = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(incl, d, 64);
    if (lane >= d) incl += y;
  }
  if (lane == 63) s_w[wid] = incl;
  __syncthreads();
  unsigned long long base = 0, all = 0;
#pragma unroll
  for (int q = 0; q < TB / 64; ++q) {
    base += q < wid ? s_w[q] : 0ull;
    all += s_w[q];
  }
  unsigned long long run = base + incl - s;
  for (uint32_t i = i0; i < i1; ++i) {
    const unsigned long long t = in[i];
    out[i] = run;
    run += t;
  }
  return all;
}

}  // namespace gh
