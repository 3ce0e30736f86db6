// GPU encoder of the compressed.huff format: the reference's
// encoder.cu pipeline (histogram :118-140, cuencoder :142-355, cu_get_gaparray
// :358-379) re-designed for gfx950.  Byte-identical to the host encoder
// (gh_core.cpp gh_encode_write), which restates the reference's packing: codewords
// MSB-first inside u32 words; for every codeword crossing a 128-bit boundary, the
// nibble (end bit mod 16) at the index of the segment it starts in, 8 nibbles per
// u32, LSB-first.
//
// Kernels (input resident in HBM, 8 KiB chunks of 512 threads x 16 bytes; 4 KiB of 256
// until round 6: the write kernel's per-chunk work (two barriers, the last word's
// completion, edge gap words) is then spread over twice the bytes, cfg4 1.05 -> 0.93 ms):
//   gh_enc_hist_kernel   byte histogram; LDS counters replicated 32x (lane & 31), so
//                        one instruction's lanes collide at most 2-way even on the
//                        skewed r=0.9 data; 256 u64 atomics per workgroup.
//   (host)               package-merge + canonical codes (gh::plan_from_counts).
//   gh_enc_bits_kernel   code bits per chunk (u32).
//   gh_enc_scan_kernel   exclusive scan of the chunk bits in blocks of 8192 chunks,
//   gh_enc_blkscan_kernel  then of the block totals (u64).
//   gh_enc_write_kernel  one chunk per workgroup: block scan of the lanes' bits,
//                        codewords OR-ed
//                        into a zeroed LDS image of the chunk's words (positions in
//                        32 bits relative to the chunk's gap-word-aligned base),
//                        then written with coalesced stores.  No payload atomics: a
//                        chunk owns the words whose first bit it holds, and its last
//                        lane encodes the next chunk's first symbols (< 32 bits) to
//                        complete its last word.  Gap nibbles likewise in LDS; the two
//                        edge gap words of a chunk (shared with its neighbours) are
//                        atomicOr-ed into the zeroed gap array, the rest stored.
//   gh_enc_index_kernel  (gh_ectx_index, after an encode) the seek index from the chunk
//                        offsets: see the kernel.
//   gh_enc_merge_kernel  (gh_ectx_merge_device) ORs an encode's words and gap words into
//                        the stream's device-resident arrays: see enc_merge_span.
// Batched encode (gh_ebatch_*): many inputs with their own codes, wave-sized units; its
// kernels are in gh_ebatch.hip, its host side at the end of this file.
// Byte planes (gh_planes_load, gh_planes_load_device): a batched encode whose streams are the
// coded byte planes of typed tensors; the split kernel is in gh_planes_split.hip.
// Plane choice (gh_pmask_device): which planes to code, from the tensors' own bytes; its
// kernels are in gh_pmask.hip.
// Sliced encode (gh_ectx_encode_slice): the same kernels on an input that is one slice of
// a longer stream; the block scan starts at the slice's first stream bit and the write
// kernel's SLICE variant indexes its outputs from the slice's origin; the index kernel's
// SLICE variant (gh_ectx_index_slice) emits the entries the slice owns.
// Traffic: N (histogram, plan step) + 2N + C + gaps (encode) bytes.  A single pass
// with a decoupled look-back (one 4 KiB chunk per workgroup) measured 2.85 ms on
// cfg4, slower than these three kernels: its workgroups waited on their nearest
// predecessors' aggregates.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "gaphuff.h"
#include "gh_hip.hpp"
#include "gh_internal.hpp"
#include "gh_planes.hpp"
#include "gh_pm_flat.hpp"
#include "gh_pmask.hpp"
#include "gh_units.hpp"
#include "gh_wave.hpp"

namespace gh {

#ifndef GH_ENC_TB
#define GH_ENC_TB 512
#endif
constexpr int ETB = GH_ENC_TB;           // threads per workgroup
constexpr int EBPT = 16;                 // input bytes per thread
constexpr int ECHUNK = ETB * EBPT;       // input bytes per chunk
constexpr int EREP = 32;                 // histogram replicas
// LDS image of a chunk from its gap-word-aligned base: up to 1023 bits before it,
// 16 bits per byte, the last word's completion (< 32 + 16 bits).  These are the bounds;
// the write kernel's image is sized at launch for the code's longest codeword (dynamic
// LDS: 9-bit codes, cfg4, take 4.7 KB per 4 KiB instead of 8.3)
constexpr int EWORDS = (1024 + ECHUNK * GH_MAX_CODE_LEN + 64) / 32 + 2;
constexpr int EGAPW = (1024 + ECHUNK * GH_MAX_CODE_LEN) / 1024 + 2;

__device__ __forceinline__ uint32_t enc_byte(const uint4& v, int k) {
  const uint32_t w = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
  return (w >> (8 * (k & 3))) & 0xFFu;
}

// 16 input bytes of thread t of chunk c (bytes past n read as "absent": 0x100).
__device__ __forceinline__ void enc_load(const uint8_t* in, uint64_t n, uint64_t base, uint32_t (&b)[EBPT]) {
  if (base + EBPT <= n) {
    const uint4 v = *(const uint4*)(in + base);
#pragma unroll
    for (int k = 0; k < EBPT; ++k) b[k] = enc_byte(v, k);
  } else {
#pragma unroll
    for (int k = 0; k < EBPT; ++k) b[k] = base + k < n ? (uint32_t)in[base + k] : 0x100u;
  }
}

__global__ __launch_bounds__(ETB) void gh_enc_hist_kernel(const uint8_t* in, uint64_t n,
                                                          unsigned long long* count) {
  __shared__ uint32_t h[256 * EREP];
  const int tid = threadIdx.x;
  for (int i = tid; i < 256 * EREP; i += ETB) h[i] = 0;
  __syncthreads();
  const uint32_t rep = (uint32_t)tid & (EREP - 1);
  const uint64_t nchunks = (n + ECHUNK - 1) / ECHUNK;
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    uint32_t b[EBPT];
    enc_load(in, n, c * ECHUNK + (uint64_t)tid * EBPT, b);
#pragma unroll
    for (int k = 0; k < EBPT; ++k)
      if (b[k] < 256u) atomicAdd(&h[b[k] * EREP + rep], 1u);
  }
  __syncthreads();
  for (int v = tid; v < 256; v += ETB) {
    unsigned long long s = 0;
#pragma unroll
    for (int r = 0; r < EREP; ++r) s += h[v * EREP + ((r + v) & (EREP - 1))];
    if (s) atomicAdd(&count[v], s);
  }
}

// Workgroup exclusive scan of one u32 per thread; returns the exclusive prefix and
// sets total.  s_red: NWAVE u32 of LDS.
__device__ __forceinline__ uint32_t enc_block_scan(uint32_t x, uint32_t* s_red, uint32_t& total) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  uint32_t incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(incl, d, 64);
    if (lane >= d) incl += y;
  }
  if (lane == 63) s_red[wid] = incl;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int q = 0; q < ETB / 64; ++q) {
    const uint32_t v = s_red[q];
    before += q < wid ? v : 0u;
    total += v;
  }
  return before + incl - x;
}

// Persistent: workgroup b takes chunk groups (b + EBQ*k*G + j*G, j < EBQ); the next
// group's bytes (EBQ 16-byte loads per thread: the bytes in flight per CU set this
// kernel's bandwidth) are loaded before the current group's reduction.  Loads are
// unconditional (chunk index clamped, input padded past n), bytes past n masked by index.
#ifndef GH_ENC_NT
#define GH_ENC_NT 3  // (round 4: 3) write kernel, bits: 1 input loads nontemporal, 2 payload word stores nontemporal; 4 bits-kernel loads nontemporal
#endif
#ifndef GH_ENC_OOB
#define GH_ENC_OOB 1  // write kernel: padding stores out of a buffer resource's range (dropped) instead of to a junk dword
#endif
#ifndef GH_ENC_UOR
#define GH_ENC_UOR 1  // write kernel: a quad's first two (1: three) image words ORed unconditionally
#endif
#ifndef GH_ENC_LSUM
#define GH_ENC_LSUM 1  // write kernel: lengths summed from the entries' low halves (no per-entry mask)
#endif
#ifndef GH_ENC_BQ
#define GH_ENC_BQ 2  // chunks in flight per thread (4 measured slower: 246 vs 229 us on cfg4)
#endif
#ifndef GH_ENC_BREP
#define GH_ENC_BREP 32  // code-length table copies in LDS (lane l reads copy l mod BREP: no bank conflicts at 32)
#endif
constexpr int EBQ = GH_ENC_BQ;
constexpr int EBREP = GH_ENC_BREP;
__global__ __launch_bounds__(ETB) void gh_enc_bits_kernel(const uint8_t* in, uint64_t n, uint32_t nchunks,
                                                          const uint32_t* lut, uint32_t* chunk_bits) {
  __shared__ uint32_t s_lenr[256 * EBREP];
  __shared__ uint32_t s_red[2][EBQ][ETB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int i = tid; i < 256 * EBREP; i += ETB) s_lenr[i] = lut[i / EBREP] & 0xFFu;
  const uint32_t* s_len = s_lenr + (lane & (EBREP - 1));  // entry b of this lane's copy: s_len[b * EBREP]
  const uint32_t G = gridDim.x;
  auto ld = [&](uint32_t cc) {
    const uint8_t* src = in + (uint64_t)min(cc, nchunks - 1) * ECHUNK + (uint64_t)tid * EBPT;
    if (GH_ENC_NT & 4) {
      typedef unsigned int v4u __attribute__((ext_vector_type(4)));
      const v4u t = __builtin_nontemporal_load((const v4u*)src);
      return make_uint4(t.x, t.y, t.z, t.w);
    }
    return *(const uint4*)src;
  };
  auto chunk_bits_of = [&](const uint4& v, uint32_t cc) {
    const uint64_t ib = (uint64_t)cc * ECHUNK + (uint64_t)tid * EBPT;
    uint32_t bits = 0;
    if (ib + EBPT <= n) {
#pragma unroll
      for (int k = 0; k < EBPT; ++k) bits += s_len[enc_byte(v, k) * EBREP];
    } else {
      const uint32_t rem = ib < n ? (uint32_t)(n - ib) : 0u;
#pragma unroll
      for (int k = 0; k < EBPT; ++k) bits += (uint32_t)k < rem ? s_len[enc_byte(v, k) * EBREP] : 0u;
    }
    return bits;
  };
  uint32_t c = blockIdx.x;
  uint4 v[EBQ];
#pragma unroll
  for (int j = 0; j < EBQ; ++j) v[j] = ld(c + (uint32_t)j * G);
  __syncthreads();
  for (uint32_t it = 0; c < nchunks; c += EBQ * G, ++it) {
    uint32_t b[EBQ];
#pragma unroll
    for (int j = 0; j < EBQ; ++j) b[j] = chunk_bits_of(v[j], c + (uint32_t)j * G);
#pragma unroll
    for (int j = 0; j < EBQ; ++j) v[j] = ld(c + (uint32_t)(EBQ + j) * G);
#pragma unroll
    for (int j = 0; j < EBQ; ++j) {
      const uint32_t sc = wave_incl_scan(b[j]);  // lane 63: the wave total
      if (lane == 63) s_red[it & 1][j][wid] = sc;
    }
    __syncthreads();  // (double-buffered partial sums: one barrier per group)
    if (tid < EBQ) {
      uint32_t t = 0;
#pragma unroll
      for (int q = 0; q < ETB / 64; ++q) t += s_red[it & 1][tid][q];
      const uint32_t cc = c + (uint32_t)tid * G;
      if (cc < nchunks) chunk_bits[cc] = t;
    }
  }
}

// Chunk offsets in two levels.  gh_enc_scan_kernel: workgroup k scans chunks
// [8192k, 8192k + 8192) (8 consecutive per thread): local exclusive offsets and the
// block total.  gh_enc_blkscan_kernel (one workgroup): exclusive scan of the block
// totals.  The write kernel adds the two.
constexpr int SCAN_TB = 1024, SCAN_PT = 8, SCAN_BLK = SCAN_TB * SCAN_PT;
static_assert((unsigned long long)SCAN_BLK * ECHUNK * 16 < (1ull << 32), "scan block bits fit u32");
__global__ __launch_bounds__(SCAN_TB) void gh_enc_scan_kernel(const uint32_t* chunk_bits, uint32_t nchunks,
                                                              uint32_t* chunk_loc, unsigned long long* blk_tot) {
  __shared__ uint32_t s_w[SCAN_TB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t i0 = blockIdx.x * (uint32_t)SCAN_BLK + (uint32_t)tid * SCAN_PT;
  uint32_t v[SCAN_PT], t = 0;
#pragma unroll
  for (int k = 0; k < SCAN_PT; ++k) v[k] = i0 + k < nchunks ? chunk_bits[i0 + k] : 0u;
#pragma unroll
  for (int k = 0; k < SCAN_PT; ++k) {
    const uint32_t x = v[k];
    v[k] = t;  // exclusive within the thread
    t += x;
  }
  uint32_t incl = t;  // a block holds < 2^32 bits (8192 chunks x 16 x ECHUNK, ECHUNK <= 16 KiB)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(incl, d, 64);
    if (lane >= d) incl += y;
  }
  if (lane == 63) s_w[wid] = incl;
  __syncthreads();
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < SCAN_TB / 64; ++q) {
    const uint32_t x = s_w[q];
    before += q < wid ? x : 0u;
    tot += x;
  }
  const uint32_t b0 = before + incl - t;
#pragma unroll
  for (int k = 0; k < SCAN_PT; ++k)
    if (i0 + k < nchunks) chunk_loc[i0 + k] = b0 + v[k];
  if (tid == 0) blk_tot[blockIdx.x] = tot;
}
// carry0: the stream bit the input starts at (a slice's base_bit; 0 for a whole stream), so
// every chunk offset is a stream bit position.
__global__ __launch_bounds__(SCAN_TB) void gh_enc_blkscan_kernel(unsigned long long* blk, uint32_t nblk,
                                                                 unsigned long long carry0) {
  __shared__ unsigned long long s[SCAN_TB];
  const int tid = threadIdx.x;
  unsigned long long carry = carry0;
  for (uint32_t base = 0; base < nblk; base += SCAN_TB) {
    const uint32_t i = base + (uint32_t)tid;
    const unsigned long long x = i < nblk ? blk[i] : 0ull;
    s[tid] = x;
    __syncthreads();
    for (int d = 1; d < SCAN_TB; d <<= 1) {
      const unsigned long long y = tid >= d ? s[tid - d] : 0ull;
      __syncthreads();
      s[tid] += y;
      __syncthreads();
    }
    if (i < nblk) blk[i] = carry + s[tid] - x;
    carry += s[SCAN_TB - 1];
    __syncthreads();
  }
}

struct EncParams {
  const uint8_t* in;
  const uint32_t* lut;                 // 256 x {code << 8 | len}
  const uint32_t* chunk_loc;           // bit offset of each chunk within its scan block
  const unsigned long long* blk_off;   // bit offset of each scan block
  uint32_t* words;                     // W payload words
  uint32_t* gaps;                      // GW gap words, zeroed
  uint32_t* junk;                      // one dword per thread of the grid (padding stores)
  uint64_t n;
  uint32_t nchunks;
  uint32_t ewords, egapw;  // LDS image words (payload, gaps): (1024 + ECHUNK x maxlen + 64) / 32 + 2, (1024 + ECHUNK x maxlen) / 1024 + 2
  unsigned long long org;  // slice variant: the stream bit of words[0] and gaps[0], base_bit & ~1023
};

// Write-kernel LUT replicas (lane l reads copy l mod ELREP): 16 copies collide at most
// 2-way and leave room for 6 waves per SIMD; the long-code shapes (NSW >= 6: cfg4's
// r = 0.1 codes, ~8 bits per byte) take 32 (conflict-free, 3 workgroups per CU by LDS):
// cfg4 1.055 vs 1.096 ms, while cfg3 / cfg2 lose 6-11 % at 32 (round 4, gpurun_out/r04x).
#ifndef GH_ENC_LREP_LONG
#define GH_ENC_LREP_LONG 32
#endif
template <int NSW>
constexpr int enc_lrep() { return NSW * ETB * 4096 / ECHUNK >= 5 * 256 ? GH_ENC_LREP_LONG : 16; }  // (>= 0.3 words per input byte)
#ifndef GH_ENC_WPE
#define GH_ENC_WPE 4  // the write kernel's occupancy hint, waves per SIMD (6 and 8 spill)
#endif
// the write kernel's occupancy hint (its VGPR budget: 512 / waves per SIMD)
template <int NSW>
constexpr int enc_wpe() { return GH_ENC_WPE; }

// A thread's 16 codewords, combined in registers: LUT entries hold the code
// left-aligned, e = code << (32 - len) | len (len <= 16 sits in the low 5 bits, below
// the code), so a pair is one shift and one AND-OR (v_lshrrev reads only the low 5
// bits of the entry it shifts by), and two pairs make a left-aligned 64-bit quad.
// Each quad is ORed into the LDS image as up to three words.
__device__ __forceinline__ uint32_t enc_pair(uint32_t a, uint32_t c, uint32_t& len) {
  len = GH_ENC_LSUM ? (a + c) & 0xFFFFu : (a & 31u) + (c & 31u);
  return (a & 0xFFFF0000u) | ((c & 0xFFFF0000u) >> (a & 31u));
}

// Persistent: workgroup b encodes chunks b, b + G, ...  The next chunk's bytes and
// offset (and the 32 bytes after it, for its last word) are loaded while the current
// chunk is encoded; the LDS image is re-zeroed as it is written out.  NSW: payload
// store instructions per thread per chunk, a fixed count (padding stores go to the
// thread's junk dword; words past NSW * ETB loop), plus one gap-word store: loads and
// stores share one in-order counter (vmcnt), and with a fixed count of stores younger
// than the prefetch the next chunk waits for its loads with vmcnt(N) instead of also
// waiting for this chunk's stores.
// SLICE: the input is a slice of a longer stream (gaphuff.h, "sliced encode").  The block
// scan starts at the slice's base_bit, so o0, B, qs, the boundaries and the gap nibbles
// are the stream's own; what differs is the origin of the outputs (p.org, the gap word
// holding base_bit: B never lies before it) and the slice's first word: chunk 0 also
// owns the word holding base_bit, whose leading bits (the previous slice's) stay zero in
// the image.  The last word needs nothing: the completion lanes are masked by p.n.
template <int NSW, bool SLICE>
__global__ __launch_bounds__(ETB) __attribute__((amdgpu_waves_per_eu(enc_wpe<NSW>()))) void gh_enc_write_kernel(
    const EncParams p) {
  constexpr int ELREP = enc_lrep<NSW>();
  __shared__ uint32_t s_lutr[257 * ELREP];  // left-aligned entries, replicated
  __shared__ uint32_t s_red[2][ETB / 64];
  extern __shared__ uint32_t s_dyn[];  // the image (p.ewords) and its gap words (p.egapw), sized for the code's longest codeword
  uint32_t* const s_w = s_dyn;
  uint32_t* const s_g = s_dyn + p.ewords;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  uint32_t c = blockIdx.x;
  const uint32_t G = gridDim.x;
  // chunk c's inputs: its 16 bytes per lane, its offset, and (last lane) the next 32 bytes
  uint4 v = make_uint4(0, 0, 0, 0);
  uint32_t xbyte = 0;
  unsigned long long offb = 0;  // chunk offset = block part + local part, added at use
  uint32_t offl = 0;            // (an add here would wait for the loads at once)
  // every load unconditional and in bounds (the input buffer is padded by ECHUNK + 64
  // bytes past n; bytes past n are masked by index), so no branch holds a load
  auto fetch = [&](uint32_t cc) {
    const uint64_t ib = (uint64_t)cc * ECHUNK + (uint64_t)tid * EBPT;
    if (GH_ENC_NT & 1) {
      typedef unsigned int v4u __attribute__((ext_vector_type(4)));
      const v4u t = __builtin_nontemporal_load((const v4u*)(p.in + ib));
      v = make_uint4(t.x, t.y, t.z, t.w);
    } else {
      v = *(const uint4*)(p.in + ib);
    }
    offb = p.blk_off[cc / SCAN_BLK];
    offl = p.chunk_loc[cc];
    xbyte = p.in[(uint64_t)(cc + 1) * ECHUNK + (uint64_t)(lane & 31)];  // the next chunk's byte lane & 31
  };
  if (c < p.nchunks) fetch(c);
  for (int i = tid; i < 257 * ELREP; i += ETB) {
    const uint32_t v = i / ELREP < 256 ? p.lut[i / ELREP] : 0u;
    const uint32_t l = v & 0xFFu;
    s_lutr[i] = l ? ((v >> 8) << (32u - l)) | l : 0u;
  }
  for (uint32_t i = tid; i < p.ewords + p.egapw; i += ETB) s_dyn[i] = 0;
  __syncthreads();
  for (uint32_t it = 0; c < p.nchunks; c += G, ++it) {
    // this chunk's bytes (absent past n: 0x100, length 0)
    const uint64_t ib = (uint64_t)c * ECHUNK + (uint64_t)tid * EBPT;
    uint32_t b[EBPT];
    if (ib + EBPT <= p.n) {  // (divergent only in the last chunk)
#pragma unroll
      for (int k = 0; k < EBPT; ++k) b[k] = enc_byte(v, k);
    } else {
      const uint32_t rem = ib < p.n ? (uint32_t)(p.n - ib) : 0u;
#pragma unroll
      for (int k = 0; k < EBPT; ++k) b[k] = (uint32_t)k < rem ? enc_byte(v, k) : 0x100u;
    }
    const uint32_t nx = xbyte;  // this iteration's copy (fetch() overwrites xbyte)
    const uint64_t xb = (uint64_t)(c + 1) * ECHUNK;
    const unsigned long long o0 = offb + offl;
    if (c + G < p.nchunks) fetch(c + G);  // prefetch
    uint32_t e[EBPT], bits = 0;
#pragma unroll
    for (int k = 0; k < EBPT; ++k) e[k] = s_lutr[b[k] * ELREP + (tid & (ELREP - 1))];
    if (GH_ENC_LSUM) {  // the entries' low 16 bits hold only their lengths: one sum, one mask
#pragma unroll
      for (int k = 0; k < EBPT; ++k) bits += e[k];
      bits &= 0xFFFFu;
    } else {
#pragma unroll
      for (int k = 0; k < EBPT; ++k) bits += e[k] & 31u;
    }
    // block scan (double-buffered wave sums: the barrier also orders the previous
    // iteration's write-out and re-zeroing before this iteration's OR-s)
    const uint32_t incl = wave_incl_scan(bits);
    if (lane == 63) s_red[it & 1][wid] = incl;
    __syncthreads();
    uint32_t before = 0, cbits = 0;
#pragma unroll
    for (int qq = 0; qq < ETB / 64; ++qq) {
      const uint32_t x = s_red[it & 1][qq];
      before += qq < wid ? x : 0u;
      cbits += x;
    }
    const uint32_t excl = before + incl - bits;
    // positions relative to B = the chunk's offset rounded down to a gap word (1024
    // bits): 128-bit boundaries, payload words and gap words keep their alignment
    const unsigned long long B = o0 & ~1023ull;
    const uint32_t qs = (uint32_t)(o0 - B);  // chunk start
    const uint32_t qend = qs + cbits;        // chunk end (the next chunk's first bit)
    const uint32_t q0 = qs + excl;           // this thread's first bit
    // pairs and quads (left-aligned), the quads ORed into the image
    uint32_t pl[EBPT / 2], pv[EBPT / 2];
#pragma unroll
    for (int j = 0; j < EBPT / 2; ++j) pv[j] = enc_pair(e[2 * j], e[2 * j + 1], pl[j]);
    uint32_t qa = q0, qe[EBPT / 4];
#pragma unroll
    for (int i = 0; i < EBPT / 4; ++i) {
      const uint32_t l0 = pl[2 * i], m = l0 + pl[2 * i + 1];
      const unsigned long long Q = ((unsigned long long)pv[2 * i] << 32) |
                                   ((unsigned long long)pv[2 * i + 1] << (32u - l0));
      const uint32_t hi = (uint32_t)(Q >> 32), lo = (uint32_t)Q, sft = qa & 31u;
      uint32_t* wp = &s_w[qa >> 5];
      if (GH_ENC_UOR) {  // ORing zero bits is harmless: no compares, no exec-mask changes
        atomicOr(wp, hi >> sft);
        atomicOr(wp + 1, __builtin_amdgcn_alignbit(hi, lo, sft));
        if (GH_ENC_UOR == 1 || sft + m > 64u) atomicOr(wp + 2, __builtin_amdgcn_alignbit(lo, 0u, sft));
      } else {
        if (m) atomicOr(wp, hi >> sft);
        if (sft + m > 32u) atomicOr(wp + 1, __builtin_amdgcn_alignbit(hi, lo, sft));
        if (sft + m > 64u) atomicOr(wp + 2, __builtin_amdgcn_alignbit(lo, 0u, sft));
      }
      qa += m;
      qe[i] = qa;
    }
    // gap nibbles: for each 128-bit boundary strictly inside [q0, qa), the codeword
    // holding bits bd-1 and bd (quad, then pair, then codeword by compare-selects)
    for (uint32_t bd = ((q0 >> 7) + 1u) << 7; bd < qa; bd += 128u) {
      const bool i0 = bd >= qe[0], i1 = bd >= qe[1], i2 = bd >= qe[2];
      const uint32_t qs4 = i2 ? qe[2] : i1 ? qe[1] : i0 ? qe[0] : q0;
      const uint32_t la = i2 ? pl[6] : i1 ? pl[4] : i0 ? pl[2] : pl[0];
      const uint32_t lb = i2 ? pl[7] : i1 ? pl[5] : i0 ? pl[3] : pl[1];
      const uint32_t ea = i2 ? e[12] : i1 ? e[8] : i0 ? e[4] : e[0];
      const uint32_t eb = i2 ? e[14] : i1 ? e[10] : i0 ? e[6] : e[2];
      const bool second = bd >= qs4 + la;  // in the quad's second pair
      const uint32_t ps = second ? qs4 + la : qs4;
      const uint32_t lp = second ? lb : la;
      const uint32_t l1 = (second ? eb : ea) & 31u;  // the pair's first codeword
      const bool c2 = bd >= ps + l1;
      const uint32_t cs = c2 ? ps + l1 : ps;        // codeword start
      const uint32_t ce = c2 ? ps + lp : ps + l1;   // codeword end
      const uint32_t gv = ce & 15u;
      if (cs < bd && gv && cs < qend) atomicOr(&s_g[cs >> 10], gv << (4 * ((cs >> 7) & 7u)));
    }
    if (wid == ETB / 64 - 1) {
      // complete the chunk's last word (bits [qend, wend)) with the next chunk's first
      // codewords, one per lane (lanes 0..31: bytes 0..31, codes >= 1 bit); their gap
      // nibbles belong to the next chunk
      const uint32_t wend = (qend + 31u) & ~31u;
      const uint32_t ex = (lane < 32 && xb + (uint32_t)lane < p.n) ? s_lutr[nx * ELREP + (tid & (ELREP - 1))] : 0u;
      const uint32_t lx = ex & 31u;
      const uint32_t st = qend + wave_incl_scan(lx) - lx;  // this codeword's first bit
      if (lx && st < wend) {
        const uint32_t cw = ex & 0xFFFF0000u, sh = st & 31u;  // left-aligned code
        atomicOr(&s_w[st >> 5], cw >> sh);
        if (sh + lx > 32u) atomicOr(&s_w[(st >> 5) + 1], cw << (32u - sh));
      }
    }
    __syncthreads();
    // payload words whose first bit lies in [o0, o0 + cbits): local [w0, w1); the
    // image is zeroed as it is read (up to the completion word)
    const uint32_t w0 = (SLICE && c == 0) ? qs >> 5 : (qs + 31u) >> 5, w1 = (qend + 31u) >> 5;
    const unsigned long long org = SLICE ? p.org : 0ull;  // (B >= org: both multiples of 1024)
    uint32_t* wout = p.words + ((B - org) >> 5);
    uint32_t* junk = p.junk + (size_t)blockIdx.x * ETB + tid;
    // (GH_ENC_OOB) buffer stores from the chunk's base (B is workgroup-uniform), the
    // padding ones out of range: dropped, no memory traffic
    const unsigned long long Bu = rfl_u64(B);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(p.words + ((Bu - org) >> 5), 0, 0x7FFFFFF0, 0x00020000);
#pragma unroll
    for (int j = 0; j < NSW; ++j) {
      const uint32_t i = (uint32_t)tid + (uint32_t)(ETB * j);
      const uint32_t x = s_w[i < p.ewords ? i : 0u];
      if (i <= w1) s_w[i] = 0;
      if (GH_ENC_OOB) {
        const int off = (i >= w0 && i < w1) ? (int)(4u * i) : 0x7FFFFFF0;
        __builtin_amdgcn_raw_buffer_store_b32(x, rw, off, 0, (GH_ENC_NT & 2) ? 2 : 0);
      } else {
        uint32_t* d = (i >= w0 && i < w1) ? wout + i : junk;
        if (GH_ENC_NT & 2) __builtin_nontemporal_store(x, d);
        else *d = x;
      }
    }
    for (uint32_t i = tid + ETB * NSW; i <= w1; i += ETB) {
      const uint32_t x = s_w[i];
      s_w[i] = 0;
      if (i >= w0 && i < w1) wout[i] = x;
    }
    // gap words of this chunk's segments: local [0, g1]; the first and the last may
    // hold nibbles of the neighbouring chunks
    const uint32_t g1 = cbits ? (qend - 1u) >> 10 : 0u;
    uint32_t* gout = p.gaps + ((B - org) >> 10);
    static_assert(EGAPW <= ETB, "one gap word per thread");
    {
      const uint32_t i = (uint32_t)tid;
      const uint32_t x = s_g[i < p.egapw ? i : 0u];
      if (i <= g1) s_g[i] = 0;
      const bool in = cbits && i <= g1, edge = i == 0 || i == g1;
      if (GH_ENC_OOB) {  // interior: a plain store (always issued)
        const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(p.gaps + ((Bu - org) >> 10), 0, 0x7FFFFFF0, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(x, rg, (in && !edge) ? (int)(4u * i) : 0x7FFFFFF0, 0, 0);
      } else {
        *((in && !edge) ? gout + i : junk) = x;
      }
      if (in && edge && x) atomicOr(&gout[i], x);
    }
  }
}

// Seek index of the encoded stream (gaphuff.h, "random access"), from what the encode left
// on the device: offsets[k] = the number of codewords that start before payload bit
// B = S * k, S = 128 << log2_stride.  Chunk-centric, the write kernel's chunk geometry:
// workgroup b takes chunks b, b + G, ...; chunk c covers bits [o0, o0 + chunk_bits[c]) and
// owns the boundaries inside them.  A chunk that owns none is left before any input byte
// is loaded (workgroup-uniform: at large strides almost every chunk).  Otherwise the
// lanes' bits are block-scanned as in the write kernel, and the thread whose bits
// [q0, q1) hold B counts its own symbols that start before B and stores the entry.  A
// thread covers at most 256 bits and S >= 32768, so it owns at most one boundary; the
// threads' ranges partition the stream's bits and every boundary lies below their total
// (k * stride < G), so each entry has exactly one writer: no atomics, no zero-fill.
// SLICE (gh_ectx_index_slice, after a slice encode): the block scan started at the slice's
// base_bit, so every o0 is a stream bit position and the early-out, q0 / q1, k and B are
// the stream's own already.  What differs is the store: entry k goes to offsets[k - k0],
// its value is sym_base + ib + cnt (the stream offset of the slice's first byte added, in
// 64 bits), and the bound is the slice's k0 + nk (p.nblocks holds it).  The one-writer
// argument carries over by the ownership rule (gaphuff.h, "the index of a sliced stream"):
// the threads' ranges partition the slice's bits [base_bit, base_bit + bits), the slice
// owns exactly the boundaries inside them, k0 <= k < k0 + nk, so each of the nk entries
// has exactly one writer and none is left unwritten: d_index holds 8 * nk bytes, never
// zeroed.  SLICE = false keeps the parameter block and the code it had before the
// template (the slice's two fields live in a derived block).
struct EncIndexParams {
  const uint8_t* in;
  const uint32_t* lut;                 // 256 x {code << 8 | len}
  const uint32_t* chunk_bits;          // code bits of each chunk
  const uint32_t* chunk_loc;           // bit offset of each chunk within its scan block
  const unsigned long long* blk_off;   // bit offset of each scan block
  unsigned long long* offsets;         // nblocks entries
  uint64_t n, nblocks;
  uint32_t nchunks, log2_bits;         // S = 1 << log2_bits
};
struct EncIndexSliceParams : EncIndexParams {  // nblocks: the slice's k0 + nk
  unsigned long long k0, sym_base;
};

template <bool SLICE>
__global__ __launch_bounds__(ETB) void gh_enc_index_kernel(
    const std::conditional_t<SLICE, EncIndexSliceParams, EncIndexParams> p) {
  __shared__ uint32_t s_lenr[256 * EBREP];
  __shared__ uint32_t s_red[2][ETB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int i = tid; i < 256 * EBREP; i += ETB) s_lenr[i] = p.lut[i / EBREP] & 0xFFu;
  const uint32_t* s_len = s_lenr + (lane & (EBREP - 1));  // entry b of this lane's copy: s_len[b * EBREP]
  __syncthreads();
  const uint32_t sh = p.log2_bits;
  const unsigned long long smask = (1ull << sh) - 1ull;
  uint32_t it = 0;  // chunks scanned so far (the wave sums are double-buffered)
  for (uint32_t c = blockIdx.x; c < p.nchunks; c += gridDim.x) {
    const unsigned long long o0 = p.blk_off[c / SCAN_BLK] + p.chunk_loc[c];
    const unsigned long long end = o0 + p.chunk_bits[c];
    if ((((o0 + smask) >> sh) << sh) >= end) continue;  // no boundary in [o0, end)
    const uint64_t ib = (uint64_t)c * ECHUNK + (uint64_t)tid * EBPT;
    // (in bounds: the input buffer is padded past n; bytes past n are masked by index)
    const uint4 v = *(const uint4*)(p.in + ib);
    uint32_t l[EBPT], bits = 0;
    if (ib + EBPT <= p.n) {  // (divergent only in the last chunk)
#pragma unroll
      for (int k = 0; k < EBPT; ++k) l[k] = s_len[enc_byte(v, k) * EBREP];
    } else {
      const uint32_t rem = ib < p.n ? (uint32_t)(p.n - ib) : 0u;
#pragma unroll
      for (int k = 0; k < EBPT; ++k) l[k] = (uint32_t)k < rem ? s_len[enc_byte(v, k) * EBREP] : 0u;
    }
#pragma unroll
    for (int k = 0; k < EBPT; ++k) bits += l[k];
    const uint32_t incl = wave_incl_scan(bits);
    if (lane == 63) s_red[it & 1][wid] = incl;
    __syncthreads();  // (one barrier per scanned chunk: the other buffer is the previous chunk's)
    uint32_t before = 0;
#pragma unroll
    for (int q = 0; q < ETB / 64; ++q) before += q < wid ? s_red[it & 1][q] : 0u;
    ++it;
    const unsigned long long q0 = o0 + before + (incl - bits), q1 = q0 + bits;
    const unsigned long long k = (q0 + smask) >> sh, B = k << sh;  // the first boundary at or past q0
    if (B < q1 && k < p.nblocks) {
      uint32_t pos = 0, cnt = 0;  // bits before each symbol, relative to q0
      const uint32_t rel = (uint32_t)(B - q0);
#pragma unroll
      for (int j = 0; j < EBPT; ++j) {
        cnt += pos < rel ? 1u : 0u;
        pos += l[j];
      }
      if constexpr (SLICE) p.offsets[k - p.k0] = p.sym_base + ib + cnt;
      else p.offsets[k] = ib + cnt;
    }
  }
}

// gh_ectx_merge_device: OR a slice's words into the stream's arrays.  One span is n source
// words s[0 .. n) for destination words d[0 .. n) of a zeroed (or partly merged) array.
// Only the span's first and last word can hold a neighbouring slice's bits (slices
// partition the stream's bits; a word or gap word strictly inside a slice's extent lies
// wholly inside its bits), so those two are ORed with device-scope atomics and the rest is
// stored plainly: a span of at most two words is all-atomic.  Interior, when source and
// destination agree modulo 16 bytes: a scalar head up to 16-byte alignment, a uint4
// grid-stride body, a scalar tail; otherwise dwords.  The payload always agrees: the slice
// buffer starts at stream bit org = base_bit & ~1023, so source word lead + i and
// destination word word0 + i sit at the same offset from 128-byte-aligned bases (the
// caller's arrays are 16-byte aligned at least).  The gap words agree when gapw0 is a
// multiple of 4; they are 1 / 32 of the payload's bytes.  Bandwidth-bound: one read and
// one write of the slice.
__device__ __forceinline__ void enc_merge_span(const uint32_t* __restrict__ s, uint32_t* __restrict__ d, uint64_t n,
                                               uint64_t tid, uint64_t nth) {
  if (n == 0) return;
  if (tid == 0) {
    __hip_atomic_fetch_or(&d[0], s[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n > 1) __hip_atomic_fetch_or(&d[n - 1], s[n - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (n <= 2) return;
  const uint64_t lo = 1, hi = n - 1;  // the interior [lo, hi)
  if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) != 0) {
    for (uint64_t i = lo + tid; i < hi; i += nth) d[i] = s[i];
    return;
  }
  const uint64_t a = min(hi, lo + ((4u - (uint32_t)(((uintptr_t)(d + lo) >> 2) & 3u)) & 3u));  // head [lo, a)
  const uint64_t b = a + ((hi - a) & ~3ull);                                                    // body [a, b)
  if (lo + tid < a) d[lo + tid] = s[lo + tid];
  const uint4* s4 = (const uint4*)(s + a);
  uint4* d4 = (uint4*)(d + a);
  for (uint64_t i = tid; i < (b - a) / 4; i += nth) d4[i] = s4[i];
  if (b + tid < hi) d[b + tid] = s[b + tid];
}

struct EncMergeParams {
  const uint32_t* sw;  // the slice's payload words: source word i is stream word word0 + i
  uint32_t* dw;        // &d_payload[word0]
  uint64_t nw;
  const uint32_t* sg;  // the slice's gap words
  uint32_t* dg;        // &d_gap_words[gapw0]
  uint64_t ng;
};
constexpr int MERGE_TB = 256;
__global__ __launch_bounds__(MERGE_TB) void gh_enc_merge_kernel(const EncMergeParams p) {
  const uint64_t tid = (uint64_t)blockIdx.x * MERGE_TB + threadIdx.x, nth = (uint64_t)gridDim.x * MERGE_TB;
  enc_merge_span(p.sw, p.dw, p.nw, tid, nth);
  enc_merge_span(p.sg, p.dg, p.ng, tid, nth);
}

#include "gh_ebatch.hip"
#include "gh_planes_split.hip"
#include "gh_pmask.hip"

}  // namespace gh

using namespace gh;

struct gh_ectx {
  int device = 0;
  int num_cu = 0;
  Stream stream;
  uint64_t n = 0;
  DevBuf d_in;                                 // the input, padded (grown on demand, as the buffers below)
  DevBuf d_count;                              // 256 u64
  DevBuf d_lut;                                // 256 u32
  DevBuf d_chunk_bits, d_chunk_off;            // u32 per chunk; u32 local offsets, then u64 per scan block
  DevBuf d_words, d_gaps;
  DevBuf d_junk;                               // write kernel padding stores: one dword per thread
  const uint32_t* d_loc = nullptr;             // the last encode's chunk offsets: views into d_chunk_off
  const unsigned long long* d_blk = nullptr;
  DevBuf d_index;                              // gh_ectx_index: the entries
  gh_encode_plan plan{};
  bool planned = false, encoded = false;
  uint64_t counts[256] = {};                   // histogram of the loaded input, when `counted`
  bool counted = false;
  bool sliced = false;                         // the last encode was a slice encode: `slice`
  std::string shape;                           // the last encode's write kernel (gh_ectx_kernel_shape)
  gh_slice slice{};
  EventPair ev;
  Event ev_in;                                 // gh_ectx_load_device: the producer stream's position
  ~gh_ectx() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }  // (then the members free their memory and events, the stream last)
};

extern "C" int gh_ectx_create(int device, gh_ectx** out) {
  if (!out) return fail(GH_E_ARG, "null ctx pointer");
  *out = nullptr;
  int num_cu = 0;
  if (int rc = open_device(device, "no HIP device visible (the GPU encoder has no CPU fallback)", &num_cu)) return rc;
  std::unique_ptr<gh_ectx> e(new gh_ectx());  // (a failure below frees what was made)
  e->device = device;
  e->num_cu = num_cu;
  if (int rc = e->stream.create()) return rc;
  if (int rc = e->d_count.alloc(256 * 8)) return rc;
  if (int rc = e->d_lut.alloc(256 * 4)) return rc;
  if (int rc = e->ev.create()) return rc;
  *out = e.release();
  return GH_OK;
}

extern "C" int gh_ectx_destroy(gh_ectx* e) {
  delete e;
  return GH_OK;
}

extern "C" int gh_ectx_load(gh_ectx* e, const uint8_t* in, uint64_t n) {
  if (!e || (n && !in)) return fail(GH_E_ARG, "null argument");
  GH_HIP(hipSetDevice(e->device));
  // padded: the write kernel's loads are unconditional (up to a chunk + 32 bytes past n)
  if (int rc = e->d_in.reserve(n + ECHUNK + 64)) return rc;
  if (n) GH_HIP(hipMemcpyAsync(e->d_in.get(), in, n, hipMemcpyHostToDevice, e->stream));
  GH_HIP(hipStreamSynchronize(e->stream));
  e->n = n;
  e->planned = e->encoded = e->counted = e->sliced = false;
  return GH_OK;
}

extern "C" int gh_ectx_load_device(gh_ectx* e, const void* d_in, uint64_t n, void* hip_stream) {
  if (!e || (n && !d_in)) return fail(GH_E_ARG, "null argument");
  GH_HIP(hipSetDevice(e->device));
  e->planned = e->encoded = e->counted = e->sliced = false;  // (the input buffer changes from here on)
  e->n = 0;
  if (int rc = e->d_in.reserve(n + ECHUNK + 64)) return rc;
  if (n) {
    // after what the producer's stream holds now, then device to device on the context's stream
    if (int rc = stream_follow(e->ev_in, hip_stream, e->stream)) return rc;
    GH_HIP(hipMemcpyAsync(e->d_in.get(), d_in, n, hipMemcpyDefault, e->stream));
  }
  GH_HIP(hipStreamSynchronize(e->stream));
  e->n = n;
  return GH_OK;
}

// GH_ENC_GRID=k (tests): at most k workgroups for the encoder's persistent kernels
// (histogram, bits, write), so a short input gives each workgroup many chunks.  It only
// lowers a grid; read at each launch.
static uint32_t enc_grid_cap(uint32_t grid) {
  if (const char* eg = getenv("GH_ENC_GRID")) grid = (uint32_t)std::clamp<long>(atol(eg), 1, (long)grid);
  return grid;
}

// Byte histogram of the loaded input into e->counts (synchronous).
static int ectx_hist(gh_ectx* e) {
  GH_HIP(hipMemsetAsync(e->d_count.get(), 0, 256 * 8, e->stream));
  const uint64_t nchunks = ceil_div(e->n, ECHUNK);
  if (nchunks) {
    const uint32_t grid = enc_grid_cap((uint32_t)std::min<uint64_t>(nchunks, 4ull * e->num_cu));
    hipLaunchKernelGGL(gh_enc_hist_kernel, dim3(grid), dim3(ETB), 0, e->stream, e->d_in.get<uint8_t>(), e->n,
                       e->d_count.get<unsigned long long>());
    GH_HIP(hipGetLastError());
  }
  GH_HIP(hipMemcpyAsync(e->counts, e->d_count.get(), 256 * 8, hipMemcpyDeviceToHost, e->stream));
  GH_HIP(hipStreamSynchronize(e->stream));
  e->counted = true;
  return GH_OK;
}

extern "C" int gh_ectx_plan(gh_ectx* e, int force_version, gh_encode_plan* plan) {
  if (!e) return fail(GH_E_ARG, "null ctx");
  GH_HIP(hipSetDevice(e->device));
  e->planned = e->encoded = e->sliced = false;
  int rc = ectx_hist(e);
  if (rc) return rc;
  gh_encode_plan& pl = e->plan;
  std::memset(&pl, 0, sizeof(pl));
  pl.n = e->n;
  std::memcpy(pl.count, e->counts, sizeof(pl.count));
  rc = plan_from_counts(&pl, force_version);
  if (rc) return rc;
  e->planned = true;
  if (plan) *plan = pl;
  return GH_OK;
}

extern "C" int gh_ectx_counts(gh_ectx* e, uint64_t counts[256]) {
  if (!e || !counts) return fail(GH_E_ARG, "null argument");
  GH_HIP(hipSetDevice(e->device));
  e->planned = e->encoded = e->sliced = false;
  const int rc = ectx_hist(e);
  if (rc) return rc;
  std::memcpy(counts, e->counts, sizeof(e->counts));
  return GH_OK;
}

// A picked write kernel: its launch pointer and the name of its template instantiation
// (gh_ectx_kernel_shape, gh_enc_kernel_shapes, gh_enc_kernel_shape_for), both from the one
// template argument list, as the decoder's pickers (gh_decode.hip).
struct EncKern {
  const void* fn;
  const char* name;
};
template <int NSW, bool SLICE>
static EncKern enc_write_kern() {
  static const std::string n = "enc_write<" + std::to_string(NSW) + ",slice=" + (SLICE ? "1" : "0") + ">";
  return {(const void*)gh_enc_write_kernel<NSW, SLICE>, n.c_str()};
}
template <bool SLICE>
static EncKern enc_write_kernel(int need) {
  return need <= 1   ? enc_write_kern<1, SLICE>()
         : need <= 2 ? enc_write_kern<2, SLICE>()
         : need <= 3 ? enc_write_kern<3, SLICE>()
         : need <= 4 ? enc_write_kern<4, SLICE>()
         : need <= 5 ? enc_write_kern<5, SLICE>()
         : need <= 6 ? enc_write_kern<6, SLICE>()
                     : enc_write_kern<9, SLICE>();
}
constexpr int ENC_NEED_MAX = 9;  // the largest NSW: 9 x ETB words hold a chunk at 16 bits per byte

// The write kernel of an input of n bytes and `bits` code bits (a whole stream or a slice).
// Payload words per chunk ~ ECHUNK * W / n: NSW = store instructions per thread.
static EncKern enc_write_kernel_for(uint64_t n, uint64_t bits, bool slice) {
  const double wpc = (double)ECHUNK * (double)ceil_div(bits, 32) / (double)std::max<uint64_t>(n, 1) + 2.0;
  const int need = (int)std::ceil(wpc * 1.05 / ETB);
  return slice ? enc_write_kernel<true>(need) : enc_write_kernel<false>(need);
}

// Every name enc_write_kernel_for can return, one per line: the picker enumerated over its
// argument domain.  No device.
static std::string all_enc_kernel_shapes() {
  std::string s;
  for (int slice = 0; slice <= 1; ++slice) {
    const char* last = nullptr;
    for (int need = 1; need <= ENC_NEED_MAX; ++need) {
      const char* n = slice ? enc_write_kernel<true>(need).name : enc_write_kernel<false>(need).name;
      if (n != last) s += std::string(n) + "\n";
      last = n;
    }
  }
  return s;
}

// The device encode of the loaded input under pl, as code bits [base_bit, base_bit + bits)
// of pl's stream: the whole stream (slice = false, base_bit 0, bits = pl.bits) or a slice
// of it.  d_words[0] / d_gaps[0] are the payload / gap word holding stream bit
// org = base_bit & ~1023 (a whole stream: words 0).
static int ectx_encode_run(gh_ectx* e, const gh_encode_plan& pl, bool slice, uint64_t base_bit, uint64_t bits,
                           float* kernel_ms) {
  for (int v = 0; v < 256; ++v)
    if (pl.len[v] > GH_MAX_CODE_LEN) return fail(GH_E_TABLE, "code longer than 16 bits");
  uint32_t lut[256];
  for (int v = 0; v < 256; ++v) lut[v] = (pl.code[v] << 8) | pl.len[v];
  const uint64_t nchunks = ceil_div(e->n, ECHUNK);
  const uint64_t org = base_bit & ~1023ull, end = base_bit + bits;
  const uint64_t NW = ceil_div(end, 32) - (org >> 5);    // a whole stream: pl.w
  const uint64_t GW = ceil_div(end, 1024) - (org >> 10);  // a whole stream: ceil(pl.g / 8)
  if (int rc = e->d_chunk_bits.reserve(4 * (nchunks + 1))) return rc;
  if (int rc = e->d_chunk_off.reserve(4 * (nchunks + 1) + 8 * (nchunks / SCAN_BLK + 2) + 64)) return rc;
  if (int rc = e->d_words.reserve(4 * (NW + 4))) return rc;
  if (int rc = e->d_gaps.reserve(4 * (GW + 4))) return rc;
  if (nchunks >= (1ull << 32)) return fail(GH_E_ARG, "input too large for the GPU encoder");
  GH_HIP(hipMemcpyAsync(e->d_lut.get(), lut, sizeof(lut), hipMemcpyHostToDevice, e->stream));
  GH_HIP(hipEventRecord(e->ev.a, e->stream));
  GH_HIP(hipMemsetAsync(e->d_gaps.get(), 0, 4 * (GW + 4), e->stream));
  e->shape.clear();  // (an empty input launches no kernel)
  if (nchunks) {
    const EncKern kern = enc_write_kernel_for(e->n, bits, slice);
    const void* wk = kern.fn;
    e->shape = kern.name;
    // the LDS image holds a chunk at the code's longest codeword
    uint32_t maxlen = 1;
    for (int v = 0; v < 256; ++v) maxlen = std::max<uint32_t>(maxlen, pl.len[v]);
    const uint32_t ew = (1024u + ECHUNK * maxlen + 64u) / 32u + 2u, eg = (1024u + ECHUNK * maxlen) / 1024u + 2u;
    if (ew > (uint32_t)EWORDS || eg > (uint32_t)EGAPW) return fail(GH_E_TABLE, "code longer than 16 bits");
    const size_t dyn = 4ull * (ew + eg);
    int pb = 0, pw = 0;  // persistent grids: what is resident at once
    GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pb, (const void*)gh_enc_bits_kernel, ETB, 0));
    GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pw, wk, ETB, dyn));
    const uint32_t gb = enc_grid_cap((uint32_t)std::min<uint64_t>(nchunks, (uint64_t)std::max(pb, 1) * e->num_cu));
    const uint8_t* d_in = e->d_in.get<uint8_t>();
    const uint32_t* d_lut = e->d_lut.get<uint32_t>();
    uint32_t* d_chunk_bits = e->d_chunk_bits.get<uint32_t>();
    unsigned long long* d_chunk_off = e->d_chunk_off.get<unsigned long long>();
    hipLaunchKernelGGL(gh_enc_bits_kernel, dim3(gb), dim3(ETB), 0, e->stream, d_in, e->n, (uint32_t)nchunks,
                       d_lut, d_chunk_bits);
    const uint32_t nblk = (uint32_t)ceil_div(nchunks, SCAN_BLK);
    uint32_t* loc = (uint32_t*)d_chunk_off;
    unsigned long long* blk = d_chunk_off + (nchunks + 2) / 2 + 1;  // after the local offsets
    hipLaunchKernelGGL(gh_enc_scan_kernel, dim3(nblk), dim3(SCAN_TB), 0, e->stream, d_chunk_bits,
                       (uint32_t)nchunks, loc, blk);
    hipLaunchKernelGGL(gh_enc_blkscan_kernel, dim3(1), dim3(SCAN_TB), 0, e->stream, blk, nblk,
                       (unsigned long long)base_bit);
    const uint32_t gw = enc_grid_cap((uint32_t)std::min<uint64_t>(nchunks, (uint64_t)std::max(pw, 1) * e->num_cu));
    if (int rc = e->d_junk.reserve(4ull * gw * ETB)) return rc;
    e->d_loc = loc;
    e->d_blk = blk;
    EncParams p{d_in, d_lut, loc, blk, e->d_words.get<uint32_t>(), e->d_gaps.get<uint32_t>(),
                e->d_junk.get<uint32_t>(), e->n, (uint32_t)nchunks, ew, eg, org};
    void* args[] = {&p};
    GH_HIP(hipLaunchKernel(wk, dim3(gw), dim3(ETB), args, dyn, e->stream));
    GH_HIP(hipGetLastError());
  }
  GH_HIP(hipEventRecord(e->ev.b, e->stream));
  GH_HIP(hipStreamSynchronize(e->stream));
  if (kernel_ms) return e->ev.elapsed(kernel_ms);
  return GH_OK;
}

extern "C" int gh_ectx_encode(gh_ectx* e, float* kernel_ms) {
  if (!e) return fail(GH_E_ARG, "null ctx");
  if (!e->planned) return fail(GH_E_STATE, "gh_ectx_encode before gh_ectx_plan");
  GH_HIP(hipSetDevice(e->device));
  e->encoded = e->sliced = false;
  const int rc = ectx_encode_run(e, e->plan, false, 0, e->plan.bits, kernel_ms);
  if (rc) return rc;
  e->encoded = true;
  return GH_OK;
}

extern "C" int gh_ectx_encode_slice(gh_ectx* e, const gh_encode_plan* sp, uint64_t base_bit, gh_slice* out,
                                    float* kernel_ms) {
  if (!e || !sp) return fail(GH_E_ARG, "null argument");
  GH_HIP(hipSetDevice(e->device));
  e->encoded = e->sliced = false;  // (the buffers of an earlier encode are reused)
  if (!e->counted) {
    const int rc = ectx_hist(e);
    if (rc) return rc;
  }
  uint64_t bits = 0;
  for (int v = 0; v < 256; ++v) {
    if (e->counts[v] && sp->len[v] == 0) return fail(GH_E_TABLE, "a byte of the input has no code in the plan");
    bits += e->counts[v] * sp->len[v];
  }
  gh_slice sl;
  if (gh_slice_extent(base_bit, bits, &sl) || base_bit + bits > sp->bits)
    return fail(GH_E_ARG, "slice ends past the plan's bit total");
  const int rc = ectx_encode_run(e, *sp, true, base_bit, bits, kernel_ms);
  if (rc) return rc;
  e->slice = sl;
  e->sliced = true;
  if (out) *out = sl;
  return GH_OK;
}

extern "C" int gh_ectx_kernel_shape(gh_ectx* e, char* buf, size_t cap) {
  if (!e) return fail(GH_E_ARG, "null ctx");
  if (!e->encoded && !e->sliced) return fail(GH_E_STATE, "gh_ectx_kernel_shape before an encode");
  return copy_name(e->shape, buf, cap);
}

extern "C" int gh_enc_kernel_shapes(char* buf, size_t cap) { return copy_name(all_enc_kernel_shapes(), buf, cap); }

extern "C" int gh_enc_kernel_shape_for(uint64_t n, uint64_t bits, int slice, char* buf, size_t cap) {
  if (slice != 0 && slice != 1) return fail(GH_E_ARG, "slice is 0 or 1");
  if (bits / GH_MAX_CODE_LEN > n || (bits / GH_MAX_CODE_LEN == n && bits % GH_MAX_CODE_LEN))
    return fail(GH_E_ARG, "more than 16 code bits per input byte");
  return copy_name(n ? enc_write_kernel_for(n, bits, slice != 0).name : "", buf, cap);
}

extern "C" int gh_ectx_download_slice(gh_ectx* e, uint32_t* words, uint64_t words_cap, uint32_t* gapw,
                                      uint64_t gaps_cap) {
  if (!e) return fail(GH_E_ARG, "null ctx");
  if (!e->sliced) return fail(GH_E_STATE, "gh_ectx_download_slice: the last encode was not a slice encode");
  const gh_slice& sl = e->slice;
  if (words_cap < sl.nwords || gaps_cap < sl.ngapw) return fail(GH_E_SMALL, "slice buffer too small");
  if ((sl.nwords && !words) || (sl.ngapw && !gapw)) return fail(GH_E_ARG, "null argument");
  GH_HIP(hipSetDevice(e->device));
  // the device buffers start at the gap word holding base_bit: up to 31 words before word0
  const uint64_t lead = sl.word0 - ((sl.base_bit & ~1023ull) >> 5);
  if (sl.ngapw) GH_HIP(hipMemcpyAsync(gapw, e->d_gaps.get(), 4 * sl.ngapw, hipMemcpyDeviceToHost, e->stream));
  if (sl.nwords) GH_HIP(hipMemcpyAsync(words, e->d_words.get<uint32_t>() + lead, 4 * sl.nwords, hipMemcpyDeviceToHost, e->stream));
  GH_HIP(hipStreamSynchronize(e->stream));
  return GH_OK;
}

extern "C" int gh_ectx_download(gh_ectx* e, void* out, uint64_t out_len) {
  if (!e || !out) return fail(GH_E_ARG, "null argument");
  if (!e->encoded) return fail(GH_E_STATE, "gh_ectx_download before gh_ectx_encode");
  const gh_encode_plan& pl = e->plan;
  if (out_len < pl.file_bytes) return fail(GH_E_SMALL, "output buffer too small");
  GH_HIP(hipSetDevice(e->device));
  uint8_t* o = (uint8_t*)out;
  const size_t hdr = encode_header(&pl, o);
  const uint64_t GW = ceil_div(pl.g, GH_GAPS_PER_WORD);
  if (GW) GH_HIP(hipMemcpyAsync(o + hdr, e->d_gaps.get(), 4 * GW, hipMemcpyDeviceToHost, e->stream));
  if (pl.w) GH_HIP(hipMemcpyAsync(o + hdr + 4 * GW, e->d_words.get(), 4 * pl.w, hipMemcpyDeviceToHost, e->stream));
  GH_HIP(hipStreamSynchronize(e->stream));
  return GH_OK;
}

// The index kernel reads the input, the code lengths, the chunk bits and the two-level
// chunk offsets of the last encode; nothing of the encode's output.
extern "C" int gh_ectx_index(gh_ectx* e, uint32_t log2_stride, void* out, uint64_t out_len, float* kernel_ms) {
  if (!e || !out) return fail(GH_E_ARG, "null argument");
  if (!e->encoded) return fail(GH_E_STATE, "gh_ectx_index before gh_ectx_encode");
  const gh_encode_plan& pl = e->plan;
  const uint64_t bytes = gh_index_bytes(pl.g, log2_stride);
  if (bytes == 0) return fail(GH_E_ARG, "index stride outside 2^8 .. 2^20 segments");
  if (out_len < bytes) return fail(GH_E_SMALL, "index buffer too small");
  GH_HIP(hipSetDevice(e->device));
  uint8_t* o = (uint8_t*)out;
  const uint64_t nblocks = (bytes - 40) / 8 - 1;
  const uint64_t nchunks = ceil_div(e->n, ECHUNK);
  if (int rc = e->d_index.reserve(8 * nblocks)) return rc;
  GH_HIP(hipEventRecord(e->ev.a, e->stream));
  if (nblocks) {  // (then N > 0: the encode ran its kernels)
    int pc = 0;
    GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, (const void*)gh_enc_index_kernel<false>, ETB, 0));
    uint32_t grid = (uint32_t)std::min<uint64_t>(nchunks, (uint64_t)std::max(pc, 1) * e->num_cu);
    if (const char* eg = getenv("GH_ENC_INDEX_GRID"))  // tests: few workgroups, many chunks each
      grid = (uint32_t)std::clamp<long>(atol(eg), 1, (long)grid);
    const EncIndexParams p{e->d_in.get<uint8_t>(), e->d_lut.get<uint32_t>(), e->d_chunk_bits.get<uint32_t>(),
                           e->d_loc, e->d_blk, e->d_index.get<unsigned long long>(), e->n, nblocks,
                           (uint32_t)nchunks, 7u + log2_stride};
    hipLaunchKernelGGL(gh_enc_index_kernel<false>, dim3(grid), dim3(ETB), 0, e->stream, p);
    GH_HIP(hipGetLastError());
  }
  GH_HIP(hipEventRecord(e->ev.b, e->stream));
  if (nblocks) GH_HIP(hipMemcpyAsync(o + 40, e->d_index.get(), 8 * nblocks, hipMemcpyDeviceToHost, e->stream));
  GH_HIP(hipStreamSynchronize(e->stream));
  if (kernel_ms)
    if (int rc = e->ev.elapsed(kernel_ms)) return rc;
  index_header(log2_stride, pl.n, pl.g, nblocks + 1, o);
  std::memcpy(o + 40 + 8 * nblocks, &pl.n, 8);
  return GH_OK;
}

// The entries the last slice encode owns: the index kernel's SLICE variant over the same
// leftovers (the chunk offsets are stream bit positions: the block scan started at
// base_bit), then one copy of the nk entries.
extern "C" int gh_ectx_index_slice(gh_ectx* e, uint64_t sym_base, uint32_t log2_stride, uint64_t* entries,
                                   uint64_t cap, uint64_t* k0, uint64_t* nk, float* kernel_ms) {
  if (!e || !k0 || !nk || (cap && !entries)) return fail(GH_E_ARG, "null argument");
  if (!e->sliced) return fail(GH_E_STATE, "gh_ectx_index_slice: the last encode was not a slice encode");
  if (int rc = gh_index_slice_extent(e->slice.base_bit, e->slice.bits, log2_stride, k0, nk)) return rc;
  if (cap < *nk) return fail(GH_E_SMALL, "entry buffer too small");
  GH_HIP(hipSetDevice(e->device));
  const uint64_t nchunks = ceil_div(e->n, ECHUNK), n_own = *nk;
  if (n_own)
    if (int rc = e->d_index.reserve(8 * n_own)) return rc;
  GH_HIP(hipEventRecord(e->ev.a, e->stream));
  if (n_own) {  // (then the slice holds bits: the encode ran its kernels)
    int pc = 0;
    GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, (const void*)gh_enc_index_kernel<true>, ETB, 0));
    uint32_t grid = (uint32_t)std::min<uint64_t>(nchunks, (uint64_t)std::max(pc, 1) * e->num_cu);
    if (const char* eg = getenv("GH_ENC_INDEX_GRID"))  // tests: few workgroups, many chunks each
      grid = (uint32_t)std::clamp<long>(atol(eg), 1, (long)grid);
    EncIndexSliceParams p{};
    static_cast<EncIndexParams&>(p) = EncIndexParams{e->d_in.get<uint8_t>(), e->d_lut.get<uint32_t>(),
                                                     e->d_chunk_bits.get<uint32_t>(), e->d_loc, e->d_blk,
                                                     e->d_index.get<unsigned long long>(), e->n, *k0 + n_own,
                                                     (uint32_t)nchunks, 7u + log2_stride};
    p.k0 = *k0;
    p.sym_base = sym_base;
    hipLaunchKernelGGL(gh_enc_index_kernel<true>, dim3(grid), dim3(ETB), 0, e->stream, p);
    GH_HIP(hipGetLastError());
  }
  GH_HIP(hipEventRecord(e->ev.b, e->stream));
  if (n_own) GH_HIP(hipMemcpyAsync(entries, e->d_index.get(), 8 * n_own, hipMemcpyDeviceToHost, e->stream));
  GH_HIP(hipStreamSynchronize(e->stream));
  if (kernel_ms)
    if (int rc = e->ev.elapsed(kernel_ms)) return rc;
  return GH_OK;
}

extern "C" int gh_ectx_merge_device(gh_ectx* e, uint32_t* d_payload, uint64_t payload_words, uint32_t* d_gap_words,
                                    uint64_t gap_words, void* hip_stream) {
  if (!e) return fail(GH_E_ARG, "null ctx");
  if (!e->sliced && !e->encoded) return fail(GH_E_STATE, "gh_ectx_merge_device before an encode");
  gh_slice sl = e->slice;
  if (!e->sliced)  // a whole encode is the slice at bit 0
    if (gh_slice_extent(0, e->plan.bits, &sl)) return GH_E_ARG;
  if ((sl.nwords && !d_payload) || (sl.ngapw && !d_gap_words)) return fail(GH_E_ARG, "null argument");
  if (sl.word0 > payload_words || sl.nwords > payload_words - sl.word0 || sl.gapw0 > gap_words ||
      sl.ngapw > gap_words - sl.gapw0)
    return fail(GH_E_ARG, "slice extents outside the destination arrays");
  if (((uintptr_t)d_payload | (uintptr_t)d_gap_words) & 15u)
    return fail(GH_E_ARG, "destination arrays must be 16-byte aligned");
  GH_HIP(hipSetDevice(e->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)e->stream;
  if (sl.nwords || sl.ngapw) {
    // the device buffers start at the gap word holding base_bit: up to 31 words before word0
    const uint64_t lead = sl.word0 - ((sl.base_bit & ~1023ull) >> 5);
    const EncMergeParams p{e->d_words.get<uint32_t>() + lead, d_payload + sl.word0, sl.nwords,
                           e->d_gaps.get<uint32_t>(), d_gap_words + sl.gapw0, sl.ngapw};
    // a uint4 per thread, not a persistent grid: the copy yardstick's finding (gh_bw.hip: 6.1
    // against 4.4-4.9 TB/s for grid-stride loops; this kernel at 8 workgroups per CU: 4.2)
    const uint64_t want = ceil_div(std::max<uint64_t>(sl.nwords / 4 + 2, 1), MERGE_TB);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, 0x7fffffffull);
    hipLaunchKernelGGL(gh_enc_merge_kernel, dim3(grid), dim3(MERGE_TB), 0, st, p);
    GH_HIP(hipGetLastError());
  }
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

// One-shot sliced encode (gaphuff.h).  Slice i: bytes [n i / K, n (i + 1) / K) on device
// devs[i % ng], in a gh_ectx of its own; a host thread per distinct device takes that
// device's slices in turn.  Two passes with the stream-wide plan between them: the first
// loads the slices and takes their histograms, the second encodes every slice at its
// scanned bit offset and downloads it.  The merge runs on the calling thread, in slice
// order (neighbouring slices share their edge words).
// ix (gh_encode_sharded_index; NULL: no index): every slice's context also emits the index
// entries the slice owns, right after its encode, and the calling thread stores them into
// the image of gh_index_image_init.
struct ShardedIndex {
  uint32_t log2_stride;
  void* out;
  uint64_t len;
  float* ms;
};
static int encode_sharded_run(const uint8_t* in, uint64_t n, const gh_opts* o, uint32_t nslices, int force_version,
                              void* out, uint64_t out_len, gh_encode_plan* plan_out, float* kernel_ms,
                              const ShardedIndex* ix) {
  if ((n && !in) || !out || nslices == 0) return fail(GH_E_ARG, "null argument or no slices");
  if (ix && !ix->out) return fail(GH_E_ARG, "null argument");
  if (ix && gh_index_bytes(0, ix->log2_stride) == 0) return fail(GH_E_ARG, "index stride outside 2^8 .. 2^20 segments");
  const int ng = (o && o->ngpus > 1) ? o->ngpus : 1;
  const uint32_t K = nslices;
  std::vector<int> dev(K);
  for (uint32_t i = 0; i < K; ++i) dev[i] = (o && o->devices) ? o->devices[i % ng] : (ng > 1 ? (int)(i % ng) : 0);
  std::vector<int> devs(dev);  // the distinct devices: one host thread each
  std::sort(devs.begin(), devs.end());
  devs.erase(std::unique(devs.begin(), devs.end()), devs.end());
  const int nd = (int)devs.size();
  std::vector<gh_ectx*> ctx(K, nullptr);
  auto cleanup = [&]() {
    for (auto*& c : ctx) {
      gh_ectx_destroy(c);
      c = nullptr;
    }
  };
  // f(i) for every slice i, the slices of one device in turn on that device's thread
  auto per_device = [&](auto f) {
    std::vector<int> rc(nd, GH_OK);
    std::vector<std::string> msg(nd);
    auto run = [&](int d) {
      for (uint32_t i = 0; i < K && !rc[d]; ++i)
        if (dev[i] == devs[d] && (rc[d] = f(i))) msg[d] = gh_last_error();
    };
    if (nd == 1) {
      run(0);
    } else {
      std::vector<std::thread> th;
      for (int d = 0; d < nd; ++d) th.emplace_back(run, d);
      for (auto& t : th) t.join();
    }
    for (int d = 0; d < nd; ++d)
      if (rc[d]) {
        set_error(msg[d]);
        return rc[d];
      }
    return (int)GH_OK;
  };
  auto cut = [&](uint32_t i) { return (uint64_t)((unsigned __int128)n * i / K); };
  std::vector<uint64_t> counts((size_t)K * 256, 0);
  int rc = per_device([&](uint32_t i) {
    int r = gh_ectx_create(dev[i], &ctx[i]);
    if (!r) r = gh_ectx_load(ctx[i], in + cut(i), cut(i + 1) - cut(i));
    if (!r) r = gh_ectx_counts(ctx[i], &counts[(size_t)i * 256]);
    return r;
  });
  gh_encode_plan* plan = new gh_encode_plan;
  std::vector<uint64_t> base(K + 1, 0);
  if (!rc) {
    uint64_t sum[256] = {};
    for (uint32_t i = 0; i < K; ++i)
      for (int v = 0; v < 256; ++v) sum[v] += counts[(size_t)i * 256 + v];
    rc = gh_encode_plan_from_counts(sum, force_version, plan);
  }
  if (!rc) {
    if (plan_out) *plan_out = *plan;
    if (out_len < plan->file_bytes) rc = fail(GH_E_SMALL, "output buffer too small");
    else if (ix && ix->len < gh_index_bytes(plan->g, ix->log2_stride)) rc = fail(GH_E_SMALL, "index buffer too small");
  }
  std::vector<gh_slice> sl(K);
  std::vector<std::vector<uint32_t>> words(K), gapw(K);
  std::vector<float> ms(K, 0.f);
  std::vector<std::vector<uint64_t>> ent(K);  // slice i's entries [ek0[i], ek0[i] + ent[i].size())
  std::vector<uint64_t> ek0(K, 0);
  std::vector<float> ims(K, 0.f);
  if (!rc) {
    for (uint32_t i = 0; i < K; ++i) {  // the slices' bit totals, scanned
      uint64_t b = 0;
      for (int v = 0; v < 256; ++v) b += counts[(size_t)i * 256 + v] * plan->len[v];
      base[i + 1] = base[i] + b;
    }
    rc = per_device([&](uint32_t i) {
      int r = gh_ectx_encode_slice(ctx[i], plan, base[i], &sl[i], &ms[i]);
      if (!r) {
        words[i].resize(sl[i].nwords);
        gapw[i].resize(sl[i].ngapw);
        r = gh_ectx_download_slice(ctx[i], words[i].data(), words[i].size(), gapw[i].data(), gapw[i].size());
      }
      if (!r && ix) {
        uint64_t nk = 0;
        r = gh_index_slice_extent(sl[i].base_bit, sl[i].bits, ix->log2_stride, &ek0[i], &nk);
        if (!r) {
          ent[i].resize(nk);
          r = gh_ectx_index_slice(ctx[i], cut(i), ix->log2_stride, ent[i].data(), nk, &ek0[i], &nk, &ims[i]);
        }
      }
      gh_ectx_destroy(ctx[i]);  // (this device's memory goes back before its next slice)
      ctx[i] = nullptr;
      return r;
    });
  }
  cleanup();
  if (!rc) rc = gh_encode_image_init(plan, out, out_len);
  for (uint32_t i = 0; i < K && !rc; ++i) rc = gh_slice_merge(out, out_len, plan, &sl[i], words[i].data(), gapw[i].data());
  if (!rc && kernel_ms) {
    std::map<int, float> per_dev;
    for (uint32_t i = 0; i < K; ++i) per_dev[dev[i]] += ms[i];
    *kernel_ms = 0.f;
    for (auto& d : per_dev) *kernel_ms = std::max(*kernel_ms, d.second);
  }
  if (!rc && ix) {
    rc = gh_index_image_init(plan, ix->log2_stride, ix->out, ix->len);
    for (uint32_t i = 0; i < K && !rc; ++i) rc = gh_index_slice_merge(ix->out, ix->len, ek0[i], ent[i].size(), ent[i].data());
    if (!rc && ix->ms) {
      std::map<int, float> per_dev;
      for (uint32_t i = 0; i < K; ++i) per_dev[dev[i]] += ims[i];
      *ix->ms = 0.f;
      for (auto& d : per_dev) *ix->ms = std::max(*ix->ms, d.second);
    }
  }
  delete plan;
  return rc;
}

extern "C" int gh_encode_sharded(const uint8_t* in, uint64_t n, const gh_opts* o, uint32_t nslices,
                                 int force_version, void* out, uint64_t out_len, gh_encode_plan* plan_out,
                                 float* kernel_ms) {
  return encode_sharded_run(in, n, o, nslices, force_version, out, out_len, plan_out, kernel_ms, nullptr);
}

extern "C" int gh_encode_sharded_index(const uint8_t* in, uint64_t n, const gh_opts* o, uint32_t nslices,
                                       int force_version, void* out, uint64_t out_len, gh_encode_plan* plan_out,
                                       float* kernel_ms, uint32_t log2_stride, void* index_out, uint64_t index_len,
                                       float* index_ms) {
  const ShardedIndex ix{log2_stride, index_out, index_len, index_ms};
  return encode_sharded_run(in, n, o, nslices, force_version, out, out_len, plan_out, kernel_ms, &ix);
}

// ---- batched encode (gaphuff.h; kernels: gh_ebatch.hip; host layout: gh::ebatch_*_plan) ---
constexpr uint32_t EBATCH_LAUNCHES = 5;  // two arena memsets, then bits, scan, write
static const char* const EBATCH_SHAPE = "ebatch<lut=1>";

struct gh_ebatch {
  EventPair ev_hist, ev_code;
  EventPair ev_split;                      // gh_planes_load_device: around the split kernel
  bool split_timed = false;                // the last load was gh_planes_load_device and launched it
  DevBuf in, unit0, items;                 // the loaded batch
  DevBuf code;                             // one EBatchDesc per stream, then 256 table entries per stream
  DevBuf counts;                           // 256 u64 per stream
  DevBuf recs;                             // gh_batchenc_plan_device: one EBatchCodeRec per stream
  DevBuf unit_bits, unit_off, flags;       // encode scratch; flags: 4 summary words, then a status word per stream
  DevBuf payload, gaps;                    // the output arenas
  EBatchInPlan inp;
  EBatchOutPlan outp;
  std::vector<uint64_t> n;
  std::vector<gh_encode_plan> plans;
  uint32_t nstreams = 0;
  uint64_t out_bytes = 0;
  float hist_ms = 0, code_ms = 0, plan_host_ms = 0;
  bool loaded = false, planned = false;
  bool counts_on_device = false;  // a device plan: plans[i].count[] is filled by the first plan_of
  // gh_pmask_device: buffers, events and results of its own (the batch's state is not touched)
  DevBuf pm_desc;                 // PMaskTensor per tensor, then unit0 and q0 (ntensors + 1 each)
  DevBuf pm_counts;               // 256 u64 per candidate plane, then plane_bytes and masks
  DevBuf pm_recs, pm_tables;      // the code kernel's outputs (the tables are scratch)
  Event pm_ev[4];                 // before the histogram, after it, after the code, after the decide
  uint32_t pm_nplanes = 0;
  bool pm_done = false;
  BatchQueue q;  // (last: its destructor waits for the encode before the buffers above go)
};

extern "C" int gh_ebatch_create(int device, gh_ebatch** out) {
  if (!out) return fail(GH_E_ARG, "null batch pointer");
  *out = nullptr;
  std::unique_ptr<gh_ebatch> b(new gh_ebatch());
  if (int rc = b->q.create(device, "no HIP device visible (the GPU encoder has no CPU fallback)")) return rc;
  if (int rc = b->ev_hist.create()) return rc;
  if (int rc = b->ev_code.create()) return rc;
  *out = b.release();
  return GH_OK;
}

extern "C" int gh_ebatch_destroy(gh_ebatch* b) {
  delete b;
  return GH_OK;
}

// The descriptors' load-time half: where every stream's bytes are.
static std::vector<EBatchDesc> ebatch_descs(const gh_ebatch* b) {
  std::vector<EBatchDesc> d(b->nstreams);
  for (uint32_t i = 0; i < b->nstreams; ++i) {
    d[i] = EBatchDesc{};
    d[i].in_off = b->inp.ext[i].in_off;
    d[i].n = b->n[i];
  }
  return d;
}

// A load's first half: the previous batch retired, the input plan of ns streams of n[i] bytes.
static int ebatch_load_plan(gh_ebatch* b, const uint64_t* n, uint32_t ns, EBatchInPlan& inp) {
  GH_HIP(hipSetDevice(b->q.device));
  if (int rc = b->q.quiesce()) return rc;  // the previous batch's encode reads what is replaced
  b->loaded = b->planned = b->split_timed = false;
  return ebatch_in_plan(n, ns, inp);
}

// Its second half, up to the arena's bytes: the batch's sizes, the unit prefix and the
// descriptors uploaded, the input arena reserved.
static int ebatch_load_reserve(gh_ebatch* b, const uint64_t* n, uint32_t ns, EBatchInPlan&& inp) {
  b->n.assign(n, n + ns);
  b->nstreams = ns;
  b->inp = std::move(inp);
  const EBatchInPlan& ip = b->inp;
  std::vector<uint32_t> unit0(ns + 1);
  for (uint32_t i = 0; i < ns; ++i) unit0[i] = (uint32_t)ip.ext[i].unit0;
  unit0[ns] = (uint32_t)ip.nunits;
  if (int rc = upload_at_least(b->unit0, unit0.data(), 4ull * (ns + 1))) return rc;
  // (room for the tables too: gh_ebatch_plan uploads the descriptors again, with them)
  if (int rc = b->code.reserve(std::max<uint64_t>((sizeof(EBatchDesc) + 1024ull) * ns, 16))) return rc;
  if (int rc = upload_at_least(b->code, ebatch_descs(b).data(), sizeof(EBatchDesc) * (uint64_t)ns)) return rc;
  return b->in.reserve(std::max<uint64_t>(ip.in_bytes, 16));
}

// src[i]: stream i's bytes, host memory or (device) device memory.
static int ebatch_load(gh_ebatch* b, const std::vector<const uint8_t*>& src, const uint64_t* n, bool device,
                       void* hip_stream) {
  const uint32_t ns = (uint32_t)src.size();
  EBatchInPlan inp;
  if (int rc = ebatch_load_plan(b, n, ns, inp)) return rc;
  for (uint32_t i = 0; i < ns; ++i)
    if (n[i] && !src[i]) return fail(GH_E_ARG, "stream " + std::to_string(i) + ": null input pointer");
  if (int rc = ebatch_load_reserve(b, n, ns, std::move(inp))) return rc;
  const EBatchInPlan& ip = b->inp;
  if (!device) {
    // the arena is assembled in host memory, padding included, and goes up in one copy
    std::vector<uint8_t> stage(ip.in_bytes, 0);
    for (uint32_t i = 0; i < ns; ++i)
      if (n[i]) std::memcpy(stage.data() + ip.ext[i].in_off, src[i], n[i]);
    if (int rc = upload_arena(b->q.device, b->in, stage.data(), stage.size())) return rc;
  } else if (ip.in_bytes) {
    std::vector<EBatchCopyItem> items(ns);
    for (uint32_t i = 0; i < ns; ++i) items[i] = EBatchCopyItem{src[i], n[i], ip.ext[i].in_off, ip.ext[i].in_bytes};
    if (int rc = upload_at_least(b->items, items.data(), sizeof(EBatchCopyItem) * (uint64_t)ns)) return rc;
    // after what the producer's stream holds now, then one copy kernel on the batch's stream
    if (int rc = b->q.follow(hip_stream)) return rc;
    hipLaunchKernelGGL(gh_ebatch_copy_kernel, dim3(std::min<uint32_t>(ns, 4096u), EB_COPY_Y), dim3(256), 0, b->q.stream,
                       b->items.get<EBatchCopyItem>(), ns, b->in.get<uint8_t>());
    GH_HIP(hipGetLastError());
    GH_HIP(hipStreamSynchronize(b->q.stream));
  }
  b->loaded = true;
  return GH_OK;
}

extern "C" int gh_ebatch_load(gh_ebatch* b, const uint8_t* const* in, const uint64_t* n, uint32_t nstreams) {
  if (!b || (nstreams && (!in || !n))) return fail(GH_E_ARG, "null argument");
  if (nstreams > EBATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  return ebatch_load(b, std::vector<const uint8_t*>(in, in + nstreams), n, false, nullptr);
}

extern "C" int gh_ebatch_load_device(gh_ebatch* b, const gh_ebatch_item* items, uint32_t nstreams, void* hip_stream) {
  if (!b || (nstreams && !items)) return fail(GH_E_ARG, "null argument");
  if (nstreams > EBATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  std::vector<const uint8_t*> src(nstreams);
  std::vector<uint64_t> n(nstreams);
  for (uint32_t i = 0; i < nstreams; ++i) {
    src[i] = (const uint8_t*)items[i].d_in;
    n[i] = items[i].n;
  }
  return ebatch_load(b, src, n.data(), true, hip_stream);
}

// ---- byte planes (gaphuff.h; kernel: gh_planes_split.hip; layout: gh_planes_layout) ----------
// The layout of a tensor list and what both loads derive from it: n[s] of every coded plane's
// stream and the prefix of the tensors' unit counts.
struct PlanesList {
  std::vector<gh_planes_slot> slots;
  std::vector<uint64_t> n;
  std::vector<uint32_t> unit0;  // ntensors + 1
  uint32_t nstreams = 0;
  uint64_t stored_bytes = 0;
};

static int planes_list(const gh_planes_item* items, uint32_t nt, const void* stored, uint64_t stored_len, PlanesList& pl) {
  pl.slots.resize((size_t)PLANES_MAX_E * std::max(nt, 1u));
  if (int rc = gh_planes_layout(items, nt, pl.slots.data(), &pl.nstreams, &pl.stored_bytes)) return rc;
  if (pl.stored_bytes && !stored) return fail(GH_E_ARG, "null stored arena");
  if (stored_len < pl.stored_bytes) return fail(GH_E_SMALL, "stored arena smaller than the stored planes");
  pl.n.resize(pl.nstreams);
  pl.unit0.resize(nt + 1);
  uint64_t units = 0;
  for (uint32_t t = 0; t < nt; ++t) {
    if (items[t].nelem && !items[t].data) return fail(GH_E_ARG, "tensor " + std::to_string(t) + ": null pointer");
    pl.unit0[t] = (uint32_t)units;
    units += planes_units(items[t].nelem);  // (< 2^31 + 2^54)
    if (units >= PLANES_MAX_UNITS) return fail(GH_E_ARG, "tensor " + std::to_string(t) + ": the list reaches 2^31 work units");
    for (uint32_t p = 0; p < items[t].elem_size; ++p)
      if (pl.slots[PLANES_MAX_E * t + p].stream != GH_PLANES_STORED) pl.n[pl.slots[PLANES_MAX_E * t + p].stream] = items[t].nelem;
  }
  pl.unit0[nt] = (uint32_t)units;
  return GH_OK;
}

extern "C" int gh_planes_load(gh_ebatch* b, const gh_planes_item* items, uint32_t ntensors, void* stored,
                              uint64_t stored_len) {
  if (!b || (ntensors && !items)) return fail(GH_E_ARG, "null argument");
  PlanesList pl;
  if (int rc = planes_list(items, ntensors, stored, stored_len, pl)) return rc;
  // the host split: coded planes into buffers of their own, stored planes into the caller's arena
  std::vector<std::vector<uint8_t>> coded(pl.nstreams);
  std::vector<const uint8_t*> src(pl.nstreams);
  if (pl.stored_bytes) std::memset(stored, 0, pl.stored_bytes);
  for (uint32_t t = 0; t < ntensors; ++t) {
    void* planes[PLANES_MAX_E] = {};
    for (uint32_t p = 0; p < items[t].elem_size; ++p) {
      const gh_planes_slot& s = pl.slots[PLANES_MAX_E * t + p];
      if (s.stream != GH_PLANES_STORED) {
        coded[s.stream].resize(std::max<uint64_t>(items[t].nelem, 1));
        planes[p] = coded[s.stream].data();
        src[s.stream] = coded[s.stream].data();
      } else {
        planes[p] = (uint8_t*)stored + s.stored_off;
      }
    }
    if (int rc = gh_planes_split_host(&items[t], planes)) return rc;
  }
  return ebatch_load(b, src, pl.n.data(), false, nullptr);
}

extern "C" int gh_planes_load_device(gh_ebatch* b, const gh_planes_item* items, uint32_t ntensors, void* d_stored,
                                     uint64_t stored_len, void* hip_stream) {
  if (!b || (ntensors && !items)) return fail(GH_E_ARG, "null argument");
  if ((uintptr_t)d_stored & 15u) return fail(GH_E_ARG, "stored arena not 16-byte aligned");
  PlanesList pl;
  if (int rc = planes_list(items, ntensors, d_stored, stored_len, pl)) return rc;
  const uint32_t ns = pl.nstreams;
  EBatchInPlan inp;
  if (int rc = ebatch_load_plan(b, pl.n.data(), ns, inp)) return rc;
  if (int rc = ebatch_load_reserve(b, pl.n.data(), ns, std::move(inp))) return rc;
  if (pl.unit0[ntensors]) {
    // the tensors' descriptors, then their unit prefix, in one upload
    const size_t dbytes = sizeof(PlanesTensor) * (size_t)ntensors;
    std::vector<uint8_t> up(dbytes + 4ull * (ntensors + 1));
    PlanesTensor* d = (PlanesTensor*)up.data();
    for (uint32_t t = 0; t < ntensors; ++t) {
      d[t] = PlanesTensor{};
      d[t].data = (uint8_t*)items[t].data;
      d[t].nelem = items[t].nelem;
      d[t].elem = items[t].elem_size;
      d[t].mask = items[t].coded_mask;
      for (uint32_t p = 0; p < items[t].elem_size; ++p) {
        const gh_planes_slot& s = pl.slots[PLANES_MAX_E * t + p];
        d[t].stream[p] = s.stream;
        d[t].off[p] = s.stream != GH_PLANES_STORED ? b->inp.ext[s.stream].in_off : s.stored_off;
      }
    }
    std::memcpy(up.data() + dbytes, pl.unit0.data(), 4ull * (ntensors + 1));
    if (int rc = upload_at_least(b->items, up.data(), up.size())) return rc;
    PlanesSplitParams sp{};
    sp.desc = b->items.get<PlanesTensor>();
    sp.unit0 = (const uint32_t*)(b->items.get<uint8_t>() + dbytes);
    sp.in = b->in.get<uint8_t>();
    sp.stored = (uint8_t*)d_stored;
    sp.ntensors = ntensors;
    sp.nunits = pl.unit0[ntensors];
    // GH_PLANES_GRID=k (tests): k workgroups, so that one wave walks many units and tensors
    const uint32_t grid = unit_grid("GH_PLANES_GRID", sp.nunits, PL_WAVES, b->q.num_cu);
    // after what the producer's stream holds now, then one split kernel on the batch's stream
    if (int rc = b->ev_split.create()) return rc;
    if (int rc = b->q.follow(hip_stream)) return rc;
    GH_HIP(hipEventRecord(b->ev_split.a, b->q.stream));
    hipLaunchKernelGGL(gh_planes_split_kernel, dim3(grid), dim3(PL_TB), 0, b->q.stream, sp);
    GH_HIP(hipGetLastError());
    GH_HIP(hipEventRecord(b->ev_split.b, b->q.stream));
    GH_HIP(hipStreamSynchronize(b->q.stream));
    b->split_timed = true;
  }
  b->loaded = true;
  return GH_OK;
}

extern "C" int gh_planes_load_times(gh_ebatch* b, float* kernel_ms) {
  if (!b || !kernel_ms) return fail(GH_E_ARG, "null argument");
  *kernel_ms = 0;
  if (!b->loaded) return fail(GH_E_STATE, "gh_planes_load_times before a load");
  return b->split_timed ? b->ev_split.elapsed(kernel_ms) : (int)GH_OK;
}

// ---- plane choice (gaphuff.h; kernels: gh_pmask.hip; rule: gh_pmask.hpp) ---------------------
constexpr bool PMASK_MERGE_DEFAULT = true;  // ("Plane choice": the measurement)

extern "C" int gh_pmask_device(gh_ebatch* b, const gh_planes_item* items, uint32_t ntensors, uint32_t* masks,
                               uint64_t* plane_bytes, void* hip_stream, gh_pmask_report* rep) {
  if (rep) *rep = gh_pmask_report{};
  if (!b || (ntensors && (!items || !masks))) return fail(GH_E_ARG, "null argument");
  // the numbering and the unit prefix
  std::vector<uint32_t> pre(2 * ((size_t)ntensors + 1));  // unit0, then q0
  uint32_t* unit0 = pre.data();
  uint32_t* q0 = pre.data() + ntensors + 1;
  uint64_t units = 0;
  uint32_t nplanes = 0;
  for (uint32_t t = 0; t < ntensors; ++t) {
    const std::string who = "tensor " + std::to_string(t) + ": ";
    if (!planes_elem_ok(items[t].elem_size)) return fail(GH_E_ARG, who + "element size not 1, 2, 4 or 8");
    if (items[t].nelem && !items[t].data) return fail(GH_E_ARG, who + "null pointer");
    unit0[t] = (uint32_t)units;
    q0[t] = nplanes;
    units += planes_units(items[t].nelem);  // (< 2^31 + 2^54)
    if (units >= PLANES_MAX_UNITS) return fail(GH_E_ARG, who + "the list reaches 2^31 work units");
    if (!pmask_next_q0(nplanes, items[t].elem_size, &nplanes)) return fail(GH_E_ARG, who + "more than 2^24 candidate planes");
  }
  unit0[ntensors] = (uint32_t)units;
  q0[ntensors] = nplanes;
  b->pm_nplanes = 0;  // (gh_pmask_counts sees the last call that succeeded, or nothing)
  b->pm_done = !ntensors;
  if (!ntensors) return GH_OK;
  GH_HIP(hipSetDevice(b->q.device));
  // one upload: the tensors' descriptors, then the two prefixes
  const size_t dbytes = sizeof(PMaskTensor) * (size_t)ntensors;
  std::vector<uint8_t> up(dbytes + 4 * pre.size());
  PMaskTensor* d = (PMaskTensor*)up.data();
  for (uint32_t t = 0; t < ntensors; ++t) d[t] = PMaskTensor{(const uint8_t*)items[t].data, items[t].nelem, q0[t], items[t].elem_size};
  std::memcpy(up.data() + dbytes, pre.data(), 4 * pre.size());
  if (int rc = upload_at_least(b->pm_desc, up.data(), up.size())) return rc;
  // counts[nplanes][256], plane_bytes[8 ntensors] (u64), masks[ntensors]: zeroed by one memset,
  // the last two read back by one copy
  const uint64_t cbytes = 2048ull * nplanes, obytes = (8ull * PLANES_MAX_E + 4ull) * ntensors;
  if (int rc = b->pm_counts.reserve(cbytes + obytes)) return rc;
  if (int rc = b->pm_recs.reserve(sizeof(EBatchCodeRec) * (uint64_t)nplanes)) return rc;
  if (int rc = b->pm_tables.reserve(1024ull * nplanes)) return rc;
  for (Event& e : b->pm_ev)
    if (int rc = e.create()) return rc;
  PMaskParams hp{};
  hp.desc = b->pm_desc.get<PMaskTensor>();
  hp.unit0 = (const uint32_t*)(b->pm_desc.get<uint8_t>() + dbytes);
  hp.counts = b->pm_counts.get<unsigned long long>();
  hp.ntensors = ntensors;
  hp.nunits = unit0[ntensors];
  const uint32_t* d_q0 = hp.unit0 + ntensors + 1;
  unsigned long long* d_pb = (unsigned long long*)(b->pm_counts.get<uint8_t>() + cbytes);
  uint32_t* d_masks = (uint32_t*)(d_pb + (uint64_t)PLANES_MAX_E * ntensors);
  const hipStream_t st = b->q.stream;
  // after what the producer's stream holds now, then the four launches on the batch's stream
  if (int rc = b->q.follow(hip_stream)) return rc;
  GH_HIP(hipMemsetAsync(b->pm_counts.get(), 0, cbytes + obytes, st));
  GH_HIP(hipEventRecord(b->pm_ev[0], st));
  if (hp.nunits) {
    // GH_PLANES_GRID=k (tests): k workgroups, so that one wave walks many units and tensors;
    // else at most the workgroups the LDS keeps resident (five of 32 KiB per CU)
    const uint32_t grid = getenv("GH_PLANES_GRID") ? unit_grid("GH_PLANES_GRID", hp.nunits, PM_WAVES, b->q.num_cu)
                                                   : (uint32_t)std::clamp<uint64_t>(ceil_div(hp.nunits, PM_WAVES), 1,
                                                                                    5ull * (uint64_t)b->q.num_cu);
    const char* em = getenv("GH_PMASK_MERGE");  // (tests, measurements)
    if (em ? atoi(em) != 0 : PMASK_MERGE_DEFAULT)
      hipLaunchKernelGGL(gh_pmask_hist_kernel<true>, dim3(grid), dim3(PM_TB), 0, st, hp);
    else
      hipLaunchKernelGGL(gh_pmask_hist_kernel<false>, dim3(grid), dim3(PM_TB), 0, st, hp);
    GH_HIP(hipGetLastError());
  }
  GH_HIP(hipEventRecord(b->pm_ev[1], st));
  {
    // GH_EBATCH_GRID=k (tests): k workgroups walk all planes
    const uint32_t grid = unit_grid("GH_EBATCH_GRID", nplanes, 1, b->q.num_cu);
    hipLaunchKernelGGL(gh_ebatch_code_kernel, dim3(grid), dim3(EB_TB), 0, st, hp.counts, b->pm_tables.get<uint32_t>(),
                       b->pm_recs.get<EBatchCodeRec>(), nplanes);
    GH_HIP(hipGetLastError());
  }
  GH_HIP(hipEventRecord(b->pm_ev[2], st));
  hipLaunchKernelGGL(gh_pmask_decide_kernel, dim3((nplanes + 255u) / 256u), dim3(256), 0, st,
                     b->pm_recs.get<EBatchCodeRec>(), hp.desc, d_q0, ntensors, nplanes, d_pb, d_masks);
  GH_HIP(hipGetLastError());
  GH_HIP(hipEventRecord(b->pm_ev[3], st));
  // the one read-back: sizes, then masks
  std::vector<uint8_t> back(obytes);
  GH_HIP(hipMemcpyAsync(back.data(), d_pb, obytes, hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  const uint64_t* pb = (const uint64_t*)back.data();
  std::memcpy(masks, back.data() + 8ull * PLANES_MAX_E * ntensors, 4ull * ntensors);
  if (plane_bytes) std::memcpy(plane_bytes, pb, 8ull * PLANES_MAX_E * ntensors);
  if (rep) {
    rep->ntensors = ntensors;
    rep->launches = GH_PMASK_LAUNCHES;
    for (uint32_t t = 0; t < ntensors; ++t) {
      rep->raw_bytes += items[t].nelem * items[t].elem_size;
      rep->coded_planes += (uint32_t)__builtin_popcount(masks[t]);
      for (uint32_t p = 0; p < items[t].elem_size; ++p)
        rep->chosen_bytes += pmask_chosen_bytes(pb[(size_t)PLANES_MAX_E * t + p], items[t].nelem);
    }
    GH_HIP(hipEventElapsedTime(&rep->hist_ms, b->pm_ev[0], b->pm_ev[1]));
    GH_HIP(hipEventElapsedTime(&rep->code_ms, b->pm_ev[1], b->pm_ev[2]));
    GH_HIP(hipEventElapsedTime(&rep->decide_ms, b->pm_ev[2], b->pm_ev[3]));
  }
  b->pm_nplanes = nplanes;
  b->pm_done = true;
  return GH_OK;
}

extern "C" int gh_pmask_counts(gh_ebatch* b, uint32_t plane, uint64_t counts[256]) {
  if (!b || !counts) return fail(GH_E_ARG, "null argument");
  if (!b->pm_done) return fail(GH_E_STATE, "gh_pmask_counts before a gh_pmask_device");
  if (plane >= b->pm_nplanes) return fail(GH_E_ARG, "no such candidate plane");
  GH_HIP(hipSetDevice(b->q.device));
  GH_HIP(hipMemcpy(counts, b->pm_counts.get<uint8_t>() + 2048ull * plane, 2048, hipMemcpyDeviceToHost));
  return GH_OK;
}

static EBatchParams ebatch_params(const gh_ebatch* b) {
  EBatchParams p{};
  p.desc = b->code.get<EBatchDesc>();
  p.tables = (const uint32_t*)(b->code.get<uint8_t>() + sizeof(EBatchDesc) * (uint64_t)b->nstreams);
  p.unit0 = b->unit0.get<uint32_t>();
  p.in = b->in.get<uint8_t>();
  p.counts = b->counts.get<unsigned long long>();
  p.unit_bits = b->unit_bits.get<uint32_t>();
  p.unit_off = b->unit_off.get<unsigned long long>();
  p.payload = b->payload.get<uint32_t>();
  p.gaps = b->gaps.get<uint32_t>();
  p.summary = b->flags.get<unsigned int>();
  p.status = p.summary ? p.summary + 4 : nullptr;
  p.nstreams = b->nstreams;
  p.nunits = (uint32_t)b->inp.nunits;
  return p;
}

// Enqueues every stream's histogram on the batch's stream (ns > 0): counts zeroed, one launch
// between the ev_hist events.
static int ebatch_hist(gh_ebatch* b) {
  const uint32_t ns = b->nstreams;
  const uint64_t nunits = b->inp.nunits;
  if (int rc = b->counts.reserve(2048ull * ns)) return rc;
  GH_HIP(hipMemsetAsync(b->counts.get(), 0, 2048ull * ns, b->q.stream));
  GH_HIP(hipEventRecord(b->ev_hist.a, b->q.stream));
  if (nunits) {
    const EBatchParams p = ebatch_params(b);
    // GH_EBATCH_GRID=k (tests): k workgroups for the per-unit kernels, here and at encode time
    const uint32_t grid = unit_grid("GH_EBATCH_GRID", nunits, EB_WAVES, b->q.num_cu);
    hipLaunchKernelGGL(gh_ebatch_hist_kernel, dim3(grid), dim3(EB_TB), 0, b->q.stream, p);
    GH_HIP(hipGetLastError());
  }
  GH_HIP(hipEventRecord(b->ev_hist.b, b->q.stream));
  return GH_OK;
}

// The output layout from the streams' plans: out_bytes, outp, and the descriptors' plan-time
// half (d: ebatch_descs).
static int ebatch_layout(gh_ebatch* b, std::vector<EBatchDesc>& d) {
  const uint32_t ns = b->nstreams;
  std::vector<uint64_t> w(ns), g(ns);
  b->out_bytes = 0;
  for (uint32_t i = 0; i < ns; ++i) {
    w[i] = b->plans[i].w;
    g[i] = b->plans[i].g;
    b->out_bytes += b->plans[i].file_bytes;
  }
  if (int rc = ebatch_out_plan(w.data(), g.data(), ns, b->outp)) return rc;
  for (uint32_t i = 0; i < ns; ++i) {
    d[i].pay_off = b->outp.ext[i].pay_off;
    d[i].gap_off = b->outp.ext[i].gap_off;
    d[i].bits = b->plans[i].bits;
  }
  return GH_OK;
}

// The arenas and the encode's scratch for the planned batch.
static int ebatch_reserve_out(gh_ebatch* b) {
  const uint64_t nunits = b->inp.nunits;
  if (int rc = b->payload.reserve(std::max<uint64_t>(4 * b->outp.pay_words, 16))) return rc;
  if (int rc = b->gaps.reserve(std::max<uint64_t>(4 * b->outp.gap_words, 16))) return rc;
  if (int rc = b->unit_bits.reserve(std::max<uint64_t>(4 * nunits, 16))) return rc;
  if (int rc = b->unit_off.reserve(8 * (nunits + 1))) return rc;
  return b->flags.reserve(16 + 4ull * b->nstreams);
}

extern "C" int gh_ebatch_plan(gh_ebatch* b, int force_version, int threads) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded) return fail(GH_E_STATE, "gh_ebatch_plan before a load");
  GH_HIP(hipSetDevice(b->q.device));
  if (int rc = b->q.quiesce()) return rc;  // (the tables of the last encode are replaced)
  b->planned = false;
  b->counts_on_device = false;
  const uint32_t ns = b->nstreams;
  // 1. every stream's histogram: one launch, 2. one read-back
  std::vector<uint64_t> counts(256ull * ns, 0);
  b->hist_ms = b->code_ms = 0;
  if (ns) {
    if (int rc = ebatch_hist(b)) return rc;
    GH_HIP(hipMemcpyAsync(counts.data(), b->counts.get(), 2048ull * ns, hipMemcpyDeviceToHost, b->q.stream));
    GH_HIP(hipStreamSynchronize(b->q.stream));
    if (int rc = b->ev_hist.elapsed(&b->hist_ms)) return rc;
  }
  // 3. the host plans, threaded over streams (streams are handed out by a shared counter)
  const auto t0 = std::chrono::steady_clock::now();
  b->plans.assign(ns, gh_encode_plan{});
  int nt = threads > 0 ? threads : (int)std::min(std::max(std::thread::hardware_concurrency(), 1u), 32u);
  nt = (int)std::min<uint64_t>((uint64_t)nt, std::max<uint64_t>(ns / 16, 1));
  std::atomic<uint32_t> next{0};
  std::vector<int> rcs(nt, GH_OK);
  std::vector<std::string> msgs(nt);
  auto work = [&](int t) {
    for (;;) {
      const uint32_t i = next.fetch_add(1);
      if (i >= ns || rcs[t]) return;
      gh_encode_plan& pl = b->plans[i];
      pl.n = b->n[i];
      std::memcpy(pl.count, &counts[256ull * i], sizeof(pl.count));
      int rc = plan_from_counts(&pl, force_version);
      if (!rc)
        for (int v = 0; v < 256; ++v)
          if (pl.len[v] > GH_MAX_CODE_LEN) rc = fail(GH_E_TABLE, "code longer than 16 bits");
      if (rc) {
        rcs[t] = rc;
        msgs[t] = "stream " + std::to_string(i) + ": " + gh_last_error();
      }
    }
  };
  if (nt <= 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
    for (auto& t : th) t.join();
  }
  for (int t = 0; t < nt; ++t)
    if (rcs[t]) return fail(rcs[t], msgs[t]);
  b->plan_host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // 5. the output arenas (before the upload: the descriptors hold their offsets)
  std::vector<EBatchDesc> d = ebatch_descs(b);
  if (int rc = ebatch_layout(b, d)) return rc;
  // 4. one upload: the descriptors, then every stream's 256 left-aligned entries
  if (ns) {
    std::vector<uint8_t> up((sizeof(EBatchDesc) + 1024ull) * ns);
    uint32_t* tab = (uint32_t*)(up.data() + sizeof(EBatchDesc) * (uint64_t)ns);
    for (uint32_t i = 0; i < ns; ++i) {
      const gh_encode_plan& pl = b->plans[i];
      for (int v = 0; v < 256; ++v) {
        const uint32_t l = pl.len[v];
        tab[256ull * i + v] = l ? (pl.code[v] << (32u - l)) | l : 0u;
      }
    }
    std::memcpy(up.data(), d.data(), sizeof(EBatchDesc) * (uint64_t)ns);
    GH_HIP(hipMemcpy(b->code.get(), up.data(), up.size(), hipMemcpyHostToDevice));
  }
  if (int rc = ebatch_reserve_out(b)) return rc;
  b->planned = true;
  return GH_OK;
}

extern "C" int gh_batchenc_plan_device(gh_ebatch* b, int force_version) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded) return fail(GH_E_STATE, "gh_batchenc_plan_device before a load");
  GH_HIP(hipSetDevice(b->q.device));
  if (int rc = b->q.quiesce()) return rc;  // (the tables of the last encode are replaced)
  b->planned = false;
  b->counts_on_device = false;
  const uint32_t ns = b->nstreams;
  // 1. every stream's histogram, 2. every stream's code: its table where the encode kernels
  // read it, its record for the host, 3. one read-back of the records
  std::vector<EBatchCodeRec> recs(ns);
  b->hist_ms = b->code_ms = 0;
  if (ns) {
    if (int rc = b->recs.reserve(sizeof(EBatchCodeRec) * (uint64_t)ns)) return rc;
    if (int rc = ebatch_hist(b)) return rc;
    GH_HIP(hipEventRecord(b->ev_code.a, b->q.stream));
    {
      // GH_EBATCH_GRID=k (tests): k workgroups walk all streams
      const uint32_t grid = unit_grid("GH_EBATCH_GRID", ns, 1, b->q.num_cu);
      const EBatchParams p = ebatch_params(b);
      hipLaunchKernelGGL(gh_ebatch_code_kernel, dim3(grid), dim3(EB_TB), 0, b->q.stream, p.counts,
                         const_cast<uint32_t*>(p.tables), b->recs.get<EBatchCodeRec>(), ns);
      GH_HIP(hipGetLastError());
    }
    GH_HIP(hipEventRecord(b->ev_code.b, b->q.stream));
    GH_HIP(hipMemcpyAsync(recs.data(), b->recs.get(), sizeof(EBatchCodeRec) * (uint64_t)ns, hipMemcpyDeviceToHost,
                          b->q.stream));
    GH_HIP(hipStreamSynchronize(b->q.stream));
    if (int rc = b->ev_hist.elapsed(&b->hist_ms)) return rc;
    if (int rc = b->ev_code.elapsed(&b->code_ms)) return rc;
  }
  // 4. the plans from the records: build_canon is the tripwire for the kernel's code (the
  // scan kernel's GH_ST_LAYOUT is the one for its bit total)
  const auto t0 = std::chrono::steady_clock::now();
  b->plans.resize(ns);  // (every plan is cleared by the thread that fills it)
  const auto plan_one = [&](uint32_t i) -> int {
    const EBatchCodeRec& r = recs[i];
    gh_encode_plan& pl = b->plans[i];
    pl = gh_encode_plan{};
    const auto who = [i] { return "stream " + std::to_string(i) + ": "; };
    if (r.nsyms > GH_MAX_SYMBOLS || (r.nsyms == 0) != (b->n[i] == 0))
      return fail(GH_E_TABLE, who() + "device-built code: bad symbol count");
    pl.n = b->n[i];
    pl.nsyms = r.nsyms;
    std::memcpy(pl.syms, r.syms, sizeof(gh_sym) * r.nsyms);
    Canon c;
    if (build_canon(pl.syms, pl.nsyms, c)) return fail(GH_E_TABLE, who() + "device-built code: " + gh_last_error());
    for (uint32_t k = 0; k < pl.nsyms; ++k) {
      pl.code[c.sym[k]] = c.code[k];
      pl.len[c.sym[k]] = c.len[k];
    }
    pl.bits = r.bits;
    if (int rc = plan_sizes(&pl, force_version)) return fail(rc, who() + gh_last_error());
    return GH_OK;
  };
  {
    // a stream costs about a microsecond (8 KB cleared, build_canon's 256 steps): a thread per
    // 256 streams, each taking a contiguous run; the error message is its thread's own
    const int nt = (int)std::min<uint64_t>(std::min(std::max(std::thread::hardware_concurrency(), 1u), 32u),
                                           std::max<uint64_t>(ns / 256, 1));
    std::vector<int> rcs(nt, GH_OK);
    std::vector<std::string> msgs(nt);
    const auto work = [&](int t) {
      const uint32_t i1 = (uint32_t)((uint64_t)ns * (t + 1) / nt);
      for (uint32_t i = (uint32_t)((uint64_t)ns * t / nt); i < i1 && !rcs[t]; ++i)
        if (int rc = plan_one(i)) {
          rcs[t] = rc;
          msgs[t] = gh_last_error();
        }
    };
    if (nt <= 1) {
      work(0);
    } else {
      std::vector<std::thread> th;
      for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
      for (auto& t : th) t.join();
    }
    for (int t = 0; t < nt; ++t)
      if (rcs[t]) return fail(rcs[t], msgs[t]);
  }
  b->plan_host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // 5. the output arenas, 6. one upload: the descriptors (the tables are on the device)
  std::vector<EBatchDesc> d = ebatch_descs(b);
  if (int rc = ebatch_layout(b, d)) return rc;
  if (ns) GH_HIP(hipMemcpy(b->code.get(), d.data(), sizeof(EBatchDesc) * (uint64_t)ns, hipMemcpyHostToDevice));
  if (int rc = ebatch_reserve_out(b)) return rc;
  b->counts_on_device = ns != 0;
  b->planned = true;
  return GH_OK;
}

extern "C" int gh_batchenc_plan_times(gh_ebatch* b, float* hist_ms, float* code_ms, float* host_ms) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->planned) return fail(GH_E_STATE, "gh_batchenc_plan_times before a plan");
  if (hist_ms) *hist_ms = b->hist_ms;
  if (code_ms) *code_ms = b->code_ms;
  if (host_ms) *host_ms = b->plan_host_ms;
  return GH_OK;
}

extern "C" int gh_ebatch_plan_of(gh_ebatch* b, uint32_t stream, gh_encode_plan* out) {
  if (!b || !out) return fail(GH_E_ARG, "null argument");
  if (!b->planned) return fail(GH_E_STATE, "gh_ebatch_plan_of before a plan");
  if (stream >= b->nstreams) return fail(GH_E_ARG, "no such stream in the batch");
  if (b->counts_on_device) {
    // a device plan leaves the histograms where the code kernel read them: all of them back once
    GH_HIP(hipSetDevice(b->q.device));
    std::vector<uint64_t> counts(256ull * b->nstreams);
    GH_HIP(hipMemcpy(counts.data(), b->counts.get(), 2048ull * b->nstreams, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < b->nstreams; ++i) std::memcpy(b->plans[i].count, &counts[256ull * i], sizeof(b->plans[i].count));
    b->counts_on_device = false;
  }
  *out = b->plans[stream];
  return GH_OK;
}

extern "C" int gh_ebatch_encode(gh_ebatch* b, void* hip_stream, int timed) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->planned) return fail(GH_E_STATE, "gh_ebatch_encode before a plan");
  GH_HIP(hipSetDevice(b->q.device));
  const EBatchParams p = ebatch_params(b);
  // encodes of one batch share its scratch and its arenas: they run in the order they were made
  hipStream_t st;
  if (int rc = b->q.begin(hip_stream, timed != 0, &st)) return rc;
  // (no memset of the flags: the scan kernel writes every status word and the summary)
  if (b->outp.pay_words) GH_HIP(hipMemsetAsync(b->payload.get(), 0, 4 * b->outp.pay_words, st));
  if (b->outp.gap_words) GH_HIP(hipMemsetAsync(b->gaps.get(), 0, 4 * b->outp.gap_words, st));
  if (b->nstreams) {
    const uint32_t grid = unit_grid("GH_EBATCH_GRID", p.nunits, EB_WAVES, b->q.num_cu);
    if (p.nunits) hipLaunchKernelGGL(gh_ebatch_bits_kernel, dim3(grid), dim3(EB_TB), 0, st, p);
    hipLaunchKernelGGL(gh_ebatch_scan_kernel, dim3(1), dim3(EB_SCAN_TB), 0, st, p);
    if (p.nunits) hipLaunchKernelGGL(gh_ebatch_write_kernel, dim3(grid), dim3(EB_TB), 0, st, p);
    GH_HIP(hipGetLastError());
  }
  return b->q.end(st);
}

extern "C" int gh_ebatch_wait(gh_ebatch* b, gh_ebatch_report* rep) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (rep) *rep = gh_ebatch_report{};
  if (!b->planned || !b->q.enqueued) return fail(GH_E_STATE, "gh_ebatch_wait without an encode since the plan");
  GH_HIP(hipSetDevice(b->q.device));
  float ms = 0;
  if (int rc = b->q.wait(&ms)) return rc;
  unsigned int sum[2] = {0, 0};
  if (b->nstreams) GH_HIP(hipMemcpy(sum, b->flags.get(), sizeof(sum), hipMemcpyDeviceToHost));
  if (rep) {
    rep->in_bytes = b->inp.sum_n;
    rep->out_bytes = b->out_bytes;
    rep->nstreams = b->nstreams;
    rep->status = sum[1];
    rep->hist_ms = b->hist_ms;
    rep->plan_host_ms = b->plan_host_ms;
    rep->kernel_ms = ms;
    rep->launches = EBATCH_LAUNCHES;
  }
  if (sum[0])
    return fail(GH_E_HIP, std::to_string(sum[0]) + " stream(s) of the batch: device bit total differs from the plan's");
  return GH_OK;
}

extern "C" int gh_ebatch_sizes(gh_ebatch* b, uint64_t* file_bytes, uint32_t cap) {
  if (!b || (cap && !file_bytes)) return fail(GH_E_ARG, "null argument");
  if (!b->planned) return fail(GH_E_STATE, "gh_ebatch_sizes before a plan");
  if (cap < b->nstreams) return fail(GH_E_SMALL, "size array smaller than the batch");
  for (uint32_t i = 0; i < b->nstreams; ++i) file_bytes[i] = b->plans[i].file_bytes;
  return GH_OK;
}

extern "C" int gh_ebatch_download(gh_ebatch* b, uint32_t stream, void* out, uint64_t out_len) {
  if (!b || !out) return fail(GH_E_ARG, "null argument");
  if (!b->planned || !b->q.enqueued) return fail(GH_E_STATE, "gh_ebatch_download before an encode");
  if (stream >= b->nstreams) return fail(GH_E_ARG, "no such stream in the batch");
  const gh_encode_plan& pl = b->plans[stream];
  if (out_len < pl.file_bytes) return fail(GH_E_SMALL, "output buffer too small");
  GH_HIP(hipSetDevice(b->q.device));
  GH_HIP(hipEventSynchronize(b->q.done));
  uint8_t* o = (uint8_t*)out;
  const size_t hdr = encode_header(&pl, o);
  const uint64_t GW = ceil_div(pl.g, GH_GAPS_PER_WORD);
  const EBatchOutExtent& e = b->outp.ext[stream];
  if (GW) GH_HIP(hipMemcpy(o + hdr, b->gaps.get<uint32_t>() + e.gap_off, 4 * GW, hipMemcpyDeviceToHost));
  if (pl.w) GH_HIP(hipMemcpy(o + hdr + 4 * GW, b->payload.get<uint32_t>() + e.pay_off, 4 * pl.w, hipMemcpyDeviceToHost));
  return GH_OK;
}

extern "C" int gh_ebatch_items(gh_ebatch* b, gh_batch_item* items, uint32_t cap) {
  if (!b || (cap && !items)) return fail(GH_E_ARG, "null argument");
  if (!b->planned) return fail(GH_E_STATE, "gh_ebatch_items before a plan");
  if (cap < b->nstreams) return fail(GH_E_SMALL, "item array smaller than the batch");
  for (uint32_t i = 0; i < b->nstreams; ++i) {
    const gh_encode_plan& pl = b->plans[i];
    const EBatchOutExtent& e = b->outp.ext[i];
    items[i] = gh_batch_item{pl.syms, pl.nsyms, pl.n, pl.w, pl.g, b->payload.get<uint32_t>() + e.pay_off,
                             b->gaps.get<uint32_t>() + e.gap_off};
  }
  return GH_OK;
}

extern "C" int gh_ebatch_kernel_shape(gh_ebatch* b, char* buf, size_t cap) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->planned) return fail(GH_E_STATE, "gh_ebatch_kernel_shape before a plan");
  return copy_name(b->inp.nunits ? EBATCH_SHAPE : "", buf, cap);
}

extern "C" int gh_ebatch_kernel_shapes(char* buf, size_t cap) { return copy_name(std::string(EBATCH_SHAPE) + "\n", buf, cap); }
