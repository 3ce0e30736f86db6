// Internal helpers shared by the host library (gh_core.cpp) and the HIP decoder
// (gh_decode.hip).  The host-only HIP helpers (the GH_HIP error macro and the owners of
// device memory, streams and events) are in gh_hip.hpp.  Not part of the C ABI.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gaphuff.h"

namespace gh {

// Thread-local last-error message behind gh_last_error().
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

// Canonical code of a stream's (symbol,length) list in file order, restating the
// code assignment shared by the encoder (package_merge.cpp:168-181) and the
// decoder's table builder (get_table.cpp:70-83): code starts at 0 for the first
// (most frequent) entry and steps as code = (code+1) << (len[i+1]-len[i]).
struct Canon {
  uint32_t nsyms = 0;
  uint32_t minlen = 0, maxlen = 0;
  uint8_t sym[GH_MAX_SYMBOLS] = {};     // file order
  uint8_t len[GH_MAX_SYMBOLS] = {};
  uint32_t code[GH_MAX_SYMBOLS] = {};   // right-aligned code value
  // Per-length canonical ranges on a 16-bit left-aligned scale.
  uint32_t count[GH_MAX_CODE_LEN + 2] = {};
  uint32_t base16[GH_MAX_CODE_LEN + 2] = {};   // first code of length l << (16-l)
  uint32_t limit16[GH_MAX_CODE_LEN + 2] = {};  // base16[l] + count[l] << (16-l)
  uint32_t first[GH_MAX_CODE_LEN + 2] = {};    // file index of first length-l code
};

// Builds `c` from a stream's symbol list; returns GH_OK or GH_E_TABLE.
int build_canon(const gh_sym* syms, uint32_t nsyms, Canon& c);

// Decode one codeword from the top bits of `w16` (16 bits, left-aligned).
// Returns the length (1..16) and the file index, or 0 when the bits fall outside
// the code space.
inline uint32_t canon_decode16(const Canon& c, uint32_t w16, uint32_t* index) {
  for (uint32_t l = c.minlen; l <= c.maxlen; ++l) {
    if (c.count[l] == 0) continue;
    if (w16 < c.limit16[l]) {
      *index = c.first[l] + ((w16 - c.base16[l]) >> (16 - l));
      return l;
    }
  }
  return 0;
}

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Copies s and its terminating NUL into buf[0..cap): the kernel-name queries of the
// decoder and the encoder.
inline int copy_name(const std::string& s, char* buf, size_t cap) {
  if (!buf) return fail(GH_E_ARG, "null argument");
  if (s.size() + 1 > cap) return fail(GH_E_SMALL, "name buffer too small");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return GH_OK;
}

// Host plan of a batched decode (gaphuff.h, "batched decode"): where every stream's words,
// gap words, work units and output bytes lie.  Host arithmetic only (gh_core.cpp), shared
// by gh_batch_load / gh_batch_load_device (gh_decode.hip) and tests/sanitize/batch_fuzz.cpp.
constexpr uint32_t BATCH_UNIT_SEGS = 256;              // segments per work unit (one wave block)
constexpr uint32_t BATCH_MAX_STREAMS = 1u << 24;
constexpr uint64_t BATCH_MAX_G = (1ull << 32) - 256;   // per-stream segments, exclusive
constexpr uint64_t BATCH_MAX_UNITS = 1ull << 31;       // work units of a batch, exclusive
struct BatchExtent {
  uint64_t pay_off;    // first payload word in the payload arena (a multiple of 4: 16 bytes)
  uint64_t pay_words;  // words the stream owns there: 4 G + 4 (0 when G = 0), W copied, the rest zero
  uint64_t gap_off;    // first gap word in the gap arena
  uint64_t gap_words;  // ceil(G / 8)
  uint64_t unit0;      // first work unit; the stream has ceil(G / 256) of them
  uint64_t out_off;    // first output byte (gh_batch_layout)
};
struct BatchPlan {
  std::vector<BatchExtent> ext;  // nstreams entries
  uint64_t pay_words = 0, gap_words = 0, nunits = 0, out_bytes = 0;  // arena sizes, units, output arena
};
// GH_E_ARG beyond the limits above, on W outside [4G - 3, 4G] (W = 0 when G = 0) and on
// sums that overflow; the message names the stream's index.
int batch_plan(const uint64_t* n, const uint64_t* w, const uint64_t* g, uint32_t nstreams, BatchPlan& out);

// Host layout of a batched encode (gaphuff.h, "batched encode").  Host arithmetic only
// (gh_core.cpp), shared by gh_ebatch_load / gh_ebatch_load_device / gh_ebatch_plan
// (gh_encode.hip) and tests/sanitize/ebatch_fuzz.cpp.
constexpr uint32_t EBATCH_UNIT_BYTES = GH_EBATCH_UNIT_BYTES;  // input bytes per work unit (one wave)
constexpr uint32_t EBATCH_TAIL_BYTES = 32;                    // bytes a unit's last word can need past it
constexpr uint32_t EBATCH_MAX_STREAMS = 1u << 24;
constexpr uint64_t EBATCH_MAX_UNITS = 1ull << 31;             // work units of a batch, exclusive
struct EBatchInExtent {
  uint64_t in_off;    // first input byte in the input arena (a multiple of 16)
  uint64_t in_bytes;  // bytes the stream owns there: whole units + the tail (0 when n = 0), zero past n
  uint64_t unit0;     // first work unit; the stream has ceil(n / 1024) of them
};
struct EBatchInPlan {
  std::vector<EBatchInExtent> ext;  // nstreams entries
  uint64_t in_bytes = 0, nunits = 0, sum_n = 0;
};
struct EBatchOutExtent {
  uint64_t pay_off, pay_words;  // first payload word in the payload arena (a multiple of 4); round_up(W, 4)
  uint64_t gap_off, gap_words;  // first gap word in the gap arena (a multiple of 4); round_up(ceil(G / 8), 4)
};
struct EBatchOutPlan {
  std::vector<EBatchOutExtent> ext;
  uint64_t pay_words = 0, gap_words = 0;  // arena sizes
};
// GH_E_ARG beyond the limits above and on sums that overflow; the message names the stream.
int ebatch_in_plan(const uint64_t* n, uint32_t nstreams, EBatchInPlan& out);
// w[i] payload words and g[i] segments of stream i (G = ceil(W / 4), as every encode plan
// gives: GH_E_ARG otherwise).
int ebatch_out_plan(const uint64_t* w, const uint64_t* g, uint32_t nstreams, EBatchOutPlan& out);

// The tensors of an element gather as its kernels see them (gaphuff.h, "element gather"): by
// gh_planes_layout, with data null and off[p] a stored plane's stored_off (0 for a coded plane).
// Host arithmetic only (gh_core.cpp), shared by gh_pgather_plan and gh_pgather_device.
// GH_E_ARG as gh_planes_layout, and for a tensor of 2^40 bytes or more; *max_coded: the largest
// number of coded planes of a tensor.
struct PlanesTensor;
int pgather_descs(const gh_planes_item* items, uint32_t ntensors, std::vector<PlanesTensor>& desc,
                  uint32_t* nstreams, uint64_t* stored_bytes, uint32_t* max_coded);

// Encoder plan from plan->n and plan->count[] (symbol order, package-merge lengths,
// canonical codes, sizes, header version); shared by the host and GPU encoders.
int plan_from_counts(gh_encode_plan* plan, int force_version);
// Its last step, also gh_batchenc_plan_device's: w, g, version and file_bytes from plan->n,
// plan->nsyms and plan->bits.  GH_E_ARG when force_version = 1 cannot hold the sizes.
int plan_sizes(gh_encode_plan* plan, int force_version);
// Writes the image header; returns its size.  out must hold file_bytes - payload.
size_t encode_header(const gh_encode_plan* plan, uint8_t* out);
// Writes a seek index image's header (40 bytes, any alignment); returns its size.
size_t index_header(uint32_t log2_stride, uint64_t n, uint64_t g, uint64_t nentries, uint8_t* out);

// Host memory <-> device memory through the device's pinned staging buffers
// (gh_io.cpp): each 32 MiB chunk is copied to / from a pinned buffer by a few host
// threads while the DMA of the previous chunk runs (hipMemcpyAsync), so shards on
// different devices, loaded from different host threads, move concurrently.
int h2d_staged(int device, const void* src, uint64_t n, void* dst);
int d2h_staged(int device, const void* src, uint64_t n, void* dst);
// Large copies go through the staging unless GH_H2D=pageable (measurements).
bool use_staged(uint64_t n);

}  // namespace gh
