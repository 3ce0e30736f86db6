// batch_fuzz — the batched decode's host plan under AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_batch_sanitize.py (CPU, no GPU calls).
// gh::batch_plan and gh_batch_layout plan random batches: empty streams, streams at the
// work-unit edges G = 255, 256 and 257, W anywhere in [4G - 3, 4G], sizes in heap blocks of
// exactly nstreams entries.  Every extent is checked against a naive recomputation, every
// padded extent against its neighbours (no overlap, the alignment the kernels load with, the
// words a wave block reads inside the extent), and the limits against their refusals.
// Usage: batch_fuzz [iterations] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gaphuff.h"
#include "gh_internal.hpp"

// gh_io.cpp's file entry points call into the device context (csrc/gh_decode.hip),
// which this host-only build does not link: stand-ins that fail like a box with no GPU.
extern "C" {
int gh_ctx_output(gh_ctx*, void**, uint64_t*) { return GH_E_NODEV; }
int gh_ctx_device(gh_ctx*, int*) { return GH_E_NODEV; }
int gh_ctx_report(gh_ctx*, void*, gh_report*) { return GH_E_NODEV; }
int gh_ctx_load_device(gh_ctx*, const gh_stream*, uint64_t, uint64_t, const uint32_t*, uint64_t,
                       const uint32_t*, uint64_t) {
  return GH_E_NODEV;
}
}

#define FAIL(...)                         \
  do {                                    \
    std::fprintf(stderr, "batch_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);    \
    std::fprintf(stderr, "\n");           \
    return 1;                             \
  } while (0)

static uint64_t* heap_copy(const std::vector<uint64_t>& v) {
  uint64_t* p = (uint64_t*)std::malloc(v.size() ? v.size() * 8 : 1);
  if (!v.empty()) std::memcpy(p, v.data(), v.size() * 8);
  return p;
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  unsigned long long streams_seen = 0;
  for (long it = 0; it < iters; ++it) {
    const uint32_t ns = (uint32_t)(rng() % 40);
    std::vector<uint64_t> n(ns), w(ns), g(ns);
    for (uint32_t i = 0; i < ns; ++i) {
      switch (rng() % 6) {
        case 0: g[i] = 0; break;                      // the empty stream
        case 1: g[i] = 255 + rng() % 3; break;        // the unit edge
        case 2: g[i] = 256 * (1 + rng() % 8) + rng() % 3 - 1; break;
        case 3: g[i] = 1 + rng() % 8; break;
        default: g[i] = 1 + rng() % 5000;
      }
      w[i] = g[i] ? 4 * g[i] - rng() % 4 : 0;
      n[i] = g[i] ? rng() % (16 * g[i] * 8 + 1) : 0;  // (at most 128 one-bit codewords per segment)
    }
    uint64_t *hn = heap_copy(n), *hw = heap_copy(w), *hg = heap_copy(g);
    gh::BatchPlan p;
    if (gh::batch_plan(hn, hw, hg, ns, p) != GH_OK) FAIL("a valid batch was refused: %s", gh_last_error());
    uint64_t* off = (uint64_t*)std::malloc((ns + 1) * 8);
    if (gh_batch_layout(hn, ns, off) != GH_OK) FAIL("gh_batch_layout refused a valid batch");
    if (p.ext.size() != ns) FAIL("extent count");
    uint64_t pay = 0, gap = 0, units = 0, bytes = 0;
    for (uint32_t i = 0; i < ns; ++i) {
      const gh::BatchExtent& e = p.ext[i];
      // the naive recomputation
      const uint64_t want_pay = g[i] ? 4 * g[i] + 4 : 0, want_gap = (g[i] + 7) / 8;
      if (e.pay_off != pay || e.pay_words != want_pay) FAIL("stream %u: payload extent", i);
      if (e.gap_off != gap || e.gap_words != want_gap) FAIL("stream %u: gap extent", i);
      if (e.unit0 != units || e.out_off != bytes || off[i] != bytes) FAIL("stream %u: unit or output offset", i);
      // 16-byte aligned payload and output; W words and the zero padding inside the extent;
      // the last segment's four words and the look-ahead word inside it too
      if (e.pay_off % 4 || e.out_off % 16) FAIL("stream %u: alignment", i);
      if (w[i] > e.pay_words || (g[i] && 4 * (g[i] - 1) + 5 > e.pay_words)) FAIL("stream %u: words outside the extent", i);
      if (g[i] && (g[i] - 1) / 8 >= e.gap_words) FAIL("stream %u: gap nibble outside the extent", i);
      // no overlap: the next extent starts where this one ends (checked by the running sums)
      pay += want_pay;
      gap += want_gap;
      units += (g[i] + 255) / 256;
      bytes += (n[i] + 15) / 16 * 16;
      if (bytes - e.out_off < n[i]) FAIL("stream %u: output extent shorter than N", i);
    }
    if (p.pay_words != pay || p.gap_words != gap || p.nunits != units || p.out_bytes != bytes || off[ns] != bytes)
      FAIL("arena totals");
    // refusals: W outside [4G - 3, 4G], G at the limit, the unit total, an output overflow
    if (ns) {
      const uint32_t k = (uint32_t)(rng() % ns);
      gh::BatchPlan q;
      const uint64_t keep_w = hw[k], keep_g = hg[k], keep_n = hn[k];
      hw[k] = hg[k] ? 4 * hg[k] + 1 : 1;
      if (gh::batch_plan(hn, hw, hg, ns, q) != GH_E_ARG) FAIL("W > 4G was accepted");
      if (keep_g > 1) {
        hw[k] = 4 * keep_g - 4;
        if (gh::batch_plan(hn, hw, hg, ns, q) != GH_E_ARG) FAIL("W < 4G - 3 was accepted");
      }
      hg[k] = gh::BATCH_MAX_G;
      hw[k] = 4 * hg[k];
      if (gh::batch_plan(hn, hw, hg, ns, q) != GH_E_ARG) FAIL("G = 2^32 - 256 was accepted");
      hg[k] = gh::BATCH_MAX_G - 1;  // fine on its own: 2^24 - 1 units
      hw[k] = 4 * hg[k];
      if (gh::batch_plan(hn, hw, hg, ns, q) != GH_OK) FAIL("G = 2^32 - 257 was refused");
      hg[k] = keep_g;
      hw[k] = keep_w;
      hn[k] = ~0ull - rng() % 15;
      if (gh::batch_plan(hn, hw, hg, ns, q) != GH_E_ARG) FAIL("an output overflow was accepted (plan)");
      if (gh_batch_layout(hn, ns, off) != GH_E_ARG) FAIL("an output overflow was accepted (layout)");
      hn[k] = keep_n;
    }
    if (it % 2000 == 0) {  // 2^31 units: 128 streams of 2^24 units each
      std::vector<uint64_t> bn(128, 0), bg(128, (1ull << 32) - 512), bw(128);  // 2^24 - 2 units each ...
      for (size_t i = 0; i < bg.size(); ++i) bw[i] = 4 * bg[i];
      gh::BatchPlan q;
      if (gh::batch_plan(bn.data(), bw.data(), bg.data(), 128, q) != GH_OK) FAIL("2^31 - 256 units were refused");
      bn.resize(129, 0);
      bg.resize(129, 256 * 256);  // ... and 256 more: exactly 2^31
      bw.resize(129, 4 * 256 * 256);
      if (gh::batch_plan(bn.data(), bw.data(), bg.data(), 129, q) != GH_E_ARG) FAIL("2^31 units were accepted");
      if (gh::batch_plan(nullptr, nullptr, nullptr, 1, q) != GH_E_ARG) FAIL("null arrays were accepted");
      if (gh::batch_plan(nullptr, nullptr, nullptr, 0, q) != GH_OK || q.nunits || q.out_bytes) FAIL("the empty batch");
      uint64_t one = 0;
      if (gh_batch_layout(nullptr, 1, &one) != GH_E_ARG || gh_batch_layout(&one, 1, nullptr) != GH_E_ARG)
        FAIL("gh_batch_layout accepted a null pointer");
      if (gh_batch_layout(nullptr, 0, &one) != GH_OK || one != 0) FAIL("gh_batch_layout of no streams");
    }
    streams_seen += ns;
    std::free(hn);
    std::free(hw);
    std::free(hg);
    std::free(off);
  }
  std::printf("batch_fuzz: %ld iterations ok (%llu streams)\n", iters, streams_seen);
  return 0;
}
