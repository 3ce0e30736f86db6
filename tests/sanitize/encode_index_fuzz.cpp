// encode_index_fuzz — the host encoder's seek index under AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_encode_index_sanitize.py (CPU, no GPU
// calls).  gh_encode_index gets random inputs (0 bytes to a few hundred KiB, now and then
// a few MiB so that the thread count really splits the input; flat histograms over a
// random alphabet, skewed geometric ones with codewords up to 16 bits, one-symbol inputs),
// random strides and random thread counts.  The input lives in a heap block of exactly
// its length and the image in a heap block of exactly gh_index_bytes bytes, at an even or
// an odd address, so any read or write past either and any misaligned store is reported.
// Every image is parsed back and checked against a brute-force walk over the code lengths.
// Usage: encode_index_fuzz [iterations] [seed]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gaphuff.h"

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

#define FAIL(...)                                \
  do {                                           \
    std::fprintf(stderr, "encode_index_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);           \
    std::fprintf(stderr, "\n");                  \
    return 1;                                    \
  } while (0)

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 300;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  unsigned long long entries_seen = 0;
  gh_encode_plan* plan = new gh_encode_plan;
  for (long it = 0; it < iters; ++it) {
    // the input
    uint64_t n;
    switch (rng() % 8) {
      case 0: n = rng() % 20; break;
      case 1: n = it % 40 == 1 ? (2u << 20) + rng() % (2u << 20) : rng() % 5000; break;
      default: n = rng() % (400u << 10);
    }
    uint8_t* in = (uint8_t*)std::malloc(n ? n : 1);
    const int kind = (int)(rng() % 3);
    if (kind == 0) {  // flat over a random alphabet
      const uint32_t a = 1 + (uint32_t)(rng() % 256), base = (uint32_t)(rng() % 256);
      for (uint64_t i = 0; i < n; ++i) in[i] = (uint8_t)(base + rng() % a);
    } else if (kind == 1) {  // skewed: geometric, long codewords
      std::geometric_distribution<int> geo(0.3 + 0.4 * (double)(rng() % 100) / 100.0);
      for (uint64_t i = 0; i < n; ++i) in[i] = (uint8_t)std::min(geo(rng), 255);
    } else {  // one symbol, with a few others
      std::memset(in, (int)(rng() % 256), n);
      for (uint64_t j = 0, m = rng() % 4; j < m && n; ++j) in[rng() % n] = (uint8_t)rng();
    }
    if (gh_encode_plan_make(in, n, 1 + (int)(rng() % 4), rng() % 4 == 0 ? 2 : 0, plan) != GH_OK)
      FAIL("plan: %s", gh_last_error());
    // mostly small strides (many entries per input), sometimes any the format allows
    const uint32_t k = GH_INDEX_MIN_LOG2 +
                       (uint32_t)(rng() % (rng() % 3 ? 3 : GH_INDEX_MAX_LOG2 - GH_INDEX_MIN_LOG2 + 1));
    const int threads = 1 + (int)(rng() % 9);
    const uint64_t bytes = gh_index_bytes(plan->g, k);
    if (bytes < 48) FAIL("gh_index_bytes returned %llu", (unsigned long long)bytes);
    // the image: a block of exactly `bytes` bytes, at an even or an odd address
    const size_t odd = (size_t)(it & 1);
    uint8_t* heap = (uint8_t*)std::malloc(bytes + odd);
    uint8_t* img = heap + odd;
    std::memset(img, 0xA5, bytes);
    if (gh_encode_index(in, plan, k, threads, img, bytes) != GH_OK) FAIL("refused: %s", gh_last_error());
    gh_index ix;
    if (gh_index_parse(img, bytes, &ix) != GH_OK) FAIL("the image does not parse: %s", gh_last_error());
    if (ix.log2_stride != k || ix.n != n || ix.g != plan->g) FAIL("header fields differ from the plan");
    // the brute-force walk: offsets[b] = the number of i with start(i) < S * b
    const uint64_t S = (uint64_t)GH_SEGMENT_BITS << k, nblocks = ix.nentries - 1;
    std::vector<uint64_t> want(nblocks + 1, 0);
    {
      uint64_t pos = 0, b = 0;
      for (uint64_t i = 0; i < n; ++i) {
        while (b < nblocks && pos >= S * b) want[b++] = i;
        pos += plan->len[in[i]];
      }
      while (b < nblocks && S * b < pos) want[b++] = n;  // boundaries inside the last codeword
      if (b != nblocks || pos != plan->bits) FAIL("the walk found %llu of %llu blocks", (unsigned long long)b, (unsigned long long)nblocks);
      want[nblocks] = n;
    }
    for (uint64_t b = 0; b <= nblocks; ++b) {
      uint64_t got;
      std::memcpy(&got, (const uint8_t*)ix.offsets + 8 * b, 8);
      if (got != want[b])
        FAIL("n = %llu, stride 2^%u, %d threads: entry %llu is %llu, the walk gives %llu", (unsigned long long)n, k,
             threads, (unsigned long long)b, (unsigned long long)got, (unsigned long long)want[b]);
    }
    entries_seen += nblocks + 1;
    // another thread count: the same bytes
    {
      uint8_t* again = (uint8_t*)std::malloc(bytes);
      if (gh_encode_index(in, plan, k, 1 + (int)(rng() % 9), again, bytes) != GH_OK || std::memcmp(again, img, bytes))
        FAIL("the image depends on the thread count");
      std::free(again);
    }
    // refusals: nothing may be written past a short buffer
    {
      uint8_t* sm = (uint8_t*)std::malloc(bytes - 1);
      if (gh_encode_index(in, plan, k, threads, sm, bytes - 1) != GH_E_SMALL) FAIL("a short buffer was not GH_E_SMALL");
      std::free(sm);
      if (gh_encode_index(in, plan, GH_INDEX_MIN_LOG2 - 1, threads, img, bytes) != GH_E_ARG ||
          gh_encode_index(in, plan, GH_INDEX_MAX_LOG2 + 1, threads, img, bytes) != GH_E_ARG)
        FAIL("a bad stride was accepted");
      if (gh_encode_index(in, nullptr, k, threads, img, bytes) != GH_E_ARG ||
          gh_encode_index(in, plan, k, threads, nullptr, bytes) != GH_E_ARG)
        FAIL("a null pointer was accepted");
      // an input of another bit total (when the code has two lengths to tell apart)
      if (n && plan->nsyms > 1) {
        const uint8_t a = plan->syms[0].symbol, z = plan->syms[plan->nsyms - 1].symbol;
        const uint64_t at = rng() % n;
        const uint8_t keep = in[at];
        in[at] = keep == a ? z : a;
        if (plan->len[in[at]] != plan->len[keep] && gh_encode_index(in, plan, k, threads, img, bytes) != GH_E_ARG)
          FAIL("an input that does not match the plan was accepted");
        in[at] = keep;
      }
    }
    std::free(heap);
    std::free(in);
  }
  delete plan;
  std::printf("encode_index_fuzz: %ld iterations ok (%llu entries)\n", iters, entries_seen);
  return 0;
}
