// encode_slices_fuzz — the host's sliced encode under AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_encode_slices_sanitize.py (CPU, no GPU
// calls).  Each iteration takes a random input (0 bytes to a few hundred KiB, now and then
// a few MiB so that the thread count really splits a slice; flat histograms over a random
// alphabet, skewed geometric ones with codewords up to 16 bits, one-symbol inputs), cuts it
// at random points (repeated points: empty slices), plans the stream from the slices'
// summed histograms, encodes every slice with a random thread count into heap blocks of
// exactly the reported extents, and merges them, in a shuffled order, into an image of
// exactly file_bytes bytes at an even or an odd address (and an odd symbol count already
// leaves the word area unaligned).  The image must equal gh_encode_write's.
// Usage: encode_slices_fuzz [iterations] [seed]
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

#define FAIL(...)                                 \
  do {                                            \
    std::fprintf(stderr, "encode_slices_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);            \
    std::fprintf(stderr, "\n");                   \
    return 1;                                     \
  } while (0)

struct Part {
  gh_slice s;
  uint32_t* words;
  uint32_t* gapw;
};

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 300;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  unsigned long long slices_seen = 0;
  gh_encode_plan* plan = new gh_encode_plan;
  gh_encode_plan* whole = new gh_encode_plan;
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
    // the cuts: K slices, some of them empty, sometimes clustered (seams inside one word)
    const uint32_t K = 1 + (uint32_t)(rng() % (rng() % 4 ? 6 : 40));
    std::vector<uint64_t> cut(K + 1, 0);
    cut[K] = n;
    const uint64_t near = rng() % (n + 1);
    for (uint32_t i = 1; i < K; ++i) cut[i] = rng() % 3 ? rng() % (n + 1) : std::min<uint64_t>(n, near + rng() % 8);
    std::sort(cut.begin(), cut.end());
    // the stream's plan from the slices' histograms, summed
    uint64_t sum[256] = {};
    for (uint32_t i = 0; i < K; ++i)
      for (uint64_t j = cut[i]; j < cut[i + 1]; ++j) sum[in[j]]++;
    const int force = rng() % 4 == 0 ? 2 : 0;
    if (gh_encode_plan_from_counts(sum, force, plan) != GH_OK) FAIL("plan from counts: %s", gh_last_error());
    if (gh_encode_plan_make(in, n, 1 + (int)(rng() % 4), force, whole) != GH_OK) FAIL("plan: %s", gh_last_error());
    if (std::memcmp(plan, whole, sizeof(*plan))) FAIL("the plan from counts differs from gh_encode_plan_make's");
    if (plan->file_bytes > gh_encode_bound(n)) FAIL("file_bytes above gh_encode_bound");
    // every slice into blocks of exactly its extents
    std::vector<Part> parts(K);
    uint64_t base = 0;
    for (uint32_t i = 0; i < K; ++i) {
      const uint8_t* p = in + cut[i];
      const uint64_t m = cut[i + 1] - cut[i];
      Part& pt = parts[i];
      const int threads = 1 + (int)(rng() % 5);
      const int rc0 = gh_encode_slice(p, m, plan, base, threads, nullptr, 0, nullptr, 0, &pt.s);
      if (rc0 != (pt.s.nwords || pt.s.ngapw ? GH_E_SMALL : GH_OK)) FAIL("sizing call returned %d: %s", rc0, gh_last_error());
      gh_slice want;
      if (gh_slice_extent(base, pt.s.bits, &want) != GH_OK || std::memcmp(&want, &pt.s, sizeof(want)))
        FAIL("extents differ from gh_slice_extent's");
      pt.words = pt.s.nwords ? (uint32_t*)std::malloc(4 * pt.s.nwords) : nullptr;
      pt.gapw = pt.s.ngapw ? (uint32_t*)std::malloc(4 * pt.s.ngapw) : nullptr;
      if (pt.words) std::memset(pt.words, 0xA5, 4 * pt.s.nwords);
      if (pt.gapw) std::memset(pt.gapw, 0xA5, 4 * pt.s.ngapw);
      gh_slice again;
      if (gh_encode_slice(p, m, plan, base, threads, pt.words, pt.s.nwords, pt.gapw, pt.s.ngapw, &again) != GH_OK)
        FAIL("slice %u refused: %s", i, gh_last_error());
      if (std::memcmp(&again, &pt.s, sizeof(again))) FAIL("the extents changed between calls");
      // a cap one short: refused, nothing written past it
      if (pt.s.nwords > 1) {
        uint32_t* sm = (uint32_t*)std::malloc(4 * (pt.s.nwords - 1));
        if (gh_encode_slice(p, m, plan, base, threads, sm, pt.s.nwords - 1, pt.gapw, pt.s.ngapw, &again) != GH_E_SMALL)
          FAIL("a short words buffer was not GH_E_SMALL");
        std::free(sm);
      }
      base += pt.s.bits;
      ++slices_seen;
    }
    if (base != plan->bits) FAIL("the slices hold %llu bits, the plan %llu", (unsigned long long)base, (unsigned long long)plan->bits);
    // the last slice one bit further: past the plan's total
    {
      gh_slice s;
      if (gh_encode_slice(in + cut[K - 1], n - cut[K - 1], plan, base - parts[K - 1].s.bits + 1, 1, nullptr, 0, nullptr,
                          0, &s) != GH_E_ARG)
        FAIL("a slice ending past the plan's bits was accepted");
    }
    // merged, in a shuffled order, into an image of exactly file_bytes bytes
    const uint64_t bytes = plan->file_bytes;
    const size_t odd = (size_t)(it & 1);
    uint8_t* heap = (uint8_t*)std::malloc(bytes + odd);
    uint8_t* img = heap + odd;
    std::memset(img, 0xA5, bytes);
    if (gh_encode_image_init(plan, img, bytes - 1) != GH_E_SMALL) FAIL("a short image was not GH_E_SMALL");
    if (gh_encode_image_init(plan, img, bytes) != GH_OK) FAIL("image init: %s", gh_last_error());
    std::vector<uint32_t> order(K);
    for (uint32_t i = 0; i < K; ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    for (uint32_t i : order)
      if (gh_slice_merge(img, bytes, plan, &parts[i].s, parts[i].words, parts[i].gapw) != GH_OK)
        FAIL("merge of slice %u: %s", i, gh_last_error());
    uint8_t* ref = (uint8_t*)std::malloc(bytes);
    if (gh_encode_write(in, plan, 1 + (int)(rng() % 5), ref, bytes) != GH_OK) FAIL("gh_encode_write: %s", gh_last_error());
    if (std::memcmp(img, ref, bytes)) {
      uint64_t at = 0;
      while (img[at] == ref[at]) ++at;
      FAIL("n = %llu, %u slices: the merged image differs from gh_encode_write's at byte %llu of %llu",
           (unsigned long long)n, K, (unsigned long long)at, (unsigned long long)bytes);
    }
    std::free(ref);
    std::free(heap);
    for (Part& pt : parts) {
      std::free(pt.words);
      std::free(pt.gapw);
    }
    std::free(in);
  }
  delete plan;
  delete whole;
  std::printf("encode_slices_fuzz: %ld iterations ok (%llu slices)\n", iters, slices_seen);
  return 0;
}
