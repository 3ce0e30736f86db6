// index_slices_fuzz — the host's sliced seek index under AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_index_slices_sanitize.py (CPU, no GPU
// calls).  Each iteration takes a random input (as encode_slices_fuzz: 0 bytes to a few
// hundred KiB, now and then a few MiB so that the thread count really splits a slice;
// flat, skewed and one-symbol histograms), cuts it at random points (repeated points: empty
// slices), and for a random stride asks every slice for the entries it owns
// (gh_encode_index_slice, a random thread count) into a heap block of exactly nk entries.
// The k0 values must chain and the nk values sum to nblocks.  The entries are stored, in a
// shuffled order, into an image of exactly gh_index_bytes bytes at an odd address
// (gh_index_image_init, gh_index_slice_merge); the image must equal gh_encode_index's and
// parse.
// Usage: index_slices_fuzz [iterations] [seed]
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
    std::fprintf(stderr, "index_slices_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);           \
    std::fprintf(stderr, "\n");                  \
    return 1;                                    \
  } while (0)

struct Part {
  uint64_t k0, nk;
  uint64_t* ent;
};

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 300;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  unsigned long long slices_seen = 0, entries_seen = 0;
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
    // the cuts: K slices, some of them empty, sometimes clustered
    const uint32_t K = 1 + (uint32_t)(rng() % (rng() % 4 ? 6 : 40));
    std::vector<uint64_t> cut(K + 1, 0);
    cut[K] = n;
    const uint64_t near = rng() % (n + 1);
    for (uint32_t i = 1; i < K; ++i) cut[i] = rng() % 3 ? rng() % (n + 1) : std::min<uint64_t>(n, near + rng() % 8);
    std::sort(cut.begin(), cut.end());
    const uint32_t k = GH_INDEX_MIN_LOG2 + (uint32_t)(rng() % 3 ? rng() % 3 : rng() % 13);
    const uint64_t bytes = gh_index_bytes(plan->g, k);
    if (bytes == 0) FAIL("gh_index_bytes refused stride 2^%u", k);
    const uint64_t nblocks = (bytes - 40) / 8 - 1;
    // every slice's entries into a block of exactly nk entries
    std::vector<Part> parts(K);
    uint64_t base = 0, next_k = 0;
    for (uint32_t i = 0; i < K; ++i) {
      const uint8_t* p = in + cut[i];
      const uint64_t m = cut[i + 1] - cut[i];
      uint64_t bits = 0;
      for (uint64_t j = 0; j < m; ++j) bits += plan->len[p[j]];
      Part& pt = parts[i];
      const int threads = 1 + (int)(rng() % 5);
      const int rc0 = gh_encode_index_slice(p, m, plan, base, cut[i], k, threads, nullptr, 0, &pt.k0, &pt.nk);
      if (rc0 != (pt.nk ? GH_E_SMALL : GH_OK)) FAIL("sizing call returned %d: %s", rc0, gh_last_error());
      uint64_t k0 = 0, nk = 0;
      if (gh_index_slice_extent(base, bits, k, &k0, &nk) != GH_OK || k0 != pt.k0 || nk != pt.nk)
        FAIL("extents differ from gh_index_slice_extent's");
      if (pt.k0 != next_k) FAIL("slice %u: k0 = %llu does not chain (%llu)", i, (unsigned long long)pt.k0, (unsigned long long)next_k);
      next_k = pt.k0 + pt.nk;
      pt.ent = pt.nk ? (uint64_t*)std::malloc(8 * pt.nk) : nullptr;
      if (pt.ent) std::memset(pt.ent, 0xA5, 8 * pt.nk);
      if (gh_encode_index_slice(p, m, plan, base, cut[i], k, threads, pt.ent, pt.nk, &k0, &nk) != GH_OK)
        FAIL("slice %u refused: %s", i, gh_last_error());
      if (k0 != pt.k0 || nk != pt.nk) FAIL("the extents changed between calls");
      for (uint64_t j = 0; j < pt.nk; ++j)
        if (pt.ent[j] < cut[i] || pt.ent[j] > cut[i + 1]) FAIL("slice %u: entry outside [sym_base, sym_base + n]", i);
      if (pt.nk > 1) {  // a cap one short: refused, nothing written
        uint64_t* sm = (uint64_t*)std::malloc(8 * (pt.nk - 1));
        if (gh_encode_index_slice(p, m, plan, base, cut[i], k, threads, sm, pt.nk - 1, &k0, &nk) != GH_E_SMALL)
          FAIL("a short entry buffer was not GH_E_SMALL");
        std::free(sm);
      }
      base += bits;
      ++slices_seen;
      entries_seen += pt.nk;
    }
    if (base != plan->bits) FAIL("the slices hold %llu bits, the plan %llu", (unsigned long long)base, (unsigned long long)plan->bits);
    if (next_k != nblocks) FAIL("the slices own %llu entries of %llu", (unsigned long long)next_k, (unsigned long long)nblocks);
    // stored, in a shuffled order, into an image of exactly `bytes` bytes at an odd address
    uint8_t* heap = (uint8_t*)std::malloc(bytes + 1);
    uint8_t* img = heap + 1;
    std::memset(img, 0xA5, bytes);
    if (gh_index_image_init(plan, k, img, bytes - 1) != GH_E_SMALL) FAIL("a short image was not GH_E_SMALL");
    if (gh_index_image_init(plan, k, img, bytes) != GH_OK) FAIL("image init: %s", gh_last_error());
    std::vector<uint32_t> order(K);
    for (uint32_t i = 0; i < K; ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    for (uint32_t i : order) {
      if (gh_index_slice_merge(img, bytes - 1, parts[i].k0, parts[i].nk, parts[i].ent) != GH_E_SMALL)
        FAIL("a merge into a short image was not GH_E_SMALL");
      if (parts[i].nk && gh_index_slice_merge(img, bytes, nblocks + 1 - parts[i].nk, parts[i].nk, parts[i].ent) != GH_E_ARG)
        FAIL("a merge past the image's entries was accepted");
      if (gh_index_slice_merge(img, bytes, parts[i].k0, parts[i].nk, parts[i].ent) != GH_OK)
        FAIL("merge of slice %u: %s", i, gh_last_error());
    }
    uint8_t* ref = (uint8_t*)std::malloc(bytes);
    if (gh_encode_index(in, plan, k, 1 + (int)(rng() % 5), ref, bytes) != GH_OK) FAIL("gh_encode_index: %s", gh_last_error());
    if (std::memcmp(img, ref, bytes)) {
      uint64_t at = 0;
      while (img[at] == ref[at]) ++at;
      FAIL("n = %llu, %u slices, stride 2^%u: the merged index differs from gh_encode_index's at byte %llu of %llu",
           (unsigned long long)n, K, k, (unsigned long long)at, (unsigned long long)bytes);
    }
    gh_index ix;
    if (gh_index_parse(img, bytes, &ix) != GH_OK) FAIL("the merged index does not parse: %s", gh_last_error());
    std::free(ref);
    std::free(heap);
    for (Part& pt : parts) std::free(pt.ent);
    std::free(in);
  }
  delete plan;
  std::printf("index_slices_fuzz: %ld iterations ok (%llu slices, %llu entries)\n", iters, slices_seen, entries_seen);
  return 0;
}
