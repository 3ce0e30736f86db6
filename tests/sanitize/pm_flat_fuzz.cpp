// pm_flat_fuzz — the level-by-level package-merge (csrc/gh_pm_flat.hpp) under
// AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_pm_flat_sanitize.py (CPU, no GPU calls).
// The header is the text the batched encoder's code kernel compiles for the device.  Random
// sorted histograms of five kinds (uniform, tiny counts with many ties, geometric and
// power-of-two counts that make the 16-bit limit bind, exponential), counts and lengths in
// heap blocks of exactly n entries (counts below 2^42: a package weighs at most 2^15 times the
// largest count, so no weight wraps):
//   gh_package_merge_flat's lengths equal gh_package_merge's;
//   the levels driven here item by item, as the kernel's threads place them: every position
//   below m_l = min(2n - 2, n + floor(m_{l-1} / 2)) is filled exactly once, no item lands
//   at or past n + packages, the list is sorted, no level holds more than 2n - 2 items;
//   the trace over those levels gives the same lengths, non-increasing in sorted rank, with
//   a Kraft sum of exactly 1 (n >= 2);
//   pm_canon_bases / pm_canon_entry give build_canon's codes for the file order.
// Usage: pm_flat_fuzz [iterations] [seed]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gaphuff.h"
#include "gh_internal.hpp"
#include "gh_pm_flat.hpp"

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

#define FAIL(...)                           \
  do {                                      \
    std::fprintf(stderr, "pm_flat_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);      \
    std::fprintf(stderr, "\n");             \
    return 1;                               \
  } while (0)

using namespace gh;

static std::vector<uint64_t> histogram(std::mt19937_64& rng, int kind, uint32_t n) {
  std::vector<uint64_t> c(n);
  const double base = 1.2 + 0.8 * (double)(rng() % 1000) / 1000.0;
  const double mean = 1.0 + (double)(rng() % 5000);
  for (uint32_t i = 0; i < n; ++i) {
    switch (kind) {
      case 0: c[i] = 1 + rng() % (1u << 20); break;
      case 1: c[i] = 1 + rng() % 3; break;
      case 2: c[i] = (uint64_t)std::max(1.0, std::pow(base, (double)std::min(i, 40u)) * (0.5 + (double)(rng() % 1000) / 1000.0)); break;
      case 3: c[i] = 1ull << (rng() % 41); break;
      default: c[i] = (uint64_t)std::max(1.0, -mean * std::log(1.0 - (double)(rng() % 1000000) / 1000001.0)); break;
    }
  }
  std::sort(c.begin(), c.end());
  return c;
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 4000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  unsigned long long limited = 0;
  for (long it = 0; it < iters; ++it) {
    const uint32_t n = it % 16 == 0 ? 256u : it % 16 == 1 ? (uint32_t)(1 + it / 16 % 3) : 2u + (uint32_t)(rng() % 255);
    const std::vector<uint64_t> hist = histogram(rng, (int)(it % 5), n);
    uint64_t* c = (uint64_t*)std::malloc(8 * n);
    uint8_t* lazy = (uint8_t*)std::malloc(n);
    uint8_t* flat = (uint8_t*)std::malloc(n);
    std::memcpy(c, hist.data(), 8 * n);
    if (gh_package_merge(c, n, lazy) != GH_OK) FAIL("it %ld: gh_package_merge: %s", it, gh_last_error());
    if (gh_package_merge_flat(c, n, flat) != GH_OK) FAIL("it %ld: gh_package_merge_flat: %s", it, gh_last_error());
    if (std::memcmp(lazy, flat, n)) FAIL("it %ld (n = %u): the two forms' lengths differ", it, n);
    if (n >= 2) {
      // the levels, item by item
      const uint32_t need = pm_need(n);
      if (need != 2 * n - 2) FAIL("pm_need");
      std::vector<uint64_t> prev(c, c + n), next;
      uint32_t* mask = (uint32_t*)std::calloc(PM_LEVELS * PM_MASK_WORDS, 4);
      uint32_t* pre = (uint32_t*)std::calloc(PM_LEVELS * PM_MASK_WORDS, 4);
      uint32_t* nl = (uint32_t*)std::malloc(4 * PM_LEVELS);
      uint32_t m = n;
      for (uint32_t l = 1; l < PM_LEVELS; ++l) {
        const uint32_t np = m / 2, mn = pm_next_items(n, m);
        if (mn > need || mn != std::min(need, n + np)) FAIL("it %ld: level %u holds %u items", it, l + 1, mn);
        next.assign(mn, 0);
        std::vector<int> filled(mn, 0);
        for (uint32_t j = 0; j < n; ++j) {
          const uint32_t pos = pm_leaf_pos(c, prev.data(), np, j);
          if (pos >= n + np) FAIL("it %ld: level %u leaf %u at %u of %u", it, l + 1, j, pos, n + np);
          if (pos < need) {
            if (pos >= mn || filled[pos]++) FAIL("it %ld: level %u position %u taken twice or past the list", it, l + 1, pos);
            next[pos] = c[j];
            mask[l * PM_MASK_WORDS + (pos >> 5)] |= 1u << (pos & 31u);
          }
        }
        for (uint32_t i = 0; i < np; ++i) {
          const uint64_t P = pm_package(prev.data(), i);
          const uint32_t pos = pm_package_pos(c, n, i, P);
          if (pos >= n + np) FAIL("it %ld: level %u package %u at %u of %u", it, l + 1, i, pos, n + np);
          if (pos < need) {
            if (pos >= mn || filled[pos]++) FAIL("it %ld: level %u position %u taken twice or past the list", it, l + 1, pos);
            next[pos] = P;
          }
        }
        for (uint32_t p = 0; p < mn; ++p) {
          if (!filled[p]) FAIL("it %ld: level %u position %u empty", it, l + 1, p);
          if (p && next[p] < next[p - 1]) FAIL("it %ld: level %u not sorted at %u", it, l + 1, p);
        }
        pm_mask_prefix(mask + l * PM_MASK_WORDS, pre + l * PM_MASK_WORDS);
        m = mn;
        prev.swap(next);
      }
      pm_trace(mask, pre, n, nl);
      uint64_t kraft = 0;
      uint32_t cnt[PM_LEVELS + 1] = {}, base[PM_LEVELS + 1], first[PM_LEVELS + 1];
      for (uint32_t j = 0; j < n; ++j) {
        const uint32_t len = pm_length(nl, j);
        if (len != flat[j] || len < 1 || len > PM_LEVELS) FAIL("it %ld: trace gives %u for leaf %u, the library %u", it, len, j, flat[j]);
        if (j && len > flat[j - 1]) FAIL("it %ld: lengths grow with the count at %u", it, j);
        kraft += 1ull << (PM_LEVELS - len);
        cnt[len]++;
      }
      if (kraft != 1ull << PM_LEVELS) FAIL("it %ld (n = %u): Kraft sum %llu / 65536", it, n, (unsigned long long)kraft);
      limited += flat[0] == PM_LEVELS;
      // the canonical code of the file order (most frequent first)
      gh_sym* syms = (gh_sym*)std::malloc(sizeof(gh_sym) * n);
      for (uint32_t f = 0; f < n; ++f) syms[f] = gh_sym{(uint8_t)f, flat[n - 1 - f]};
      Canon canon;
      if (build_canon(syms, n, canon)) FAIL("it %ld: build_canon: %s", it, gh_last_error());
      pm_canon_bases(cnt, base, first);
      for (uint32_t f = 0; f < n; ++f) {
        const uint32_t len = syms[f].length;
        if (pm_canon_entry(base, first, f, len) != ((canon.code[f] << (32u - len)) | len))
          FAIL("it %ld: canonical entry of file position %u", it, f);
      }
      if (pm_canon_entry(base, first, 0, 0) != 0 || pm_canon_entry(base, first, 0, 17) != 0) FAIL("entry of a bad length");
      std::free(syms);
      std::free(mask);
      std::free(pre);
      std::free(nl);
    } else if (flat[0] != 1) {
      FAIL("n = 1: length %u", flat[0]);
    }
    std::free(c);
    std::free(lazy);
    std::free(flat);
  }
  // the refusals
  uint64_t one = 1;
  uint8_t out = 0;
  if (gh_package_merge_flat(nullptr, 1, &out) != GH_E_ARG || gh_package_merge_flat(&one, 1, nullptr) != GH_E_ARG ||
      gh_package_merge_flat(&one, GH_MAX_SYMBOLS + 1, &out) != GH_E_ARG || gh_package_merge_flat(nullptr, 0, &out) != GH_OK)
    FAIL("refusals");
  if (iters >= 1000 && limited == 0) FAIL("no histogram reached the 16-bit limit");
  std::printf("pm_flat_fuzz: %ld iterations ok (%llu at the 16-bit limit)\n", iters, limited);
  return 0;
}
