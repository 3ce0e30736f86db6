// batch_raw_fuzz — the segment transition functions of the batched raw load
// (csrc/gh_raw_trans.hpp) and their host twin gh_batchraw_gaps_host under AddressSanitizer +
// UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_batch_raw_sanitize.py (CPU, no GPU calls).
// The header is the text the raw load's kernels compile for the device.  Random canonical
// codes with maxlen 1..16, complete and incomplete, over words that are valid streams (random
// codewords packed MSB-first) or arbitrary garbage, in heap blocks of exactly W words and
// exactly ceil(G / 8) gap words (W = 0 and W not a multiple of 4 included):
//   gh_batchraw_gaps_host equals a plain sequential walk from bit 0 under the same lookup
//   rule (a pattern outside the code advances maxlen bits);
//   every T_j nibble, recomputed here through trans_walk, lies in 0..15, and chaining the
//   T_j gives the same entries;
//   trans_compose: identity on both sides, associativity and agreement with trans_apply on
//   random functions;
//   a buffer one word short is refused with GH_E_SMALL and not written.
// Usage: batch_raw_fuzz [iterations] [seed]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gaphuff.h"
#include "gh_internal.hpp"
#include "gh_raw_trans.hpp"

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

#define FAIL(...)                             \
  do {                                        \
    std::fprintf(stderr, "batch_raw_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);        \
    std::fprintf(stderr, "\n");               \
    return 1;                                 \
  } while (0)

using namespace gh;

// A canonical (symbol, length) list with the given maxlen: lengths drawn so that the Kraft
// sum stays <= 1; `complete` then fills the rest of the code space with maxlen codewords
// (as far as 256 symbols allow).
static std::vector<gh_sym> random_code(std::mt19937_64& rng, uint32_t maxlen, bool complete) {
  std::vector<uint32_t> lens;
  uint64_t left = 1ull << maxlen;  // free code space on the maxlen scale
  const uint32_t want = 1 + (uint32_t)(rng() % 40);
  lens.push_back(maxlen);
  left -= 1;
  while (lens.size() < want && left) {
    const uint32_t l = 1 + (uint32_t)(rng() % maxlen);
    const uint64_t cost = 1ull << (maxlen - l);
    if (cost > left) continue;
    lens.push_back(l);
    left -= cost;
  }
  if (complete) {
    for (uint32_t l = 1; l <= maxlen && left; ++l)  // largest pieces first
      while (lens.size() < 256 && left >= (1ull << (maxlen - l))) {
        lens.push_back(l);
        left -= 1ull << (maxlen - l);
      }
  }
  std::sort(lens.begin(), lens.end());
  std::vector<uint32_t> perm(256);
  for (uint32_t i = 0; i < 256; ++i) perm[i] = i;
  std::shuffle(perm.begin(), perm.end(), rng);
  std::vector<gh_sym> syms(lens.size());
  for (size_t i = 0; i < lens.size(); ++i) syms[i] = gh_sym{(uint8_t)perm[i], (uint8_t)lens[i]};
  return syms;
}

static uint32_t bits16(const uint32_t* words, uint64_t w, uint64_t p) {
  const uint64_t i = p >> 5;
  const uint64_t two = ((uint64_t)(i < w ? words[i] : 0u) << 32) | (i + 1 < w ? words[i + 1] : 0u);
  return (uint32_t)(two >> (48 - (p & 31))) & 0xFFFFu;
}

static uint32_t length_at(const Canon& c, const uint32_t* words, uint64_t w, uint64_t p) {
  uint32_t index;
  const uint32_t l = canon_decode16(c, bits16(words, w, p), &index);
  return l ? l : c.maxlen;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 2000;
  std::mt19937_64 rng(argc > 2 ? (uint64_t)std::atoll(argv[2]) : 1);

  // the compose laws on random functions
  for (int it = 0; it < 2000; ++it) {
    const unsigned long long f = rng(), g = rng(), h = rng();
    if (trans_compose(trans_identity(), f) != f || trans_compose(f, trans_identity()) != f) FAIL("identity law");
    if (trans_compose(trans_compose(f, g), h) != trans_compose(f, trans_compose(g, h))) FAIL("associativity");
    for (uint32_t x = 0; x < 16; ++x) {
      if (trans_apply(trans_compose(f, g), x) != trans_apply(g, trans_apply(f, x))) FAIL("compose is not `then` after `first`");
      if (trans_apply(trans_identity(), x) != x || trans_apply(f, x) > 15) FAIL("apply");
    }
  }

  for (int it = 0; it < iters; ++it) {
    const uint32_t maxlen = 1 + (uint32_t)(rng() % 16);
    const bool complete = rng() % 2;
    const std::vector<gh_sym> syms = random_code(rng, maxlen, complete);
    Canon c;
    if (build_canon(syms.data(), (uint32_t)syms.size(), c)) FAIL("iteration %d: the drawn code is not canonical: %s", it, gh_last_error());
    // sizes around the unit edges (256 segments = 1024 words) and tiny ones; W = 0 sometimes
    static const uint64_t edges[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 1020, 1021, 1023, 1024, 1025, 1028, 2047, 2049, 3075};
    const uint64_t w = it % 3 == 0 ? edges[rng() % (sizeof(edges) / sizeof(edges[0]))] : rng() % 700;
    const uint64_t g = ceil_div(w, 4), ngapw = ceil_div(g, GH_GAPS_PER_WORD);
    uint32_t* words = new uint32_t[w];  // exactly W words: a read past them is caught
    if (rng() % 2) {
      for (uint64_t i = 0; i < w; ++i) words[i] = (uint32_t)rng();  // garbage
    } else {
      std::fill(words, words + w, 0u);  // a valid stream: random codewords, MSB first
      uint64_t p = 0;
      while (true) {
        const uint32_t k = (uint32_t)(rng() % c.nsyms), l = c.len[k];
        if (p + l > 32 * w) break;
        for (uint32_t b = 0; b < l; ++b, ++p)
          if ((c.code[k] >> (l - 1 - b)) & 1u) words[p >> 5] |= 0x80000000u >> (p & 31);
      }
    }
    uint32_t* got = new uint32_t[ngapw];
    std::fill(got, got + ngapw, 0xDEADBEEFu);
    if (int rc = gh_batchraw_gaps_host(syms.data(), (uint32_t)syms.size(), words, w, got, ngapw))
      FAIL("iteration %d: gh_batchraw_gaps_host = %d (%s)", it, rc, gh_last_error());
    // the plain sequential walk from bit 0
    std::vector<uint32_t> want(ngapw, 0u), entry(g + 1, 0u);
    uint64_t p = 0;
    for (uint64_t j = 1; j < g; ++j) {
      while (p < 128 * j) p += length_at(c, words, w, p);
      entry[j] = (uint32_t)(p - 128 * j);
      if (entry[j] > 15) FAIL("iteration %d: an entry past 15", it);
      want[(j - 1) / GH_GAPS_PER_WORD] |= entry[j] << (4 * ((j - 1) % GH_GAPS_PER_WORD));
    }
    if (ngapw && std::memcmp(got, want.data(), 4 * ngapw) != 0)
      FAIL("iteration %d: gap words differ from the sequential walk (maxlen %u, complete %d, W %llu)", it, maxlen,
           (int)complete, (unsigned long long)w);
    // T_j through the shared walk: nibbles in range, and the chain reproduces the entries
    uint32_t e = 0;
    for (uint64_t j = 0; j < g; ++j) {
      unsigned long long f = 0;
      for (uint32_t x = 0; x < 16; ++x) {
        uint64_t q = 128 * j + x;
        const uint32_t t = trans_walk(x, [&]() {
          const uint32_t l = length_at(c, words, w, q);
          q += l;
          return l;
        });
        if (t > 15 || q != 128 * (j + 1) + t) FAIL("iteration %d: T_%llu(%u) out of range", it, (unsigned long long)j, x);
        f |= trans_nibble(x, t);
      }
      if (e != entry[j]) FAIL("iteration %d: chained entry of segment %llu differs", it, (unsigned long long)j);
      e = trans_apply(f, e);
    }
    // one word short: refused, nothing written
    if (ngapw) {
      uint32_t* small = new uint32_t[ngapw - 1];
      std::fill(small, small + (ngapw - 1), 0xDEADBEEFu);
      if (gh_batchraw_gaps_host(syms.data(), (uint32_t)syms.size(), words, w, small, ngapw - 1) != GH_E_SMALL)
        FAIL("iteration %d: a short buffer was not refused", it);
      for (uint64_t i = 0; i + 1 < ngapw; ++i)
        if (small[i] != 0xDEADBEEFu) FAIL("iteration %d: a refused call wrote", it);
      delete[] small;
    }
    delete[] got;
    delete[] words;
  }
  // W = 0 with no code at all, and segments with an empty code
  if (gh_batchraw_gaps_host(nullptr, 0, nullptr, 0, nullptr, 0) != GH_OK) FAIL("the empty stream");
  uint32_t one = 0, out = 0;
  if (gh_batchraw_gaps_host(nullptr, 0, &one, 1, &out, 1) != GH_E_TABLE) FAIL("segments with an empty code");
  std::printf("%d iterations ok\n", iters);
  return 0;
}
