// index_fuzz — the seek-index parser and locate under AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_index_sanitize.py (CPU, no GPU calls).
// Every image lives in a heap block of exactly its length, at an even or an odd address,
// so any read past it and any misaligned load is reported.  Covers gh_index_bytes,
// gh_index_parse and gh_index_locate on valid, random, truncated and corrupted images;
// on a valid image locate's answer is checked against a linear search.
// Usage: index_fuzz [iterations] [seed]
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

static uint64_t g_sink = 0;

static void put64(std::vector<uint8_t>& b, size_t at, uint64_t v) { std::memcpy(&b[at], &v, 8); }

// A valid image for g segments: random steps of at most 143 * stride.
static std::vector<uint8_t> make_index(std::mt19937_64& rng, uint32_t k, uint64_t g, std::vector<uint64_t>* offs) {
  const uint64_t bytes = gh_index_bytes(g, k);
  if (bytes == 0) std::abort();
  std::vector<uint8_t> b(bytes, 0);
  const uint64_t ne = (bytes - 40) / 8;
  std::vector<uint64_t> o(ne, 0);
  for (uint64_t i = 1; i < ne; ++i) o[i] = o[i - 1] + (rng() % 4 == 0 ? 0 : rng() % ((143ull << k) + 1));
  put64(b, 0, GH_INDEX_MAGIC);
  const uint32_t h[2] = {k, 0};
  std::memcpy(&b[8], h, 8);
  put64(b, 16, o[ne - 1]);
  put64(b, 24, g);
  put64(b, 32, ne);
  for (uint64_t i = 0; i < ne; ++i) put64(b, 40 + 8 * i, o[i]);
  if (offs) *offs = o;
  return b;
}

// Parse from an exact-size heap copy at address parity `odd`; on success touch every
// entry and run locate on `tries` ranges (valid and not).  Returns the parse result.
static int check(const std::vector<uint8_t>& buf, size_t claimed_len, int odd, std::mt19937_64& rng, int tries) {
  uint8_t* heap = (uint8_t*)std::malloc(buf.size() + 1 + (size_t)odd);
  uint8_t* p = heap + odd;
  if (!buf.empty()) std::memcpy(p, buf.data(), buf.size());
  gh_index ix;
  const int rc = gh_index_parse(p, claimed_len, &ix);
  if (rc == GH_OK) {
    const uint8_t* e = (const uint8_t*)ix.offsets;
    for (uint64_t i = 0; i < 8 * ix.nentries; ++i) g_sink += e[i];
    for (int t = 0; t < tries; ++t) {
      uint64_t lo = rng() % (ix.n + 2), hi = rng() % (ix.n + 2), b = 0, en = 0, sk = 0;
      if (rng() % 4) { if (lo > hi) std::swap(lo, hi); }
      if (gh_index_locate(&ix, lo, hi, &b, &en, &sk) == GH_OK) g_sink += b + en + sk;
    }
  }
  std::free(heap);
  return rc;
}

static std::vector<uint8_t> mutate(const std::vector<uint8_t>& src, std::mt19937_64& rng) {
  std::vector<uint8_t> b = src;
  switch (rng() % 5) {
    case 0:  // truncate
      b.resize(rng() % (b.size() + 1));
      break;
    case 1:  // flip bytes, mostly in the header
      for (int k = 0, m = 1 + (int)(rng() % 6); k < m && !b.empty(); ++k)
        b[rng() % (rng() % 2 ? std::min<size_t>(b.size(), 48) : b.size())] = (uint8_t)rng();
      break;
    case 2: {  // overwrite one u32/u64 field with an extreme value
      static const uint64_t ext[] = {0, 1, 7, 21, 0x7fffffffull, 0xffffffffull, 1ull << 40, 1ull << 61, ~0ull};
      if (b.size() >= 16) {
        const size_t o = 8 * (rng() % (b.size() / 8 - 1)) + (rng() % 8 ? 0 : rng() % 8);
        const uint64_t v = ext[rng() % 9];
        std::memcpy(&b[std::min(o, b.size() - 8)], &v, (rng() & 1) ? 8 : 4);
      }
      break;
    }
    case 3:  // extend with junk
      for (int k = 0, m = (int)(rng() % 64); k < m; ++k) b.push_back((uint8_t)rng());
      break;
    default:  // pure noise behind a good magic
      for (size_t i = 8; i < b.size(); ++i) b[i] = (uint8_t)rng();
  }
  return b;
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  if (gh_index_bytes(1000, 7) != 0 || gh_index_bytes(1000, 21) != 0 || gh_index_bytes(0, 8) != 48) {
    std::fprintf(stderr, "index_fuzz: gh_index_bytes\n");
    return 1;
  }
  long parsed = 0;
  for (long it = 0; it < iters; ++it) {
    const uint32_t k = 8 + (uint32_t)(rng() % 13);
    const uint64_t g = (rng() % 40) * (1ull << k) / 8 + (rng() % 3);
    std::vector<uint64_t> o;
    const std::vector<uint8_t> good = make_index(rng, k, g, &o);
    // a valid image parses, and locate agrees with a linear search
    {
      uint8_t* heap = (uint8_t*)std::malloc(good.size() + 1);
      uint8_t* p = heap + (it & 1);
      std::memcpy(p, good.data(), good.size());
      gh_index ix;
      if (gh_index_parse(p, good.size(), &ix) != GH_OK) {
        std::fprintf(stderr, "index_fuzz: a valid image was refused: %s\n", gh_last_error());
        return 1;
      }
      const uint64_t n = ix.n, nb = ix.nentries - 1;
      for (int t = 0; t < 8 && n > 0; ++t) {
        uint64_t lo = rng() % (n + 1), hi = rng() % (n + 1), b = 0, e = 0, sk = 0;
        if (lo > hi) std::swap(lo, hi);
        if (gh_index_locate(&ix, lo, hi, &b, &e, &sk) != GH_OK) { std::fprintf(stderr, "index_fuzz: locate failed\n"); return 1; }
        if (lo == hi) continue;
        uint64_t kk = 0, m = 0;
        for (uint64_t i = 0; i < nb; ++i) if (o[i] <= lo) kk = i;
        while (o[m] < hi) ++m;
        if (b != (kk << k) || e != std::min<uint64_t>(m << k, g) || sk != lo - o[kk]) {
          std::fprintf(stderr, "index_fuzz: locate(%llu, %llu) disagrees with the linear search\n",
                       (unsigned long long)lo, (unsigned long long)hi);
          return 1;
        }
      }
      uint64_t b, e, sk;
      if (gh_index_locate(&ix, n, n + 1, &b, &e, &sk) != GH_E_ARG || gh_index_locate(&ix, 1, 0, &b, &e, &sk) != GH_E_ARG) {
        std::fprintf(stderr, "index_fuzz: a bad range was accepted\n");
        return 1;
      }
      std::free(heap);
    }
    const std::vector<uint8_t> bad = mutate(good, rng);
    parsed += check(bad, bad.size(), (int)(rng() & 1), rng, 4) == GH_OK;
    // a claimed length shorter than the buffer (never longer: the caller owns the length)
    if (!bad.empty()) (void)check(bad, rng() % bad.size(), (int)(rng() & 1), rng, 2);
  }
  std::printf("index_fuzz: %ld iterations ok (%ld mutants parsed, sink %llu)\n", iters, parsed,
              (unsigned long long)(g_sink & 0xff));
  return 0;
}
