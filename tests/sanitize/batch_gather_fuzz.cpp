// batch_gather_fuzz — the batched gather plan's arithmetic, run on the CPU under
// AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources with -fsanitize=address,undefined; run by
// tests/test_batch_gather_sanitize.py (CPU, no GPU calls).  csrc/gh_batch_range.hpp is the
// text the planning kernels (csrc/gh_batch_gather.hip) compile: here its functions run the
// kernels' three steps item by item -- br_locate per range, a serial exclusive scan with the
// scan kernel's decision whether the plan stands, br_piece per piece slot found by
// gr_piece_range -- over heap blocks of exactly the sizes the batch allocates: nstreams + 1
// unit prefixes, nunits + 1 scan entries, nstreams sizes and status words, nranges range
// records, and a piece buffer of exactly gh_gather_piece_bound(nranges, bytes, 8) pieces.
// Any read or write past one of them is reported.  The pieces, their count, the byte total
// and the flagged-range count are checked against gh_batchdec_plan.
// Usage: batch_gather_fuzz [iterations] [seed]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gaphuff.h"
#include "gh_batch_range.hpp"

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

// A heap block of exactly n elements (n = 0: one byte, never touched).
template <class T>
struct Block {
  T* p;
  explicit Block(uint64_t n) : p((T*)std::malloc(n ? n * sizeof(T) : 1)) {
    if (!p) std::abort();
  }
  ~Block() { std::free(p); }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
};

#define FAIL(...)                                \
  do {                                           \
    std::fprintf(stderr, "batch_gather_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);           \
    std::fprintf(stderr, "\n");                  \
    return 1;                                    \
  } while (0)

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  unsigned long long pieces_seen = 0, flagged_seen = 0;
  for (long it = 0; it < iters; ++it) {
    // a batch: streams of 0 .. 9 units; non-last units hold 2048 .. 36608 codewords, at and
    // just above the minimum most of the time (the bound is tight there), last ones 1 .. 36608
    const uint32_t ns = 1 + (uint32_t)(rng() % 24);
    Block<uint32_t> unit0(ns + 1);
    unit0.p[0] = 0;
    for (uint32_t s = 0; s < ns; ++s) unit0.p[s + 1] = unit0.p[s] + (uint32_t)(rng() % 10);
    const uint32_t nunits = unit0.p[ns];
    Block<uint64_t> unit_off(nunits + 1ull);
    Block<uint64_t> n(ns);
    Block<uint32_t> status(ns);
    unit_off.p[0] = 0;
    for (uint32_t s = 0; s < ns; ++s) {
      for (uint32_t u = unit0.p[s]; u < unit0.p[s + 1]; ++u) {
        const uint64_t step = u + 1 == unit0.p[s + 1] ? 1 + rng() % 36608
                              : rng() % 4             ? 2048 + rng() % 3
                                                      : 2048 + rng() % (36608 - 2048 + 1);
        unit_off.p[u + 1] = unit_off.p[u] + step;
      }
      const uint64_t total = unit_off.p[unit0.p[s + 1]] - unit_off.p[unit0.p[s]];
      const uint64_t pad = rng() % 144;
      n.p[s] = rng() % 2 ? total : total > pad ? total - pad : std::min<uint64_t>(total, 1);
      status.p[s] = rng() % 5 == 0 ? GH_ST_BADCODE : 0u;
    }
    const bool use_status = rng() % 3 != 0;
    // ranges: on and next to unit offsets, empty, whole streams, random, repeats
    const uint32_t nr = (uint32_t)(rng() % 32);
    Block<gh_brange> rs(nr);
    uint64_t want_total = 0;
    uint32_t want_bad = 0;
    for (uint32_t t = 0; t < nr; ++t) {
      const uint32_t s = (uint32_t)(rng() % ns);
      const uint64_t N = n.p[s], nu = unit0.p[s + 1] - unit0.p[s], base = unit_off.p[unit0.p[s]];
      uint64_t lo, hi;
      switch (rng() % 6) {
        case 0: {
          const uint64_t e = unit_off.p[unit0.p[s] + rng() % (nu + 1)] - base;
          lo = e + rng() % 3;
          lo = lo ? lo - 1 : 0;
          hi = lo + rng() % 3;
          break;
        }
        case 1:
          lo = hi = rng() % (N + 1);
          break;
        case 2:
          lo = 0, hi = N;
          break;
        case 3: {  // from one byte before a unit offset over a few units to one byte past another
          const uint64_t a = rng() % (nu + 1), b = std::min<uint64_t>(a + rng() % 6, nu);
          const uint64_t ea = unit_off.p[unit0.p[s] + a] - base, eb = unit_off.p[unit0.p[s] + b] - base;
          lo = ea ? ea - 1 : 0;
          hi = eb + 1;
          break;
        }
        case 4:
          if (t) {
            rs.p[t] = rs.p[rng() % t];
            want_total += rs.p[t].hi - rs.p[t].lo;
            want_bad += use_status && status.p[rs.p[t].stream];
            continue;
          }
          [[fallthrough]];
        default:
          lo = rng() % (N + 1);
          hi = rng() % (N + 1);
          if (lo > hi) std::swap(lo, hi);
      }
      lo = std::min(lo, N);
      hi = std::min(std::max(hi, lo), N);
      rs.p[t] = gh_brange{s, lo, hi};
      want_total += hi - lo;
      want_bad += use_status && status.p[s];
    }
    // the reference plan
    uint64_t np = ~0ull, total = ~0ull;
    uint32_t nbad = ~0u;
    const uint32_t* stp = use_status ? status.p : nullptr;
    gh_batchdec_plan(unit0.p, unit_off.p, n.p, stp, ns, rs.p, nr, nullptr, 0, &np, &total, &nbad);
    Block<gh_gather_piece> ref(np);
    uint64_t np2 = 0, total2 = 0;
    uint32_t nbad2 = 0;
    if (gh_batchdec_plan(unit0.p, unit_off.p, n.p, stp, ns, rs.p, nr, ref.p, np, &np2, &total2, &nbad2) != GH_OK ||
        np2 != np || total2 != total || total != want_total || nbad != want_bad || nbad2 != nbad)
      FAIL("gh_batchdec_plan: %s", gh_last_error());
    // ---- the device plan's steps ----
    const uint64_t dst_len = want_total, cap = gh_gather_piece_bound(nr, dst_len, 8);
    if (np > cap) FAIL("%llu pieces exceed the bound %llu (%u ranges, %llu bytes)", (unsigned long long)np,
                       (unsigned long long)cap, nr, (unsigned long long)dst_len);
    Block<gh::RangeLoc> loc(nr);
    Block<uint32_t> slot(nr);
    Block<uint64_t> dst0(nr);
    Block<gh_gather_piece> pcs(cap);
    const auto n_of = [&](uint32_t s) { return n.p[s]; };
    const auto st_of = [&](uint32_t s) { return use_status ? status.p[s] : 0u; };
    uint32_t bad_ranges = 0;
    for (uint32_t i = 0; i < nr; ++i) {
      bool flagged;
      loc.p[i] = gh::br_locate(unit0.p, unit_off.p, n_of, st_of, ns, rs.p[i], &flagged);
      bad_ranges += flagged;
    }
    uint64_t sum_c = 0, sum_l = 0;
    for (uint32_t i = 0; i < nr; ++i) {
      slot.p[i] = (uint32_t)sum_c;
      dst0.p[i] = sum_l;
      if (loc.p[i].count == gh::GR_BAD_RANGE) FAIL("a valid range was refused");
      sum_c += loc.p[i].count;
      sum_l += loc.p[i].len;
    }
    if (sum_l != total) FAIL("out_bytes %llu, expected %llu", (unsigned long long)sum_l, (unsigned long long)total);
    if (sum_c != np) FAIL("npieces %llu, expected %llu", (unsigned long long)sum_c, (unsigned long long)np);
    if (bad_ranges != nbad) FAIL("bad_ranges %u, expected %u", bad_ranges, nbad);
    if (sum_l > dst_len || sum_c > cap) FAIL("the plan does not stand");
    for (uint64_t q = 0; q < sum_c; ++q) {
      const uint32_t a = gh::gr_piece_range(slot.p, nr, q);
      if (q - slot.p[a] >= loc.p[a].count) FAIL("slot %llu lies in no range", (unsigned long long)q);
      pcs.p[q] = gh::br_piece(unit0.p, unit_off.p, rs.p[a], loc.p[a], q - slot.p[a], dst0.p[a]);
    }
    for (uint64_t q = 0; q < np; ++q) {
      const gh_gather_piece &x = pcs.p[q], &y = ref.p[q];
      if (x.dst != y.dst || x.block != y.block || x.a != y.a || x.b != y.b || x.pad != 0)
        FAIL("piece %llu: {%llu, %u, %u, %u}, gh_batchdec_plan has {%llu, %u, %u, %u}", (unsigned long long)q,
             (unsigned long long)x.dst, x.block, x.a, x.b, (unsigned long long)y.dst, y.block, y.a, y.b);
      // a piece lies inside its unit and inside the output
      if (x.block >= nunits || x.a >= x.b || x.b > unit_off.p[x.block + 1] - unit_off.p[x.block] ||
          x.dst + (x.b - x.a) > dst_len)
        FAIL("piece %llu leaves its unit or the output", (unsigned long long)q);
    }
    pieces_seen += np;
    flagged_seen += nbad;
    // bad ranges are flagged by locate
    bool f;
    const uint64_t n0 = n.p[0];
    if (gh::br_locate(unit0.p, unit_off.p, n_of, st_of, ns, gh_brange{ns, 0, 0}, &f).count != gh::GR_BAD_RANGE ||
        gh::br_locate(unit0.p, unit_off.p, n_of, st_of, ns, gh_brange{0, n0, n0 + 1}, &f).count != gh::GR_BAD_RANGE ||
        gh::br_locate(unit0.p, unit_off.p, n_of, st_of, ns, gh_brange{0, 1, 0}, &f).count != gh::GR_BAD_RANGE ||
        gh::br_locate(unit0.p, unit_off.p, n_of, st_of, ns, gh_brange{~0ull, 0, 0}, &f).count != gh::GR_BAD_RANGE)
      FAIL("a bad range was accepted");
  }
  std::printf("batch_gather_fuzz: %ld iterations ok (%llu pieces, %llu ranges on flagged streams)\n", iters, pieces_seen,
              flagged_seen);
  return 0;
}
