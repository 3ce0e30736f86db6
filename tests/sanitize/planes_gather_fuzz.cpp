// planes_gather_fuzz — the element gather's host code under AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_planes_gather_sanitize.py (CPU, no GPU calls).
//   plan   random tensor lists (element sizes 1, 2, 4, 8, every mask, nelem at the lane and unit
//          edges) and random element ranges (empty, whole, repeated, edges) through
//          gh_pgather_plan, with the ranges, byte ranges and offsets in heap blocks of exact
//          size, against a naive recomputation; flagged streams; the sizing call; every refusal.
//   join   the range join's per-lane text (pg_join_lane of csrc/gh_planes_gather.hpp, the text
//          the kernel compiles) over every lane of every unit of those ranges, lanes past a
//          range's end included: the staging buffer filled as the inner gather fills it, the
//          stored arena and the destination (at a random byte shift) in heap blocks of exact
//          size, against the scalar rule dst[k * E + p] = tensor[(lo + k) * E + p].
// Usage: planes_gather_fuzz [iterations] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gaphuff.h"
#include "gh_internal.hpp"
#include "gh_planes.hpp"
#include "gh_planes_gather.hpp"

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
    std::fprintf(stderr, "planes_gather_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);            \
    std::fprintf(stderr, "\n");                   \
    return 1;                                     \
  } while (0)

static const uint32_t ELEMS[4] = {1, 2, 4, 8};
static const uint64_t EDGES[] = {0, 1, 15, 16, 17, 64, 1023, 1024, 1025, 2049};
constexpr uint8_t FILL = 0xA5;

template <class T>
static T* heap_of(uint64_t n) {
  return (T*)std::malloc(n ? n * sizeof(T) : 1);
}

static void join_range(const gh::PgView& v, const gh::PlanesTensor& d) {
  const uint64_t lanes = gh::planes_units(v.len) * gh::PLANES_UNIT_ELEMS;  // every lane of every unit
  for (uint64_t i0 = 0; i0 < lanes; i0 += gh::PLANES_GROUP) {
    switch (d.elem) {
      case 1: gh::pg_join_lane<1>(v, d, i0); break;
      case 2: gh::pg_join_lane<2>(v, d, i0); break;
      case 4: gh::pg_join_lane<4>(v, d, i0); break;
      default: gh::pg_join_lane<8>(v, d, i0); break;
    }
  }
}

static int one(std::mt19937_64& rng) {
  auto pick = [&](uint64_t n) { return n ? rng() % n : 0; };
  const uint32_t nt = 1 + (uint32_t)pick(6);
  gh_planes_item* items = heap_of<gh_planes_item>(nt);
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t e = ELEMS[pick(4)];
    const uint64_t edge = EDGES[pick(sizeof(EDGES) / sizeof(EDGES[0]))];
    items[t] = gh_planes_item{nullptr, pick(3) ? edge : edge + pick(40), e, (uint32_t)pick(1ull << e)};
    if (pick(4) == 0) items[t].coded_mask = 1u << (e - 1);
  }
  gh_planes_slot* slots = heap_of<gh_planes_slot>(8ull * nt);
  uint32_t ns = 0;
  uint64_t stored_bytes = 0;
  if (gh_planes_layout(items, nt, slots, &ns, &stored_bytes) != GH_OK) FAIL("layout refused a valid list");
  // the tensors, and the stored arena from their planes by the scalar rule
  std::vector<std::vector<uint8_t>> data(nt);
  uint8_t* stored = heap_of<uint8_t>(stored_bytes);
  std::memset(stored, 0, stored_bytes);
  for (uint32_t t = 0; t < nt; ++t) {
    data[t].resize(items[t].nelem * items[t].elem_size);
    for (uint8_t& b : data[t]) b = (uint8_t)rng();
    for (uint32_t p = 0; p < items[t].elem_size; ++p)
      if (slots[8 * t + p].stream == GH_PLANES_STORED)
        for (uint64_t i = 0; i < items[t].nelem; ++i)
          stored[slots[8 * t + p].stored_off + i] = data[t][gh::planes_src_index(i, items[t].elem_size, p)];
  }
  // the ranges: rows of 16 k elements at multiples of 16 (the vector path), edges, anything
  const uint32_t nr = (uint32_t)pick(24);
  gh_erange* ranges = heap_of<gh_erange>(nr);
  for (uint32_t i = 0; i < nr; ++i) {
    const uint64_t t = pick(nt), n = items[t].nelem;
    uint64_t lo = pick(n + 1), hi = lo + pick(n - lo + 1);
    switch (pick(5)) {
      case 0: lo &= ~15ull; hi = lo + ((hi - lo) & ~15ull); break;
      case 1: lo = 0; hi = n; break;
      case 2: hi = lo; break;
      case 3:
        lo = EDGES[pick(9)] < n ? EDGES[pick(9)] : n;
        if (lo > n) lo = n;
        hi = lo + pick(n - lo + 1);
        break;
      default: break;
    }
    ranges[i] = gh_erange{t, lo, hi};
  }
  uint32_t* status = heap_of<uint32_t>(ns);
  for (uint32_t s = 0; s < ns; ++s) status[s] = pick(7) == 0 ? GH_ST_BADCODE : 0;
  // naive recomputation
  std::vector<gh_brange> want;
  std::vector<uint64_t> wso(nr), wdo(nr);
  uint64_t wstage = 0, wdst = 0;
  uint32_t wbad = 0;
  for (uint32_t i = 0; i < nr; ++i) {
    const uint64_t t = ranges[i].tensor, len = ranges[i].hi - ranges[i].lo;
    wso[i] = wstage;
    wdo[i] = wdst;
    bool flagged = false;
    for (uint32_t p = 0; p < items[t].elem_size; ++p)
      if (slots[8 * t + p].stream != GH_PLANES_STORED) {
        want.push_back(gh_brange{slots[8 * t + p].stream, ranges[i].lo, ranges[i].hi});
        wstage += len;
        flagged |= status[slots[8 * t + p].stream] != 0;
      }
    wdst += len * items[t].elem_size;
    wbad += flagged;
  }
  uint64_t nb = 7, ob = 7;
  uint32_t bad = 7;
  uint64_t* so = heap_of<uint64_t>(nr);
  uint64_t* dof = heap_of<uint64_t>(nr);
  int rc = gh_pgather_plan(items, nt, status, ranges, nr, nullptr, 0, &nb, so, dof, &ob, &bad);
  if (rc != (want.empty() ? GH_OK : GH_E_SMALL) || nb != want.size() || ob != wdst || bad != wbad) FAIL("sizing call");
  gh_brange* br = heap_of<gh_brange>(nb);
  rc = gh_pgather_plan(items, nt, status, ranges, nr, br, nb, &nb, so, dof, &ob, &bad);
  if (rc != GH_OK || nb != want.size() || ob != wdst || bad != wbad) FAIL("plan: rc %d", rc);
  for (uint64_t k = 0; k < nb; ++k)
    if (br[k].stream != want[k].stream || br[k].lo != want[k].lo || br[k].hi != want[k].hi) FAIL("byte range %llu", (unsigned long long)k);
  for (uint32_t i = 0; i < nr; ++i)
    if (so[i] != wso[i] || dof[i] != wdo[i]) FAIL("offsets of range %u", i);
  if (nb) {  // one slot short
    gh_brange* shortbuf = heap_of<gh_brange>(nb - 1);
    if (gh_pgather_plan(items, nt, status, ranges, nr, shortbuf, nb - 1, &nb, so, dof, &ob, &bad) != GH_E_SMALL) FAIL("short buffer accepted");
    std::free(shortbuf);
  }
  // refusals: each leaves the counts zero
  if (nr) {
    gh_erange* r2 = heap_of<gh_erange>(nr);
    for (int k = 0; k < 3; ++k) {
      std::memcpy(r2, ranges, nr * sizeof(gh_erange));
      gh_erange& x = r2[pick(nr)];
      if (k == 0) x.tensor = nt + pick(3);
      if (k == 1) { x.lo = x.hi + 1 + pick(3); }
      if (k == 2) x.hi = items[x.tensor].nelem + 1 + pick(3);
      if (k == 2 && x.lo > x.hi) x.lo = 0;
      nb = ob = 7;
      bad = 7;
      if (gh_pgather_plan(items, nt, status, r2, nr, br, want.size(), &nb, so, dof, &ob, &bad) != GH_E_ARG || nb || ob || bad)
        FAIL("refusal %d", k);
    }
    std::free(r2);
    if (gh_pgather_plan(items, nt, status, nullptr, nr, br, want.size(), &nb, so, dof, &ob, &bad) != GH_E_ARG) FAIL("null ranges");
    if (gh_pgather_plan(items, nt, status, ranges, nr, br, want.size(), nullptr, so, dof, &ob, &bad) != GH_E_ARG) FAIL("null count");
  }
  // the join: staging as the inner gather leaves it, flagged ranges skipped as the kernel skips them
  gh_pgather_plan(items, nt, status, ranges, nr, br, want.size(), &nb, so, dof, &ob, &bad);
  std::vector<gh::PlanesTensor> desc;
  uint32_t ns2 = 0, maxc = 0;
  uint64_t sb2 = 0;
  if (gh::pgather_descs(items, nt, desc, &ns2, &sb2, &maxc) != GH_OK || ns2 != ns || sb2 != stored_bytes) FAIL("descs");
  uint8_t* stage = heap_of<uint8_t>(wstage);
  for (uint32_t i = 0; i < nr; ++i) {
    const uint64_t t = ranges[i].tensor, len = ranges[i].hi - ranges[i].lo;
    uint32_t c = 0;
    for (uint32_t p = 0; p < items[t].elem_size; ++p)
      if ((items[t].coded_mask >> p) & 1u) {
        for (uint64_t k = 0; k < len; ++k)
          stage[so[i] + c * len + k] = data[t][gh::planes_src_index(ranges[i].lo + k, items[t].elem_size, p)];
        ++c;
      }
  }
  const uint64_t shift = pick(3) ? 0 : pick(17);
  uint8_t* dst = heap_of<uint8_t>(shift + wdst);
  std::memset(dst, FILL, shift + wdst);
  for (uint32_t i = 0; i < nr; ++i) {
    const gh::PlanesTensor& d = desc[ranges[i].tensor];
    const gh::PgLoc loc = gh::pg_locate([&](uint32_t t) -> const gh::PlanesTensor& { return desc[t]; },
                                        [&](uint32_t s) { return status[s]; }, nt, ranges[i]);
    if (loc.ncoded == gh::PG_BAD) FAIL("a valid range refused");
    if (loc.flagged) continue;
    gh::PgView v{};
    v.stage = stage;
    v.stored = stored;
    v.dst = dst + shift;
    v.lo = ranges[i].lo;
    v.len = ranges[i].hi - ranges[i].lo;
    v.stage_off = so[i];
    v.dst_off = dof[i];
    v.vec = gh::pg_vec_ok(v.stage_off, v.lo, v.len, (uint64_t)(uintptr_t)v.dst + v.dst_off, loc.ncoded);
    join_range(v, d);
  }
  for (uint64_t k = 0; k < shift; ++k)
    if (dst[k] != FILL) FAIL("a byte before the destination written");
  // later ranges may overwrite nothing of earlier ones (the layout is tight): check range by range
  for (uint32_t i = 0; i < nr; ++i) {
    const uint64_t t = ranges[i].tensor, len = ranges[i].hi - ranges[i].lo, e = items[t].elem_size;
    bool flagged = false;
    for (uint32_t p = 0; p < e; ++p)
      if (slots[8 * t + p].stream != GH_PLANES_STORED) flagged |= status[slots[8 * t + p].stream] != 0;
    for (uint64_t k = 0; k < len * e; ++k) {
      const uint8_t w = flagged ? FILL : data[t][ranges[i].lo * e + k];
      if (dst[shift + dof[i] + k] != w) FAIL("range %u byte %llu (E %llu, shift %llu)", i, (unsigned long long)k, (unsigned long long)e, (unsigned long long)shift);
    }
  }
  std::free(dst);
  std::free(stage);
  std::free(br);
  std::free(dof);
  std::free(so);
  std::free(status);
  std::free(ranges);
  std::free(stored);
  std::free(slots);
  std::free(items);
  return 0;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
  // refusals that need no list
  uint64_t nb = 1, ob = 1;
  uint32_t bad = 1;
  if (gh_pgather_plan(nullptr, 0, nullptr, nullptr, 0, nullptr, 0, &nb, nullptr, nullptr, &ob, &bad) != GH_OK || nb || ob || bad)
    FAIL("the empty plan");
  gh_planes_item odd{nullptr, 10, 3, 1}, huge{nullptr, 1ull << 39, 2, 2};
  gh_erange r{0, 0, 1};
  uint64_t so = 0, dof = 0;
  if (gh_pgather_plan(&odd, 1, nullptr, &r, 1, nullptr, 0, &nb, &so, &dof, &ob, &bad) != GH_E_ARG) FAIL("element size 3 accepted");
  if (gh_pgather_plan(&huge, 1, nullptr, &r, 1, nullptr, 0, &nb, &so, &dof, &ob, &bad) != GH_E_ARG) FAIL("a 2^40-byte tensor accepted");
  for (int it = 0; it < iters; ++it)
    if (one(rng)) {
      std::fprintf(stderr, "planes_gather_fuzz: iteration %d failed\n", it);
      return 1;
    }
  std::printf("%d iterations ok\n", iters);
  return 0;
}
