// planes_fuzz — the byte planes' host code under AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_planes_sanitize.py (CPU, no GPU calls).
//   layout     random item lists (element sizes 1, 2, 4, 8, every mask, nelem at the lane and
//              unit edges) through gh_planes_layout, in heap blocks of exactly ntensors items
//              and 8 ntensors slots, against a naive recomputation; every refusal.
//   twins      gh_planes_split_host / gh_planes_join_host with the tensor and every plane in
//              heap blocks of exact size, against the scalar rule src[i * E + p]; the vector
//              rule of csrc/gh_planes.hpp (planes_split16 / planes_join16) on random groups.
//   container  gh_planes_image_write, then gh_planes_parse over the valid image (in a heap
//              block of exact size), every truncation of it (or 64 random ones when it is
//              long) and random bit flips: a parse that succeeds must give views inside the
//              block, which are then read.
// Usage: planes_fuzz [iterations] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gaphuff.h"
#include "gh_internal.hpp"
#include "gh_planes.hpp"

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

#define FAIL(...)                          \
  do {                                     \
    std::fprintf(stderr, "planes_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);     \
    std::fprintf(stderr, "\n");            \
    return 1;                              \
  } while (0)

static const uint32_t ELEMS[4] = {1, 2, 4, 8};
static const uint64_t EDGES[] = {0, 1, 15, 16, 17, 1023, 1024, 1025, 2049};

static uint8_t* heap_bytes(uint64_t n) { return (uint8_t*)std::malloc(n ? n : 1); }

template <uint32_t E>
static int group_check(std::mt19937_64& rng) {
  uint32_t w[4 * E], pl[E][4], back[4 * E];
  for (uint32_t& x : w) x = (uint32_t)rng();
  gh::planes_split16<E>(w, pl);
  const uint8_t* src = (const uint8_t*)w;
  for (uint32_t p = 0; p < E; ++p)
    for (uint32_t i = 0; i < 16; ++i)
      if (((const uint8_t*)pl[p])[i] != src[gh::planes_src_index(i, E, p)]) return 1;
  gh::planes_join16<E>(pl, back);
  return std::memcmp(w, back, sizeof(w)) != 0;
}

// Reads every view of a parsed container (ASan checks them against the block).
static uint64_t touch(const gh_planes_image& im) {
  uint64_t sum = 0;
  for (uint32_t p = 0; p < im.elem_size; ++p) {
    const uint8_t* b = (const uint8_t*)im.plane[p];
    for (uint64_t i = 0; i < im.plane_bytes[p]; ++i) sum += b[i];
    if ((im.coded_mask >> p) & 1u) {
      const gh_stream& s = im.stream[p];
      for (uint32_t i = 0; i < s.nsyms; ++i) sum += s.syms[i].length;
      for (uint64_t i = 0; i < 4 * s.w; ++i) sum += ((const uint8_t*)s.payload)[i];
      for (uint64_t i = 0; i < 4 * ((s.g + 7) / 8); ++i) sum += ((const uint8_t*)s.gap_words)[i];
    }
  }
  return sum;
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 2000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  unsigned long long tensors_seen = 0, parsed_ok = 0, sink = 0;
  for (long it = 0; it < iters; ++it) {
    // ---- layout ---------------------------------------------------------------------------
    const uint32_t nt = (uint32_t)(rng() % 24);
    gh_planes_item* items = (gh_planes_item*)std::malloc(nt ? nt * sizeof(gh_planes_item) : 1);
    gh_planes_slot* slots = (gh_planes_slot*)std::malloc(nt ? 8 * nt * sizeof(gh_planes_slot) : 1);
    for (uint32_t t = 0; t < nt; ++t) {
      const uint32_t e = ELEMS[rng() % 4];
      const uint64_t nelem = rng() % 3 == 0 ? EDGES[rng() % 9] : rng() % 5000;
      items[t] = gh_planes_item{nullptr, nelem, e, (uint32_t)(rng() % (1u << e))};
    }
    uint32_t ns = 77;
    uint64_t sb = 77;
    if (gh_planes_layout(items, nt, slots, &ns, &sb) != GH_OK) FAIL("a valid list was refused: %s", gh_last_error());
    uint32_t want_ns = 0;
    uint64_t want_at = 0;
    for (uint32_t t = 0; t < nt; ++t)
      for (uint32_t p = 0; p < 8; ++p) {
        const gh_planes_slot& s = slots[8 * t + p];
        if (p < items[t].elem_size && ((items[t].coded_mask >> p) & 1u)) {
          if (s.stream != want_ns++ || s.stored_off != 0) FAIL("tensor %u plane %u: coded slot", t, p);
        } else if (p < items[t].elem_size) {
          if (s.stream != GH_PLANES_STORED || s.stored_off != want_at || want_at % 16) FAIL("tensor %u plane %u: stored slot", t, p);
          want_at += (items[t].nelem + 15) / 16 * 16;
        } else if (s.stream != GH_PLANES_STORED || s.stored_off != 0) {
          FAIL("tensor %u plane %u: absent slot", t, p);
        }
      }
    if (ns != want_ns || sb != want_at) FAIL("totals");
    if (nt) {  // refusals
      const uint32_t k = (uint32_t)(rng() % nt);
      const gh_planes_item keep = items[k];
      const uint32_t bad_e[] = {0, 3, 5, 6, 7, 9, 16};
      items[k].elem_size = bad_e[rng() % 7];
      if (gh_planes_layout(items, nt, slots, &ns, &sb) != GH_E_ARG) FAIL("a bad element size was accepted");
      items[k] = keep;
      items[k].coded_mask = 1u << keep.elem_size;
      if (gh_planes_layout(items, nt, slots, &ns, &sb) != GH_E_ARG) FAIL("a mask >= 1 << E was accepted");
      items[k] = keep;
      items[k].coded_mask = 0;
      items[k].nelem = ~0ull - rng() % 15;  // round_up(nelem, 16) overflows
      if (gh_planes_layout(items, nt, slots, &ns, &sb) != GH_E_ARG) FAIL("an overflowing nelem was accepted");
      items[k] = keep;
      if (gh_planes_layout(items, nt, nullptr, &ns, &sb) != GH_E_ARG || gh_planes_layout(nullptr, nt, slots, &ns, &sb) != GH_E_ARG ||
          gh_planes_layout(items, nt, slots, nullptr, &sb) != GH_E_ARG || gh_planes_layout(items, nt, slots, &ns, nullptr) != GH_E_ARG)
        FAIL("a null pointer was accepted");
    }
    if (it % 500 == 0) {
      // a sum that overflows; more than 2^24 coded planes; the empty list
      gh_planes_item two[2] = {{nullptr, 1ull << 63, 2, 0}, {nullptr, 1ull << 63, 2, 0}};
      gh_planes_slot s16[16];
      if (gh_planes_layout(two, 2, s16, &ns, &sb) != GH_E_ARG) FAIL("a stored arena of 2^65 bytes was accepted");
      if (gh_planes_layout(nullptr, 0, nullptr, &ns, &sb) != GH_OK || ns || sb) FAIL("the empty list");
    }
    if (it == 0) {  // (once: 2^24 slots)
      const uint32_t many = (1u << 21) + 1;  // x 8 coded planes = 2^24 + 8
      std::vector<gh_planes_item> big(many, gh_planes_item{nullptr, 1, 8, 0xFF});
      std::vector<gh_planes_slot> bs(8ull * many);
      if (gh_planes_layout(big.data(), many, bs.data(), &ns, &sb) != GH_E_ARG) FAIL("2^24 + 8 coded planes were accepted");
      if (gh_planes_layout(big.data(), many - 1, bs.data(), &ns, &sb) != GH_OK || ns != (1u << 24)) FAIL("2^24 coded planes were refused");
    }
    tensors_seen += nt;
    std::free(items);
    std::free(slots);

    // ---- the vector rule on one group -------------------------------------------------------
    if (group_check<1>(rng) || group_check<2>(rng) || group_check<4>(rng) || group_check<8>(rng)) FAIL("the vector rule");

    // ---- twins --------------------------------------------------------------------------------
    const uint32_t e = ELEMS[rng() % 4];
    const uint64_t nelem = rng() % 2 ? EDGES[rng() % 9] : rng() % 3000;
    uint8_t* src = heap_bytes(nelem * e);
    for (uint64_t i = 0; i < nelem * e; ++i) src[i] = (uint8_t)(rng() % 5 ? rng() % 4 : rng());  // (compressible)
    uint8_t* planes[8] = {};
    for (uint32_t p = 0; p < e; ++p) planes[p] = heap_bytes(nelem);
    const uint32_t mask = (uint32_t)(rng() % (1u << e));
    gh_planes_item item{src, nelem, e, mask};
    if (gh_planes_split_host(&item, (void* const*)planes) != GH_OK) FAIL("split: %s", gh_last_error());
    for (uint32_t p = 0; p < e; ++p)
      for (uint64_t i = 0; i < nelem; ++i)
        if (planes[p][i] != src[i * e + p]) FAIL("split: E %u nelem %llu plane %u byte %llu", e, (unsigned long long)nelem, p, (unsigned long long)i);
    uint8_t* back = heap_bytes(nelem * e);
    gh_planes_item jitem{back, nelem, e, mask};
    if (gh_planes_join_host(&jitem, (const void* const*)planes) != GH_OK) FAIL("join: %s", gh_last_error());
    if (nelem && std::memcmp(back, src, nelem * e)) FAIL("join: E %u nelem %llu", e, (unsigned long long)nelem);
    item.elem_size = 3;
    if (gh_planes_split_host(&item, (void* const*)planes) != GH_E_ARG) FAIL("split accepted E = 3");
    item.elem_size = e;

    // ---- container ----------------------------------------------------------------------------
    std::vector<std::vector<uint8_t>> coded(e);
    const void* pp[8] = {};
    uint64_t pb[8] = {};
    for (uint32_t p = 0; p < e; ++p) {
      if (!((mask >> p) & 1u)) {
        pp[p] = planes[p];
        pb[p] = nelem;
        continue;
      }
      gh_encode_plan plan;
      if (gh_encode_plan_make(planes[p], nelem, 1, 0, &plan) != GH_OK) FAIL("plan: %s", gh_last_error());
      coded[p].resize(plan.file_bytes);
      if (gh_encode_write(planes[p], &plan, 1, coded[p].data(), coded[p].size()) != GH_OK) FAIL("encode: %s", gh_last_error());
      pp[p] = coded[p].data();
      pb[p] = coded[p].size();
    }
    uint64_t total = 0;
    if (gh_planes_image_bytes(e, pb, &total) != GH_OK) FAIL("image_bytes: %s", gh_last_error());
    uint8_t* img = heap_bytes(total);
    if (total && gh_planes_image_write(&item, pp, pb, img, total - 1) != GH_E_SMALL) FAIL("a short output was accepted");
    if (gh_planes_image_write(&item, pp, pb, img, total) != GH_OK) FAIL("image_write: %s", gh_last_error());
    gh_planes_image im;
    if (gh_planes_parse(img, total, &im) != GH_OK) FAIL("a valid container was refused: %s", gh_last_error());
    if (im.nelem != nelem || im.elem_size != e || im.coded_mask != mask) FAIL("parsed header");
    for (uint32_t p = 0; p < e; ++p) {
      if (im.plane_bytes[p] != pb[p] || ((const uint8_t*)im.plane[p] - img) % 8) FAIL("plane %u: view", p);
      if (pb[p] && std::memcmp(im.plane[p], pp[p], pb[p])) FAIL("plane %u: bytes", p);
    }
    sink += touch(im);
    // truncations: every one is refused
    for (int k = 0; k < 64 && total; ++k) {
      const uint64_t cut = total <= 64 ? (uint64_t)k % total : rng() % total;
      uint8_t* part = heap_bytes(cut);
      if (cut) std::memcpy(part, img, cut);
      const int rc = gh_planes_parse(part, cut, &im);
      // (the last plane ends the file: every cut loses bytes a plane needs)
      if (rc == GH_OK) FAIL("a container cut from %llu to %llu bytes was accepted", (unsigned long long)total, (unsigned long long)cut);
      if (rc != GH_E_FORMAT) FAIL("a truncated container gave %d", rc);
      std::free(part);
    }
    // bit flips: any result, no access outside the block
    for (int k = 0; k < 32 && total; ++k) {
      uint8_t* flip = heap_bytes(total);
      std::memcpy(flip, img, total);
      const int nflip = 1 + (int)(rng() % 3);
      for (int f = 0; f < nflip; ++f) {
        // mostly in the header and the plane sizes, where the structure is
        const uint64_t at = rng() % 4 ? rng() % std::min<uint64_t>(total, 24 + 8 * e + 64) : rng() % total;
        flip[at] ^= (uint8_t)(1u << (rng() % 8));
      }
      const int rc = gh_planes_parse(flip, total, &im);
      if (rc == GH_OK) {
        sink += touch(im);
        ++parsed_ok;
      } else if (rc != GH_E_FORMAT) {
        FAIL("a flipped container gave %d", rc);
      }
      std::free(flip);
    }
    std::free(img);
    std::free(back);
    std::free(src);
    for (uint32_t p = 0; p < e; ++p) std::free(planes[p]);
  }
  std::printf("planes_fuzz: %ld iterations ok (%llu tensors, %llu flipped containers still parsed, sum %llu)\n", iters,
              tensors_seen, parsed_ok, sink);
  return 0;
}
