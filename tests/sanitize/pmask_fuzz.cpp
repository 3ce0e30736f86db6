// pmask_fuzz — the plane choice's host code under AddressSanitizer + UBSan.
//
// Built by `make -C cse375-finalproj-huffman-decoding_amd asan` from this file plus the
// library's host sources (csrc/gh_core.cpp, csrc/gh_io.cpp) with
// -fsanitize=address,undefined; run by tests/test_pmask_sanitize.py (CPU, no GPU calls).
//   host     random tensor lists (element sizes 1, 2, 4, 8, nelem at the lane and unit edges and
//            around the tie sizes, constant, skewed and uniform bytes), every tensor in a heap
//            block of exactly nelem * E bytes at a random alignment, items, masks and sizes in
//            blocks of exact size, through gh_pmask_host against a naive recomputation: a scalar
//            histogram per plane, gh_encode_plan_from_counts, fb < nelem.
//   counts   the same lists through gh_pmask_from_counts with the counts in a block of exactly
//            nplanes x 256 words; every refusal of both entry points.
//   header   the shared arithmetic of csrc/gh_pmask.hpp: pmask_file_bytes against the plan's
//            file_bytes on random (bits, nsyms, n) around 2^31, and pmask_tensor_of on the lists'
//            own numbering.
// Usage: pmask_fuzz [iterations] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gaphuff.h"
#include "gh_internal.hpp"
#include "gh_pmask.hpp"

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
    std::fprintf(stderr, "pmask_fuzz: "); \
    std::fprintf(stderr, __VA_ARGS__);    \
    std::fprintf(stderr, "\n");           \
    return 1;                             \
  } while (0)

static const uint32_t ELEMS[4] = {1, 2, 4, 8};
static const uint64_t EDGES[] = {0, 1, 15, 16, 17, 29, 30, 31, 33, 34, 35, 1023, 1024, 1025, 2049};

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 500;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 375);
  unsigned long long tensors_seen = 0, coded_seen = 0, stored_seen = 0;
  for (long it = 0; it < iters; ++it) {
    // ---- a list, every tensor in its own exact block at a random alignment ----------------
    const uint32_t nt = (uint32_t)(rng() % 12);
    gh_planes_item* items = (gh_planes_item*)std::malloc(nt ? nt * sizeof(gh_planes_item) : 1);
    uint32_t* masks = (uint32_t*)std::malloc(nt ? nt * sizeof(uint32_t) : 1);
    uint64_t* sizes = (uint64_t*)std::malloc(nt ? 8 * nt * sizeof(uint64_t) : 1);
    std::vector<uint8_t*> blocks(nt);
    std::vector<uint32_t> q0(nt + 1, 0);
    for (uint32_t t = 0; t < nt; ++t) {
      const uint32_t e = ELEMS[rng() % 4];
      const uint64_t nelem = rng() % 3 == 0 ? EDGES[rng() % 15] : rng() % 6000;
      const uint64_t nb = nelem * e, shift = rng() % 16;
      // the tensor's bytes end where the block ends; its start is `shift` bytes into it
      blocks[t] = (uint8_t*)std::malloc(nb + shift ? nb + shift : 1);
      uint8_t* data = blocks[t] + shift;
      const unsigned kind = (unsigned)(rng() % 3);
      for (uint64_t i = 0; i < nb; ++i) {
        const uint32_t p = (uint32_t)(i % e);
        data[i] = kind == 0 || (p & 1u) ? (uint8_t)((rng() & 0xFF) >> (rng() % 7))  // skewed
                  : kind == 1           ? (uint8_t)(0x40 + p)                         // constant planes
                                        : (uint8_t)rng();                             // uniform
      }
      items[t] = gh_planes_item{nelem ? data : nullptr, nelem, e, (uint32_t)rng()};  // (the mask is ignored)
      q0[t + 1] = q0[t] + e;
    }
    const uint32_t nplanes = q0[nt];
    // ---- the naive recomputation ------------------------------------------------------------
    uint64_t* counts = (uint64_t*)std::calloc(nplanes ? 256ull * nplanes : 1, sizeof(uint64_t));
    std::vector<uint32_t> want_mask(nt, 0);
    std::vector<uint64_t> want_size(8ull * nt, 0);
    for (uint32_t t = 0; t < nt; ++t) {
      const uint32_t e = items[t].elem_size;
      const uint8_t* src = (const uint8_t*)items[t].data;
      for (uint32_t p = 0; p < e; ++p) {
        uint64_t* c = counts + 256ull * (q0[t] + p);
        for (uint64_t i = 0; i < items[t].nelem; ++i) ++c[src[i * e + p]];
        if (!items[t].nelem) continue;
        gh_encode_plan plan;
        if (gh_encode_plan_from_counts(c, 0, &plan)) FAIL("plan: %s", gh_last_error());
        want_size[8ull * t + p] = plan.file_bytes;
        if (plan.file_bytes < items[t].nelem) {
          want_mask[t] |= 1u << p;
          ++coded_seen;
        } else {
          ++stored_seen;
        }
        if (gh::pmask_file_bytes(plan.bits, plan.nsyms, plan.n) != plan.file_bytes) FAIL("pmask_file_bytes differs from the plan");
        if (gh::pmask_tensor_of(q0.data(), nt, q0[t] + p) != t) FAIL("pmask_tensor_of");
      }
      ++tensors_seen;
    }
    // ---- the two entry points -----------------------------------------------------------------
    for (int which = 0; which < 2; ++which) {
      std::memset(masks, 0xEE, nt * sizeof(uint32_t));
      std::memset(sizes, 0xEE, 8ull * nt * sizeof(uint64_t));
      const int rc = which ? gh_pmask_from_counts(counts, items, nt, masks, sizes) : gh_pmask_host(items, nt, masks, sizes);
      if (rc != GH_OK) FAIL("entry %d refused a valid list: %s", which, gh_last_error());
      for (uint32_t t = 0; t < nt; ++t) {
        if (masks[t] != want_mask[t]) FAIL("entry %d tensor %u: mask 0x%x, want 0x%x", which, t, masks[t], want_mask[t]);
        for (uint32_t p = 0; p < 8; ++p)
          if (sizes[8ull * t + p] != want_size[8ull * t + p]) FAIL("entry %d tensor %u plane %u: size", which, t, p);
      }
      // the sizes are optional
      if ((which ? gh_pmask_from_counts(counts, items, nt, masks, nullptr) : gh_pmask_host(items, nt, masks, nullptr)) != GH_OK)
        FAIL("entry %d without sizes", which);
      for (uint32_t t = 0; t < nt; ++t)
        if (masks[t] != want_mask[t]) FAIL("entry %d tensor %u: mask without sizes", which, t);
    }
    // ---- refusals -----------------------------------------------------------------------------
    if (nt) {
      if (gh_pmask_host(nullptr, nt, masks, sizes) != GH_E_ARG || gh_pmask_host(items, nt, nullptr, sizes) != GH_E_ARG)
        FAIL("gh_pmask_host accepted a null");
      if (gh_pmask_from_counts(nullptr, items, nt, masks, sizes) != GH_E_ARG ||
          gh_pmask_from_counts(counts, nullptr, nt, masks, sizes) != GH_E_ARG ||
          gh_pmask_from_counts(counts, items, nt, nullptr, sizes) != GH_E_ARG)
        FAIL("gh_pmask_from_counts accepted a null");
      const uint32_t k = (uint32_t)(rng() % nt);
      const gh_planes_item keep = items[k];
      const uint32_t bad_e[] = {0, 3, 5, 6, 7, 9, 16};
      items[k].elem_size = bad_e[rng() % 7];
      if (gh_pmask_host(items, nt, masks, sizes) != GH_E_ARG || gh_pmask_from_counts(counts, items, nt, masks, sizes) != GH_E_ARG)
        FAIL("a bad element size was accepted");
      items[k] = keep;
      if (keep.nelem) {
        items[k].data = nullptr;
        if (gh_pmask_host(items, nt, masks, sizes) != GH_E_ARG) FAIL("a null tensor was accepted");
        items[k] = keep;
      }
      // counts that do not sum to nelem: one count more, one less, another nelem
      uint64_t* c = counts + 256ull * (q0[k] + rng() % keep.elem_size);
      const uint32_t v = (uint32_t)(rng() % 256);
      ++c[v];
      if (gh_pmask_from_counts(counts, items, nt, masks, sizes) != GH_E_ARG) FAIL("one count too many was accepted");
      --c[v];
      if (keep.nelem) {
        uint32_t u = 0;
        while (!c[u]) ++u;
        --c[u];
        if (gh_pmask_from_counts(counts, items, nt, masks, sizes) != GH_E_ARG) FAIL("one count too few was accepted");
        ++c[u];
      }
      items[k].nelem = keep.nelem + 1;
      if (gh_pmask_from_counts(counts, items, nt, masks, sizes) != GH_E_ARG) FAIL("a wrong nelem was accepted");
      items[k] = keep;
      if (gh_pmask_from_counts(counts, items, nt, masks, sizes) != GH_OK) FAIL("the restored list was refused");
    }
    if (gh_pmask_host(nullptr, 0, nullptr, nullptr) != GH_OK || gh_pmask_from_counts(nullptr, nullptr, 0, nullptr, nullptr) != GH_OK)
      FAIL("an empty list was refused");
    // ---- the size formula around the 64-bit header's limits -----------------------------------
    {
      gh_encode_plan plan;
      std::memset(&plan, 0, sizeof(plan));
      const uint64_t lim = 1ull << 31;
      const uint64_t around[] = {lim - 1, lim, lim + 1, 32 * lim - 32, 32 * lim - 31, 128 * lim - 128, 128 * lim - 127, rng() % (256 * lim)};
      plan.bits = around[rng() % 8];
      plan.n = rng() % 2 ? around[rng() % 3] : plan.bits / (1 + rng() % 16);
      plan.nsyms = (uint32_t)(rng() % 257);
      if (gh::plan_sizes(&plan, 0) != GH_OK) FAIL("plan_sizes");
      if (gh::pmask_file_bytes(plan.bits, plan.nsyms, plan.n) != plan.file_bytes)
        FAIL("pmask_file_bytes(%llu, %u, %llu)", (unsigned long long)plan.bits, plan.nsyms, (unsigned long long)plan.n);
    }
    for (uint8_t* b : blocks) std::free(b);
    std::free(counts);
    std::free(sizes);
    std::free(masks);
    std::free(items);
  }
  if (!coded_seen || !stored_seen) FAIL("the lists never took both decisions");
  std::printf("pmask_fuzz: %ld iterations ok (%llu tensors, %llu planes coded, %llu stored)\n", iters, tensors_seen, coded_seen,
              stored_seen);
  return 0;
}
