// Plane choice (gaphuff.h, "plane choice"), included by gh_encode.hip after gh_planes_split.hip:
// the two kernels of gh_pmask_device.  Between them runs gh_ebatch_code_kernel (gh_ebatch.hip),
// as it is, on the counts the first one leaves.  No reference counterpart.
//
//   gh_pmask_hist_kernel    the byte histogram of every plane of every tensor, straight from
//                           the tensors: counts[q][256] u64 in candidate order (gh_pmask.hpp).
//   gh_pmask_decide_kernel  one thread per candidate plane: the image's size from the code
//                           kernel's record (bits, nsyms) and the coded / stored decision, both
//                           by gh_pmask.hpp.
//
// The histogram's unit of work is the split kernel's: PLANES_UNIT_ELEMS = 1024 consecutive
// elements of one tensor, unit0[0 .. ntensors] the prefix of the tensors' unit counts, the walk
// gh_units.hpp's.  Lane l owns elements [16 l, 16 l + 16) and makes E 16-byte loads
// (planes_tensor_load, gh_planes_split.hip: a tensor whose pointer is not 16-byte aligned, and
// the lane that straddles nelem, load byte by byte under the scalar bound, so exactly nelem * E
// bytes of a tensor are read).  E divides 16, so byte k of any of those loads belongs to plane
// k & (E - 1): the plain variant counts the bytes where they are, without a transpose.
//
// Counters: the wave's own LDS region of 8 x 256 u32 (8 KiB, 32 KiB per workgroup) holds 8 / E
// replicas of the tensor's E x 256 counters; lane l counts into replica l & (8 / E - 1), so the
// lanes that meet on a hot bin are 64 E / 8 and not 64.  The replicas are summed as they are
// flushed with u64 global atomics into counts[(q0 + p) * 256 + sym], when the wave's run leaves
// the tensor and after PM_FLUSH_UNITS units (a unit adds at most 1024 to a counter).
// No wave waits for another and there is no barrier; every loop is bounded by counts the host
// knows.
//
// Hot bins.  An all-zero plane sends all 16 atomics of all 64 lanes to one LDS address.  The
// MERGE variant transposes the lane's group (planes_split16) and, when the 16 bytes a lane holds
// of a plane are all equal, issues one atomic of 16 in place of 16 atomics of 1; other groups
// count byte by byte.  Which variant runs by default was decided by measurement (DESIGN.md,
// "Plane choice"); GH_PMASK_MERGE=0/1 selects one (tests, scripts/bench_pmask.py).

constexpr int PM_TB = 256;  // threads per workgroup: four waves, four counter regions
constexpr int PM_WAVES = PM_TB / 64;
constexpr uint32_t PM_COUNTERS = PLANES_MAX_E * 256;  // per wave
constexpr uint32_t PM_FLUSH_UNITS = 1u << 21;         // counters are u32: flushed every 2^31 elements at the latest
static_assert(PM_WAVES * PM_COUNTERS * 4 <= 32 * 1024, "the waves' counters fit 32 KiB");
static_assert((unsigned long long)PM_FLUSH_UNITS * PLANES_UNIT_ELEMS < (1ull << 32), "a counter cannot overflow between flushes");

// One tensor as the histogram kernel sees it (device memory, 24 bytes).
struct PMaskTensor {
  const uint8_t* data;  // nelem * elem bytes, any alignment
  unsigned long long nelem;
  uint32_t q0, elem;    // its first candidate plane; 1, 2, 4, 8
};
static_assert(sizeof(PMaskTensor) == 24, "PMaskTensor layout");

struct PMaskParams {
  const PMaskTensor* desc;
  const uint32_t* unit0;       // ntensors + 1
  unsigned long long* counts;  // [nplanes][256], zeroed
  uint32_t ntensors, nunits;
};

// The lane's 16 elements of unit blk into its replica of the wave's counters, h[p * 256 + sym].
template <uint32_t E, bool MERGE>
__device__ __forceinline__ void pmask_count_unit(const PMaskTensor& d, uint32_t blk, int lane, uint32_t* hw) {
  uint32_t* h = hw + ((uint32_t)lane & (PLANES_MAX_E / E - 1u)) * (E * 256u);
  const unsigned long long i0 = (unsigned long long)blk * PLANES_UNIT_ELEMS + (uint32_t)lane * PLANES_GROUP;
  const uint32_t rem = i0 >= d.nelem ? 0u : d.nelem - i0 >= PLANES_GROUP ? PLANES_GROUP : (uint32_t)(d.nelem - i0);
  if (!rem) return;
  const bool vec = (((uintptr_t)d.data) & 15u) == 0;
  uint32_t w[4 * E];
  planes_tensor_load<E>(d.data + i0 * E, rem, vec, w);
  if (rem == PLANES_GROUP) {
    if constexpr (MERGE) {
      uint32_t pl[E][4];
      planes_split16<E>(w, pl);
#pragma unroll
      for (uint32_t p = 0; p < E; ++p) {
        const uint32_t x = pl[p][0];
        if (x == pl[p][1] && x == pl[p][2] && x == pl[p][3] && x == (x & 0xFFu) * 0x01010101u) {
          atomicAdd(&h[p * 256u + (x & 0xFFu)], PLANES_GROUP);
        } else {
#pragma unroll
          for (uint32_t k = 0; k < 16; ++k) atomicAdd(&h[p * 256u + ((pl[p][k >> 2] >> (8u * (k & 3u))) & 0xFFu)], 1u);
        }
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 16 * E; ++k)
        atomicAdd(&h[(k & (E - 1u)) * 256u + ((w[k >> 2] >> (8u * (k & 3u))) & 0xFFu)], 1u);
    }
  } else {
    // the lane that straddles nelem: its first rem * E bytes (w is zero past them)
    const uint32_t nb = rem * E;
#pragma unroll
    for (uint32_t k = 0; k < 16 * E; ++k)
      if (k < nb) atomicAdd(&h[(k & (E - 1u)) * 256u + ((w[k >> 2] >> (8u * (k & 3u))) & 0xFFu)], 1u);
  }
}

template <bool MERGE>
__global__ __launch_bounds__(PM_TB) void gh_pmask_hist_kernel(const PMaskParams p) {
  __shared__ uint32_t s_cnt[PM_WAVES][PM_COUNTERS];
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* h = s_cnt[wid];
#pragma unroll
  for (uint32_t k = 0; k < PM_COUNTERS / 64; ++k) h[(uint32_t)lane + 64u * k] = 0;
  ebatch_wave_sync();
  // the wave's counters of tensor d into its planes' global counts, and back to zero
  auto flush = [&](const PMaskTensor& d) {
    ebatch_wave_sync();
    const uint32_t per = 256u * d.elem;  // counters of one replica: i is p * 256 + sym
    for (uint32_t k = 0; k < 4u * d.elem; ++k) {
      const uint32_t i = (uint32_t)lane + 64u * k;
      uint32_t c = 0;
      for (uint32_t r = 0; r < PM_COUNTERS; r += per) {  // (8 / elem replicas)
        c += h[r + i];
        h[r + i] = 0;
      }
      if (c) atomicAdd(&p.counts[256ull * d.q0 + i], (unsigned long long)c);
    }
    ebatch_wave_sync();
  };
  uint32_t u0, u1;
  unit_run<PM_WAVES>(p.nunits, wid, u0, u1);
  UnitCursor c;
  PMaskTensor d{};
  uint32_t since = 0;  // units counted since the last flush
  for (uint32_t u = u0; u < u1; ++u) {
    const bool first = c.s == 0xFFFFFFFFu;
    const bool changed = unit_enter(p.unit0, p.ntensors, u, c);
    if ((changed && !first) || since == PM_FLUSH_UNITS) {
      flush(d);  // (d is still the tensor the counters belong to)
      since = 0;
    }
    if (changed) d = p.desc[c.s];
    switch (d.elem) {  // (wave-uniform)
      case 1: pmask_count_unit<1, MERGE>(d, c.blk, lane, h); break;
      case 2: pmask_count_unit<2, MERGE>(d, c.blk, lane, h); break;
      case 4: pmask_count_unit<4, MERGE>(d, c.blk, lane, h); break;
      default: pmask_count_unit<8, MERGE>(d, c.blk, lane, h); break;
    }
    ++since;
  }
  if (c.s != 0xFFFFFFFFu) flush(d);
}

// out: plane_bytes[8 * ntensors] u64, then masks[ntensors] u32, zeroed with the counts.
__global__ __launch_bounds__(256) void gh_pmask_decide_kernel(const EBatchCodeRec* recs, const PMaskTensor* desc,
                                                               const uint32_t* q0, uint32_t ntensors, uint32_t nplanes,
                                                               unsigned long long* plane_bytes, uint32_t* masks) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= nplanes) return;
  const uint32_t t = pmask_tensor_of(q0, ntensors, q), pl = q - q0[t];
  const unsigned long long nelem = desc[t].nelem;
  if (!nelem) return;
  const unsigned long long fb = pmask_file_bytes(recs[q].bits, recs[q].nsyms, nelem);
  plane_bytes[(unsigned long long)PLANES_MAX_E * t + pl] = fb;
  if (pmask_coded(fb, nelem)) atomicOr(&masks[t], 1u << pl);
}
