// Element gather (gaphuff.h, "element gather"), included by gh_decode.hip after
// gh_planes_join.hip: the kernels of gh_pgather_device around the batched gather, which runs
// between them as it is.  The per-range arithmetic is gh_planes_gather.hpp's, the text the host
// plan and the CPU fuzz program run.  No reference counterpart.
//
//   gh_pgather_locate_kernel  one thread per element range: validate (pg_locate), write what the
//                             range adds to the four sums below, count the ranges on a flagged
//                             tensor, once each.
//   gh_pgather_scan_kernel    ONE workgroup, gh_gplan_scan_kernel's structure (chunks of
//                             PGS_CHUNK ranges with a running carry) over four sums instead of
//                             two: byte ranges (C), staging bytes ((hi - lo) C), destination
//                             bytes ((hi - lo) E) and work units (ceil((hi - lo) / 1024)).
//                             Thread 0 decides whether the plan stands and publishes the totals.
//   gh_pgather_expand_kernel  one thread per element range writes its C byte ranges at its
//                             scanned slot; the slots from the total to the host's bound (the
//                             list's largest C times nranges: the host does not know the total)
//                             get empty ranges.  When the plan does not stand every slot is an
//                             empty range but the first, which has lo > hi: the batched gather
//                             refuses it on its own and writes nothing.
//   gh_pgather_join_kernel    gh_planes_join_kernel's shape: four waves per workgroup, no LDS,
//                             no barrier, no wave waits for another.  A wave takes a contiguous
//                             run of the published units (unit_run), 1024 elements of one range
//                             each; lane l owns 16 of them (pg_join_lane).  On entering a range
//                             it loads the range, its offsets and its tensor and ORs the status
//                             words of the tensor's coded streams: a flagged range is skipped by
//                             every wave.  A non-zero status word of this gather or of the inner
//                             one ends the kernel before its first store.
//
// Bounds: the scan and expand loops by nranges and the host's slot bound; the unit walk by the
// published unit count (at most nranges + dst_len / 1024, which the host checked against 2^31)
// and the range search by nranges; a lane reads bytes [lo, hi) of a plane (16-byte loads only
// where all 16 lie inside) and stores inside [dst_off, dst_off + (hi - lo) E), which the scan
// has checked against dst_len.

constexpr int PGS_TB = 512;  // the scan's one workgroup
constexpr int PGS_ITEMS = 4;  // ranges per thread per chunk
constexpr int PGS_CHUNK = PGS_TB * PGS_ITEMS;

// words: [0] status, [1] byte ranges, [2..3] destination bytes, [4..5] staging bytes,
// [6] ranges on flagged tensors, [7] units, [8] zero (the inner status when there is no inner gather)
struct PgatherParams {
  const gh_erange* ranges;
  const PlanesTensor* desc;
  const unsigned int* stream_status;  // the decode's per-stream status words
  const unsigned int* inner_status;   // the batched gather's status word
  PgLoc* loc;                         // nranges
  gh_brange* branges;                 // nslots
  unsigned long long* stage_off;      // nranges
  unsigned long long* dst_off;        // nranges
  uint32_t* slot;                     // nranges: a range's first byte range
  uint32_t* unit0;                    // nranges + 1
  unsigned int* words;
  const uint8_t* stage;
  const uint8_t* stored;
  uint8_t* dst;
  uint64_t dst_len, nslots;
  uint32_t nranges, ntensors;
};

__global__ __launch_bounds__(GP_TB) void gh_pgather_locate_kernel(const PgatherParams p) {
  const unsigned long long i = (unsigned long long)blockIdx.x * GP_TB + threadIdx.x;
  if (i >= p.nranges) return;
  const PgLoc loc = pg_locate([&](uint32_t t) -> const PlanesTensor& { return p.desc[t]; },
                              [&](uint32_t s) { return p.stream_status[s]; }, p.ntensors, p.ranges[i]);
  p.loc[i] = loc;
  if (loc.flagged) atomicAdd(p.words + 6, 1u);
}

__global__ __launch_bounds__(PGS_TB) void gh_pgather_scan_kernel(const PgatherParams p) {
  __shared__ unsigned long long s_sum[4][PGS_TB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long carry[4] = {0, 0, 0, 0};  // byte ranges, staging bytes, destination bytes, units
  int bad = 0;
  for (unsigned long long base = 0; base < p.nranges; base += PGS_CHUNK) {
    const unsigned long long i0 = base + (unsigned long long)tid * PGS_ITEMS;
    unsigned long long v[PGS_ITEMS][4], t[4] = {0, 0, 0, 0}, incl[4];
#pragma unroll
    for (int u = 0; u < PGS_ITEMS; ++u) {
      v[u][0] = v[u][1] = v[u][2] = v[u][3] = 0;
      if (i0 + u < p.nranges) {
        const PgLoc loc = p.loc[i0 + u];
        if (loc.ncoded == PG_BAD) {
          bad = 1;
        } else {
          v[u][0] = loc.ncoded;
          v[u][1] = loc.stage;
          v[u][2] = loc.dst;
          v[u][3] = loc.units;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] += v[u][k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      incl[k] = wave_incl_scan_u64(t[k], lane);
      if (lane == 63) s_sum[k][wv] = incl[k];
    }
    __syncthreads();
    unsigned long long ex[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned long long before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < PGS_TB / 64; ++w) {
        const unsigned long long s = s_sum[k][w];
        before += w < wv ? s : 0ull;
        all += s;
      }
      ex[k] = carry[k] + before + (incl[k] - t[k]);
      carry[k] += all;
    }
#pragma unroll
    for (int u = 0; u < PGS_ITEMS; ++u) {
      if (i0 + u < p.nranges) {
        p.slot[i0 + u] = (uint32_t)ex[0];  // (below 8 nranges <= 2^24)
        p.stage_off[i0 + u] = ex[1];
        p.dst_off[i0 + u] = ex[2];
        p.unit0[i0 + u] = (uint32_t)ex[3];  // (meaningful when the plan stands: then below 2^31)
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) ex[k] += v[u][k];
    }
    __syncthreads();  // s_sum is rewritten by the next chunk
  }
  const int any_bad = __syncthreads_or(bad);
  if (tid == 0) {
    unsigned int st = 0;
    if (any_bad) st |= GH_ST_RANGE;
    if (carry[2] > p.dst_len) st |= GH_ST_DSTSMALL;
    p.words[0] = st;
    p.words[1] = (unsigned int)carry[0];
    p.words[2] = (unsigned int)carry[2];
    p.words[3] = (unsigned int)(carry[2] >> 32);
    p.words[4] = (unsigned int)carry[1];
    p.words[5] = (unsigned int)(carry[1] >> 32);
    p.words[7] = st ? 0u : (unsigned int)carry[3];
    p.unit0[p.nranges] = st ? 0u : (uint32_t)carry[3];
  }
}

__global__ __launch_bounds__(GP_TB) void gh_pgather_expand_kernel(const PgatherParams p) {
  const unsigned long long i = (unsigned long long)blockIdx.x * GP_TB + threadIdx.x;
  const unsigned long long nt = (unsigned long long)gridDim.x * GP_TB;
  const bool stands = p.words[0] == 0;
  if (stands && i < p.nranges) {
    const gh_erange r = p.ranges[i];
    const PlanesTensor& d = p.desc[r.tensor];  // (valid: the plan stands)
    const unsigned long long at = p.slot[i];
    if (at + pg_popc(d.mask) <= p.nslots) pg_emit(d, r, p.branges + at);  // (always: nslots is the list's largest C times nranges)
  }
  // the slots no range fills: empty ranges of stream 0 (a batch with a slot has a stream)
  for (unsigned long long q = (stands ? (unsigned long long)p.words[1] : 0ull) + i; q < p.nslots; q += nt)
    p.branges[q] = (!stands && q == 0) ? gh_brange{0, 1, 0} : gh_brange{0, 0, 0};
}

template <uint32_t E>
__device__ __forceinline__ void pgather_join_unit(const PgView& v, const PlanesTensor& d, uint32_t blk, int lane) {
  pg_join_lane<E>(v, d, (unsigned long long)blk * PLANES_UNIT_ELEMS + (uint32_t)lane * PLANES_GROUP);
}

__global__ __launch_bounds__(PJ_TB) void gh_pgather_join_kernel(const PgatherParams p) {
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (__builtin_amdgcn_readfirstlane((int)(p.words[0] | *p.inner_status)) != 0) return;  // refused: nothing is written
  const uint32_t nunits = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.words[7]);
  uint32_t u0, u1;
  unit_run<PJ_WAVES>(nunits, wid, u0, u1);
  UnitCursor c;
  PlanesTensor d{};
  PgView v{};
  v.stage = p.stage;
  v.stored = p.stored;
  v.dst = p.dst;
  bool bad = false;
  for (uint32_t u = u0; u < u1; ++u) {
    if (unit_enter(p.unit0, p.nranges, u, c)) {
      const gh_erange r = p.ranges[c.s];
      d = p.desc[r.tensor];
      unsigned int st = 0;
      for (uint32_t q = 0; q < PLANES_MAX_E; ++q)
        if ((d.mask >> q) & 1u) st |= p.stream_status[d.stream[q]];
      bad = __builtin_amdgcn_readfirstlane((int)st) != 0;
      v.lo = rfl_u64(r.lo);
      v.len = rfl_u64(r.hi - r.lo);
      v.stage_off = rfl_u64(p.stage_off[c.s]);
      v.dst_off = rfl_u64(p.dst_off[c.s]);
      v.vec = pg_vec_ok(v.stage_off, v.lo, v.len, (uint64_t)(uintptr_t)p.dst + v.dst_off, pg_popc(d.mask));
    }
    if (bad) continue;  // (counted by the scan)
    switch (d.elem) {  // (wave-uniform)
      case 1: pgather_join_unit<1>(v, d, c.blk, lane); break;
      case 2: pgather_join_unit<2>(v, d, c.blk, lane); break;
      case 4: pgather_join_unit<4>(v, d, c.blk, lane); break;
      default: pgather_join_unit<8>(v, d, c.blk, lane); break;
    }
  }
}
