// Batched load of gap-less (raw) streams (gaphuff.h, "batched gap-less decode"), included by
// gh_decode.hip after gh_batch.hip.  No reference counterpart.  The gap array of every stream
// of a batch is built on the device, exactly, by a scan of segment transition functions
// (gh_raw_trans.hpp): no speculation, no verify/repair loop, no read-back.
//
//   gh_batchraw_trans_kernel  per unit of 256 segments: T_j of every segment (16 lanes per
//                             segment, lane = the walk's start bit x; four segments per wave
//                             step), stored 8 bytes per segment, and the unit's aggregate
//                             A_u = T_last o ... o T_first;
//   gh_batchraw_chain_kernel  per stream: entry[first unit + k + 1] = A_k(entry[first unit + k]),
//                             entry[first unit] = 0; a wave takes a stream and compose-scans
//                             64 aggregates per step;
//   gh_batchraw_apply_kernel  per unit: compose-scan of the stored T_j applied to the unit's
//                             entry; gap nibble j = e_{j+1}, 0 for j >= G - 1; the unit's gap
//                             words are stored whole.
//
// The trans and apply kernels walk the batch's units as the count and write kernels do
// (unit_run, batch_enter: no wave waits for another, no workgroup barrier); the table kernel
// must have run.  A walk from x reads bits [128 j + x, 128 j + 160): the five words
// batch_segment loads, inside the stream's own 4 G + 4 word extent.

constexpr uint32_t BR_T_BYTES = 8u * BATCH_UNIT_SEGS;  // a unit's T_j: in the scratch and staged in the LDS
constexpr uint32_t BR_CHAIN_TB = 256;
static_assert(BA_REGION % 16 == 0, "the staged T_j start 16-byte aligned");
static_assert((BA_TB / 64) * (BA_REGION + BR_T_BYTES) <= 64 * 1024, "table regions and staged T_j fit the LDS");

// OR over the 16 lanes of a DPP row, to every lane of the row: row_ror 1, 2, 4, 8.
__device__ __forceinline__ uint32_t row_or16(uint32_t v) {
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);
  return v;
}

// Inclusive wave scan under trans_compose (not commutative: lane i gets f_i o ... o f_0).
__device__ __forceinline__ unsigned long long wave_compose_scan(unsigned long long f, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long before = __shfl_up(f, d, 64);
    if (lane >= d) f = trans_compose(before, f);
  }
  return f;
}

__device__ __forceinline__ unsigned long long lane_u64(unsigned long long v, int src) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

// The four consecutive functions a lane holds, composed in segment order.
__device__ __forceinline__ unsigned long long compose4(const unsigned long long (&t)[4]) {
  return trans_compose(trans_compose(trans_compose(t[0], t[1]), t[2]), t[3]);
}

template <bool FB>
__global__ __launch_bounds__(BA_TB) void gh_batchraw_trans_kernel(const BatchParams bp, unsigned long long* trans,
                                                                   unsigned long long* agg) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[(BA_TB / 64) * (BA_REGION + BR_T_BYTES)];
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* region = smem + wid * BA_REGION;
  const uint32_t* s_fb = (const uint32_t*)region;
  const uint32_t* s_lut = (const uint32_t*)(region + FB_BYTES);
  unsigned long long* s_t = (unsigned long long*)(smem + (BA_TB / 64) * BA_REGION + wid * BR_T_BYTES);
  const uint32_t x = (uint32_t)lane & 15u, row = (uint32_t)lane >> 4;
  uint32_t u0, u1;
  unit_run<BA_TB / 64>(bp.nunits, wid, u0, u1);
  BatchUnit un;
  for (uint32_t u = u0; u < u1; ++u) {
    batch_enter(bp, u, un, region, lane);
    const BatchDesc& d = un.d;
    const uint32_t seg0 = un.c.blk * BATCH_UNIT_SEGS;
    for (uint32_t step = 0; step < BATCH_UNIT_SEGS / 4; ++step) {
      const uint32_t k = 4u * step + row;  // segment of the unit
      const uint32_t seg = seg0 + k, sc = min(seg, d.nseg - 1u);  // (loads clamped, never skipped)
      const uint32_t* pay = bp.payload + d.pay_off + 4ull * sc;
      const uint4 w = ws_ld16(pay);
      Win v = make_win(w, pay[4], (int)x);
      uint32_t off = 0;
      const uint32_t t = trans_walk(x, [&]() {
        uint32_t bad = 0;  // (patterns outside the code are the count kernel's to flag)
        const uint32_t len = batch_lookup<FB>(v, off, s_lut, s_fb, d, bad) & 31u;
        batch_advance(v, off, len);
        return len;
      });
      const unsigned long long nib = trans_nibble(x, t);
      const unsigned long long f = ((unsigned long long)row_or16((uint32_t)(nib >> 32)) << 32) | row_or16((uint32_t)nib);
      if (x == 0) s_t[k] = seg < d.nseg ? f : TRANS_IDENTITY;
    }
    __builtin_amdgcn_wave_barrier();  // (one wave's LDS operations complete in order)
    // lane l: segments 4 l .. 4 l + 3 of the unit, to the scratch and into the unit's aggregate
    unsigned long long t4[4];
    unsigned long long* g = trans + (unsigned long long)u * BATCH_UNIT_SEGS + 4 * lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = t4[q] = s_t[4 * lane + q];
    const unsigned long long all = wave_compose_scan(compose4(t4), lane);
    if (lane == 63) agg[u] = all;
    __builtin_amdgcn_wave_barrier();  // the next unit's stores follow these reads
  }
}

// One wave per stream (grid-strided): the entry of every unit after the stream's first.
__global__ __launch_bounds__(BR_CHAIN_TB) void gh_batchraw_chain_kernel(const uint32_t* unit0, uint32_t nstreams,
                                                                         const unsigned long long* agg, uint32_t* entry) {
  const int lane = threadIdx.x & 63;
  const uint32_t nw = gridDim.x * (BR_CHAIN_TB / 64), gw = blockIdx.x * (BR_CHAIN_TB / 64) + (threadIdx.x >> 6);
  for (uint32_t s = gw; s < nstreams; s += nw) {
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)unit0[s]);
    const uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)unit0[s + 1]);
    if (end - first < 2u) continue;  // no unit, or one: its entry is the stream's first bit
    uint32_t e = 0;                  // entry of unit `at`
    for (uint32_t at = first; at + 1u < end; at += 64u) {
      const uint32_t i = at + (uint32_t)lane;
      const unsigned long long f = wave_compose_scan(i + 1u < end ? agg[i] : TRANS_IDENTITY, lane);
      if (i + 1u < end) entry[i + 1u] = trans_apply(f, e);
      e = trans_apply(lane_u64(f, 63), e);
    }
  }
}

// Per unit: the gap words of its 256 segments from the stored T_j and the unit's entry.
__global__ __launch_bounds__(BA_TB) void gh_batchraw_apply_kernel(const BatchParams bp, const unsigned long long* trans,
                                                                   const uint32_t* entry, uint32_t* gaps) {
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t u0, u1;
  unit_run<BA_TB / 64>(bp.nunits, wid, u0, u1);
  UnitCursor c;
  uint32_t nseg = 0;
  unsigned long long gap_off = 0;
  for (uint32_t u = u0; u < u1; ++u) {
    if (unit_enter(bp.unit0, bp.nstreams, u, c)) {
      nseg = (uint32_t)__builtin_amdgcn_readfirstlane((int)bp.desc[c.s].nseg);
      gap_off = rfl_u64(bp.desc[c.s].gap_off);
    }
    const unsigned long long* g = trans + (unsigned long long)u * BATCH_UNIT_SEGS + 4 * lane;
    const unsigned long long t4[4] = {g[0], g[1], g[2], g[3]};
    const unsigned long long incl = wave_compose_scan(compose4(t4), lane);
    const unsigned long long before = __shfl_up(incl, 1, 64);
    const uint32_t e0 = c.blk == 0 ? 0u : entry[u];  // (wave-uniform)
    uint32_t e = lane == 0 ? e0 : trans_apply(before, e0);
    // nibble j holds e_{j+1}; the stream's last nibble and the tail of its last word hold 0
    const uint32_t j0 = c.blk * BATCH_UNIT_SEGS + 4u * (uint32_t)lane;
    uint32_t h = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      e = trans_apply(t4[q], e);
      h |= (j0 + q + 1u < nseg ? e : 0u) << (4u * q);
    }
    const uint32_t hi = (uint32_t)__shfl_down((int)h, 1, 64);
    const uint32_t wi = c.blk * (BATCH_UNIT_SEGS / 8u) + ((uint32_t)lane >> 1);  // gap word of the stream
    if ((lane & 1) == 0 && wi < (nseg + 7u) / 8u) gaps[gap_off + wi] = h | (hi << 16);
  }
}
