// Batched gather (gaphuff.h, "batched gather"), included by gh_decode.hip after gh_batch.hip.
// No reference counterpart.
//
// Byte ranges (stream, lo, hi) of a resident batch.  The count and scan kernels of a decode
// (gh_batch.hip) leave seg_cnt (codewords per segment) and unit_off (exclusive scan of the
// codewords per unit) on the device: a seek index of stride 2^8 for every stream.  The
// plan over it is cut by three kernels, the per-range arithmetic being gh_batch_range.hpp's:
//
//   gh_bgplan_locate_kernel  one thread per range: validate, binary-search the stream's
//                            units, write {first unit, pieces, bytes}; count the ranges on
//                            flagged streams (they keep their bytes and get no pieces);
//   gh_gplan_scan_kernel     (gh_gather_plan.hip, as it is) one workgroup: every range's
//                            first piece slot and first output byte, and whether the plan
//                            stands; the published piece count is 0 when it does not;
//   gh_bgplan_emit_kernel    one thread per piece.
//
// gh_batch_gather_kernel<FB> then decodes the pieces: 256 threads, four waves, each wave
// with its own table region in the LDS (BA_REGION), no workgroup barrier and no wave waiting
// for another.  A wave takes a contiguous run of the pieces (unit_run over the published
// count), finds a piece's stream by unit_stream_of on its unit and reloads its tables only
// when the stream changes.  Per piece each lane reads its four seg_cnt bytes; a wave scan
// gives every segment its first position s0 inside the unit; a segment whose [s0, s0 + cnt)
// meets [a, b) walks its first min(cnt, b - s0) codewords and stores symbol k to
// out[dst + s0 + k - a] when s0 + k >= a (plain byte stores).  A chain (64 consecutive
// segments) none of whose segments takes part is not loaded and not walked.  The loop is the
// write kernel's: at most 160 rounds, left by __any(more).
//
// Bounds: the piece loop by the published count, the stream search by nstreams, the walk by
// 160; batch_segment clamps its loads to the stream's own padded extents; a store lands in
// [dst, dst + b - a) of its piece, and the scan has checked the pieces' bytes against dst_len.

struct BgplanParams {
  const gh_brange* ranges;
  const BatchDesc* desc;
  const uint32_t* unit0;
  const unsigned long long* unit_off;
  const unsigned int* stream_status;  // the decode's per-stream status words
  RangeLoc* loc;
  const uint32_t* slot;
  const unsigned long long* dst0;
  gh_gather_piece* pieces;
  unsigned int* status;       // this gather's GH_ST_* word
  const unsigned int* npieces;
  unsigned int* bad_ranges;   // zeroed before the locate kernel
  uint64_t cap;
  uint32_t nranges, nstreams;
};

__global__ __launch_bounds__(GP_TB) void gh_bgplan_locate_kernel(const BgplanParams p) {
  const unsigned long long i = (unsigned long long)blockIdx.x * GP_TB + threadIdx.x;
  if (i >= p.nranges) return;
  bool flagged;
  p.loc[i] = br_locate(
      p.unit0, (const uint64_t*)p.unit_off, [&](uint32_t s) { return (uint64_t)p.desc[s].n; },
      [&](uint32_t s) { return p.stream_status[s]; }, p.nstreams, p.ranges[i], &flagged);
  if (flagged) atomicAdd(p.bad_ranges, 1u);
}

__global__ __launch_bounds__(GP_TB) void gh_bgplan_emit_kernel(const BgplanParams p) {
  const unsigned long long np = *p.npieces;  // 0: the plan does not stand
  const unsigned long long nt = (unsigned long long)gridDim.x * GP_TB;
  for (unsigned long long q = (unsigned long long)blockIdx.x * GP_TB + threadIdx.x; q < np; q += nt) {
    if (q >= p.cap) {  // (the scan publishes no count above cap: never expected)
      atomicOr(p.status, (unsigned)GH_ST_PIECES);
      break;
    }
    const uint32_t a = gr_piece_range(p.slot, p.nranges, q);
    p.pieces[q] = br_piece(p.unit0, (const uint64_t*)p.unit_off, p.ranges[a], p.loc[a], q - p.slot[a], p.dst0[a]);
  }
}

struct BatchGatherParams {
  BatchParams bp;  // out: the gather's destination
  const gh_gather_piece* pieces;
  const unsigned int* d_npieces;
};

template <bool FB>
__global__ __launch_bounds__(BA_TB) void gh_batch_gather_kernel(const BatchGatherParams gp) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[(BA_TB / 64) * BA_REGION];
  const BatchParams& bp = gp.bp;
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* region = smem + wid * BA_REGION;
  const uint32_t* s_fb = (const uint32_t*)region;
  const uint32_t* s_lut = (const uint32_t*)(region + FB_BYTES);
  const uint32_t np = (uint32_t)__builtin_amdgcn_readfirstlane((int)*gp.d_npieces);
  uint32_t q0, q1;
  unit_run<BA_TB / 64>(np, wid, q0, q1);
  BatchUnit un;
  for (uint32_t q = q0; q < q1; ++q) {
    const gh_gather_piece pc = gp.pieces[q];
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc.block);
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc.a);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc.b);
    const unsigned long long dst = rfl_u64(pc.dst);
    if (a >= b || u >= bp.nunits) continue;  // a unit without symbols; (no plan names a unit past the batch)
    // pieces come in request order: the next one may lie in any stream, before or after
    if (un.c.s == 0xFFFFFFFFu || u < un.c.first || u >= un.c.end) un.c.s = 0xFFFFFFFFu;
    batch_enter(bp, u, un, region, lane);
    uint32_t cc[BA_U], s0[BA_U], act = 0, at = 0;
#pragma unroll
    for (int c = 0; c < BA_U; ++c) {
      const uint32_t seg = un.c.blk * (uint32_t)(64 * BA_U) + (uint32_t)(64 * c + lane);
      cc[c] = seg < un.d.nseg ? bp.seg_cnt[(unsigned long long)u * (64 * BA_U) + (uint32_t)(64 * c + lane)] : 0u;
      const uint32_t incl = wave_incl_scan(cc[c]);
      s0[c] = at + (incl - cc[c]);  // the segment's first position inside the unit
      at += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      if (__any(s0[c] < b && s0[c] + cc[c] > a)) act |= 1u << c;
    }
    Win v[BA_U];
    uint32_t off[BA_U], k[BA_U], kbeg[BA_U], kend[BA_U];
    unsigned long long base[BA_U];
#pragma unroll
    for (int c = 0; c < BA_U; ++c) {
      off[c] = 0;
      k[c] = 0;
      kbeg[c] = kend[c] = 0;
      base[c] = 0;
      if (act & (1u << c)) {  // (wave-uniform)
        int R;
        v[c] = batch_segment(bp, un, c, lane, R);
        const bool part = s0[c] < b && s0[c] + cc[c] > a;
        kend[c] = part ? min(cc[c], b - s0[c]) : 0u;
        kbeg[c] = a > s0[c] ? a - s0[c] : 0u;
        base[c] = dst + s0[c] - a;  // symbol k goes to base + k; used for k >= kbeg only, where it is >= dst
      }
    }
    for (int it = 0; it < 160; ++it) {
      bool more = false;
#pragma unroll
      for (int c = 0; c < BA_U; ++c) {
        if (act & (1u << c)) {
          uint32_t bad = 0;  // (flagged by the count pass where it matters)
          const uint32_t e = batch_lookup<FB>(v[c], off[c], s_lut, s_fb, un.d, bad);
          if (k[c] >= kbeg[c] && k[c] < kend[c]) bp.out[base[c] + k[c]] = (uint8_t)(e >> 8);
          ++k[c];
          batch_advance(v[c], off[c], e & 31u);
          more |= k[c] < kend[c];
        }
      }
      if (!__any(more)) break;
    }
  }
}
