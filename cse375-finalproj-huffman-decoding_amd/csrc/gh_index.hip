// Seek-index build (gaphuff.h, "random access"), included by gh_decode.hip after
// gh_wsplit.hip.  No reference counterpart: the reference decodes whole streams only.
//
// The index holds one output offset per index block of 2^k segments (k >= 8): the number
// of codewords that start before the block.  A segment's codewords (those starting in
// [128i + gap[i-1], 128(i+1)), gh_wsplit.hip) are counted exactly as by
// gh_ws_count_kernel: the count table of gh_lut.hpp in LDS, U = 4 chains of 64 lanes,
// GL lookups per window shift, the canonical fallback (FB) for codes longer than the
// table and for incomplete codes.  What differs is the work split and the output: a wave
// owns whole index blocks w, w + nwaves, ..., walks a block's 2^k / 256 wave blocks with
// the next one's loads in flight, and stores one 64-bit count per index block.  No
// per-segment byte is written and no ranges are cut; the scan of the block counts to
// offsets runs on the host (the offsets end up there anyway).
//
// p.w carries the stream (payload, gaps, nseg, gap_nib0, first_start, last_end), the
// table (lut, kbits, lut_bytes; one copy in LDS) and the fallback tables; its range and
// output fields are unused.

struct IdxParams {
  WsParams w;
  unsigned long long* counts;  // codewords per index block
  uint32_t nblocks;            // index blocks = ceil(nseg >> log2_stride)
  uint32_t log2_stride;        // log2 segments per index block, >= 8
};

constexpr int IDX_U = 4;     // chains per lane: a wave block is 256 segments, the smallest stride
constexpr int IDX_TB = 256;  // threads per workgroup

template <int U, int TBK, int GL, bool FB = false>
__global__ __launch_bounds__(TBK) void gh_index_count_kernel(const IdxParams ip) {
  static_assert(!FB || GL <= 2, "fallback lookups take up to 16 bits: two per window shift");
  static_assert(64 * U == 256, "an index block (>= 256 segments) is a whole number of wave blocks");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const WsParams& p = ip.w;
  const int tid = threadIdx.x, lane = tid & 63;
  // index bits -> byte offset of a u32 entry (the e-window's S without FB)
  const uint32_t sh = 30u - p.kbits;
  const uint32_t amask = ((1u << p.kbits) - 1u) << 2;
  uint32_t* s_fb = (uint32_t*)(smem + p.lut_bytes);
  uint32_t bad = 0;
  ws_lut_to_lds<TBK>(p, smem, tid);
  if constexpr (FB) ws_fb_to_lds<TBK>(p, s_fb, tid);
  check_lds_base(smem, p.status);
  __syncthreads();
  const uint32_t nw = gridDim.x * (uint32_t)(TBK / 64);
  const uint32_t nb = (p.nseg + 64 * U - 1) / (64 * U);  // wave blocks of the stream
  const uint32_t bpi = 1u << (ip.log2_stride - 8u);      // wave blocks per index block
  uint4 w[U];
  uint32_t w4[U], ga[U], gb[U];
  const uint32_t ib0 = blockIdx.x * (uint32_t)(TBK / 64) + (uint32_t)(tid >> 6);
  // (index block ib < nblocks starts at wave block ib * bpi < nb: never empty)
  if (ib0 < ip.nblocks) ws_load<U>(p, ib0 * bpi, lane, w, w4, ga, gb);
  for (uint32_t ib = ib0; ib < ip.nblocks; ib += nw) {
    const uint32_t b0 = ib * bpi, b1 = min(b0 + bpi, nb);
    uint32_t tot = 0;  // per lane: at most 2^12 wave blocks x 4 chains x 144 codewords
    for (uint32_t blk = b0; blk < b1; ++blk) {
      Win v[U];
      int R[U];
      uint32_t cnt[U];
      bool act[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t seg = blk * (uint32_t)(64 * U) + (uint32_t)(64 * u + lane);
        act[u] = seg < p.nseg;
        const int start = seg == 0 ? (int)p.first_start : (int)gap_nib(ga[u], p.gap_nib0 + seg - 1u);
        const int E = (p.last_end && seg == p.nseg - 1u) ? (int)p.last_end
                                                         : 128 + (int)gap_nib(gb[u], p.gap_nib0 + seg);
        v[u] = FB ? make_win(w[u], w4[u], start) : make_ewin(w[u], w4[u], start, sh);
        R[u] = act[u] ? E - start : 0;
        cnt[u] = 0;
      }
      // prefetch the wave's next wave block: the next of this index block, else the first
      // of its next index block (always issued, clamped: a fixed load count)
      ws_load<U>(p, blk + 1 < b1 ? blk + 1 : min((ib + nw) * bpi, nb - 1), lane, w, w4, ga, gb);
      for (int g = 0; g < 160; ++g) {
        uint32_t rm[U], q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          rm[u] = ws_rmask<FB>(R[u]);
          q[u] = 0u;
        }
#pragma unroll
        for (int j = 0; j < GL; ++j) {
          uint32_t e[U], xs[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const uint32_t x = j == 0 ? v[u].d0 : __builtin_amdgcn_alignbit(v[u].d0, v[u].d1, q[u]);
            xs[u] = x;
            e[u] = lds_u32_nowait(FB ? (x >> sh) & amask : x & amask);
          }
          lds_wait(e);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if constexpr (FB) {
              if ((e[u] & 0xFFFFu) == 0u) {
                // only a lookup that starts before the segment end may flag the stream
                uint32_t b = 0;
                const uint32_t l = ws_canon(s_fb, xs[u] >> 16, p.fb_lo, p.fb_hi, b) & 31u;
                bad |= ((int)(0u - q[u]) < R[u]) ? b : 0u;
                e[u] = l | ((1u << (l - 1u)) << 16);
              }
            }
            // cnt += popcount(end mask & rm); rm >>= b; q -= b  (as gh_ws_count_kernel)
            uint32_t m;
            asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD"
                : "=v"(m) : "v"(e[u]), "v"(rm[u]));
            cnt[u] = __builtin_popcount(m) + cnt[u];
            asm("v_ashrrev_i32 %0, %1, %0" : "+v"(rm[u]) : "v"(e[u]));
            asm("v_sub_u32_sdwa %0, %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
                : "+v"(q[u]) : "v"(e[u]));
          }
        }
        bool more = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          win_shift(v[u], q[u]);  // q = -consumed (1..31 bits): v_alignbit reads q & 31 = 32 - consumed
          R[u] += (int)q[u];
          more |= R[u] > 0;
        }
        if (!__any(more)) break;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) tot += act[u] ? cnt[u] : 0u;
    }
    const unsigned long long t64 = wave_sum_u64(tot);
    if (lane == 0) ip.counts[ib] = t64;
  }
  if (FB && __any(bad != 0) && lane == 0) atomicOr(p.status, (unsigned)GH_ST_BADCODE);
}
