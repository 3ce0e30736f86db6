// Batched range gather (gaphuff.h, "random access"), included by gh_decode.hip after
// gh_index.hip.  No reference counterpart: the reference decodes whole streams only.
//
// offsets[k] of the seek index is the output position of index block k's first symbol, so
// an index block decodes on its own.  The host planner (gh_gather_plan, gh_core.cpp) cuts
// a batch of byte ranges into pieces {dst, block, a, b}: decode index block `block`, keep
// the symbols at positions [a, b) of the block, store them at out[dst ...].  A wave owns
// whole pieces w, w + nwaves, ...; no wave waits for another, and there is no workgroup
// barrier after the table load.
//
// Per piece the wave walks the block's wave blocks (256 segments: 4 chains of 64 lanes) in
// order with a running symbol position `pos`:
//   * every wave block is counted exactly as by gh_index_count_kernel (the count table in
//     LDS, GL lookups per window shift, the canonical fallback FB), and a DPP scan of the
//     counts gives every segment its position;
//   * a wave block that ends at or before a only advances pos (count rate);
//   * any other is decoded a second time from the words still in registers, one codeword
//     per lookup of a single-symbol table {len | symbol << 8} (an entry without a
//     codeword: the canonical fallback, whose result has the same layout), and symbol s is
//     stored to out[dst + s - a] when a <= s < b: plain byte stores (the gather is bound
//     by latency, not by store bandwidth).  A lane stops at the last symbol it keeps;
//   * the walk stops once pos >= b.  A walk that runs out of segments before b flags
//     GH_ST_BADCODE (the index is another stream's): no byte is left undecoded silently.
// first_start, last_end and the padding symbols past N need no rule of their own: the
// planner asks for no position at or past N, so the clip at b covers them.
//
// gp.w carries the stream, the count table (lut, kbits, lut_bytes) and the fallback
// tables as IdxParams.w does, and the gather's output buffer in `out`.  The piece count is
// gp.npieces, or *gp.d_npieces when the plan was built on the device (gh_gather_plan.hip).

struct GatherParams {
  WsParams w;
  const gh_gather_piece* pieces;
  const uint32_t* sym_lut;  // 1 << sym_bits entries {len | symbol << 8}; 0: no codeword of <= sym_bits bits
  uint32_t npieces;
  const uint32_t* d_npieces;  // non-null: the piece count lies in device memory (the device plan's)
  uint32_t log2_stride;     // log2 segments per index block, >= 8
  uint32_t sym_bits;        // 2 .. 12
};

constexpr int GA_U = 4;     // chains per lane: a wave block is 256 segments, the smallest stride
constexpr int GA_TB = 256;  // threads per workgroup

template <int U, int TBK, int GL, bool FB = false>
__global__ __launch_bounds__(TBK) void gh_gather_kernel(const GatherParams gp) {
  static_assert(!FB || GL <= 2, "fallback lookups take up to 16 bits: two per window shift");
  static_assert(64 * U == 256, "an index block (>= 256 segments) is a whole number of wave blocks");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const WsParams& p = gp.w;
  const int tid = threadIdx.x, lane = tid & 63;
  // index bits -> byte offset of a u32 entry (the e-window's S without FB)
  const uint32_t sh = 30u - p.kbits;
  const uint32_t amask = ((1u << p.kbits) - 1u) << 2;
  // LDS: count table, symbol table, fallback tables
  const uint32_t sym0 = p.lut_bytes, sym_bytes = 4u << gp.sym_bits, ssh = 32u - gp.sym_bits;
  uint32_t* s_fb = (uint32_t*)(smem + sym0 + sym_bytes);
  uint32_t bad = 0;
  ws_lut_to_lds<TBK>(p, smem, tid);
  for (uint32_t i = tid; i < sym_bytes / 16; i += TBK) ((uint4*)(smem + sym0))[i] = ((const uint4*)gp.sym_lut)[i];
  if constexpr (FB) ws_fb_to_lds<TBK>(p, s_fb, tid);
  check_lds_base(smem, p.status);
  __syncthreads();
  const uint32_t nw = gridDim.x * (uint32_t)(TBK / 64);
  // (the grid of a device-planned gather is sized by a bound: a wave may find no piece)
  const uint32_t npieces = gp.d_npieces ? (uint32_t)__builtin_amdgcn_readfirstlane((int)*gp.d_npieces) : gp.npieces;
  const uint32_t nb = (p.nseg + 64 * U - 1) / (64 * U);  // wave blocks of the stream
  const uint32_t bpi = 1u << (gp.log2_stride - 8u);      // wave blocks per index block
  uint4 w[U];
  uint32_t w4[U], ga[U], gb[U];
  uint32_t have = 0xFFFFFFFFu;  // the wave block whose words w holds (wave-uniform)
  bool cut = false;             // a walk ran out of segments before its b
  for (unsigned long long i = blockIdx.x * (uint32_t)(TBK / 64) + (uint32_t)(tid >> 6); i < npieces; i += nw) {
    const gh_gather_piece pc = gp.pieces[i];
    const uint32_t pa = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc.a);
    const uint32_t pb = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc.b);
    const uint32_t kb = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc.block);
    const unsigned long long dst = rfl_u64(pc.dst);
    // the first wave block of the wave's next piece (prefetched behind this piece's last)
    uint32_t nxt = kb;
    if (i + nw < npieces) nxt = (uint32_t)__builtin_amdgcn_readfirstlane((int)gp.pieces[i + nw].block);
    const uint32_t nxt0 = (uint32_t)min((unsigned long long)nxt * bpi, (unsigned long long)(nb - 1u));
    if ((unsigned long long)kb * bpi >= nb) {  // no such block in this stream
      cut = true;
      continue;
    }
    const uint32_t b0 = kb * bpi, b1 = min(b0 + bpi, nb);
    uint32_t pos = 0;  // symbols of the index block before wave block blk (< 143 * 2^20)
    for (uint32_t blk = b0; blk < b1 && pos < pb; ++blk) {
      if (have != blk) ws_load<U>(p, blk, lane, w, w4, ga, gb);
      uint4 wc[U];
      uint32_t w4c[U];
      Win v[U];
      int R[U], start[U];
      uint32_t cnt[U];
      bool act[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t seg = blk * (uint32_t)(64 * U) + (uint32_t)(64 * u + lane);
        act[u] = seg < p.nseg;
        start[u] = seg == 0 ? (int)p.first_start : (int)gap_nib(ga[u], p.gap_nib0 + seg - 1u);
        const int E = (p.last_end && seg == p.nseg - 1u) ? (int)p.last_end
                                                         : 128 + (int)gap_nib(gb[u], p.gap_nib0 + seg);
        wc[u] = w[u];
        w4c[u] = w4[u];
        v[u] = FB ? make_win(wc[u], w4c[u], start[u]) : make_ewin(wc[u], w4c[u], start[u], sh);
        R[u] = act[u] ? E - start[u] : 0;
        cnt[u] = 0;
      }
      // prefetch the wave's next wave block: the next of this index block, else the first
      // of its next piece (always issued, clamped: a fixed load count)
      have = blk + 1 < b1 ? blk + 1 : nxt0;
      ws_load<U>(p, have, lane, w, w4, ga, gb);
      // ---- count (as gh_index_count_kernel) ----
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
      // ---- positions: chain u's segments follow chain u-1's ----
      uint32_t s0[U], cc[U], total = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        cc[u] = act[u] ? cnt[u] : 0u;
        const uint32_t incl = wave_incl_scan(cc[u]);
        s0[u] = pos + total + (incl - cc[u]);
        total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      }
      if (pos + total > pa) {
        // ---- decode again: the symbols k of each segment with pa <= s0 + k < pb ----
        uint32_t k[U], kend[U], off[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          v[u] = make_win(wc[u], w4c[u], start[u]);
          kend[u] = (s0[u] < pb && s0[u] + cc[u] > pa) ? min(cc[u], pb - s0[u]) : 0u;
          k[u] = 0;
          off[u] = 0;  // bits of d0 consumed (0..31)
        }
        for (int it = 0; it < 160; ++it) {  // (a segment holds at most 143 codewords)
          uint32_t e[U], xs[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            xs[u] = (uint32_t)(((((unsigned long long)v[u].d0) << 32) | v[u].d1) >> (32u - off[u]));
            e[u] = lds_u32_nowait(sym0 + ((xs[u] >> ssh) << 2));
          }
          lds_wait(e);
          bool more = false;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if constexpr (FB) {
              if ((e[u] & 31u) == 0u) {  // (flagged by the count above where it matters)
                uint32_t b = 0;
                e[u] = ws_canon(s_fb, xs[u] >> 16, p.fb_lo, p.fb_hi, b);  // (symbol << 8) | length
              }
            }
            const uint32_t s = s0[u] + k[u];
            if (k[u] < kend[u] && s >= pa) p.out[dst + (unsigned long long)(s - pa)] = (uint8_t)(e[u] >> 8);
            ++k[u];
            off[u] += e[u] & 31u;
            if (off[u] >= 32u) {
              v[u].d0 = v[u].d1;
              v[u].d1 = v[u].d2;
              v[u].d2 = v[u].d3;
              v[u].d3 = v[u].d4;
              v[u].d4 = 0u;
              off[u] -= 32u;
            }
            more |= k[u] < kend[u];
          }
          if (!__any(more)) break;
        }
      }
      pos += total;
    }
    cut |= pos < pb;
  }
  if (__any(bad != 0 || cut) && lane == 0) atomicOr(p.status, (unsigned)GH_ST_BADCODE);
}
