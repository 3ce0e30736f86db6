// Tile kernel: the decode of grouped codes (complete, 3 <= len <= 12, e.g. BASELINE's
// r = 0.1 and r = 0.5 data), included by gh_decode.hip.  Reference counterpart:
// gpu_dec_l1_l2 (decoder/src/decoder.cu:454-730) — its per-segment count (:529-569),
// decoupled look-back (:571-653) and second decode that writes the bytes (:655-728) — as
// ONE decode pass per segment in one persistent kernel.
//
// 1024-thread workgroups (16 waves), U segments per lane, a tile = U * 1024 consecutive
// segments; wave w of a workgroup owns the 64 * U consecutive segments [64Uw, 64U(w+1))
// of its tile, lane l the segments 64Uw + Ul .. 64Uw + Ul + U - 1 (lane-major,
// GH_TILE_LMAJ; chain u of lane l is segment 64Uw + Ul + u).  Workgroup 0 is the round
// leader; the D = grid - 1 others decode: workgroup b takes tiles b, b + D, b + 2D, ...
// (static round robin; grid <= 2048).  Iteration k of a decoding workgroup, every wave
// on its own (no workgroup barrier after the prologue):
//
//   decode tile k into registers (one codeword per lookup, G codewords per window shift;
//     a codeword is kept iff it starts before the segment end: the reference's rule)
//     - mid-decode: load the global prefix of tile k-LAG
//   copy tile k-LAG out of the wave's staging buffer (its prefix has had LAG-1 iterations
//     to arrive) with a fixed store count, reading aligned 16-byte LDS chunk pairs and
//     shifting them in registers; the next tile's loads are issued just before
//   wave scan of the counts -> the wave's total to LDS, an LDS arrival counter; the last
//     wave to arrive scans the 16 totals and publishes tile k's aggregate
//   stage tile k: every wave writes its own 64U segments into its own buffer; a tile
//     larger than staging waits for its prefix and stores its bytes from registers
//
// The leader takes the rounds (tiles rD .. rD + D - 1) in order: it waits for a round's
// aggregates, scans them and publishes every tile's global exclusive prefix.  The start
// of the next round stays in its registers, so the serial chain of round starts never
// crosses workgroups (rotating the leader role among the decoding workgroups made every
// round pay one cross-workgroup hand-off on that chain: 0.73 vs 0.70 ms on cfg4).
//
// Issue priority by arrival rank: the waves that arrived last at their previous tile gate
// the next aggregate, so they take priority 3, the first arrivals 0.
//
// Known piece offsets: the output offset of every wave's piece is a pure function of the
// loaded shard.  The kernel above (the chained one) records each of them in the plan's
// piece_off table where it copies the piece out.  Once the host has seen such a decode
// finish with status 0, later decodes of the same load run the KNOWN instantiation of the
// same template: no leader (all `grid` workgroups decode), no granules, prefixes, arrival
// counters or polls.  A wave loads its piece's offset and the next one with the tile's
// words, stages the piece at the 16-byte phase of its output offset, so that LDS chunk c is
// output chunk c, and copies it out with one aligned LDS read per chunk.  Its own scanned
// total must equal the difference of the two offsets (GH_ST_OFFSETS otherwise, and nothing
// is written for that piece).  The one thing its waves still share is an LDS word, the
// furthest iteration any of them has reached: a wave issues at the priority of its lag
// behind it (without that the waves drift apart and the kernel is 9 % slower than the
// chained one on cfg4, with it 7 % faster).
//
// The alternatives of the round-3/4 build knobs (copy-out interleaving, batched reads,
// early loads, priority rotations, ...) and of the round-5/6 ones (tiles by ticket with a
// frontier leader, a held tile, a second prefetched tile, a late prefix load, sparser
// polls, paired staging stores, compiler-waited LUT reads, unaligned or DPP-shared
// copy-out reads: DESIGN.md, tile-kernel section, records each measurement) measured
// slower or no better and were removed, as were the C-coded borrow count and the
// per-codeword placement barrier.  Build knobs left: TB, U, LAG, LMAJ (the chain-major
// segment order, for comparison) and KLAG (the known-offsets copy-out's placement).
// Diagnostic builds only: GH_TILE_STAMPS, GH_TILE_ABLATE.

#ifndef GH_TILE_TB
#define GH_TILE_TB 1024
#endif
constexpr int TILE_TB = GH_TILE_TB;  // threads per workgroup
#ifndef GH_TILE_U
#define GH_TILE_U 3
#endif
constexpr int TILE_U = GH_TILE_U;  // segments per lane, codes of >= 4-bit codewords
constexpr int TILE_U3 = 2;    // segments per lane, codes with 3-bit codewords
constexpr int TILE_NS = 4;    // 16-byte stores per lane per copy-out (NS * 64 chunks cover a wave's piece)
constexpr int TILE_SCAP = 20; // staging bytes per segment, codes of >= 4-bit codewords
constexpr int TILE_MIDG = 2;  // decode group after which the prefix of tile k-LAG is loaded (again)
constexpr int STAGE_PAD = 16; // region byte STAGE_PAD + i = piece byte i
#ifndef GH_TILE_LAG
#define GH_TILE_LAG 2
#endif
constexpr int TILE_LAG = GH_TILE_LAG;  // a tile is copied out LAG iterations after it is decoded (LAG buffers)
constexpr int TILE_SLOTS = 16;  // per-tile wave totals / offsets / arrival counters / prefixes in LDS, by k mod 16
#ifndef GH_TILE_STAMPS
#define GH_TILE_STAMPS 0  // diagnostic builds only: per-phase s_memtime deltas of waves 0 and 4
#endif
#if GH_TILE_STAMPS
#define TSTAMP(i) (ts[i] = __builtin_amdgcn_s_memtime())
#else
#define TSTAMP(i) ((void)0)
#endif
#ifndef GH_TILE_LMAJ
#define GH_TILE_LMAJ 1  // lane-major segments: lane l of a wave decodes its segments U*l .. U*l + U - 1
#endif
#ifndef GH_TILE_KLAG
#define GH_TILE_KLAG 0  // known offsets: a piece is copied out in the iteration that stages it (0) or
                        // in the next one, before that one's staging (1); one buffer per wave either way
#endif
constexpr int TILE_KLAG = GH_TILE_KLAG;
static_assert(TILE_KLAG == 0 || TILE_KLAG == 1, "GH_TILE_KLAG: 0 or 1");
#ifndef GH_TILE_ABLATE
#define GH_TILE_ABLATE 0  // diagnostic builds only (make variant), bits: 1 no decode, 2 no staging
                          // stores, 4 no prefix wait (a fake offset), 8 no copy-out, 16 even LUT
                          // entries only (no LUT bank conflicts), 32 pieces copied out to 16-byte
                          // aligned offsets (wrong output)
#endif
typedef unsigned int tile_v4u __attribute__((ext_vector_type(4)));
// 16-byte global store of the copy-out: streaming (the output is never re-read, so it
// should not displace the payload lines in L2; cfg4 0.574-0.579 vs 0.578-0.588 ms)
__device__ __forceinline__ void tile_st16(uint4* d, const uint4& v) {
  __builtin_nontemporal_store(tile_v4u{v.x, v.y, v.z, v.w}, (tile_v4u*)d);
}

struct TileParams {
  const uint32_t* payload;       // local segment j owns words [4j, 4j+4); +1 look-ahead, zero padded
  const uint32_t* gaps;          // gap words; nibble (gap_nib0 + j - 1) = start of local segment j>=1
  const uint32_t* lut;           // 2^K u32 {len | sym << 8 | len << 23}
  uint8_t* out;
  unsigned long long* granules;  // one per tile: its symbol count (flag 1)
  unsigned long long* prefix;    // one per tile: its global exclusive prefix (flag 2, by the leader)
  unsigned int* status;
  unsigned long long* total;
  unsigned long long* stats;     // poll counters (reported as slow_lookbacks)
  unsigned long long out_cap;
  unsigned long long nseg;
  unsigned int gap_nib0, first_start, ntiles, kbits, lgr, epoch;
  unsigned int lut_bytes;        // LUT bytes in LDS (replicated: 4 << (K + lgr))
  unsigned int idle_block;       // a block that exits at once (>= grid: none)
  unsigned int stage_bytes;      // one wave's staging region (16 + its piece + margin, a multiple of 16)
  unsigned int kbits_c;          // (gh_mtile.hip) the count table's width
  unsigned int fb_hi;            // (gh_mtile.hip, codes longer than the tables) the longest codeword
  unsigned long long* piece_off;  // (tile kernel) [16 ntiles + 1] output offset of wave w's piece of tile t at
                                  // 16 t + w, then the shard's total: written by the chained kernel,
                                  // read by the known-offsets one
  uint4* stamps;                // GH_TILE_STAMPS builds: [grid][2 waves][128 iterations][2] phase deltas
  unsigned long long* tstamps;   // GH_TILE_STAMPS builds: 100 MHz times: [ntiles] aggregate left, [ntiles]
                                 // prefix obtained by wave 0 (bit 63: polled), [rounds] round published
};

// LDS of the tile kernel: LUT, 2 x NW staging regions (one per wave and buffer), the
// per-tile wave totals, offsets and arrival counters (TILE_SLOTS tiles), leader wave totals.
// stage_bytes: one wave's region.
inline size_t tile_lds_bytes(size_t lut_bytes, size_t stage_bytes) {
  return lut_bytes + TILE_LAG * (TILE_TB / 64) * stage_bytes + TILE_SLOTS * (2 * (TILE_TB / 64) + 1) * 4 +
         TILE_SLOTS * 12 + 4 * (TILE_TB / 64) + 4 * TILE_SLOTS + 32;
}
// ... of its known-offsets instantiation: the LUT and one staging region per wave.
inline size_t tile_lds_bytes_known(size_t lut_bytes, size_t stage_bytes) {
  return lut_bytes + (TILE_TB / 64) * stage_bytes + 32;
}

// v_perm selectors of the symbol placement (a LUT entry carries its symbol in byte 1;
// v_perm_b32 D, S0, S1, sel: selector bytes 0-3 take S1's bytes, 4-7 S0's).  Four
// consecutive symbols make one output dword in three ops: two pairs, then the dword.
constexpr uint32_t PERM_PAIR = 0x07060501u;   // (S0 = later entry, S1 = earlier): bytes 0, 1 = their symbols
constexpr uint32_t PERM_QUAD = 0x05040100u;   // (S0 = pair 2-3, S1 = pair 0-1): the dword
constexpr uint32_t PERM_THIRD = 0x07050100u;  // (S0 = entry 2, S1 = pair 0-1): a dword cut short after three symbols

// e-window of a segment starting at bit `start` (0..15): e-stream bit 0 is segment
// bit start - S (bits before the segment read as 0); requires 16 <= S <= 31.  The
// lookup address of the codeword at window bit p is then
// alignbit(e0, e1, 32 - p) & (mask << (2 + lgr)) | lane_offset: two VALU ops.
__device__ __forceinline__ void make_ewin(uint4 w, uint32_t w4, int start, uint32_t S, uint32_t (&e)[5]) {
  const uint32_t r = S - (uint32_t)start;  // 1..31
  e[0] = __builtin_amdgcn_alignbit(0u, w.x, r);
  e[1] = __builtin_amdgcn_alignbit(w.x, w.y, r);
  e[2] = __builtin_amdgcn_alignbit(w.y, w.z, r);
  e[3] = __builtin_amdgcn_alignbit(w.z, w.w, r);
  e[4] = __builtin_amdgcn_alignbit(w.w, w4, r);
}

// Decode state of a segment, one register Q:
//   bits 0-7    32 - bits consumed in the current group (v_alignbit reads bits 0-4);
//   bits 8-22   symbol underflow room (the entries' symbol bytes are subtracted here);
//   bits 23-31  H = bits left before the segment end, minus 1 (9 bits).
// LUT entries are {len | sym << 8 | len << 23}, so Q -= entry advances both counters in
// one op, and its borrow is set exactly when H < len: at the codeword that reaches or
// crosses the segment end, the last one the reference keeps (it keeps a codeword iff it
// starts before the end).  The count is then the index of that codeword + 1 (one
// v_cndmask on the borrow).  Past it H has wrapped to >= 500 and stays above 127 (at most
// 32 x 12 more bits are subtracted), so no later codeword borrows; an inactive segment
// starts at H = 511.
constexpr uint32_t Q_SYMROOM = 0x7FFFu << 8;
constexpr uint32_t Q_LIVE = 128u << 23;  // Q below this: the next codeword is still kept
__device__ __forceinline__ uint32_t q_init(bool act, int start) {
  return ((act ? (uint32_t)(127 - start) : 511u) << 23) | Q_SYMROOM | 32u;
}

// Wait until at most N LDS operations of the wave are outstanding (they complete in
// order), tied to v so the compiler uses it only after the wait.
template <int N>
__device__ __forceinline__ void lds_wait_n(uint32_t& v) {
  static_assert(N >= 0 && N <= 3, "lgkmcnt 0..3");
  if constexpr (N == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v)::"memory");
  else if constexpr (N == 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(v)::"memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(v)::"memory");
  else asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(v)::"memory");
}

// Decode of U segments per lane on e-windows.  Each group decodes G codewords per chain
// from e0:e1 and then shifts the windows (G * maxlen <= 32, so the group's consumed bits
// fit Q's low byte).  Codeword j of a segment goes to byte j of ow (v_perm with static
// selectors, two symbols at a time: PERM_PAIR above); dead codewords go there too and are
// never staged.  `mid()` runs once, after group TILE_MIDG (NG > TILE_MIDG).  Returns the groups run (wave-uniform: the loop stops
// once no chain of the wave is live).  The chains' lookups roll: each chain waits only
// for its own read (a counted lgkmcnt: LDS reads of a wave complete in order) and issues
// its next one at once, so U reads stay in flight and a chain's step costs one LDS round
// trip plus its own few ops (round 5: cfg4 -0.7 %, cfg5 -2 % against the chains in
// lock-step, waiting for all U reads).  A chain shifts its window at its own group end;
// the early exit, after a group of every chain, drains the next group's U reads.
// Window trim: word k holds e-positions [C + 32k, +32) after a shift, C = the bits
// consumed so far >= (gi + 1) * G * MINL (no codeword is shorter than MINL bits).  A kept
// codeword starts before segment bit 128, e-position 127 - start + S, and its lookup reads
// K bits: nothing at e-position >= 157 - lgr - start is read for a kept codeword, so a
// word lying wholly at or above 157 is no longer shifted (its stale bits reach only such
// positions; dead codewords decode garbage, never counted).
// Never-borrow prefix: a segment starts at bit <= 15 (a gap nibble; first_start is the
// nibble before the shard's first segment, 0 at a stream's start) and the host picks
// G = min(4, 32 / maxlen) (tile_kernel_for's second argument), so a code decoded with
// G = 4, 3, 2 has no codeword longer than LMAX = 8, 10, 12 bits (tile codes stop at 12).  The first NB = 112 / LMAX
// codewords of a segment then end at or before bit 15 + 112 = 127: none of them reaches
// the segment end, so none borrows, whatever the payload bits are (the lengths come from
// the LUT, not from the stream).  For them Q takes a plain subtract and cnt is left alone.
// For the same reason every active segment is still live after NB codewords: the
// liveness minimum and the exit test start at the first group that holds codeword NB
// (0-based).  A wave without a tile (the drain iterations: every chain inactive) leaves
// after group TILE_MIDG as before, on the wave-uniform `have_tile`.
template <int G, int U, int OW, int MINL, class Mid>
__device__ __forceinline__ int decode_tile_rolling(uint32_t (&e)[U][5], const int (&start)[U], const bool (&act)[U],
                                                   uint32_t (&ow)[U][OW], uint32_t (&cnt)[U], uint32_t amask,
                                                   uint32_t laneoff, bool have_tile, Mid&& mid) {
  constexpr int S = 4 * OW;
  constexpr int NG = (S + G - 1) / G;
  static_assert(G >= 2 && G <= 4, "G = min(4, 32 / maxlen) with maxlen <= 12");
  constexpr int LMAX = G >= 4 ? 8 : G == 3 ? 10 : 12;  // the longest codeword of a code decoded with this G
  static_assert(G * LMAX <= 32 && (G == 4 || (G + 1) * LMAX > 32), "LMAX is the longest maxlen with 32 / maxlen == G");
  constexpr int NB = 112 / LMAX;  // 15 (the gap nibble's range) + NB * LMAX <= 127: codewords 0 .. NB - 1 never borrow
  static_assert(15 + NB * LMAX <= 127 && NB < S, "the never-borrow prefix");
  constexpr int GLIVE = NB / G;   // the first group whose last codeword is >= NB
  static_assert(GLIVE >= TILE_MIDG && GLIVE < NG, "mid() runs before any exit");
  // (four codewords per window shift: the deferred symbol placement kept too many entries
  // live and spilled; placed per group instead)
  constexpr bool PLACE = G >= 4;
  uint32_t q[U], ent[U], hold[U], pair[U];
  auto lut_rd = [&](uint32_t a) -> uint32_t { return lds_u32_nowait(a); };
#pragma unroll
  for (int u = 0; u < U; ++u) {
    q[u] = q_init(act[u], start[u]);
    cnt[u] = 0;
#pragma unroll
    for (int k = 0; k < OW; ++k) asm volatile("" : "=v"(ow[u][k]));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) ent[u] = lut_rd((e[u][0] & amask) | laneoff);
  int gdone = NG;
#pragma clang loop unroll(full)
  for (int gi = 0; gi < NG; ++gi) {
    const int CMIN = (gi + 1) * G * MINL;  // bits consumed by the end of this group, at least
    uint32_t qmin = 0xFFFFFFFFu;
#pragma clang loop unroll(full)
    for (int j = 0; j < G; ++j) {
      const int pos = gi * G + j;
      if (pos < S) {
        const bool gend = (j == G - 1) || (pos + 1 >= S);  // this chain's last codeword of the group
        const bool last = gend && gi + 1 >= NG;             // no read after it
#pragma clang loop unroll(full)
        for (int u = 0; u < U; ++u) {
          // outstanding: chains u.. of this codeword, and chains ..u-1's next reads
          if (last) {
            if constexpr (U == 3) {
              if (u == 0) lds_wait_n<2>(ent[u]);
              else if (u == 1) lds_wait_n<1>(ent[u]);
              else lds_wait_n<0>(ent[u]);
            } else if constexpr (U == 2) {
              if (u == 0) lds_wait_n<1>(ent[u]);
              else lds_wait_n<0>(ent[u]);
            } else {
              lds_wait_n<0>(ent[u]);
            }
          } else {
            lds_wait_n<U - 1>(ent[u]);
          }
          if (pos < NB) {
            q[u] -= ent[u];  // cannot borrow (above)
          } else {
            asm("v_sub_co_u32 %0, vcc, %0, %2\n\t"
                "v_cndmask_b32_e64 %1, %1, %3, vcc"
                : "+v"(q[u]), "+v"(cnt[u]) : "v"(ent[u]), "i"(pos + 1) : "vcc");
          }
          // symbol placement: entries 0 and 2 of a dword wait for their neighbour
          if ((pos & 1) == 0) {
            hold[u] = ent[u];
          } else if ((pos & 3) == 1) {
            pair[u] = __builtin_amdgcn_perm(ent[u], hold[u], PERM_PAIR);
          } else {
            ow[u][pos >> 2] = __builtin_amdgcn_perm(__builtin_amdgcn_perm(ent[u], hold[u], PERM_PAIR), pair[u], PERM_QUAD);
          }
          if (!gend) {
            const uint32_t x = __builtin_amdgcn_alignbit(e[u][0], e[u][1], q[u]);
            ent[u] = lut_rd((x & amask) | laneoff);
          } else {
            // window shift (the trim of words no kept codeword reads: above)
            e[u][0] = __builtin_amdgcn_alignbit(e[u][0], e[u][1], q[u]);
            if (CMIN + 32 < 157) e[u][1] = __builtin_amdgcn_alignbit(e[u][1], e[u][2], q[u]);
            if (CMIN + 64 < 157) e[u][2] = __builtin_amdgcn_alignbit(e[u][2], e[u][3], q[u]);
            if (CMIN + 96 < 157) e[u][3] = __builtin_amdgcn_alignbit(e[u][3], e[u][4], q[u]);
            if (CMIN + 128 < 157) e[u][4] = __builtin_amdgcn_alignbit(e[u][4], 0u, q[u]);
            q[u] = (q[u] & 0xFFFFFF00u) | 32u;
            if (gi >= GLIVE) qmin = min(qmin, q[u]);
            if (!last) ent[u] = lut_rd((e[u][0] & amask) | laneoff);
          }
        }
      }
    }
    if (PLACE) {  // this group's symbols placed by its end
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int w0 = (gi * G) >> 2, w1 = min(OW - 1, (gi * G + G - 1) >> 2);
#pragma unroll
        for (int wi = w0; wi <= w1; ++wi) asm volatile("" : "+v"(ow[u][wi]));
      }
    }
    if (gi == TILE_MIDG) mid();
    // no segment can end before group GLIVE; a wave without a tile leaves after mid()
    if (gi + 1 < NG && (gi >= GLIVE ? !__any(qmin < Q_LIVE) : (gi == TILE_MIDG && !have_tile))) {
      // the next group's reads are in flight: drain them
#pragma unroll
      for (int u = 0; u < U; ++u) lds_wait_n<0>(ent[u]);
      // the dword this group ends in, if it is not whole: from the symbols it has
      const int pe = gi * G + G - 1;  // the last codeword decoded
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if ((pe & 3) == 0) ow[u][pe >> 2] = hold[u] >> 8;
        else if ((pe & 3) == 1) ow[u][pe >> 2] = pair[u];
        else if ((pe & 3) == 2) ow[u][pe >> 2] = __builtin_amdgcn_perm(hold[u], pair[u], PERM_THIRD);
      }
      gdone = gi + 1;
      break;
    }
  }
  return gdone;
}

// LDS store at an absolute byte address plus a constant offset (the instruction's
// offset field).
template <int OFF = 0>
__device__ __forceinline__ void lds_st32(uint32_t a, uint32_t v) {
  asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(a), "v"(v), "i"(OFF) : "memory");
}
// A waited LDS read / write at an absolute byte address (hand-offs between waves).
__device__ __forceinline__ uint32_t lds_ld_u32(uint32_t a) {
  uint32_t v;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
  return v;
}
__device__ __forceinline__ void lds_st_u32(uint32_t a, uint32_t v) {
  asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" ::"v"(a), "v"(v) : "memory");
}
// ... with the offset 4m, m a constant of the unrolled caller (1..12)
__device__ __forceinline__ void lds_st32_m(uint32_t a, uint32_t v, int m) {
  switch (m) {
    case 1: lds_st32<4>(a, v); break;
    case 2: lds_st32<8>(a, v); break;
    case 3: lds_st32<12>(a, v); break;
    case 4: lds_st32<16>(a, v); break;
    case 5: lds_st32<20>(a, v); break;
    case 6: lds_st32<24>(a, v); break;
    case 7: lds_st32<28>(a, v); break;
    case 8: lds_st32<32>(a, v); break;
    case 9: lds_st32<36>(a, v); break;
    case 10: lds_st32<40>(a, v); break;
    case 11: lds_st32<44>(a, v); break;
    default: lds_st32<0>(a + 4u * (uint32_t)m, v); break;
  }
}
// Staging of one wave's 64U consecutive segments into the wave's own region (chain u lane
// l = segment 64u + l of the wave, n[u] bytes from ow[u] at LDS byte o[u]; the first one
// at the region's 16-byte aligned start), with no other wave involved.
//
// A segment's bytes are realigned to the dwords they fall in: with ap = o - base in 1..4
// (base = o rounded down to a dword, minus 4 when o is aligned), dword m >= 1 at base + 4m
// holds segment bytes [4m - ap, +4).  Rounds m = mmax .. 1 store dword m of every segment
// unconditionally, chain by chain: a dword past a segment's end holds garbage, but it lies
// in the next one or two segments of the wave, which store that address in a LATER round
// (their base is higher, so their m for it is lower; within a round a segment's dwords
// differ from the others').  LDS operations of a wave complete in order, so the last
// store to every address is the one of the last segment that starts before it: the right
// bytes, except in each segment's first dword (base, when ap < 4), which holds the
// previous segment's tail followed by garbage.  Each segment then reads that dword back
// and puts its head bytes over the garbage (read-modify-write, in order again).  Garbage
// past the wave's last segment lands in the region's margin.  (Rounds 2-4: aligned stores
// under exec masks, a second workgroup barrier and head bytes after it: ~36 VALU and ~21
// SALU per segment.)
template <int U, int OW>
__device__ __forceinline__ void stage_wave(const uint32_t (&ow)[U][OW], const uint32_t (&n)[U], const uint32_t (&o)[U],
                                           int mmax) {
  uint32_t base[U], sh[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t ap = ((o[u] - 1u) & 3u) + 1u;
    base[u] = o[u] - ap;
    sh[u] = 4u - ap;  // v_alignbyte amount: dword m = bytes [4m - ap, +4) of the segment
  }
  auto dw = [&](int u, int m) { return __builtin_amdgcn_alignbyte(m < OW ? ow[u][m] : 0u, ow[u][m - 1], sh[u]); };
#pragma unroll
  for (int m = OW; m >= 1; --m) {
    if (m > mmax) continue;  // wave-uniform: no segment of the wave reaches dword m
#pragma unroll
    for (int u = 0; u < U; ++u) lds_st32_m(base[u], dw(u, m), m);
  }
  // head dwords: read back (the previous segment's tail + garbage), merge, store; the
  // reads are unconditional, the stores are not (a segment at an aligned offset, and the
  // empty segments past a shard's end, have no head dword)
  uint32_t rd[U];
#pragma unroll
  for (int u = 0; u < U; ++u) rd[u] = lds_u32_nowait(base[u]);
  lds_wait(rd);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t ap = o[u] - base[u];
    if (n[u] && ap < 4u) {
      const uint32_t ab = 8u * ap;  // the previous segment's bits in the dword
      lds_st32(base[u], (rd[u] & ((1u << ab) - 1u)) | (ow[u][0] << ab));
    }
  }
}

// Copy one wave's piece of a tile, staged at LDS byte stg + 16 + i = piece byte i, to
// out[goff, goff + n) (n already clamped at out_cap).  Output chunk c (16 bytes, aligned
// to the global address) is staging bytes [16c + 16 - lb, +16), lb = goff & 15: read as
// its two aligned LDS chunks and shifted in registers (below).  PHASED (the known-offsets
// kernel): the piece was staged at stg + 16 + lb instead, so output chunk c is the aligned
// LDS chunk at stg + 16 + 16c: one ds_read_b128, no shift.  Every lane issues exactly
// NS 16-byte buffer stores and one byte store (the partial head and tail chunks' bytes,
// one per lane): a lane with no chunk (byte) stores at an offset past the buffer's range,
// which the hardware drops, so no padding bytes reach memory and the store count is
// fixed.  gfx950 counts loads and stores in one in-order queue (vmcnt): with a fixed store
// count after the next tile's prefetch loads the compiler waits for those loads with a
// counted vmcnt instead of vmcnt(0), so a wave never waits for its copy-out's stores to
// be acknowledged.  The host sizes the regions so that NS * 64 chunks cover a piece.
constexpr uint32_t OOB_OFF = 0x80000000u;  // a buffer offset past every range: the store is dropped
// v, b: the data registers.  A caller that keeps them alive across its loop (as values
// carried from one copy-out to the next, "+v" below) keeps the register allocator from
// handing them to other values while the stores are in flight: the compiler waits for
// an outstanding store before its data registers are overwritten (vmcnt), so a reuse
// right after the copy-out stalled the next iteration on the stores.
template <int NS, bool PIN = true, bool PHASED = false>
__device__ __forceinline__ void copy_out_piece(uint8_t* out, uint32_t stg, unsigned long long goff, uint32_t n,
                                               int lane, tile_v4u (&v)[NS], uint32_t& b, uint32_t c0 = 0) {
  // (c0: the first chunk of this call; a piece copied in parts, 64 * NS chunks each, has
  // its edge bytes stored by the part with c0 = 0)
  // goff and n are wave-uniform; said so explicitly, the buffer resource lives in SGPRs
  // (otherwise each store became a readfirstlane "waterfall" loop, and the compiler's
  // vmcnt counting across those loops fell back to short counts at the next iteration)
  goff = rfl_u64(goff);
  n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);
  const uint32_t lb = (uint32_t)(goff & 15);
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(out + (goff - lb), 0, 0x7FFFFFF0, 0x00020000);
  // (GH_TILE_ABLATE & 128, diagnostic: 16-byte aligned LDS reads, wrong bytes)
  const uint32_t src = PHASED ? stg + 16u : (stg + 16u - ((GH_TILE_ABLATE & 128) ? 0u : lb)) & ((GH_TILE_ABLATE & 256) ? ~3u : ~0u);    // staging address of output chunk 0 (diagnostic 256: dword-aligned)
  const uint32_t cf = lb ? 1u : 0u;       // interior chunks [cf, ce)
  const uint32_t ce = n ? (lb + n) >> 4 : 0u;
  uint32_t off[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const uint32_t c = c0 + cf + (uint32_t)lane + 64u * (uint32_t)i;
    off[i] = c < ce ? 16u * c : OOB_OFF;
  }
  // edge bytes: the head chunk's [lb, min(16, lb + n)) when lb != 0, then the tail
  // chunk's [0, (lb + n) & 15) when it is another chunk; one byte per lane
  const uint32_t nh = (lb && n) ? min(16u, lb + n) - lb : 0u;
  const uint32_t tl = (lb + n) & 15u;
  const uint32_t nt = (n && tl && (ce > 0 || !lb)) ? tl : 0u;
  const uint32_t t = (uint32_t)lane;
  uint32_t k = OOB_OFF;
  if (c0 == 0u && !(GH_TILE_ABLATE & 64)) {  // (diagnostic 64: no edge bytes)
    if (t < nh) k = lb + t;
    else if (t < nh + nt) k = 16u * ce + (t - nh);
  }
  if constexpr (!PHASED) {
    // Output chunk c is staging bytes [src + 16c, +16): the last 16 - lb bytes of the
    // aligned chunk at stg + 16c and the first lb of the next.  Both aligned chunks are read
    // (an unaligned ds_read_b128 costs the copy-out several times its aligned pair: cfg4
    // window 0.53 vs 0.49 ms with the reads aligned, round 6) and shifted into place in
    // registers: output dword d = window bytes [s + 4d, +4) of P:Q, s = 16 - lb (lb = 0:
    // Q), a wave-uniform case on s >> 2 and v_alignbyte by s & 3.  Chunks go CG at a time
    // (registers), each group stored as soon as it is shifted; the store count is fixed.
    constexpr int CG = NS % 2 == 0 ? 2 : 1;
    const uint32_t sh = (16u - lb) & 15u, r = sh & 3u, m = lb ? sh >> 2 : 4u;
#pragma unroll
    for (int g0 = 0; g0 < NS; g0 += CG) {
      tile_v4u pq[CG][2];
#pragma unroll
      for (int j = 0; j < CG; ++j) {
        const int i = g0 + j;
        const uint32_t c = c0 + cf + (uint32_t)lane + 64u * (uint32_t)i;
        const uint32_t a = stg + 16u * (c < ce ? c : cf);
        asm volatile("ds_read_b128 %0, %1" : "=v"(pq[j][0]) : "v"(a) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(pq[j][1]) : "v"(a) : "memory");
      }
      if (g0 + CG >= NS) {  // the edge byte with the last group
        if (PIN) asm volatile("ds_read_u8 %0, %1" : "+v"(b) : "v"(src + (k == OOB_OFF ? 0u : k)) : "memory");
        else asm volatile("ds_read_u8 %0, %1" : "=v"(b) : "v"(src + (k == OOB_OFF ? 0u : k)) : "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = 0; j < CG; ++j) asm volatile("" : "+v"(pq[j][0]), "+v"(pq[j][1]));  // (after the wait)
      auto shift = [&](auto mc) {
        constexpr int M = decltype(mc)::value;
#pragma unroll
        for (int j = 0; j < CG; ++j) {
          if constexpr (M == 4) {
            v[g0 + j] = pq[j][1];
          } else {
            auto W = [&](int q) -> uint32_t { return q < 4 ? pq[j][0][q] : pq[j][1][q - 4]; };
#pragma unroll
            for (int d = 0; d < 4; ++d) v[g0 + j][d] = __builtin_amdgcn_alignbyte(W(M + d + 1), W(M + d), r);
          }
        }
      };
      switch (m) {
        case 0: shift(std::integral_constant<int, 0>{}); break;
        case 1: shift(std::integral_constant<int, 1>{}); break;
        case 2: shift(std::integral_constant<int, 2>{}); break;
        case 3: shift(std::integral_constant<int, 3>{}); break;
        default: shift(std::integral_constant<int, 4>{}); break;
      }
#pragma unroll
      for (int j = 0; j < CG; ++j) __builtin_amdgcn_raw_buffer_store_b128(v[g0 + j], rs, (int)off[g0 + j], 0, 2);  // nt
    }
    if (PIN) asm volatile("" : "+v"(b));
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)b, rs, (int)k, 0, 2);
    return;
  }
  // PHASED: output chunk c is the aligned LDS chunk at src + 16c
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const uint32_t c = c0 + cf + (uint32_t)lane + 64u * (uint32_t)i;
    if (PIN) asm volatile("ds_read_b128 %0, %1" : "+v"(v[i]) : "v"(src + 16u * (c < ce ? c : cf)) : "memory");
    else asm volatile("ds_read_b128 %0, %1" : "=v"(v[i]) : "v"(src + 16u * (c < ce ? c : cf)) : "memory");
  }
  if (PIN) asm volatile("ds_read_u8 %0, %1" : "+v"(b) : "v"(src + (k == OOB_OFF ? 0u : k)) : "memory");
  else asm volatile("ds_read_u8 %0, %1" : "=v"(b) : "v"(src + (k == OOB_OFF ? 0u : k)) : "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b)::"memory");
#pragma unroll
  for (int i = 0; i < NS; ++i) asm volatile("" : "+v"(v[i]));  // (after the wait: asm volatile order)
#pragma unroll
  for (int i = 0; i < NS; ++i) __builtin_amdgcn_raw_buffer_store_b128(v[i], rs, (int)off[i], 0, 2);  // nt
  __builtin_amdgcn_raw_buffer_store_b8((uint8_t)b, rs, (int)k, 0, 2);
}

// A segment's n bytes (ow, byte 0 first) stored to out[o, o + n), clamped at cap: the
// path of a tile too large for staging (byte stores; rare).
template <int OW>
__device__ __forceinline__ void store_direct(uint8_t* out, unsigned long long cap, unsigned long long o,
                                             const uint32_t (&ow)[OW], uint32_t n) {
#pragma unroll
  for (int i = 0; i < 4 * OW; ++i)
    if ((uint32_t)i < n && o + (uint32_t)i < cap) out[o + (uint32_t)i] = (uint8_t)(ow[i >> 2] >> (8 * (i & 3)));
}

__device__ __forceinline__ bool granule_ok(const TileParams& p, unsigned long long v, uint32_t flag) {
  return (uint32_t)(v >> 40) == p.epoch && (uint32_t)((v >> 38) & 3u) == flag;
}

// Poll a granule until it carries this launch's epoch with the wanted flag.  Bounded by
// wall time, 4 s of the 100 MHz clock: a persistent grid that shares the GPU with
// another kernel (another stream or process) waits for its not-yet-resident workgroups
// until that kernel's workgroups retire — a delay, not a fault.  After a timeout every
// later poll returns at once (the decode then fails with GH_E_HIP).  The clock and the
// status word are read only every 64th poll: a poll's load sits in the CU's memory
// queue behind its streaming traffic (microseconds), and the hand-off chain pays every
// extra round trip.
__device__ __forceinline__ unsigned long long poll_granule(const TileParams& p, unsigned long long* g,
                                                           uint32_t flag) {
  unsigned long long t0 = 0;
  for (uint32_t spins = 1;; ++spins) {
    const unsigned long long v = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (granule_ok(p, v, flag)) return v;
    if ((spins & 63u) == 0u) {
      if (__hip_atomic_load(p.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & GH_ST_TIMEOUT) return 0;
      const unsigned long long t = wall_clock64();
      if (t0 == 0) {
        t0 = t;
      } else if (t - t0 > 400000000ull) {
        atomicOr(p.status, (unsigned)GH_ST_TIMEOUT);
        return 0;
      }
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

// The round leader (workgroup 0): for every round r of D decoding workgroups' tiles, wait
// for the round's aggregates (thread t takes the A = ceil(D / TB) <= LEAD_A consecutive
// tiles t*A .. t*A + A - 1 of the round), scan them and publish each tile's global
// exclusive prefix; R, the start of the round, stays in a register.  (Spreading the rounds
// over the leader's waves, the next rounds' aggregates loaded ahead, measured slower:
// 0.74 vs 0.71 ms in round 3 with eight rounds in flight, 0.615 vs 0.586 ms in round 5
// with two.)
constexpr int LEAD_A = 4;
template <int TB>
__device__ __forceinline__ void tile_round_leader(const TileParams& p, uint32_t D, uint32_t* s_lead, int tid,
                                                  int lane, int wid) {
  const uint32_t A = (D + TB - 1) / TB;  // <= LEAD_A (the host caps the grid)
  const uint32_t nr = (p.ntiles + D - 1) / D;
  unsigned long long R = 0;
  for (uint32_t r = 0; r < nr; ++r) {
    const uint32_t t0 = r * D, n = min(D, p.ntiles - t0);
    uint32_t v[LEAD_A], sum = 0;
#pragma unroll
    for (int i = 0; i < LEAD_A; ++i) {
      const uint32_t j = (uint32_t)tid * A + (uint32_t)i;
      v[i] = 0;
      if ((uint32_t)i < A && j < n) {
        unsigned long long g = __hip_atomic_load(&p.granules[t0 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!granule_ok(p, g, 1)) {
          atomicAdd(p.stats + 1, 1ull);
          g = poll_granule(p, &p.granules[t0 + j], 1);
        }
        v[i] = (uint32_t)(g & GRAN_VMASK);  // a tile holds < 2^32 symbols
      }
      sum += v[i];
    }
    const uint32_t incl = wave_incl_scan(sum);
    if (lane == 63) s_lead[wid] = incl;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < TB / 64; ++q) {
      const uint32_t x = s_lead[q];
      before += (q < wid) ? x : 0u;
      total += x;
    }
    unsigned long long run = R + before + incl - sum;
#pragma unroll
    for (int i = 0; i < LEAD_A; ++i) {
      const uint32_t j = (uint32_t)tid * A + (uint32_t)i;
      if ((uint32_t)i < A && j < n)
        __hip_atomic_store(&p.prefix[t0 + j], granule(p.epoch, 2, run), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      run += v[i];
    }
    R += total;
#if GH_TILE_STAMPS
    if (tid == 0) p.tstamps[2 * p.ntiles + r] = __builtin_amdgcn_s_memrealtime();  // round r published
#endif
    __syncthreads();
  }
}

// TB threads, U segments per lane, GRP codewords per window shift, OW output words per
// segment, codewords of at least MINL bits.  Compiled for 4 waves per SIMD (128 VGPRs):
// one 1024-thread workgroup per CU, which its LUT copies and staging buffers (~157 KB of
// LDS) fill.
//
// The waves of a decoding workgroup run without a workgroup barrier: each stages its own
// segments into its own LDS region and copies its own piece out.  The tile's aggregate
// is published by the wave that arrives last at it (an LDS counter per tile slot), which
// also writes every wave's offset in the tile; a wave reads the offsets of tile k-2 only
// after its global prefix has arrived, which the aggregate (so every wave's arrival)
// precedes.  A wave can thus run at most about three tiles ahead of the slowest wave of
// its workgroup (it needs tile k-3's prefix at iteration k-1), within the TILE_SLOTS
// slots.  Where a wave copies its piece out it also records the piece's output offset in
// p.piece_off (the direct-store path too), one more store per wave and tile.
//
// KNOWN: the instantiation for a shard whose p.piece_off a chained decode has filled (the
// file header).  No leader: D = grid, workgroup b takes tiles b, b + D, ...  Its waves
// share nothing but the LUT: a wave's iteration is decode, wave scan, staging into its one
// region at the phase of its output offset, and the copy-out (TILE_KLAG: in the same
// iteration or in the next one); LDS holds the LUT and NW regions only.
typedef unsigned int tile_v2u __attribute__((ext_vector_type(2)));
template <int TB, int U, int GRP, int OW, int MINL, bool KNOWN = false>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(4, 4))) void gh_tile_kernel(const TileParams p) {
  static_assert(4 * OW >= (128 + MINL - 1) / MINL, "OW words hold every codeword a segment can start");
  static_assert(U <= TILE_U, "shapes of at most TILE_U segments per lane");
  constexpr int NW = TB / 64;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t stage_lds = p.lut_bytes;                                  // [LAG][NW] regions (KNOWN: [NW])
  // (the chained kernel's hand-off words; KNOWN has none)
  uint32_t* s_tot = (uint32_t*)(smem + p.lut_bytes + TILE_LAG * NW * p.stage_bytes);  // [SLOTS][NW] wave totals
  uint32_t* s_off = s_tot + TILE_SLOTS * NW;                                // [SLOTS][NW] wave offsets
  uint32_t* s_cnt = s_off + TILE_SLOTS * NW;                                // [SLOTS] arrivals
  unsigned long long* s_pfx = (unsigned long long*)(s_cnt + TILE_SLOTS);   // [SLOTS] prefixes (wave 0)
  uint32_t* s_ptile = (uint32_t*)(s_pfx + TILE_SLOTS);                      // [SLOTS] their tiles
  uint32_t* s_lead = s_ptile + TILE_SLOTS;                                  // [NW] (leader)
  const uint32_t cnt_lds = (uint32_t)((uint8_t*)s_cnt - smem);
  const uint32_t ptile_lds = (uint32_t)((uint8_t*)s_ptile - smem);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
#if GH_TILE_STAMPS
  // per launch (ring of 1024 by epoch): shader-clock and 100 MHz times at the leader's start
  // and end, to read the clock the kernel ran at
  unsigned long long* const lring = p.tstamps + 3ull * p.ntiles + 64 + 4ull * (p.epoch & 1023u);
  if (!KNOWN && blockIdx.x == 0 && tid == 0) {
    lring[0] = __builtin_amdgcn_s_memtime();
    lring[1] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  // decoding workgroups: every block but 0 (the leader) and p.idle_block (if < grid);
  // KNOWN: every block
  uint32_t D = gridDim.x, b = blockIdx.x;
  if constexpr (!KNOWN) {
    D = gridDim.x - 1 - (p.idle_block < gridDim.x ? 1u : 0u);
    b = blockIdx.x - 1 - (blockIdx.x > p.idle_block ? 1u : 0u);
    if (blockIdx.x == 0) {
      tile_round_leader<TB>(p, D, s_lead, tid, lane, wid);
#if GH_TILE_STAMPS
      if (tid == 0) {
        lring[2] = __builtin_amdgcn_s_memtime();
        lring[3] = __builtin_amdgcn_s_memrealtime();
      }
#endif
      return;
    }
    if (blockIdx.x == p.idle_block) return;  // the leader's CU partner (GH_TILE_IDLE): no decoding
  }
#if GH_TILE_STAMPS
  // per workgroup: shader-clock and 100 MHz times at its start and end (its clock)
  unsigned long long* const wring = p.tstamps + 3ull * p.ntiles + 64 + 4ull * 1024 + 4ull * blockIdx.x;
  if (tid == 0) {
    wring[0] = __builtin_amdgcn_s_memtime();
    wring[1] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  {  // LUT to LDS, replicated: dword i of LDS = entry i >> lgr (lane l reads copy l mod 2^lgr,
     // so up to 32 lanes of a ds_read_b32 hit distinct banks)
    const uint32_t nd = p.lut_bytes >> 2;
    uint32_t* sl = (uint32_t*)smem;
    for (uint32_t i = tid; i < nd; i += TB) sl[i] = p.lut[i >> p.lgr];
    if (!KNOWN && tid < TILE_SLOTS) {
      s_cnt[tid] = 0;
      s_ptile[tid] = 0xFFFFFFFFu;
    }
    if (KNOWN && tid == 0) *(uint32_t*)(smem + p.lut_bytes + NW * p.stage_bytes) = 0u;  // the front (below)
  }
  // (KNOWN) the front: the iteration the furthest wave of the workgroup has reached.  The
  // waves share no hand-off any more, and left alone they drift apart (wave 0 ran its
  // iteration in 7.4 K cycles, wave 4 in 9.0 K: the kernel then ends with a few waves per CU
  // still working); a wave issues at the priority of its lag behind the front, as the chained
  // kernel's waves do by their arrival rank.
  const uint32_t front_lds = p.lut_bytes + (uint32_t)NW * p.stage_bytes;
  {
  }
  const uint32_t S = 30u - p.kbits - p.lgr;
  // (GH_TILE_ABLATE & 16, diagnostic: even LUT entries only, so a read's lanes never
  // collide in a bank; wrong output)
  const uint32_t amask = (((1u << p.kbits) - 1u) << (2u + p.lgr)) & ((GH_TILE_ABLATE & 16) ? ~(1u << (2u + p.lgr)) : ~0u);
  const uint32_t laneoff = ((uint32_t)lane & ((1u << p.lgr) - 1u)) << 2;
  check_lds_base(smem, p.status);

  const uint32_t G = D;                                    // decoders (b: this one)
  const uint32_t nseg = (uint32_t)p.nseg;                 // < 2^31 (checked by the host)
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  __syncthreads();  // the LUT and the counters (the last barrier of a decoding workgroup)
  const uint32_t last_tile_k = b < p.ntiles ? (p.ntiles - 1 - b) / G : NONE;
  uint32_t cur = b, nxt = b + G;
  // the lane's segments in a tile: wave-contiguous, 64 per chain (chain u lane l: segment
  // 64u + l of the wave's 64U); lane-major (GH_TILE_LMAJ): lane l's U consecutive segments
  // Ul .. Ul + U - 1, so the staging stores of one instruction land ~U segments apart
  constexpr uint32_t CSTR = GH_TILE_LMAJ ? 1u : 64u;  // segment stride between chains
  const uint32_t lseg = (uint32_t)(wid * 64 * U) + (uint32_t)lane * (GH_TILE_LMAJ ? (uint32_t)U : 1u);
  uint4 w[U];
  uint32_t w4[U], gw[U];   // (chain-major) look-ahead and gap dword per chain
  uint32_t w63, gpair[2];  // (lane-major) lane 63's look-ahead word; the lane's gap dword pair
  unsigned long long po[2] = {0, 0};  // (KNOWN) the wave's piece's output offset and the next piece's
  auto load = [&](uint32_t t) {
    const uint32_t tc = min(t, p.ntiles - 1);
    const uint32_t seg0 = tc * (uint32_t)(U * TB) + lseg;
    if constexpr (GH_TILE_LMAJ) {
      // one lane's U consecutive segments: their 16 U bytes (chain u's look-ahead word is
      // chain u + 1's first word, chain U - 1's the next lane's first word: taken from that
      // lane's registers when the windows are made).  A lane past the shard end is clamped
      // to segment nseg, not nseg - 1: the last segment's look-ahead is word 4 nseg, which
      // the lane after the last active one must hold; it reads the zero padding (4 nseg + 16
      // words are allocated: payload word 4 (nseg + U) - 1 at most, the last one when U = 4;
      // gh_decode.hip asserts U <= 4 beside the allocation's size).
      const uint32_t sb = min(seg0, nseg);
#pragma unroll
      for (int u = 0; u < U; ++u) w[u] = *(const uint4*)(p.payload + 4ull * (sb + (uint32_t)u));
      // lane 63 has no next lane: its look-ahead word, the first word after the wave's 64 U
      // segments, is loaded by every lane from that one address (a single request; no branch
      // and the same number of loads on every path: see the copy-out's fixed store count).
      // Word 4 nseg is the last one the shard holds.
      const uint32_t s63 = (uint32_t)__builtin_amdgcn_readlane((int)seg0, 63);
      w63 = p.payload[4ull * min(s63 + (uint32_t)U, nseg)];
      // the U gap nibbles gap_nib0 + sb - 1 .. + U - 1 (the first one unused when sb = 0) lie in
      // one gap dword or in two neighbours: both, as one 8-byte load at the first one's dword
      // (at most dword gwords of the gwords + 4 allocated).  That makes U + 2 loads per lane
      // and tile (U + 1 + U before), followed by the copy-out's stores: the loop top waits
      // with one counted vmcnt for all of them, where it used to count the U gap dwords down
      // one by one.
      {
        struct __attribute__((packed, aligned(4))) gap2 { uint32_t lo, hi; };
        const gap2 g = *(const gap2*)(p.gaps + ((p.gap_nib0 + (sb ? sb - 1u : 0u)) >> 3));
        gpair[0] = g.lo;
        gpair[1] = g.hi;
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t sc = min(seg0 + (uint32_t)(64 * u), nseg - 1);
        w[u] = *(const uint4*)(p.payload + 4ull * sc);
        w4[u] = p.payload[4ull * sc + 4];
        gw[u] = p.gaps[(p.gap_nib0 + (sc ? sc - 1u : 0u)) >> 3];
      }
    }
    if constexpr (KNOWN) {
      // entries 16 t + wid and the one after it (the next wave's, the next tile's first or
      // the shard's total), with the tile's words: every lane loads the same 16 bytes (one
      // request), on every path (a clamped tile in the drain: entry <= 16 ntiles)
      struct __attribute__((packed, aligned(8))) off2 { unsigned long long at, next; };
      const off2 o2 = *(const off2*)(p.piece_off + (16ull * tc + (uint32_t)wid));
      po[0] = o2.at;
      po[1] = o2.next;
    }
  };
  const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, 0x7FFFFFF0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_po = __builtin_amdgcn_make_buffer_rsrc(p.piece_off, 0, 0x7FFFFFF0, 0x00020000);
  auto junk_stores = [&]() {  // as many stores after these loads as every iteration issues
     // after its prefetch (the copy-out's TILE_NS + 1 and, chained, the recorded offset;
     // dropped here: out of range): the loop's entry then matches its back edge, and the
     // compiler waits for the loads with a counted vmcnt
    const __amdgpu_buffer_rsrc_t rs = rs_out;
#pragma unroll
    for (int i = 0; i < TILE_NS; ++i)
      __builtin_amdgcn_raw_buffer_store_b128(tile_v4u{0, 0, 0, 0}, rs, (int)(OOB_OFF + 16u * (uint32_t)i), 0, 2);  // (distinct: not merged)
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, rs, (int)OOB_OFF, 0, 2);
    if constexpr (!KNOWN) __builtin_amdgcn_raw_buffer_store_b64(tile_v2u{0, 0}, rs_po, (int)OOB_OFF, 0, 0);
  };
  load(cur);
  junk_stores();
  if (cur >= p.ntiles) cur = NONE;
  uint32_t th[TILE_LAG];          // this wave's pieces of iterations k-1 .. k-LAG (NONE: not staged)
#pragma unroll
  for (int i = 0; i < TILE_LAG; ++i) th[i] = NONE;
  uint32_t rank = 0;              // the wave's arrival rank at its last tile, in quarters
  const uint32_t region0 = stage_lds + (uint32_t)wid * p.stage_bytes;  // buffer 0; buffer 1 at + NW * stage_bytes
  // the longest piece a region holds; KNOWN stages up to 15 bytes further in
  const uint32_t piece_cap = p.stage_bytes - (uint32_t)(STAGE_PAD + 4 * OW + 4) - (KNOWN ? 16u : 0u);
  // (KNOWN, TILE_KLAG = 1) the piece staged by the previous iteration: offset, clamped length
  unsigned long long pgoff = 0;
  uint32_t pn = 0;
  bool phave = false;
#if GH_TILE_STAMPS
  unsigned long long ts[9];
#endif
  auto body = [&](uint32_t k) -> bool {
    TSTAMP(0);
    const bool have_cur = cur < p.ntiles;
    const uint32_t t2 = th[TILE_LAG - 1];  // (chained) the piece copied out this iteration (tile k - LAG)
    const bool have2 = t2 < p.ntiles;
    bool pending = have_cur;
    if constexpr (KNOWN) {
      pending |= TILE_KLAG && phave;
    } else {
#pragma unroll
      for (int i = 0; i < TILE_LAG; ++i) pending |= th[i] < p.ntiles;
    }
    if (!pending) return false;
    if (!KNOWN && last_tile_k != NONE && k > last_tile_k + TILE_LAG + 2) {  // cannot happen; never hang the GPU
      if (lane == 0) atomicOr(p.status, (unsigned)GH_ST_TIMEOUT);
      return false;
    }
    const uint32_t slot = k % TILE_SLOTS, slot2 = (k + TILE_SLOTS - TILE_LAG) % TILE_SLOTS;
    const uint32_t buf = k % TILE_LAG;
    unsigned long long* pf2 = nullptr;
    unsigned long long gp0 = 0, gp = 0;
    if constexpr (!KNOWN) {
      // issue priority by the wave's arrival rank at its last tile (0: first of the
      // workgroup's waves): the waves that arrive last gate the tile's aggregate, so they
      // issue first (the round-3/4 rule, priority 0 after a polled prefix, was slower)
      if (rank >= 3) __builtin_amdgcn_s_setprio(3);
      else if (rank == 2) __builtin_amdgcn_s_setprio(2);
      else if (rank == 1) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
      // prefix of tile k-LAG: loaded at the top and again mid-decode; the first that
      // shows it published is used (a load at the top alone often saw it a little before it
      // was published, and the re-poll then paid a full memory round trip)
      // (every lane loads the same word, one request; no branch around the load: the
      // compiler's wait counting over such a branch fell back to vmcnt(0), which then also
      // waited for the next tile's loads issued behind it)
      pf2 = &p.prefix[have2 ? t2 : 0u];
      if (!(GH_TILE_ABLATE & 4)) gp0 = __hip_atomic_load(pf2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    auto mid = [&]() {
      if constexpr (!KNOWN)
        if (!(GH_TILE_ABLATE & 4)) gp = __hip_atomic_load(pf2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // (KNOWN) this tile's piece offsets, loaded with its words: wave-uniform, to SGPRs
    const unsigned long long g_at = KNOWN ? rfl_u64(po[0]) : 0ull, g_next = KNOWN ? rfl_u64(po[1]) : 0ull;
    if constexpr (KNOWN) {
      // issue priority by the wave's lag behind the workgroup's front (one LDS max and one
      // read per iteration; LDS operations of a wave complete in order, so the read sees the
      // wave's own max)
      asm volatile("ds_max_u32 %0, %1" ::"v"(front_lds), "v"(k) : "memory");
      const uint32_t lag = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_ld_u32(front_lds)) - k;
      if (lag >= 3) __builtin_amdgcn_s_setprio(3);
      else if (lag == 2) __builtin_amdgcn_s_setprio(2);
      else if (lag == 1) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    // ---- decode this tile (its words were loaded during the previous iteration) --------
    // Decoded unconditionally: in the last iterations (no tile) every chain is inactive
    // and the loop stops after group TILE_MIDG, on have_cur (the loads were issued,
    // clamped to the last tile).  A branch around the decode made the compiler zero the
    // output words before it every iteration and wait vmcnt(0) after it.
    const uint32_t seg0 = cur * (uint32_t)(U * TB) + lseg;
    uint32_t ow[U][OW], cnt[U];
    int gdone;
    {
      int start[U];
      bool act[U];
      uint32_t e[U][5];
      // (lane-major) chain u's gap nibble at bits [4u, +4) of gnib: the dword pair starts at
      // the dword of nibble n0 = gap_nib0 + seg0 - 1 (seg0 = 0: of nibble gap_nib0, chain 1's,
      // and chain 0 starts at first_start); an inactive lane gets any nibble.  wla: the
      // last chain's look-ahead word, the next lane's first payload word (wave_shl:1; lane 63
      // keeps the word loaded for it)
      uint32_t gnib = 0, wla = 0;
      if constexpr (GH_TILE_LMAJ) {
        const uint32_t n0 = p.gap_nib0 + (seg0 ? seg0 - 1u : 0u);
        const unsigned long long g2 = ((unsigned long long)gpair[1] << 32) | gpair[0];
        gnib = (uint32_t)(g2 >> (4u * (n0 & 7u)));
        gnib = seg0 ? gnib : gnib << 4;
        wla = (uint32_t)__builtin_amdgcn_update_dpp((int)w63, (int)w[0].x, 0x130, 0xf, 0xf, false);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t seg = seg0 + (uint32_t)u * CSTR;
        act[u] = have_cur && seg < nseg;
        if constexpr (GH_TILE_LMAJ) {
          start[u] = seg == 0 ? (int)p.first_start : (int)((gnib >> (4 * u)) & 15u);
          make_ewin(w[u], u + 1 < U ? w[u + 1 < U ? u + 1 : u].x : wla, start[u], S, e[u]);
        } else {
          start[u] = seg == 0 ? (int)p.first_start : (int)gap_nib(gw[u], p.gap_nib0 + seg - 1u);
          make_ewin(w[u], w4[u], start[u], S, e[u]);
        }
      }
      TSTAMP(1);
      if (GH_TILE_ABLATE & 1) {  // diagnostic build: no decode, 16 bytes per segment (wrong output)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          cnt[u] = act[u] ? 16u : 0u;
#pragma unroll
          for (int k2 = 0; k2 < OW; ++k2) ow[u][k2] = e[u][k2 % 5];
        }
        mid();
        gdone = (16 + GRP - 1) / GRP;
      } else {
        gdone = decode_tile_rolling<GRP, U, OW, MINL>(e, start, act, ow, cnt, amask, laneoff, have_cur, mid);
      }
    }
    // The next tile's words, right after the decode (its windows are dead, so the
    // registers are free; issued during the decode they raised its register peak past
    // 128): they have the rest of the iteration (~6 K cycles) to arrive.  Issued after the
    // copy-out instead they had ~3 K cycles, and the next decode waited ~1.3 K cycles for
    // them.  They follow the prefix loads, whose waits therefore do not include them
    // (vmcnt is one in-order queue).
    load(nxt);
    TSTAMP(2);
    // ---- wave scans: the segments' offsets in the wave's piece, the piece's length -------
    uint32_t bpos[U], wave_tot = 0;
    if constexpr (GH_TILE_LMAJ) {  // lane l's segments are consecutive: one scan of their sum
      uint32_t sl = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) sl += cnt[u];
      const uint32_t incl = wave_incl_scan(sl);
      uint32_t run = incl - sl;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bpos[u] = run;
        run += cnt[u];
      }
      wave_tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) bpos[u] = wave_incl_scan(cnt[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t ct = (uint32_t)__builtin_amdgcn_readlane((int)bpos[u], 63);
        bpos[u] += wave_tot - cnt[u];
        wave_tot += ct;
      }
    }
    if constexpr (KNOWN) {
      TSTAMP(3);
      TSTAMP(4);
      // ---- the guard: the piece's scanned length against the table ------------------------
      // (the whole defence against a stale or foreign table: a piece that disagrees writes
      // nothing and fails the decode)
      const bool ok = have_cur && g_next - g_at == (unsigned long long)wave_tot;
      const bool staged = ok && wave_tot <= piece_cap;
      const uint32_t lb = (uint32_t)g_at & 15u;
      const uint32_t ncp = (!staged || g_at >= p.out_cap) ? 0u : (uint32_t)min<unsigned long long>(wave_tot, p.out_cap - g_at);
      tile_v4u cv[TILE_NS];
      uint32_t cb;
      // (TILE_KLAG = 1) the previous iteration's piece out of the region, before this
      // one's goes in (the copy-out waits for its LDS reads before it stores)
      if constexpr (TILE_KLAG == 1)
        if (!(GH_TILE_ABLATE & 8)) copy_out_piece<TILE_NS, false, true>(p.out, region0, pgoff, pn, lane, cv, cb);
#if GH_TILE_STAMPS
      const unsigned long long ta = __builtin_amdgcn_s_memtime();
#endif
      // ---- stage this tile's piece at the phase of its output offset ------------------------
      // a piece larger than the region stores its bytes straight from registers, at once;
      // one that fails the guard sets GH_ST_OFFSETS
      if (have_cur && !staged) {
        if (ok) {
#pragma unroll
          for (int u = 0; u < U; ++u) store_direct(p.out, p.out_cap, g_at + bpos[u], ow[u], cnt[u]);
        } else if (lane == 0) {
          atomicOr(p.status, (unsigned)GH_ST_OFFSETS);
        }
        // (rare path) drain its data-dependent stores here, so that the compiler's wait
        // for the next tile's loads stays a counted vmcnt on the common path
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      } else if (have_cur && !(GH_TILE_ABLATE & 2)) {
        const uint32_t sbase = region0 + STAGE_PAD + lb;
        uint32_t o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) o[u] = sbase + bpos[u];
        stage_wave<U, OW>(ow, cnt, o, min(OW, (GRP * gdone + 3) >> 2));
      }
      if (wid == NW - 1 && cur == p.ntiles - 1 && ok && lane == 0) *p.total = g_next;
#if GH_TILE_STAMPS
      const unsigned long long tb = __builtin_amdgcn_s_memtime();
#endif
      if constexpr (TILE_KLAG == 0) {
        // the staging stores have landed before the copy-out reads them back
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (!(GH_TILE_ABLATE & 8)) copy_out_piece<TILE_NS, false, true>(p.out, region0, g_at, ncp, lane, cv, cb);
      } else {
        pgoff = g_at;
        pn = ncp;
        phave = staged;
      }
#if GH_TILE_STAMPS
      // (the chained kernel's columns: copy-out, then stage)
      const unsigned long long tc = __builtin_amdgcn_s_memtime();
      ts[5] = ts[4] + (ta - ts[4]) + (tc - tb);
      ts[6] = ts[5] + (tb - ta);
#endif
    } else {
    // ---- arrival at tile k: the last wave to arrive publishes its aggregate ------------
    uint32_t tile_total = 0;
    if (have_cur) {
      uint32_t old = 0;
      if (lane == 0) {
        s_tot[slot * NW + wid] = wave_tot;
        asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(old) : "v"(cnt_lds + 4u * slot), "v"(1u)
                     : "memory");
      }
      const uint32_t arr = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
      rank = (4u * arr) / NW;
      if (arr == NW - 1) {
        // every wave's total of this tile is in LDS (each wave stored it before its add)
        const uint32_t x = lane < NW ? s_tot[slot * NW + lane] : 0u;
        const uint32_t xi = wave_incl_scan(x);
        if (lane < NW) s_off[slot * NW + lane] = xi - x;
        tile_total = (uint32_t)__builtin_amdgcn_readlane((int)xi, NW - 1);
        if (lane == 0) {
          s_cnt[slot] = 0;
          // the offsets are in LDS before the aggregate leaves (a wave reads them once the
          // prefix this aggregate leads to has arrived)
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __hip_atomic_store(&p.granules[cur], granule(p.epoch, 1, tile_total), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
#if GH_TILE_STAMPS
          p.tstamps[cur] = __builtin_amdgcn_s_memrealtime();  // tile cur's aggregate left
#endif
        }
      }
    }
    TSTAMP(3);
    // ---- the prefix of tile k-LAG -> this wave's piece's output offset -------------------
    unsigned long long goff = 0;
    uint32_t n2 = 0;
    bool rec = false;  // goff is the piece's true offset: recorded for the known-offsets decodes
    if (have2 && (GH_TILE_ABLATE & 4)) {
      goff = ((unsigned long long)t2 * (U * TB * 16) + (uint32_t)wid * (U * 64 * 16)) % (p.out_cap - (U * TB * 32));
      n2 = s_tot[slot2 * NW + wid];
    } else if (have2) {
      // The wave's own early loads (top of the iteration, mid-decode) when they already
      // show the prefix; else the LDS post of the first wave of the workgroup that saw it,
      // or the wave's own poll, whichever comes first (the poll posts what it finds).
      unsigned long long g = rfl_u64(gp0);  // wave-uniform: each waits for its own load only
      bool polled = false, got = true;  // (polled: GH_TILE_STAMPS builds)
      (void)polled;
      if (!granule_ok(p, g, 2)) g = rfl_u64(gp);
      if (!granule_ok(p, g, 2)) {
        polled = true;
        if (wid == 0 && lane == 0) atomicAdd(p.stats, 1ull);
        unsigned long long t0w = 0;
        // (two or three polls in flight measured slower: 0.440 vs 0.433 ms, round 5)
        unsigned long long pv = __hip_atomic_load(pf2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (uint32_t spins = 1;; ++spins) {
          bool found = false;
          if (lds_ld_u32(ptile_lds + 4u * slot2) == t2) {
            asm volatile("" ::: "memory");
            g = s_pfx[slot2];
            found = true;
          } else {
            g = rfl_u64(pv);
            if (granule_ok(p, g, 2)) {
              if (lane == 0) {  // post: the value, then its tile (LDS order)
                s_pfx[slot2] = g;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                lds_st_u32(ptile_lds + 4u * slot2, t2);
              }
              found = true;
            } else {
              pv = __hip_atomic_load(pf2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
          if (found) break;
          if ((spins & 63u) == 0u) {  // bounded like poll_granule: 4 s of the 100 MHz clock
            if (__hip_atomic_load(p.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & GH_ST_TIMEOUT) break;
            const unsigned long long t = wall_clock64();
            if (t0w == 0) {
              t0w = t;
            } else if (t - t0w > 400000000ull) {
              if (lane == 0) atomicOr(p.status, (unsigned)GH_ST_TIMEOUT);
              break;
            }
          }
          __builtin_amdgcn_s_sleep(1);
        }
        got = granule_ok(p, g, 2);  // false only after a timeout (then nothing is written)
      }
      // the tile's offsets were in LDS before its aggregate left, and the aggregate before
      // its prefix: read them only now (no compiler hoisting above the check)
      asm volatile("" ::: "memory");
      goff = (g & GRAN_VMASK) + s_off[slot2 * NW + wid];
      if (GH_TILE_ABLATE & 32) goff &= ~15ull;  // (diagnostic: 16-byte aligned pieces, wrong output)
      n2 = s_tot[slot2 * NW + wid];
      rec = got;
      if (wid == NW - 1 && t2 == p.ntiles - 1 && got && lane == 0) {
        *p.total = goff + n2;
        p.piece_off[16ull * p.ntiles] = goff + n2;  // the table's last entry
      }
#if GH_TILE_STAMPS
      if (wid == 0 && lane == 0) p.tstamps[p.ntiles + t2] = __builtin_amdgcn_s_memrealtime() | ((unsigned long long)polled << 63);
#endif
      n2 = (!got || goff >= p.out_cap) ? 0u : (uint32_t)min<unsigned long long>(n2, p.out_cap - goff);
    }
    TSTAMP(4);
    // ---- record the piece's offset (before the out_cap clamp) ------------------------------
    // Unconditional, like the copy-out's stores: lane 0 stores entry 16 t2 + wid, every other
    // lane, and every lane of a wave with no piece, at the dropped out-of-range offset.
    {
      const uint32_t ro = (rec && lane == 0) ? 8u * (16u * t2 + (uint32_t)wid) : OOB_OFF;
      __builtin_amdgcn_raw_buffer_store_b64(tile_v2u{(uint32_t)goff, (uint32_t)(goff >> 32)}, rs_po, (int)ro, 0, 0);
    }
    // ---- copy this wave's piece of tile k-LAG out ----------------------------------------
    // Unconditional (nothing to copy: n2 = 0, every store dropped): the same store count
    // on every path lets the compiler wait for the prefetched loads with a counted vmcnt
    // at the top of the next iteration.
    if (!(GH_TILE_ABLATE & 8)) {
      tile_v4u cv[TILE_NS];
      uint32_t cb;
      copy_out_piece<TILE_NS, false>(p.out, region0 + buf * NW * p.stage_bytes, goff, n2, lane, cv, cb);
    }
    TSTAMP(5);
    // ---- stage this tile's piece (copied out LAG iterations later) ----------------------
    // a piece larger than the region (data whose shortest codewords cluster) waits for
    // the tile's prefix instead and stores its bytes straight from registers (it has
    // published its arrival, so the prefix cannot depend on it)
    const bool staged = have_cur && wave_tot <= piece_cap;
    if (have_cur && !staged) {
      unsigned long long goffc = 0;
      bool got = true;
      if (lane == 0) {
        unsigned long long g = __hip_atomic_load(&p.prefix[cur], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!granule_ok(p, g, 2)) g = poll_granule(p, &p.prefix[cur], 2);
        got = granule_ok(p, g, 2);  // false only after a timeout (then nothing is written)
        asm volatile("" ::: "memory");
        goffc = (g & GRAN_VMASK) + s_off[slot * NW + wid];
        if (got) p.piece_off[16ull * cur + (uint32_t)wid] = goffc;
        if (wid == NW - 1 && cur == p.ntiles - 1 && got) {
          *p.total = goffc + wave_tot;
          p.piece_off[16ull * p.ntiles] = goffc + wave_tot;
        }
      }
      goffc = rfl_u64(goffc);
      if (__builtin_amdgcn_readfirstlane(got ? 1 : 0)) {
#pragma unroll
        for (int u = 0; u < U; ++u) store_direct(p.out, p.out_cap, goffc + bpos[u], ow[u], cnt[u]);
      }
      // (rare path) drain its data-dependent loads and stores here, so that the
      // compiler's wait for the next tile's loads stays a counted vmcnt on the common path
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    } else if (have_cur && !(GH_TILE_ABLATE & 2)) {
      const uint32_t sbase = region0 + buf * NW * p.stage_bytes + STAGE_PAD;
      uint32_t o[U];
#pragma unroll
      for (int u = 0; u < U; ++u) o[u] = sbase + bpos[u];
      // no segment of the wave holds more than GRP * gdone codewords: rounds above its
      // last dword are skipped
      stage_wave<U, OW>(ow, cnt, o, min(OW, (GRP * gdone + 3) >> 2));
    }
    TSTAMP(6);
#pragma unroll
    for (int i = TILE_LAG - 1; i > 0; --i) th[i] = th[i - 1];
    th[0] = staged ? cur : NONE;
    }
#if GH_TILE_STAMPS
    TSTAMP(7);
    TSTAMP(8);
    if (lane == 0 && (wid == 0 || wid == NW / 2) && k < 128) {  // the first wave of each half
      uint4* st = p.stamps + (((unsigned long long)blockIdx.x * 2 + (wid ? 1 : 0)) * 128 + k) * 2;
      st[0] = make_uint4((uint32_t)(ts[1] - ts[0]), (uint32_t)(ts[2] - ts[1]), (uint32_t)(ts[3] - ts[2]),
                         (uint32_t)(ts[4] - ts[3]));
      st[1] = make_uint4((uint32_t)(ts[5] - ts[4]), (uint32_t)(ts[6] - ts[5]), (uint32_t)(ts[7] - ts[6]),
                         (uint32_t)(ts[8] - ts[7]));
    }
#endif
    cur = nxt < p.ntiles ? nxt : NONE;
    nxt += G;
    return true;
  };
  for (uint32_t k = 0;; ++k)
    if (!body(k)) break;
#if GH_TILE_STAMPS
  if (tid == 0) {
    wring[2] = __builtin_amdgcn_s_memtime();
    wring[3] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}
