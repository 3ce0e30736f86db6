// Batched encode (gaphuff.h, "batched encode"), included by gh_encode.hip after its device
// helpers (enc_byte, enc_pair and the left-aligned entry code << (32 - len) | len are
// shared, not copied).  No reference counterpart: the reference encodes one input per call.
// The structure is the batched decoder's (gh_batch.hip), and what the two have in common is
// shared: the unit walk (stream search, cursor, a wave's run) is gh_units.hpp, the wave scan,
// rfl_u64 and the scan kernel's body (block_excl_scan) are gh_wave.hpp.
//
// A batch is many independent inputs, each with its own canonical code, packed into one
// padded input arena; the images' payload and gap words go to one payload arena and one gap
// arena (the host layout: gh::ebatch_in_plan / gh::ebatch_out_plan, gh_core.cpp).  The unit
// of work is GH_EBATCH_UNIT_BYTES = 1024 consecutive input bytes of one stream: one wave,
// 64 lanes x 16 bytes.  unit0[0 .. nstreams] is the prefix of the streams' unit counts; a
// wave finds its unit's stream by binary search there and the stream's extents in an
// EBatchDesc.
//
//   gh_ebatch_copy_kernel   device loads only: copies every stream's bytes from the caller's
//                           pointers (any byte alignment, exactly n_i bytes read) into the
//                           padded input arena, zeros after them (one launch for the batch);
//   gh_ebatch_hist_kernel   every stream's byte histogram: per-wave LDS counters, flushed
//                           with global u64 atomics into counts[stream][256] when the wave's
//                           run leaves the stream;
//   (host)                  one gh::plan_from_counts per stream, threaded over streams; or
//   gh_ebatch_code_kernel   (gh_batchenc_plan_device) one workgroup per stream: sort, the
//                           package-merge level by level (gh_pm_flat.hpp), canonical codes,
//                           the stream's table and a 528-byte record for the host; at the
//                           end of this file;
//   gh_ebatch_bits_kernel   code bits per unit (u32);
//   gh_ebatch_scan_kernel   one workgroup: exclusive u64 scan of the unit bits; a unit's bit
//                           offset inside its stream is its scan value minus that of the
//                           stream's first unit.  Every stream's total is compared with the
//                           host plan's `bits`: GH_ST_LAYOUT on a difference (a tripwire);
//   gh_ebatch_write_kernel  per unit: wave scan of the lanes' bits, the 16 codewords per lane
//                           as pairs and quads ORed into the wave's own zeroed LDS image,
//                           gap nibbles by gh_enc_write_kernel's rule, the image stored and
//                           re-zeroed.
//
// No wave waits for another and there is no workgroup barrier in the per-unit kernels: every
// wave keeps its OWN copy of the current stream's 256-entry table (and its own counters or
// image) in its own LDS region and reloads the table only when the stream changes (one
// wave's LDS operations complete in order).  A wave takes a contiguous run of units,
// [w nunits / nwaves, (w + 1) nunits / nwaves).  Every loop is bounded by counts the host
// knows (units, streams, 16 bytes per lane, at most 3 boundaries per lane): no kernel here
// can hang.  The table is kept once per wave (no replicas): 64 lanes reading one 1 KiB
// table conflict a few ways; replication was not measured.
//
// Ownership (gh_enc_write_kernel's): a unit owns the payload words whose first bit it holds
// and stores them plainly; it completes its last word from the first (at most 31) codewords
// of the next unit OF THE SAME STREAM -- the completion lanes are masked by the stream's own
// n, and the input arena pads every stream so that those loads stay inside its extent.  Gap
// words: interior ones stored plainly, the unit's first and last one (shared with its
// neighbours in the stream) ORed into the zeroed gap arena with atomics.  Streams never
// share a word: every stream's payload and gap extent starts on its own 16-byte boundary.

constexpr int EB_TB = 256;                          // threads per workgroup: four waves, four regions
constexpr int EB_WAVES = EB_TB / 64;
constexpr uint32_t EB_UNIT = GH_EBATCH_UNIT_BYTES;  // input bytes per unit
constexpr uint32_t EB_TABLE = 260;                  // entries per wave: 256, then "absent" (0), padded to 16 bytes
// LDS image of a unit from its gap-word-aligned base: up to 1023 bits before it, 16 bits per
// byte, the last word's completion (< 32 + 16 bits), two words of slack for the quads'
// unconditional ORs
constexpr uint32_t EB_WORDS = (1024 + EB_UNIT * GH_MAX_CODE_LEN + 64) / 32 + 2;
constexpr uint32_t EB_GAPW = (1024 + EB_UNIT * GH_MAX_CODE_LEN) / 1024 + 2;
constexpr int EB_SCAN_TB = 1024;
constexpr int EB_COPY_Y = 8;                        // slices a stream's bytes are copied in
constexpr uint32_t EB_FLUSH_UNITS = 1u << 21;       // histogram counters are u32: flushed every 2^31 bytes at the latest
static_assert(EB_UNIT == 64 * EBPT, "a work unit is one wave of 16-byte lanes");
static_assert(EB_UNIT == EBATCH_UNIT_BYTES, "the host layout's unit");
static_assert(EB_GAPW <= 64, "one gap word per lane");
static_assert(EB_WAVES * 4 * (EB_TABLE + EB_WORDS + EB_GAPW) <= 64 * 1024, "the waves' regions fit the LDS");

// One stream of the batch (device memory, 64 bytes).
struct EBatchDesc {
  unsigned long long in_off;   // first input byte in the input arena (a multiple of 16)
  unsigned long long n;        // input bytes
  unsigned long long pay_off;  // first payload word in the payload arena (a multiple of 4)
  unsigned long long gap_off;  // first gap word in the gap arena (a multiple of 4)
  unsigned long long bits;     // the host plan's bit total
  unsigned long long pad[3];
};
static_assert(sizeof(EBatchDesc) == 64, "EBatchDesc layout");

struct EBatchCopyItem {
  const uint8_t* src;            // caller's bytes, any alignment
  unsigned long long n;
  unsigned long long in_off, in_bytes;  // destination extent in the input arena (zero past n)
};

struct EBatchParams {
  const EBatchDesc* desc;
  const uint32_t* unit0;          // nstreams + 1
  const uint8_t* in;              // the input arena
  const uint32_t* tables;         // 256 left-aligned entries per stream
  unsigned long long* counts;     // 256 per stream (histogram)
  uint32_t* unit_bits;            // code bits per unit
  unsigned long long* unit_off;   // nunits + 1: exclusive scan of unit_bits
  uint32_t* payload;              // the payload arena (zeroed)
  uint32_t* gaps;                 // the gap arena (zeroed)
  unsigned int* status;           // per stream (GH_ST_*), written by the scan kernel
  unsigned int* summary;          // [0] streams with a status bit, [1] OR of the status words
  uint32_t nstreams, nunits;
};

__device__ __forceinline__ void ebatch_wave_sync() {
  // orders one wave's LDS operations across its lanes for the compiler (the hardware
  // completes them in order): no instruction beyond a wait
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void gh_ebatch_copy_kernel(const EBatchCopyItem* items, uint32_t nstreams,
                                                              uint8_t* in) {
  const uint32_t step = 256u * gridDim.y, t0 = blockIdx.y * 256u + threadIdx.x;
  for (uint32_t s = blockIdx.x; s < nstreams; s += gridDim.x) {
    const EBatchCopyItem it = items[s];
    uint32_t* dst = (uint32_t*)(in + it.in_off);  // (in_off and in_bytes are multiples of 16)
    const bool al = (((uintptr_t)it.src) & 3u) == 0;
    for (unsigned long long j = t0; j < it.in_bytes / 4; j += step) {
      const unsigned long long b = 4 * j;
      uint32_t x = 0;
      if (al && b + 4 <= it.n) {
        x = *(const uint32_t*)(it.src + b);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (b + k < it.n) x |= (uint32_t)it.src[b + k] << (8 * k);
      }
      dst[j] = x;
    }
  }
}

// The wave's view of the unit it is working on.
struct EBatchUnit {
  UnitCursor c;
  EBatchDesc d;
};

// Points un at unit u; returns true when the stream changed.
__device__ __forceinline__ bool ebatch_enter(const EBatchParams& p, uint32_t u, EBatchUnit& un) {
  if (!unit_enter(p.unit0, p.nstreams, u, un.c)) return false;
  un.d = p.desc[un.c.s];
  return true;
}

// The stream's table into the wave's LDS region: one 16-byte load and store per lane, and
// the "absent" entry.
__device__ __forceinline__ void ebatch_load_table(const EBatchParams& p, uint32_t s, uint32_t* s_lut, int lane) {
  ebatch_wave_sync();  // the previous stream's lookups are done
  ((uint4*)s_lut)[lane] = ((const uint4*)(p.tables + 256ull * s))[lane];
  if (lane == 0) s_lut[256] = 0u;
  ebatch_wave_sync();
}

// The lane's 16 bytes of the unit (absent past n: 0x100).  The load is unconditional: the
// arena pads every stream to whole units.
__device__ __forceinline__ void ebatch_bytes(const EBatchParams& p, const EBatchUnit& un, int lane, uint32_t (&b)[EBPT]) {
  const unsigned long long ib = (unsigned long long)un.c.blk * EB_UNIT + (uint32_t)lane * EBPT;
  const uint4 v = *(const uint4*)(p.in + un.d.in_off + ib);
  if (ib + EBPT <= un.d.n) {
#pragma unroll
    for (int k = 0; k < EBPT; ++k) b[k] = enc_byte(v, k);
  } else {
    const uint32_t rem = ib < un.d.n ? (uint32_t)(un.d.n - ib) : 0u;
#pragma unroll
    for (int k = 0; k < EBPT; ++k) b[k] = (uint32_t)k < rem ? enc_byte(v, k) : 0x100u;
  }
}

__global__ __launch_bounds__(EB_TB) void gh_ebatch_hist_kernel(const EBatchParams p) {
  __shared__ uint32_t s_cnt[EB_WAVES][256];
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* h = s_cnt[wid];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[lane + 64 * k] = 0;
  ebatch_wave_sync();
  // the wave's counters into the stream's global counts, and back to zero
  auto flush = [&](uint32_t s) {
    ebatch_wave_sync();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t c = h[lane + 64 * k];
      h[lane + 64 * k] = 0;
      if (c) atomicAdd(&p.counts[256ull * s + (uint32_t)(lane + 64 * k)], (unsigned long long)c);
    }
    ebatch_wave_sync();
  };
  uint32_t u0, u1;
  unit_run<EB_WAVES>(p.nunits, wid, u0, u1);
  EBatchUnit un;
  uint32_t since = 0;  // units counted since the last flush
  for (uint32_t u = u0; u < u1; ++u) {
    const uint32_t prev = un.c.s;
    const bool changed = ebatch_enter(p, u, un);
    if ((changed && prev != 0xFFFFFFFFu) || since == EB_FLUSH_UNITS) {
      flush(changed ? prev : un.c.s);
      since = 0;
    }
    uint32_t b[EBPT];
    ebatch_bytes(p, un, lane, b);
#pragma unroll
    for (int k = 0; k < EBPT; ++k)
      if (b[k] < 256u) atomicAdd(&h[b[k]], 1u);
    ++since;
  }
  if (un.c.s != 0xFFFFFFFFu) flush(un.c.s);
}

__global__ __launch_bounds__(EB_TB) void gh_ebatch_bits_kernel(const EBatchParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[EB_WAVES][EB_TABLE];
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* s_lut = s_tab[wid];
  uint32_t u0, u1;
  unit_run<EB_WAVES>(p.nunits, wid, u0, u1);
  EBatchUnit un;
  for (uint32_t u = u0; u < u1; ++u) {
    if (ebatch_enter(p, u, un)) ebatch_load_table(p, un.c.s, s_lut, lane);
    uint32_t b[EBPT], bits = 0;
    ebatch_bytes(p, un, lane, b);
#pragma unroll
    for (int k = 0; k < EBPT; ++k) bits += s_lut[b[k]];  // (the entries' low 16 bits hold only their lengths)
    bits &= 0xFFFFu;
    const uint32_t incl = wave_incl_scan(bits);
    if (lane == 63) p.unit_bits[u] = incl;
  }
}

// One workgroup: exclusive scan of the unit bits, then every stream's total against its plan.
__global__ __launch_bounds__(EB_SCAN_TB) void gh_ebatch_scan_kernel(const EBatchParams p) {
  __shared__ unsigned long long s_w[EB_SCAN_TB / 64];
  __shared__ unsigned int s_sum[2];
  const int tid = threadIdx.x;
  if (tid < 2) s_sum[tid] = 0;  // (ordered before the epilogue's atomics by the scan's barrier)
  const unsigned long long all = block_excl_scan<EB_SCAN_TB>(p.unit_bits, p.unit_off, p.nunits, s_w);
  if (tid == 0) p.unit_off[p.nunits] = all;
  __threadfence();
  __syncthreads();
  for (uint32_t i = tid; i < p.nstreams; i += EB_SCAN_TB) {
    const unsigned long long tot = p.unit_off[p.unit0[i + 1]] - p.unit_off[p.unit0[i]];
    const unsigned int st = tot != p.desc[i].bits ? (unsigned)GH_ST_LAYOUT : 0u;
    p.status[i] = st;
    if (st) {
      atomicAdd(&s_sum[0], 1u);
      atomicOr(&s_sum[1], st);
    }
  }
  __syncthreads();
  if (tid < 2) p.summary[tid] = s_sum[tid];
}

__global__ __launch_bounds__(EB_TB) void gh_ebatch_write_kernel(const EBatchParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[EB_WAVES][EB_TABLE];
  __shared__ uint32_t s_img[EB_WAVES][EB_WORDS];
  __shared__ uint32_t s_gap[EB_WAVES][EB_GAPW];
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* s_lut = s_tab[wid];
  uint32_t* s_w = s_img[wid];
  uint32_t* s_g = s_gap[wid];
  for (uint32_t i = lane; i < EB_WORDS; i += 64) s_w[i] = 0;
  if ((uint32_t)lane < EB_GAPW) s_g[lane] = 0;
  uint32_t u0, u1;
  unit_run<EB_WAVES>(p.nunits, wid, u0, u1);
  EBatchUnit un;
  unsigned long long off_first = 0;  // the scan value of the stream's first unit
  for (uint32_t u = u0; u < u1; ++u) {
    if (ebatch_enter(p, u, un)) {
      ebatch_load_table(p, un.c.s, s_lut, lane);
      off_first = p.unit_off[un.c.first];
    }
    ebatch_wave_sync();  // the previous unit's write-out and re-zeroing come before this unit's ORs
    // the unit's first bit inside its stream
    const unsigned long long o0 = rfl_u64(p.unit_off[u] - off_first);
    uint32_t b[EBPT];
    ebatch_bytes(p, un, lane, b);
    // the next unit's byte `lane` (lanes 0..31), for the last word: inside the stream's own
    // padded extent, and masked by the stream's own n
    const unsigned long long xb = (unsigned long long)(un.c.blk + 1u) * EB_UNIT;
    const uint32_t nx = p.in[un.d.in_off + xb + (uint32_t)(lane & 31)];
    uint32_t e[EBPT], bits = 0;
#pragma unroll
    for (int k = 0; k < EBPT; ++k) e[k] = s_lut[b[k]];
#pragma unroll
    for (int k = 0; k < EBPT; ++k) bits += e[k];  // (the entries' low 16 bits hold only their lengths)
    bits &= 0xFFFFu;
    const uint32_t incl = wave_incl_scan(bits);
    const uint32_t cbits = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    // never expected (the scan kernel flags the stream): a unit that would end past its
    // stream's planned bits stores nothing, so no store leaves the stream's extents
    if (o0 + cbits > un.d.bits) continue;
    const uint32_t excl = incl - bits;
    // positions relative to B = the unit's offset rounded down to a gap word (1024 bits):
    // 128-bit boundaries, payload words and gap words keep their alignment
    const unsigned long long B = o0 & ~1023ull;
    const uint32_t qs = (uint32_t)(o0 - B);  // unit start
    const uint32_t qend = qs + cbits;        // unit end (the next unit's first bit)
    const uint32_t q0 = qs + excl;           // this lane's first bit
    // pairs and quads (left-aligned), the quads ORed into the image
    uint32_t pl[EBPT / 2], pv[EBPT / 2];
#pragma unroll
    for (int j = 0; j < EBPT / 2; ++j) pv[j] = enc_pair(e[2 * j], e[2 * j + 1], pl[j]);
    uint32_t qa = q0, qe[EBPT / 4];
#pragma unroll
    for (int i = 0; i < EBPT / 4; ++i) {
      const uint32_t l0 = pl[2 * i], m = l0 + pl[2 * i + 1];
      const unsigned long long Q = ((unsigned long long)pv[2 * i] << 32) |
                                   ((unsigned long long)pv[2 * i + 1] << (32u - l0));
      const uint32_t hi = (uint32_t)(Q >> 32), lo = (uint32_t)Q, sft = qa & 31u;
      uint32_t* wp = &s_w[qa >> 5];  // (qa <= 1023 + 16 x 1024: wp + 2 stays inside EB_WORDS)
      atomicOr(wp, hi >> sft);       // ORing zero bits is harmless: no compares
      atomicOr(wp + 1, __builtin_amdgcn_alignbit(hi, lo, sft));
      atomicOr(wp + 2, __builtin_amdgcn_alignbit(lo, 0u, sft));
      qa += m;
      qe[i] = qa;
    }
    // gap nibbles: for each 128-bit boundary strictly inside [q0, qa), the codeword holding
    // bits bd-1 and bd (quad, then pair, then codeword by compare-selects); a lane holds at
    // most 256 bits, so at most 3 boundaries
    for (uint32_t bd = ((q0 >> 7) + 1u) << 7; bd < qa; bd += 128u) {
      const bool i0 = bd >= qe[0], i1 = bd >= qe[1], i2 = bd >= qe[2];
      const uint32_t qs4 = i2 ? qe[2] : i1 ? qe[1] : i0 ? qe[0] : q0;
      const uint32_t la = i2 ? pl[6] : i1 ? pl[4] : i0 ? pl[2] : pl[0];
      const uint32_t lb = i2 ? pl[7] : i1 ? pl[5] : i0 ? pl[3] : pl[1];
      const uint32_t ea = i2 ? e[12] : i1 ? e[8] : i0 ? e[4] : e[0];
      const uint32_t eb = i2 ? e[14] : i1 ? e[10] : i0 ? e[6] : e[2];
      const bool second = bd >= qs4 + la;  // in the quad's second pair
      const uint32_t ps = second ? qs4 + la : qs4;
      const uint32_t lp = second ? lb : la;
      const uint32_t l1 = (second ? eb : ea) & 31u;  // the pair's first codeword
      const bool c2 = bd >= ps + l1;
      const uint32_t cs = c2 ? ps + l1 : ps;        // codeword start
      const uint32_t ce = c2 ? ps + lp : ps + l1;   // codeword end
      const uint32_t gv = ce & 15u;
      if (cs < bd && gv) atomicOr(&s_g[cs >> 10], gv << (4 * ((cs >> 7) & 7u)));
    }
    {
      // complete the unit's last word (bits [qend, wend)) with the next unit's first
      // codewords, one per lane (lanes 0..31: bytes 0..31, codes >= 1 bit); their gap
      // nibbles belong to the next unit.  Past the stream's n: nothing (never the next stream)
      const uint32_t wend = (qend + 31u) & ~31u;
      const uint32_t ex = (lane < 32 && xb + (uint32_t)lane < un.d.n) ? s_lut[nx] : 0u;
      const uint32_t lx = ex & 31u;
      const uint32_t st = qend + wave_incl_scan(lx) - lx;  // this codeword's first bit
      if (lx && st < wend) {
        const uint32_t cw = ex & 0xFFFF0000u, sh = st & 31u;  // left-aligned code
        atomicOr(&s_w[st >> 5], cw >> sh);
        if (sh + lx > 32u) atomicOr(&s_w[(st >> 5) + 1], cw << (32u - sh));
      }
    }
    ebatch_wave_sync();
    // payload words whose first bit lies in [o0, o0 + cbits): local [w0, w1); the image is
    // zeroed as it is read (up to the completion word)
    const uint32_t w0 = (qs + 31u) >> 5, w1 = (qend + 31u) >> 5;
    uint32_t* wout = p.payload + un.d.pay_off + (B >> 5);
    for (uint32_t i = (uint32_t)lane; i <= w1; i += 64) {
      const uint32_t x = s_w[i];
      s_w[i] = 0;
      if (i >= w0 && i < w1) wout[i] = x;
    }
    // gap words of this unit's segments: local [0, g1]; the first and the last may hold
    // nibbles of the neighbouring units of the stream
    const uint32_t g1 = cbits ? (qend - 1u) >> 10 : 0u;
    uint32_t* gout = p.gaps + un.d.gap_off + (B >> 10);
    if (cbits && (uint32_t)lane <= g1) {
      const uint32_t x = s_g[lane];
      s_g[lane] = 0;
      if (lane == 0 || (uint32_t)lane == g1) {
        if (x) atomicOr(&gout[lane], x);
      } else {
        gout[lane] = x;
      }
    }
  }
}

// ---- codes built on the device (gh_batchenc_plan_device) ------------------------------------
// What the code kernel leaves for the host per stream: all it needs for the image's header
// and the output layout.
struct EBatchCodeRec {
  unsigned long long bits;  // sum len * count
  uint32_t nsyms, zero;
  gh_sym syms[GH_MAX_SYMBOLS];  // file order (most frequent first), zero past nsyms
};
static_assert(sizeof(EBatchCodeRec) == 528 && sizeof(gh_sym) == 2, "EBatchCodeRec layout");

// One workgroup per stream (grid-stride over streams): from counts[stream][256] to the
// stream's 256 table entries and its record.  plan_from_counts' steps (gh_core.cpp) with the
// package-merge in its level-by-level form (gh_pm_flat.hpp, the arithmetic of
// gh_package_merge_flat): stable sort of the present symbols by (count, symbol value) as
// 256 compares per thread, 15 level steps (thread t places leaf t and package t: every
// level holds at most 256 leaves and 255 packages), the trace by one thread over prefix
// popcounts, the canonical code from the counts per length as gh_batch_table_kernel forms it.
// Everything is in LDS (about 16 KB).  The only synchronisation is __syncthreads(), and no
// barrier stands inside a branch: a stream of 0 or 1 symbols runs the same steps with nothing
// to place (pm_need = 0), and ns is computed by every thread from the same LDS words.  The
// loops are bounded by nstreams, 256, 16 and the binary searches' 9 steps.
__global__ __launch_bounds__(EB_TB) void gh_ebatch_code_kernel(const unsigned long long* counts, uint32_t* tables,
                                                                EBatchCodeRec* recs, uint32_t nstreams) {
  static_assert(EB_TB == GH_MAX_SYMBOLS && EB_TB == PM_LEVELS * PM_MASK_WORDS, "a thread per symbol and per mask word");
  __shared__ uint64_t s_cnt[256];      // by symbol value
  __shared__ uint64_t s_c[256];        // sorted ascending: the leaves
  __shared__ uint64_t s_w[2][PM_MAX_ITEMS];  // the level below and the level being built
  __shared__ uint32_t s_mask[PM_LEVELS * PM_MASK_WORDS], s_pre[PM_LEVELS * PM_MASK_WORDS];
  __shared__ uint32_t s_nl[PM_LEVELS];
  __shared__ uint32_t s_lcnt[PM_LEVELS + 1], s_base[PM_LEVELS + 1], s_first[PM_LEVELS + 1];
  __shared__ uint32_t s_ent[256];                   // the table, by symbol value
  __shared__ uint32_t s_hdr[128];                   // the record's syms, two per word
  __shared__ uint8_t s_sym[256];                    // symbol value by sorted rank
  __shared__ unsigned long long s_bits[EB_WAVES];
  const uint32_t tid = threadIdx.x;
  for (uint32_t s = blockIdx.x; s < nstreams; s += gridDim.x) {
    __syncthreads();  // the previous stream's stores have read the LDS
    s_cnt[tid] = counts[256ull * s + tid];
    s_mask[tid] = 0;
    s_ent[tid] = 0;
    if (tid < 128) s_hdr[tid] = 0;
    if (tid <= PM_LEVELS) s_lcnt[tid] = 0;
    __syncthreads();
    // a. the sort: rank among the present symbols by (count, symbol value)
    const uint64_t cv = s_cnt[tid];
    uint32_t n = 0, r = 0;
    for (uint32_t u = 0; u < 256; ++u) {
      const uint64_t cu = s_cnt[u];
      n += cu != 0;
      r += cu != 0 && (cu < cv || (cu == cv && u < tid));
    }
    if (cv) {
      s_c[r] = cv;
      s_sym[r] = (uint8_t)tid;
    }
    __syncthreads();
    // b. levels 2 .. 16 (level 1 is s_c itself), then the trace
    const uint32_t need = pm_need(n);
    const uint64_t* prev = s_c;
    uint32_t m = n;
    for (uint32_t l = 1; l < PM_LEVELS; ++l) {
      uint64_t* next = s_w[l & 1];
      const uint32_t np = m / 2;  // (<= 255)
      if (tid < n) {
        const uint32_t pos = pm_leaf_pos(s_c, prev, np, tid);
        if (pos < need) {
          next[pos] = s_c[tid];
          atomicOr(&s_mask[l * PM_MASK_WORDS + (pos >> 5)], 1u << (pos & 31u));
        }
      }
      if (tid < np) {
        const uint64_t P = pm_package(prev, tid);
        const uint32_t pos = pm_package_pos(s_c, n, tid, P);
        if (pos < need) next[pos] = P;
      }
      m = pm_next_items(n, m);
      __syncthreads();
      prev = next;
    }
    {
      // thread (l, w): the leaves of level l + 1 in the words before w
      const uint32_t row = tid & ~(PM_MASK_WORDS - 1u), w = tid & (PM_MASK_WORDS - 1u);
      uint32_t pre = 0;
      for (uint32_t k = 0; k < PM_MASK_WORDS; ++k) pre += k < w ? (uint32_t)__builtin_popcount(s_mask[row + k]) : 0u;
      s_pre[tid] = pre;
    }
    __syncthreads();
    if (tid == 0) pm_trace(s_mask, s_pre, n, s_nl);
    __syncthreads();
    uint32_t len = 0;
    if (tid < n) {
      len = n == 1 ? 1u : pm_length(s_nl, tid);
      atomicAdd(&s_lcnt[len], 1u);  // (len <= 16: one per level)
    }
    // c. bits, the canonical code and file order
    const unsigned long long wb = wave_sum_u64(tid < n ? (unsigned long long)len * s_c[tid] : 0ull);
    if ((tid & 63u) == 0) s_bits[tid >> 6] = wb;
    __syncthreads();
    if (tid == 0) pm_canon_bases(s_lcnt, s_base, s_first);
    __syncthreads();
    if (tid < n) {
      const uint32_t f = n - 1u - tid, sym = s_sym[tid];
      s_ent[sym] = pm_canon_entry(s_base, s_first, f, len);
      ((uint16_t*)s_hdr)[f] = (uint16_t)(sym | (len << 8));  // {symbol, length}
    }
    __syncthreads();
    // d. the stores
    tables[256ull * s + tid] = s_ent[tid];
    uint32_t* rec = (uint32_t*)(recs + s);
    if (tid < 128) rec[4 + tid] = s_hdr[tid];
    if (tid == 128) {
      unsigned long long bits = 0;
      for (int q = 0; q < EB_WAVES; ++q) bits += s_bits[q];
      rec[0] = (uint32_t)bits;
      rec[1] = (uint32_t)(bits >> 32);
      rec[2] = n;
      rec[3] = 0;
    }
  }
}
