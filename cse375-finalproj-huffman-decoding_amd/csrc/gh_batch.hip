// Batched decode (gaphuff.h, "batched decode"), included by gh_decode.hip after
// gh_gather_plan.hip.  No reference counterpart: the reference decodes one stream per call.
// The unit walk (stream search, cursor, a wave's run) is gh_units.hpp and the scan kernel's
// body is block_excl_scan (gh_wave.hpp): both shared with the batched encode (gh_ebatch.hip).
//
// A batch is many independent streams, each with its own code, packed into one payload
// arena and one gap arena (the host plan: gh::batch_plan, gh_core.cpp).  The unit of work
// is one wave block of one stream: 256 consecutive segments, 4 chains x 64 lanes (GA_U of
// the gather).  unit0[0 .. nstreams] is the prefix of the streams' unit counts; a wave finds
// its unit's stream by binary search there and the stream's extents in a BatchDesc.
//
//   gh_batch_copy_kernel   device loads only: copies every stream's words from the caller's
//                          pointers into the padded arenas (one launch for the batch);
//   gh_batch_table_kernel  one workgroup per stream: count per length, then first / base16 /
//                          limit16, the canonical fallback words (FB_WORDS layout) and a
//                          single-codeword table {len | sym << 8} of K = min(maxlen, BA_KMAX)
//                          bits, filled by codeword: a thread per symbol stores 2^(K - l)
//                          entries; codewords longer than K and patterns outside an
//                          incomplete code keep 0 (the decode then takes the fallback);
//   gh_batch_count_kernel  counts the codewords of every segment (1 byte each) and of
//                          every unit;
//   gh_batch_scan_kernel   one workgroup: exclusive u64 scan of the unit totals, then per
//                          stream its total (the difference to the next stream's first
//                          unit), GH_ST_BADCODE when that is below N, and the batch summary;
//   gh_batch_write_kernel  decodes each unit again: symbol s of stream i goes to
//                          out[out_off[i] + s] for s < n_i only (byte stores, as the gather).
//
// No wave waits for another and there is no workgroup barrier in the count and write
// kernels: every wave keeps its OWN copy of the current stream's tables in its own LDS
// region and reloads it only when the stream changes (one wave's LDS operations complete in
// order).  A wave takes a contiguous run of units, units [w nunits / nwaves, (w + 1) nunits
// / nwaves), so a stream of several units costs it one table load.  A segment's rule is the
// wave split's: it owns the codewords that start in [start, E), E = 128 + its gap nibble;
// the stream's last segment owns those that start before bit 128, padding included (what
// last_segment_end gives the wave split).  A corrupt stream stays inside its own extents:
// loads are clamped to its segments, a segment's walk ends after its E - start bits, and
// stores are clipped at its N.

constexpr int BA_U = 4;              // chains per lane: a unit is 256 segments
constexpr int BA_TB = 256;           // threads per workgroup: four waves, four table regions
constexpr uint32_t BA_KMAX = 10;     // widest lookup table: 4 KB + FB_BYTES per wave
constexpr uint32_t BA_FBW = FB_BYTES / 4;                       // fallback words, 16-byte padded
constexpr uint32_t BA_REGION = FB_BYTES + (4u << BA_KMAX);      // LDS bytes per wave
constexpr int BA_SCAN_TB = 1024;
constexpr int BA_COPY_Y = 8;         // slices a stream's words are copied in
static_assert(64 * BA_U == (int)BATCH_UNIT_SEGS, "a work unit is one wave block");
static_assert((BA_TB / 64) * BA_REGION <= 64 * 1024, "the waves' table regions fit the LDS");

// One stream of the batch (device memory, 64 bytes).
struct BatchDesc {
  unsigned long long pay_off;   // first payload word in the arena (a multiple of 4)
  unsigned long long gap_off;   // first gap word in the arena
  unsigned long long n;         // output bytes
  unsigned long long out_off;   // first output byte in the destination
  unsigned long long tab_off;   // first table word: BA_FBW fallback words, then max(1 << kbits, 4) entries
  uint32_t nseg;
  uint32_t kbits;               // K = min(maxlen, BA_KMAX); 0 for a stream without segments
  uint32_t minlen, maxlen;
  uint32_t sym_off, nsyms;      // the stream's entries in the packed (symbol, length) list
};
static_assert(sizeof(BatchDesc) == 64, "BatchDesc layout");

struct BatchCopyItem {
  const uint32_t* pay;          // caller's words (4-byte aligned), w of them
  const uint32_t* gap;
  unsigned long long w;
  unsigned long long pay_off, pay_words;  // destination extent in the payload arena (zero past w)
  unsigned long long gap_off, gap_words;
};

struct BatchParams {
  const BatchDesc* desc;
  const uint32_t* unit0;        // nstreams + 1
  const uint32_t* payload;
  const uint32_t* gaps;
  const uint32_t* tables;
  uint8_t* seg_cnt;             // codewords per segment, 256 per unit
  uint32_t* unit_tot;           // codewords per unit
  unsigned long long* unit_off; // nunits + 1: exclusive scan of unit_tot
  unsigned int* status;         // per stream (GH_ST_*)
  unsigned long long* symbols;  // per stream: codewords counted
  unsigned int* summary;        // [0] streams with a status bit, [1] OR of the status words
  uint8_t* out;
  uint32_t nstreams, nunits;
};

__global__ __launch_bounds__(256) void gh_batch_copy_kernel(const BatchCopyItem* items, uint32_t nstreams,
                                                             uint32_t* payload, uint32_t* gaps) {
  const uint32_t step = 256u * gridDim.y, t0 = blockIdx.y * 256u + threadIdx.x;
  for (uint32_t s = blockIdx.x; s < nstreams; s += gridDim.x) {
    const BatchCopyItem it = items[s];
    for (unsigned long long i = t0; i < it.pay_words; i += step) payload[it.pay_off + i] = i < it.w ? it.pay[i] : 0u;
    for (unsigned long long i = t0; i < it.gap_words; i += step) gaps[it.gap_off + i] = it.gap[i];
  }
}

__global__ __launch_bounds__(256) void gh_batch_table_kernel(const BatchDesc* desc, const gh_sym* syms,
                                                              uint32_t* tables, uint32_t nstreams) {
  __shared__ uint32_t s_cnt[17], s_first[17], s_base[17];
  __shared__ uint32_t s_fb[BA_FBW];
  const uint32_t tid = threadIdx.x;
  for (uint32_t s = blockIdx.x; s < nstreams; s += gridDim.x) {
    const BatchDesc d = desc[s];
    if (d.nseg == 0 || d.nsyms == 0) continue;  // (the same for the whole workgroup)
    uint32_t* fb = tables + d.tab_off;
    uint32_t* lut = fb + BA_FBW;
    const uint32_t K = d.kbits, nent = max(1u << K, 4u);
    __syncthreads();  // the previous stream's tables have left the LDS
    if (tid < 17) s_cnt[tid] = 0;
    for (uint32_t i = tid; i < BA_FBW; i += 256) s_fb[i] = 0;
    for (uint32_t i = tid; i < nent; i += 256) lut[i] = 0;
    __syncthreads();
    uint32_t l = 0, sym = 0;
    if (tid < d.nsyms) {  // (nsyms <= 256, lengths 1..16 in non-decreasing order: validated by the load)
      const gh_sym e = syms[d.sym_off + tid];
      l = e.length;
      sym = e.symbol;
      atomicAdd(&s_cnt[l], 1u);
      ((uint8_t*)(s_fb + 51))[tid] = (uint8_t)sym;
    }
    __syncthreads();
    if (tid == 0) {
      // build_canon's code assignment by length: `code` is the next free code on the
      // length-l scale; limit16 is carried forward over empty lengths (fallback_tables)
      uint32_t code = 0, first = 0, run = 0;
      for (uint32_t k = 1; k <= 16; ++k) {
        code <<= 1;
        s_first[k] = first;
        s_base[k] = code << (16 - k);
        code += s_cnt[k];
        first += s_cnt[k];
        if (s_cnt[k]) run = code << (16 - k);
        s_fb[k] = run;
        s_fb[17 + k] = s_base[k];
        s_fb[34 + k] = s_first[k];
      }
    }
    __syncthreads();  // (also orders the zeroing of lut before the entries below)
    for (uint32_t i = tid; i < BA_FBW; i += 256) fb[i] = s_fb[i];
    if (tid < d.nsyms && l <= K) {
      const uint32_t code16 = s_base[l] + ((tid - s_first[l]) << (16 - l));
      const uint32_t i0 = code16 >> (16 - K), e = l | (sym << 8);
      for (uint32_t j = 0; j < (1u << (K - l)); ++j) lut[i0 + j] = e;
    }
  }
}

// The wave's view of the unit it is working on (c.blk: wave block of the stream).
struct BatchUnit {
  UnitCursor c;
  BatchDesc d;
};

// Points un at unit u; when the stream changes, copies its tables into the wave's LDS region.
__device__ __forceinline__ void batch_enter(const BatchParams& bp, uint32_t u, BatchUnit& un, uint8_t* region, int lane) {
  if (unit_enter(bp.unit0, bp.nstreams, u, un.c)) {
    un.d = bp.desc[un.c.s];
    const uint4* g = (const uint4*)(bp.tables + un.d.tab_off);
    const uint32_t n16 = (FB_BYTES + max(4u << un.d.kbits, 16u)) / 16u;
    for (uint32_t i = lane; i < n16; i += 64) ((uint4*)region)[i] = g[i];
  }
}

// Words, start bit and walk length of the lane's segment of chain c (loads clamped to the
// stream's own segments, never skipped).  R: bits from the segment's start in which its
// codewords start; 0 for a lane past the stream's end.
__device__ __forceinline__ Win batch_segment(const BatchParams& bp, const BatchUnit& un, int c, int lane, int& R) {
  const BatchDesc& d = un.d;
  const uint32_t seg = un.c.blk * (uint32_t)(64 * BA_U) + (uint32_t)(64 * c + lane);
  const uint32_t sc = min(seg, d.nseg - 1u);
  const uint32_t* pay = bp.payload + d.pay_off + 4ull * sc;
  const uint4 w = ws_ld16(pay);
  const uint32_t w4 = pay[4];
  const uint32_t* gp = bp.gaps + d.gap_off;
  const uint32_t ga = gp[(sc ? sc - 1u : 0u) >> 3], gb = gp[sc >> 3];
  const int start = sc == 0 ? 0 : (int)gap_nib(ga, sc - 1u);
  const int E = sc == d.nseg - 1u ? 128 : 128 + (int)gap_nib(gb, sc);
  R = seg < d.nseg ? E - start : 0;
  return make_win(w, w4, start);
}

// The codeword at the window position: (symbol << 8) | length.  off: bits of d0 consumed.
template <bool FB>
__device__ __forceinline__ uint32_t batch_lookup(const Win& v, uint32_t off, const uint32_t* s_lut, const uint32_t* s_fb,
                                                 const BatchDesc& d, uint32_t& bad) {
  const uint32_t x = (uint32_t)(((((unsigned long long)v.d0) << 32) | v.d1) >> (32u - off));
  uint32_t e = s_lut[x >> (32u - d.kbits)];
  if constexpr (FB) {
    if ((e & 31u) == 0u) e = ws_canon(s_fb, x >> 16, d.minlen, d.maxlen, bad);
  }
  return e;
}

__device__ __forceinline__ void batch_advance(Win& v, uint32_t& off, uint32_t len) {
  off += len;
  if (off >= 32u) {
    v.d0 = v.d1;
    v.d1 = v.d2;
    v.d2 = v.d3;
    v.d3 = v.d4;
    v.d4 = 0u;
    off -= 32u;
  }
}

template <bool FB>
__global__ __launch_bounds__(BA_TB) void gh_batch_count_kernel(const BatchParams bp) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[(BA_TB / 64) * BA_REGION];
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* region = smem + wid * BA_REGION;
  const uint32_t* s_fb = (const uint32_t*)region;
  const uint32_t* s_lut = (const uint32_t*)(region + FB_BYTES);
  uint32_t u0, u1;
  unit_run<BA_TB / 64>(bp.nunits, wid, u0, u1);
  BatchUnit un;
  for (uint32_t u = u0; u < u1; ++u) {
    batch_enter(bp, u, un, region, lane);
    Win v[BA_U];
    int R[BA_U], pos[BA_U];
    uint32_t off[BA_U], cnt[BA_U], bad = 0;
#pragma unroll
    for (int c = 0; c < BA_U; ++c) {
      v[c] = batch_segment(bp, un, c, lane, R[c]);
      pos[c] = 0;
      off[c] = 0;
      cnt[c] = 0;
    }
    for (int it = 0; it < 160; ++it) {  // (a segment holds at most 143 codewords)
      bool more = false;
#pragma unroll
      for (int c = 0; c < BA_U; ++c) {
        uint32_t b = 0;
        const uint32_t e = batch_lookup<FB>(v[c], off[c], s_lut, s_fb, un.d, b);
        const bool on = pos[c] < R[c];  // only a lookup that starts before the segment end counts, or flags
        cnt[c] += on ? 1u : 0u;
        bad |= on ? b : 0u;
        pos[c] += (int)(e & 31u);
        batch_advance(v[c], off[c], e & 31u);
        more |= pos[c] < R[c];
      }
      if (!__any(more)) break;
    }
    uint32_t tot = 0;
#pragma unroll
    for (int c = 0; c < BA_U; ++c) {
      bp.seg_cnt[(unsigned long long)u * (64 * BA_U) + (uint32_t)(64 * c + lane)] = (uint8_t)cnt[c];
      tot += (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(cnt[c]), 63);
    }
    if (lane == 0) bp.unit_tot[u] = tot;
    if (FB && __any(bad != 0) && lane == 0) atomicOr(bp.status + un.c.s, (unsigned)GH_ST_BADCODE);
  }
}

// One workgroup: exclusive scan of the unit totals, then every stream's total and status.
__global__ __launch_bounds__(BA_SCAN_TB) void gh_batch_scan_kernel(const BatchParams bp) {
  __shared__ unsigned long long s_w[BA_SCAN_TB / 64];
  const int tid = threadIdx.x;
  const unsigned long long all = block_excl_scan<BA_SCAN_TB>(bp.unit_tot, bp.unit_off, bp.nunits, s_w);
  if (tid == 0) bp.unit_off[bp.nunits] = all;
  __threadfence();
  __syncthreads();
  for (uint32_t i = tid; i < bp.nstreams; i += BA_SCAN_TB) {
    const unsigned long long tot = bp.unit_off[bp.unit0[i + 1]] - bp.unit_off[bp.unit0[i]];
    bp.symbols[i] = tot;
    const unsigned int st = bp.status[i] | (tot < bp.desc[i].n ? (unsigned)GH_ST_BADCODE : 0u);
    if (st) {
      bp.status[i] = st;
      atomicAdd(bp.summary, 1u);
      atomicOr(bp.summary + 1, st);
    }
  }
}

template <bool FB>
__global__ __launch_bounds__(BA_TB) void gh_batch_write_kernel(const BatchParams bp) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[(BA_TB / 64) * BA_REGION];
  const int lane = threadIdx.x & 63;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* region = smem + wid * BA_REGION;
  const uint32_t* s_fb = (const uint32_t*)region;
  const uint32_t* s_lut = (const uint32_t*)(region + FB_BYTES);
  uint32_t u0, u1;
  unit_run<BA_TB / 64>(bp.nunits, wid, u0, u1);
  BatchUnit un;
  for (uint32_t u = u0; u < u1; ++u) {
    batch_enter(bp, u, un, region, lane);
    // the unit's first symbol inside its stream: its scan value minus the stream's first unit's
    unsigned long long at = rfl_u64(bp.unit_off[u] - bp.unit_off[un.c.first]);
    Win v[BA_U];
    uint32_t off[BA_U], k[BA_U], kend[BA_U];
    unsigned long long dst[BA_U];
#pragma unroll
    for (int c = 0; c < BA_U; ++c) {
      int R;
      v[c] = batch_segment(bp, un, c, lane, R);
      const uint32_t cc = R > 0 ? bp.seg_cnt[(unsigned long long)u * (64 * BA_U) + (uint32_t)(64 * c + lane)] : 0u;
      const uint32_t incl = wave_incl_scan(cc);
      const unsigned long long s0 = at + (incl - cc);  // the segment's first symbol; stores are clipped at N
      kend[c] = s0 < un.d.n ? (uint32_t)min((unsigned long long)cc, un.d.n - s0) : 0u;
      dst[c] = un.d.out_off + s0;
      at += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      off[c] = 0;
      k[c] = 0;
    }
    for (int it = 0; it < 160; ++it) {
      bool more = false;
#pragma unroll
      for (int c = 0; c < BA_U; ++c) {
        uint32_t b = 0;  // (flagged by the count pass where it matters)
        const uint32_t e = batch_lookup<FB>(v[c], off[c], s_lut, s_fb, un.d, b);
        if (k[c] < kend[c]) bp.out[dst[c] + k[c]] = (uint8_t)(e >> 8);
        ++k[c];
        batch_advance(v[c], off[c], e & 31u);
        more |= k[c] < kend[c];
      }
      if (!__any(more)) break;
    }
  }
}
