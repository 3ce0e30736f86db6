// Device-side gather plan (gh_ctx_gather_device), included by gh_decode.hip after
// gh_gather.hip.  No reference counterpart.
//
// The ranges of a batch lie in device memory, so the pieces gh_gather_plan (gh_core.cpp)
// would cut are cut here, the same pieces in the same order, by three kernels in a row on
// the caller's stream; gh_gather_kernel then reads the piece count from device memory.
// The per-range arithmetic is gh_gather_range.hpp's, the text the CPU fuzz program runs.
//
//   locate  one thread per range: validate, binary-search the resident index entries for
//           the range's first block and end entry, write {k0, count, len}.
//   scan    ONE workgroup: exclusive scan of (count, len) over the ranges in chunks of
//           GP_SCAN_CHUNK with a running carry; each range gets its first piece slot and
//           its first output byte.  Thread 0 then decides whether the plan stands (no bad
//           range, bytes <= dst_len, pieces <= capacity) and publishes the piece count, 0
//           when it does not: emit and the gather kernel then find nothing to do and
//           write nothing.
//   emit    one thread per PIECE (grid-stride over the published count): a binary search
//           over the scanned slots finds the piece's range, gr_piece_block / gr_piece give
//           the piece.  A whole-stream read (one range, thousands of pieces) and a batch of
//           thousands of one-piece ranges are spread over the threads alike, the piece
//           stores are coalesced, and there is no second code path for long ranges, which
//           a thread or a wave per range would need; the price is log2(nranges) cached
//           loads per piece.
//
// No workgroup of these kernels waits for another: the kernel boundaries are the only
// synchronisation between workgroups (the scan is a single workgroup; its barriers are
// workgroup barriers).

struct GplanParams {
  const gh_range* ranges;
  const uint64_t* offsets;     // nblocks + 1 index entries
  const uint32_t* rank;        // nblocks + 1 (gh_gather_range.hpp)
  RangeLoc* loc;               // nranges
  uint32_t* slot;              // nranges: a range's first piece slot
  unsigned long long* dst0;    // nranges: a range's first output byte
  gh_gather_piece* pieces;     // cap
  unsigned int* status;        // GH_ST_* of this gather: stored by the scan, ORed by the later kernels
  unsigned int* npieces;       // the published piece count
  unsigned long long* totals;  // [0] bytes of the batch, [1] pieces of the batch (also when the plan does not stand)
  uint64_t nblocks, n, cap, dst_len;
  uint32_t nranges;
};

constexpr int GP_TB = 256;           // locate, emit
constexpr int GP_SCAN_TB = 1024;     // the scan's one workgroup
constexpr int GP_SCAN_ITEMS = 2;     // ranges per thread per chunk
constexpr int GP_SCAN_CHUNK = GP_SCAN_TB * GP_SCAN_ITEMS;

__global__ __launch_bounds__(GP_TB) void gh_gplan_locate_kernel(const GplanParams p) {
  const unsigned long long i = (unsigned long long)blockIdx.x * GP_TB + threadIdx.x;
  if (i >= p.nranges) return;
  const gh_range r = p.ranges[i];
  p.loc[i] = gr_locate(p.offsets, p.rank, p.nblocks, p.n, r.lo, r.hi);
}

__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ __launch_bounds__(GP_SCAN_TB) void gh_gplan_scan_kernel(const GplanParams p) {
  __shared__ unsigned long long s_cnt[GP_SCAN_TB / 64], s_len[GP_SCAN_TB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long carry_c = 0, carry_l = 0;  // pieces / bytes of the chunks before
  int bad = 0;
  for (unsigned long long base = 0; base < p.nranges; base += GP_SCAN_CHUNK) {
    const unsigned long long i0 = base + (unsigned long long)tid * GP_SCAN_ITEMS;
    uint32_t c[GP_SCAN_ITEMS], tc = 0;  // (a count is below 2^23 blocks: a wave's 128 sum below 2^32)
    unsigned long long l[GP_SCAN_ITEMS], tl = 0;
#pragma unroll
    for (int u = 0; u < GP_SCAN_ITEMS; ++u) {
      c[u] = 0;
      l[u] = 0;
      if (i0 + u < p.nranges) {
        const RangeLoc loc = p.loc[i0 + u];
        if (loc.count == GR_BAD_RANGE) {
          bad = 1;
        } else {
          c[u] = loc.count;
          l[u] = loc.len;
        }
      }
      tc += c[u];
      tl += l[u];
    }
    const uint32_t ic = wave_incl_scan(tc);
    const unsigned long long il = wave_incl_scan_u64(tl, lane);
    if (lane == 63) {
      s_cnt[wv] = ic;
      s_len[wv] = il;
    }
    __syncthreads();
    unsigned long long wc = 0, wl = 0, allc = 0, alll = 0;  // the waves before this one; all waves
#pragma unroll
    for (int w = 0; w < GP_SCAN_TB / 64; ++w) {
      const unsigned long long vc = s_cnt[w], vl = s_len[w];
      wc += w < wv ? vc : 0ull;
      wl += w < wv ? vl : 0ull;
      allc += vc;
      alll += vl;
    }
    unsigned long long ec = carry_c + wc + (ic - tc), el = carry_l + wl + (il - tl);
#pragma unroll
    for (int u = 0; u < GP_SCAN_ITEMS; ++u) {
      if (i0 + u < p.nranges) {
        p.slot[i0 + u] = (uint32_t)ec;  // (meaningful when the plan stands: then below cap < 2^31)
        p.dst0[i0 + u] = el;
      }
      ec += c[u];
      el += l[u];
    }
    carry_c += allc;
    carry_l += alll;
    __syncthreads();  // s_cnt / s_len are rewritten by the next chunk
  }
  const int any_bad = __syncthreads_or(bad);
  if (tid == 0) {
    unsigned int st = 0;
    if (any_bad) st |= GH_ST_RANGE;
    if (carry_l > p.dst_len) st |= GH_ST_DSTSMALL;
    if (carry_c > p.cap) st |= GH_ST_PIECES;
    *p.status = st;
    *p.npieces = st ? 0u : (unsigned int)carry_c;
    p.totals[0] = carry_l;
    p.totals[1] = carry_c;
  }
}

__global__ __launch_bounds__(GP_TB) void gh_gplan_emit_kernel(const GplanParams p) {
  const unsigned long long np = *p.npieces;  // 0: the plan does not stand
  const unsigned long long nt = (unsigned long long)gridDim.x * GP_TB;
  for (unsigned long long q = (unsigned long long)blockIdx.x * GP_TB + threadIdx.x; q < np; q += nt) {
    if (q >= p.cap) {  // (the scan publishes no count above cap: never expected)
      atomicOr(p.status, (unsigned)GH_ST_PIECES);
      break;
    }
    const uint32_t a = gr_piece_range(p.slot, p.nranges, q);
    const gh_range r = p.ranges[a];
    const uint64_t block = gr_piece_block(p.rank, p.nblocks, p.loc[a].k0, q - p.slot[a]);
    p.pieces[q] = gr_piece(p.offsets, block, r.lo, r.hi, p.dst0[a]);
  }
}
