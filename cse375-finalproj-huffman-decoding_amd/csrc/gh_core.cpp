// Host side of the gap-array Huffman codec: compressed.huff v1/v2 format, the
// boundary package-merge code-length builder, canonical codes, the encoder that
// produces the decoder's input, and the seeded synthetic-input generator.
//
// Reference behaviour restated here (file:line relative to the reference repo):
//   format ......... encoder/src/huff.cpp:186-202 (writer), decoder/src/huff.cpp:36-100
//   histogram ...... encoder/src/encoder.cu:33-140, symbols.cpp:29-43
//   sort ........... encoder/src/huff.cpp:18-22,115 (qsort ascending by count; glibc's
//                    qsort is a stable merge sort for this size, so ties keep
//                    ascending symbol order)
//   code lengths ... encoder/src/package_merge.cpp:12-166 (boundary package-merge, L=16)
//   canonical codes  package_merge.cpp:168-181
//   bit packing .... encoder/src/encoder.cu:281-347 (MSB-first inside each u32)
//   gap array ...... encoder/src/encoder.cu:307-312,358-379
//   generator ...... generate.cpp:32-47
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "gh_batch_range.hpp"
#include "gh_internal.hpp"
#include "gh_pm_flat.hpp"
#include "gh_planes.hpp"
#include "gh_planes_gather.hpp"
#include "gh_pmask.hpp"
#include "gh_raw_trans.hpp"

namespace gh {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int build_canon(const gh_sym* syms, uint32_t nsyms, Canon& c) {
  c = Canon();
  if (nsyms == 0) return GH_OK;
  if (nsyms > GH_MAX_SYMBOLS) return fail(GH_E_TABLE, "more than 256 symbols");
  bool seen[GH_MAX_SYMBOLS] = {};
  c.nsyms = nsyms;
  c.minlen = 99;
  uint32_t code = 0;
  for (uint32_t i = 0; i < nsyms; ++i) {
    const uint32_t l = syms[i].length;
    if (l < 1 || l > GH_MAX_CODE_LEN) return fail(GH_E_TABLE, "code length outside 1..16");
    if (seen[syms[i].symbol]) return fail(GH_E_TABLE, "duplicate symbol in header");
    seen[syms[i].symbol] = true;
    if (i > 0 && l < syms[i - 1].length)
      return fail(GH_E_TABLE, "lengths not non-decreasing (not canonical order)");
    if (i > 0) code = (code + 1) << (l - syms[i - 1].length);
    if (code >> l) return fail(GH_E_TABLE, "code space overflow (Kraft sum > 1)");
    c.sym[i] = syms[i].symbol;
    c.len[i] = (uint8_t)l;
    c.code[i] = code;
    c.minlen = std::min(c.minlen, l);
    c.maxlen = std::max(c.maxlen, l);
    if (c.count[l] == 0) {
      c.first[l] = i;
      c.base16[l] = code << (16 - l);
    }
    c.count[l]++;
  }
  for (uint32_t l = 1; l <= GH_MAX_CODE_LEN; ++l)
    if (c.count[l]) c.limit16[l] = c.base16[l] + (c.count[l] << (16 - l));
  return GH_OK;
}

static int n_threads(int t) {
  if (t > 0) return t;
  unsigned hc = std::thread::hardware_concurrency();
  if (hc == 0) hc = 1;
  return (int)std::min(hc, 32u);
}

template <class F>
static void parallel_for(int nt, F f) {
  if (nt <= 1) {
    f(0);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt);
  for (int t = 0; t < nt; ++t) th.emplace_back(f, t);
  for (auto& x : th) x.join();
}

// ---------------------------------------------------------------------------
// Boundary package-merge (Katajainen/Moffat/Turpin) with lazily built lists,
// behaviour-identical to encoder/src/package_merge.cpp:12-166:
//  * 16 lists; every list starts with the package {c0+c1} holding 2 leaves;
//  * a list's next package takes two items, each the lower list's pending package
//    when no leaf is left or its weight <= the next leaf, else the next leaf;
//  * the top list selects 2n-2 items starting from the two smallest leaves;
//  * a symbol's length is the number of lists whose active leaves include it.
// ---------------------------------------------------------------------------
namespace {
struct PmNode {
  uint64_t weight;
  int leaves;      // leaves used by this list up to and including this package
  int chain_idx;   // package of the next lower list last consumed (-1: none)
};

struct Pm {
  const uint64_t* c;
  int n;
  std::vector<PmNode> list[GH_MAX_CODE_LEN];

  void extend(int l) {
    const PmNode tail = list[l].back();
    PmNode nx{0, tail.leaves, tail.chain_idx};
    if (l == 0) {
      nx.chain_idx = -1;
      for (int k = 0; k < 2; ++k)
        if (nx.leaves < n) nx.weight += c[nx.leaves++];
    } else {
      for (int k = 0; k < 2; ++k) {
        const int pend = (int)list[l - 1].size() - 1;
        const uint64_t pw = list[l - 1][pend].weight;
        if (nx.leaves >= n || pw <= c[nx.leaves]) {
          nx.weight += pw;
          nx.chain_idx = pend;
          extend(l - 1);
        } else {
          nx.weight += c[nx.leaves++];
        }
      }
    }
    list[l].push_back(nx);
  }
};
}  // namespace

}  // namespace gh

using namespace gh;

extern "C" int gh_package_merge(const uint64_t* sorted_counts, uint32_t nsyms,
                                uint8_t* lengths) {
  if (!lengths || (nsyms && !sorted_counts)) return fail(GH_E_ARG, "null argument");
  if (nsyms > GH_MAX_SYMBOLS) return fail(GH_E_ARG, "too many symbols");
  if (nsyms == 0) return GH_OK;
  if (nsyms == 1) {  // package_merge.cpp:159 gives the lone symbol length 1
    lengths[0] = 1;
    return GH_OK;
  }
  const int n = (int)nsyms;
  const int L = GH_MAX_CODE_LEN;
  Pm pm;
  pm.c = sorted_counts;
  pm.n = n;
  for (int l = 0; l < L; ++l) {
    pm.list[l].reserve(2 * n);
    pm.list[l].push_back(PmNode{sorted_counts[0] + sorted_counts[1], 2, -1});
  }
  int top_leaves = 2, head = -1;
  for (int i = 2; i < 2 * (n - 1); ++i) {
    const int pend = (int)pm.list[L - 2].size() - 1;
    if (top_leaves < n && pm.list[L - 2][pend].weight > sorted_counts[top_leaves]) {
      ++top_leaves;
    } else {
      head = pend;
      pm.extend(L - 2);
    }
  }
  std::vector<int> len(n, 0);
  for (int i = 0; i < top_leaves; ++i) len[i]++;
  for (int l = L - 2, idx = head; l >= 0 && idx >= 0; --l) {
    const PmNode& nd = pm.list[l][idx];
    for (int j = 0; j < nd.leaves && j < n; ++j) len[j]++;
    idx = nd.chain_idx;
  }
  for (int i = 0; i < n; ++i) {
    if (len[i] < 1 || len[i] > L) return fail(GH_E_TABLE, "package-merge produced bad length");
    lengths[i] = (uint8_t)len[i];
  }
  return GH_OK;
}

// The same lengths by the level-by-level form (gh_pm_flat.hpp), driven serially: what one
// workgroup of gh_ebatch_code_kernel does per stream, an item at a time.
extern "C" int gh_package_merge_flat(const uint64_t* sorted_counts, uint32_t nsyms, uint8_t* lengths) {
  if (!lengths || (nsyms && !sorted_counts)) return fail(GH_E_ARG, "null argument");
  if (nsyms > GH_MAX_SYMBOLS) return fail(GH_E_ARG, "too many symbols");
  if (nsyms == 0) return GH_OK;
  if (nsyms == 1) {
    lengths[0] = 1;
    return GH_OK;
  }
  const uint64_t* c = sorted_counts;
  const uint32_t n = nsyms, need = pm_need(n);
  uint64_t w[2][PM_MAX_ITEMS];
  uint32_t mask[PM_LEVELS][PM_MASK_WORDS] = {}, pre[PM_LEVELS][PM_MASK_WORDS] = {}, nl[PM_LEVELS];
  const uint64_t* prev = c;
  uint32_t m = n;
  for (uint32_t l = 1; l < PM_LEVELS; ++l) {
    uint64_t* next = w[l & 1];
    const uint32_t np = m / 2;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t pos = pm_leaf_pos(c, prev, np, j);
      if (pos < need) {
        next[pos] = c[j];
        mask[l][pos >> 5] |= 1u << (pos & 31u);
      }
    }
    for (uint32_t i = 0; i < np; ++i) {
      const uint64_t P = pm_package(prev, i);
      const uint32_t pos = pm_package_pos(c, n, i, P);
      if (pos < need) next[pos] = P;
    }
    m = pm_next_items(n, m);
    pm_mask_prefix(mask[l], pre[l]);
    prev = next;
  }
  pm_trace(&mask[0][0], &pre[0][0], n, nl);
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t len = pm_length(nl, j);
    if (len < 1 || len > PM_LEVELS) return fail(GH_E_TABLE, "package-merge produced bad length");
    lengths[j] = (uint8_t)len;
  }
  return GH_OK;
}

// ---------------------------------------------------------------------------
// Format
// ---------------------------------------------------------------------------
template <class T>
static T rd(const uint8_t* p) {
  T v;
  std::memcpy(&v, p, sizeof(T));
  return v;
}
template <class T>
static void wr(uint8_t* p, T v) {
  std::memcpy(p, &v, sizeof(T));
}

extern "C" int gh_stream_validate(const gh_stream* s) {
  if (!s) return fail(GH_E_ARG, "null stream");
  Canon c;
  int rc = build_canon(s->syms, s->nsyms, c);
  if (rc) return rc;
  if (s->n > 0 && s->nsyms == 0) return fail(GH_E_FORMAT, "N > 0 but no symbols");
  if (s->g == 0) {
    if (s->w != 0) return fail(GH_E_FORMAT, "G = 0 but W > 0");
  } else if (s->w > 4 * s->g || s->w + 3 < 4 * s->g) {
    return fail(GH_E_FORMAT, "W inconsistent with G (need 4G-3 <= W <= 4G)");
  }
  if (s->n > 0 && s->g == 0) return fail(GH_E_FORMAT, "N > 0 but G = 0");
  // every symbol takes >= minlen bits, so N * minlen <= 32 W
  if (s->nsyms && (unsigned __int128)s->n * c.minlen > (unsigned __int128)s->w * 32)
    return fail(GH_E_FORMAT, "N too large for the payload");
  return GH_OK;
}

extern "C" int gh_stream_parse(const void* file, size_t len, gh_stream* out) {
  if (!file || !out) return fail(GH_E_ARG, "null argument");
  const uint8_t* p = (const uint8_t*)file;
  gh_stream s{};
  size_t off = 0;
  if (len < 8) return fail(GH_E_FORMAT, "file shorter than the symbol-count field");
  uint64_t first = rd<uint64_t>(p);
  if (first == GH_V2_MAGIC) {
    s.version = 2;
    off = 8;
    if (len < 16) return fail(GH_E_FORMAT, "truncated v2 header");
    first = rd<uint64_t>(p + off);
  } else {
    s.version = 1;
  }
  off += 8;
  if (first > GH_MAX_SYMBOLS) return fail(GH_E_FORMAT, "symbol count > 256");
  s.nsyms = (uint32_t)first;
  if (len < off + 2 * s.nsyms) return fail(GH_E_FORMAT, "truncated symbol table");
  s.syms = (const gh_sym*)(p + off);
  off += 2 * s.nsyms;
  if (s.version == 1) {
    if (len < off + 12) return fail(GH_E_FORMAT, "truncated size fields");
    s.n = rd<uint32_t>(p + off);
    s.w = rd<uint32_t>(p + off + 4);
    s.g = rd<uint32_t>(p + off + 8);
    off += 12;
  } else {
    if (len < off + 24) return fail(GH_E_FORMAT, "truncated size fields");
    s.n = rd<uint64_t>(p + off);
    s.w = rd<uint64_t>(p + off + 8);
    s.g = rd<uint64_t>(p + off + 16);
    off += 24;
  }
  const uint64_t gw = ceil_div(s.g, GH_GAPS_PER_WORD);
  if (gw > (len - off) / 4 || s.w > (len - off) / 4 - gw)
    return fail(GH_E_FORMAT, "file shorter than gap array + payload");
  s.gap_words = (const uint32_t*)(p + off);
  off += 4 * gw;
  s.payload = (const uint32_t*)(p + off);
  int rc = gh_stream_validate(&s);
  if (rc) return rc;
  *out = s;
  return GH_OK;
}

// ---------------------------------------------------------------------------
// Seek index (sidecar image, gaphuff.h): parse and locate.  The image is built by
// gh_ctx_build_index (gh_decode.hip) from a loaded stream, and by the encoders:
// gh_encode_index (below) and gh_ectx_index (gh_encode.hip).  Entries are read with
// memcpy: the image may sit at any alignment.
// ---------------------------------------------------------------------------
constexpr size_t IDX_HEADER = 40;

static uint64_t idx_entry(const gh_index* ix, uint64_t k) { return rd<uint64_t>((const uint8_t*)ix->offsets + 8 * k); }

extern "C" uint64_t gh_index_bytes(uint64_t g, uint32_t log2_stride) {
  if (log2_stride < GH_INDEX_MIN_LOG2 || log2_stride > GH_INDEX_MAX_LOG2) return 0;
  const uint64_t stride = 1ull << log2_stride;
  const uint64_t nblocks = g / stride + (g % stride != 0);  // < 2^56: the byte count fits
  return IDX_HEADER + 8 * (nblocks + 1);
}

extern "C" int gh_index_parse(const void* file, size_t len, gh_index* out) {
  if (!file || !out) return fail(GH_E_ARG, "null argument");
  const uint8_t* p = (const uint8_t*)file;
  if (len < IDX_HEADER) return fail(GH_E_FORMAT, "index shorter than its header");
  if (rd<uint64_t>(p) != GH_INDEX_MAGIC) return fail(GH_E_FORMAT, "not a seek index (magic)");
  gh_index ix{};
  ix.log2_stride = rd<uint32_t>(p + 8);
  if (rd<uint32_t>(p + 12) != 0) return fail(GH_E_FORMAT, "index: reserved field not zero");
  ix.n = rd<uint64_t>(p + 16);
  ix.g = rd<uint64_t>(p + 24);
  ix.nentries = rd<uint64_t>(p + 32);
  const uint64_t bytes = gh_index_bytes(ix.g, ix.log2_stride);
  if (bytes == 0) return fail(GH_E_FORMAT, "index: stride outside 2^8 .. 2^20 segments");
  if (ix.nentries != (bytes - IDX_HEADER) / 8) return fail(GH_E_FORMAT, "index: entry count does not match G and the stride");
  if (len < bytes) return fail(GH_E_FORMAT, "index shorter than its entries");
  ix.offsets = (const uint64_t*)(p + IDX_HEADER);
  if (idx_entry(&ix, 0) != 0) return fail(GH_E_FORMAT, "index: first entry not 0");
  if (idx_entry(&ix, ix.nentries - 1) != ix.n) return fail(GH_E_FORMAT, "index: last entry not N");
  // a segment holds at most 143 codewords (its codewords lie in at most 128 + 15 bits)
  const uint64_t max_step = 143ull << ix.log2_stride;
  uint64_t prev = 0;
  for (uint64_t k = 1; k < ix.nentries; ++k) {
    const uint64_t v = idx_entry(&ix, k);
    if (v < prev) return fail(GH_E_FORMAT, "index: entries decrease");
    if (v - prev > max_step) return fail(GH_E_FORMAT, "index: more symbols in a block than its segments can hold");
    prev = v;
  }
  *out = ix;
  return GH_OK;
}

extern "C" int gh_index_locate(const gh_index* ix, uint64_t lo, uint64_t hi, uint64_t* seg_begin,
                               uint64_t* seg_end, uint64_t* skip) {
  if (!ix || !ix->offsets || !seg_begin || !seg_end || !skip) return fail(GH_E_ARG, "null argument");
  if (ix->nentries == 0) return fail(GH_E_ARG, "index without entries");
  if (lo > hi || hi > ix->n) return fail(GH_E_ARG, "byte range outside [0, N]");
  *seg_begin = *seg_end = *skip = 0;
  if (lo == hi) return GH_OK;
  const uint64_t nblocks = ix->nentries - 1;
  if (nblocks == 0) return fail(GH_E_ARG, "index of an empty stream");
  // k: the last block whose first symbol is at or before lo (entry 0 is 0 <= lo)
  uint64_t a = 0, b = nblocks;  // offsets[a] <= lo; b == nblocks or offsets[b] > lo
  while (b - a > 1) {
    const uint64_t mid = a + (b - a) / 2;
    if (idx_entry(ix, mid) <= lo) a = mid; else b = mid;
  }
  const uint64_t k = a;
  // m: the first entry at or past hi (entry nblocks is N >= hi; entry 0 is 0 < hi)
  a = 0, b = nblocks;  // offsets[a] < hi <= offsets[b]
  while (b - a > 1) {
    const uint64_t mid = a + (b - a) / 2;
    if (idx_entry(ix, mid) < hi) a = mid; else b = mid;
  }
  const uint64_t m = b;
  *seg_begin = k << ix->log2_stride;
  *seg_end = std::min<uint64_t>(m << ix->log2_stride, ix->g);
  *skip = lo - idx_entry(ix, k);
  return GH_OK;
}

// Range gather plan (gh_ctx_gather): every range cut at the index entries it spans.  A
// piece never reaches past its block's symbols (b <= offsets[k+1] - offsets[k] <= 143 *
// stride < 2^32, gh_index_parse), and blocks without symbols are skipped (a == b).
extern "C" int gh_gather_plan(const gh_index* ix, const gh_range* ranges, uint32_t nranges,
                              gh_gather_piece* pieces, uint64_t cap, uint64_t* npieces,
                              uint64_t* out_bytes) {
  if (npieces) *npieces = 0;
  if (out_bytes) *out_bytes = 0;
  if (!ix || !ix->offsets || !npieces || !out_bytes || (nranges && !ranges) || (cap && !pieces))
    return fail(GH_E_ARG, "null argument");
  if (ix->nentries == 0) return fail(GH_E_ARG, "index without entries");
  const uint64_t nblocks = ix->nentries - 1;
  if (nblocks > 0xFFFFFFFFull) return fail(GH_E_ARG, "index of more than 2^32 blocks");
  uint64_t np = 0, dst = 0;
  for (uint32_t i = 0; i < nranges; ++i) {
    const uint64_t lo = ranges[i].lo, hi = ranges[i].hi;
    if (lo > hi || hi > ix->n) {
      *npieces = *out_bytes = 0;
      return fail(GH_E_ARG, "byte range outside [0, N]");
    }
    if (lo == hi) continue;  // (then N > 0: nblocks >= 1)
    // k: the last block whose first symbol is at or before lo (entry 0 is 0 <= lo)
    uint64_t a = 0, b = nblocks;  // offsets[a] <= lo; b == nblocks or offsets[b] > lo
    while (b - a > 1) {
      const uint64_t mid = a + (b - a) / 2;
      if (idx_entry(ix, mid) <= lo) a = mid; else b = mid;
    }
    uint64_t o0 = idx_entry(ix, a);
    for (uint64_t k = a; k < nblocks && o0 < hi; ++k) {
      const uint64_t o1 = idx_entry(ix, k + 1);
      const uint64_t pa = std::max(lo, o0), pb = std::min(hi, o1);
      if (pa < pb) {
        if (np < cap) pieces[np] = gh_gather_piece{dst, (uint32_t)k, (uint32_t)(pa - o0), (uint32_t)(pb - o0), 0u};
        ++np;
        dst += pb - pa;
      }
      o0 = o1;
    }
  }
  *npieces = np;
  *out_bytes = dst;
  if (np > cap) return fail(GH_E_SMALL, "piece buffer smaller than the plan");
  return GH_OK;
}

// Piece bound of a device-planned batch (derivation: gaphuff.h): every range has a first
// and a last piece, and any other piece holds at least 8 * stride of the batch's bytes.
extern "C" uint64_t gh_gather_piece_bound(uint32_t nranges, uint64_t dst_len, uint32_t log2_stride) {
  if (log2_stride < GH_INDEX_MIN_LOG2 || log2_stride > GH_INDEX_MAX_LOG2) return 0;
  return 2ull * nranges + (dst_len >> (log2_stride + 3));
}

// ---------------------------------------------------------------------------
// Batched decode: the host plan (gaphuff.h, "batched decode").  No device.
// ---------------------------------------------------------------------------
// a + b into *r; false when the sum overflows 64 bits
static bool add_u64(uint64_t a, uint64_t b, uint64_t* r) { return !__builtin_add_overflow(a, b, r); }

extern "C" int gh_batch_layout(const uint64_t* n, uint32_t nstreams, uint64_t* out_off) {
  if (!out_off || (nstreams && !n)) return fail(GH_E_ARG, "null argument");
  uint64_t at = 0;
  for (uint32_t i = 0; i < nstreams; ++i) {
    out_off[i] = at;
    uint64_t padded;
    if (!add_u64(n[i], 15, &padded) || !add_u64(at, padded & ~15ull, &at))
      return fail(GH_E_ARG, "batch output arena overflows 64 bits at stream " + std::to_string(i));
  }
  out_off[nstreams] = at;
  return GH_OK;
}

int gh::batch_plan(const uint64_t* n, const uint64_t* w, const uint64_t* g, uint32_t nstreams, BatchPlan& out) {
  out = BatchPlan();
  if (nstreams && (!n || !w || !g)) return fail(GH_E_ARG, "null argument");
  if (nstreams > BATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  out.ext.resize(nstreams);
  uint64_t pay = 0, gap = 0, units = 0, bytes = 0;
  for (uint32_t i = 0; i < nstreams; ++i) {
    const std::string who = "stream " + std::to_string(i) + ": ";
    if (g[i] >= BATCH_MAX_G) return fail(GH_E_ARG, who + "2^32 - 256 or more segments");
    if (g[i] == 0 ? w[i] != 0 : (w[i] > 4 * g[i] || w[i] + 3 < 4 * g[i]))
      return fail(GH_E_ARG, who + "W inconsistent with G (need 4G-3 <= W <= 4G)");
    BatchExtent& e = out.ext[i];
    e.pay_off = pay;
    // words [4 (G - 1), 4 G) of the last segment and the look-ahead word 4 G are loaded
    // unconditionally: 4 G + 1 words, rounded up to 16 bytes
    e.pay_words = g[i] ? 4 * g[i] + 4 : 0;
    e.gap_off = gap;
    e.gap_words = ceil_div(g[i], GH_GAPS_PER_WORD);
    e.unit0 = units;
    e.out_off = bytes;
    pay += e.pay_words;  // (< 2^24 * 2^34)
    gap += e.gap_words;
    units += ceil_div(g[i], BATCH_UNIT_SEGS);
    if (units >= BATCH_MAX_UNITS) return fail(GH_E_ARG, who + "the batch reaches 2^31 work units");
    uint64_t padded;
    if (!add_u64(n[i], 15, &padded) || !add_u64(bytes, padded & ~15ull, &bytes))
      return fail(GH_E_ARG, who + "the output arena overflows 64 bits");
  }
  out.pay_words = pay;
  out.gap_words = gap;
  out.nunits = units;
  out.out_bytes = bytes;
  return GH_OK;
}

// Batched gather: the host plan (gaphuff.h, "batched gather"), the loop form of what the plan
// kernels of gh_batch_gather.hip do with the same arithmetic (gh_batch_range.hpp).
extern "C" int gh_batchdec_plan(const uint32_t* unit0, const uint64_t* unit_off, const uint64_t* n,
                                const uint32_t* stream_status, uint32_t nstreams, const gh_brange* ranges,
                                uint32_t nranges, gh_gather_piece* pieces, uint64_t cap, uint64_t* npieces,
                                uint64_t* out_bytes, uint32_t* bad_ranges) {
  if (npieces) *npieces = 0;
  if (out_bytes) *out_bytes = 0;
  if (bad_ranges) *bad_ranges = 0;
  if (!unit0 || !unit_off || !npieces || !out_bytes || !bad_ranges || (nstreams && !n) || (nranges && !ranges) ||
      (cap && !pieces))
    return fail(GH_E_ARG, "null argument");
  uint64_t np = 0, dst = 0;
  uint32_t bad = 0;
  for (uint32_t i = 0; i < nranges; ++i) {
    bool flagged;
    const RangeLoc loc = br_locate(
        unit0, unit_off, [&](uint32_t s) { return n[s]; },
        [&](uint32_t s) { return stream_status ? stream_status[s] : 0u; }, nstreams, ranges[i], &flagged);
    if (loc.count == GR_BAD_RANGE)
      return fail(GH_E_ARG, "range " + std::to_string(i) + ": no such stream, or bytes outside [0, n] of its stream");
    bad += flagged;
    for (uint64_t j = 0; j < loc.count; ++j, ++np)
      if (np < cap) pieces[np] = br_piece(unit0, unit_off, ranges[i], loc, j, dst);
    dst += loc.len;
  }
  *npieces = np;
  *out_bytes = dst;
  *bad_ranges = bad;
  if (np > cap) return fail(GH_E_SMALL, "piece buffer smaller than the plan");
  return GH_OK;
}

// Batched gap-less load: the host twin of gh_batch_raw.hip (gaphuff.h, "batched gap-less
// decode"), cut as the kernels are: T_j of every segment (gh_raw_trans.hpp), each unit's
// aggregate, the units' entries chained, then every unit's nibbles from its entry.
extern "C" int gh_batchraw_gaps_host(const gh_sym* syms, uint32_t nsyms, const uint32_t* words, uint64_t w,
                                     uint32_t* gap_words, uint64_t cap) {
  if ((nsyms && !syms) || (w && !words)) return fail(GH_E_ARG, "null argument");
  Canon c;
  if (int rc = build_canon(syms, nsyms, c)) return rc;
  if (w && c.nsyms == 0) return fail(GH_E_TABLE, "segments but an empty code");
  const uint64_t g = ceil_div(w, 4), ngapw = ceil_div(g, GH_GAPS_PER_WORD);
  if (g >= BATCH_MAX_G) return fail(GH_E_ARG, "2^32 - 256 or more segments");
  if (cap < ngapw) return fail(GH_E_SMALL, "gap word buffer smaller than ceil(G / 8)");
  if (ngapw && !gap_words) return fail(GH_E_ARG, "null argument");
  auto word = [&](uint64_t i) { return i < w ? words[i] : 0u; };  // (zero past W, as the payload arena)
  // the batch's lookup rule at stream bit p: the canonical codeword's length, maxlen outside the code
  auto length_at = [&](uint64_t p) {
    const uint64_t two = ((uint64_t)word(p >> 5) << 32) | word((p >> 5) + 1);
    uint32_t index;
    const uint32_t l = canon_decode16(c, (uint32_t)(two >> (48 - (p & 31))) & 0xFFFFu, &index);
    return l ? l : c.maxlen;
  };
  const uint64_t nunits = ceil_div(g, BATCH_UNIT_SEGS);
  std::vector<unsigned long long> trans(g), agg(nunits, TRANS_IDENTITY);
  for (uint64_t j = 0; j < g; ++j) {
    unsigned long long f = 0;
    for (uint32_t x = 0; x < 16; ++x) {
      uint64_t p = 128 * j + x;
      f |= trans_nibble(x, trans_walk(x, [&]() {
             const uint32_t l = length_at(p);
             p += l;
             return l;
           }));
    }
    trans[j] = f;
    agg[j / BATCH_UNIT_SEGS] = trans_compose(agg[j / BATCH_UNIT_SEGS], f);
  }
  std::fill(gap_words, gap_words + ngapw, 0u);
  uint32_t entry = 0;  // of unit u: 0 at the stream's first bit
  for (uint64_t u = 0; u < nunits; ++u) {
    uint32_t e = entry;
    for (uint64_t j = u * BATCH_UNIT_SEGS; j < std::min<uint64_t>(g, (u + 1) * BATCH_UNIT_SEGS); ++j) {
      e = trans_apply(trans[j], e);  // e_{j+1}: gap nibble j, but 0 for the stream's last segment
      if (j + 1 < g) gap_words[j / GH_GAPS_PER_WORD] |= e << (4 * (j % GH_GAPS_PER_WORD));
    }
    entry = trans_apply(agg[u], entry);
  }
  return GH_OK;
}

// ---------------------------------------------------------------------------
// Batched encode: the host layout (gaphuff.h, "batched encode").  No device.
// ---------------------------------------------------------------------------
int gh::ebatch_in_plan(const uint64_t* n, uint32_t nstreams, EBatchInPlan& out) {
  out = EBatchInPlan();
  if (nstreams && !n) return fail(GH_E_ARG, "null argument");
  if (nstreams > EBATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  out.ext.resize(nstreams);
  uint64_t at = 0, units = 0, sum = 0;
  for (uint32_t i = 0; i < nstreams; ++i) {
    const std::string who = "stream " + std::to_string(i) + ": ";
    const uint64_t nu = n[i] / EBATCH_UNIT_BYTES + (n[i] % EBATCH_UNIT_BYTES ? 1 : 0);
    if (nu >= EBATCH_MAX_UNITS || (units += nu) >= EBATCH_MAX_UNITS)
      return fail(GH_E_ARG, who + "the batch reaches 2^31 work units");
    EBatchInExtent& e = out.ext[i];
    e.in_off = at;
    // every lane's 16-byte load of every unit, and the at most 32 bytes after a unit that
    // complete its last word, lie inside the stream's own extent
    e.in_bytes = nu ? nu * EBATCH_UNIT_BYTES + EBATCH_TAIL_BYTES : 0;
    e.unit0 = units - nu;
    at += e.in_bytes;  // (< 2^31 * 1024 + 2^24 * 32)
    sum += n[i];       // (< 2^41)
  }
  out.in_bytes = at;
  out.nunits = units;
  out.sum_n = sum;
  return GH_OK;
}

int gh::ebatch_out_plan(const uint64_t* w, const uint64_t* g, uint32_t nstreams, EBatchOutPlan& out) {
  out = EBatchOutPlan();
  if (nstreams && (!w || !g)) return fail(GH_E_ARG, "null argument");
  if (nstreams > EBATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  out.ext.resize(nstreams);
  uint64_t pay = 0, gap = 0;
  for (uint32_t i = 0; i < nstreams; ++i) {
    const std::string who = "stream " + std::to_string(i) + ": ";
    if (g[i] != w[i] / 4 + (w[i] % 4 ? 1 : 0)) return fail(GH_E_ARG, who + "G is not ceil(W / 4)");
    EBatchOutExtent& e = out.ext[i];
    uint64_t pw, gw;
    if (!add_u64(w[i], 3, &pw)) return fail(GH_E_ARG, who + "the payload arena overflows 64 bits");
    pw &= ~3ull;
    gw = (ceil_div(g[i], GH_GAPS_PER_WORD) + 3) & ~3ull;  // (G <= 2^62)
    e.pay_off = pay;
    e.pay_words = pw;
    e.gap_off = gap;
    e.gap_words = gw;
    if (!add_u64(pay, pw, &pay) || pay > (~0ull >> 2)) return fail(GH_E_ARG, who + "the payload arena overflows 64 bits");
    gap += gw;  // (<= pay)
  }
  out.pay_words = pay;
  out.gap_words = gap;
  return GH_OK;
}

// ---------------------------------------------------------------------------
// Encoder
// ---------------------------------------------------------------------------
extern "C" int gh_encode_plan_make(const uint8_t* in, uint64_t n, int threads,
                                   int force_version, gh_encode_plan* plan) {
  if (!plan || (n && !in)) return fail(GH_E_ARG, "null argument");
  std::memset(plan, 0, sizeof(*plan));
  plan->n = n;
  const int nt = (int)std::min<uint64_t>(n_threads(threads), std::max<uint64_t>(1, n >> 20));
  std::vector<uint64_t> hist((size_t)nt * 256, 0);
  parallel_for(nt, [&](int t) {
    const uint64_t a = n * t / nt, b = n * (t + 1) / nt;
    uint64_t* h = &hist[(size_t)t * 256];
    for (uint64_t i = a; i < b; ++i) h[in[i]]++;
  });
  for (int t = 0; t < nt; ++t)
    for (int v = 0; v < 256; ++v) plan->count[v] += hist[(size_t)t * 256 + v];
  return gh::plan_from_counts(plan, force_version);
}

// The plan from plan->n and plan->count[] (the host histogram above, or the GPU
// encoder's, gh_encode.hip).
int gh::plan_from_counts(gh_encode_plan* plan, int force_version) {
  // store_symbols (symbols.cpp:29-43): ascending symbol value, non-zero counts;
  // then a stable ascending sort by count (huff.cpp:115).
  uint32_t order[256];
  uint32_t ns = 0;
  for (uint32_t v = 0; v < 256; ++v)
    if (plan->count[v]) order[ns++] = v;
  std::stable_sort(order, order + ns,
                   [&](uint32_t a, uint32_t b) { return plan->count[a] < plan->count[b]; });
  uint64_t sc[256];
  uint8_t sl[256];
  for (uint32_t i = 0; i < ns; ++i) sc[i] = plan->count[order[i]];
  int rc = gh_package_merge(sc, ns, sl);
  if (rc) return rc;
  plan->nsyms = ns;
  // file order = most frequent first (huff.cpp:189-194)
  for (uint32_t i = 0; i < ns; ++i) {
    plan->syms[i].symbol = (uint8_t)order[ns - 1 - i];
    plan->syms[i].length = sl[ns - 1 - i];
  }
  Canon c;
  rc = build_canon(plan->syms, ns, c);
  if (rc) return rc;
  uint64_t bits = 0;
  for (uint32_t i = 0; i < ns; ++i) {
    plan->code[c.sym[i]] = c.code[i];
    plan->len[c.sym[i]] = c.len[i];
    bits += (uint64_t)c.len[i] * plan->count[c.sym[i]];
  }
  plan->bits = bits;
  return plan_sizes(plan, force_version);
}

// w, g, version and file_bytes from plan->n, plan->nsyms and plan->bits.
int gh::plan_sizes(gh_encode_plan* plan, int force_version) {
  const uint64_t bits = plan->bits;
  const uint32_t ns = plan->nsyms;
  plan->g = ceil_div(bits, GH_SEGMENT_BITS);
  plan->w = ceil_div(bits, 32);
  const uint64_t lim = 1ull << 31;
  plan->version = (plan->n >= lim || plan->w >= lim || plan->g >= lim) ? 2 : 1;
  if (force_version == 2) plan->version = 2;
  if (force_version == 1 && plan->version == 2)
    return fail(GH_E_ARG, "stream too large for the v1 (32-bit) header");
  const uint64_t hdr = (plan->version == 2 ? 16 : 8) + 2ull * ns + (plan->version == 2 ? 24 : 12);
  plan->file_bytes = hdr + 4 * ceil_div(plan->g, GH_GAPS_PER_WORD) + 4 * plan->w;
  return GH_OK;
}

// Header of the compressed image (encoder/src/huff.cpp:186-196; v2: 64-bit sizes
// behind a magic); returns its size in bytes.
size_t gh::encode_header(const gh_encode_plan* plan, uint8_t* out) {
  size_t off = 0;
  if (plan->version == 2) {
    wr<uint64_t>(out, GH_V2_MAGIC);
    off = 8;
  }
  wr<uint64_t>(out + off, plan->nsyms);
  off += 8;
  for (uint32_t i = 0; i < plan->nsyms; ++i) {
    out[off++] = plan->syms[i].symbol;
    out[off++] = plan->syms[i].length;
  }
  if (plan->version == 2) {
    wr<uint64_t>(out + off, plan->n);
    wr<uint64_t>(out + off + 8, plan->w);
    wr<uint64_t>(out + off + 16, plan->g);
    off += 24;
  } else {
    wr<uint32_t>(out + off, (uint32_t)plan->n);
    wr<uint32_t>(out + off + 4, (uint32_t)plan->w);
    wr<uint32_t>(out + off + 8, (uint32_t)plan->g);
    off += 12;
  }
  return off;
}

extern "C" int gh_encode_plan_from_counts(const uint64_t counts[256], int force_version, gh_encode_plan* plan) {
  if (!counts || !plan) return fail(GH_E_ARG, "null argument");
  std::memset(plan, 0, sizeof(*plan));
  for (int v = 0; v < 256; ++v) {
    plan->count[v] = counts[v];
    plan->n += counts[v];
  }
  return gh::plan_from_counts(plan, force_version);
}

extern "C" uint64_t gh_encode_bound(uint64_t n) {
  // 16 bits per byte: W = ceil(n / 2) words, G = ceil(n / 8) segments; v2 header, 256 symbols
  const uint64_t w = ceil_div(n, 2), g = ceil_div(n, 8);
  return 16 + 2ull * GH_MAX_SYMBOLS + 24 + 4 * ceil_div(g, GH_GAPS_PER_WORD) + 4 * w;
}

extern "C" int gh_slice_extent(uint64_t base_bit, uint64_t bits, gh_slice* out) {
  if (!out) return fail(GH_E_ARG, "null argument");
  if (base_bit + bits < base_bit) return fail(GH_E_ARG, "slice end overflows 64 bits");
  out->base_bit = base_bit;
  out->bits = bits;
  out->word0 = base_bit >> 5;
  out->gapw0 = base_bit >> 10;
  out->nwords = bits ? ((base_bit + bits - 1) >> 5) + 1 - out->word0 : 0;
  out->ngapw = bits ? ((base_bit + bits - 1) >> 10) + 1 - out->gapw0 : 0;
  return GH_OK;
}

// The host encoder's body: bytes in[0..n) as the slice at base_bit (gaphuff.h, "sliced
// encode"); the whole stream is the slice at bit 0.  Threaded: per-thread bit totals, an
// exclusive scan, then every thread packs its own bits; the words and gap words that two
// threads (or two slices) share are ORed.  words / gaps are indexed from the slice's
// word0 / gapw0; `zeroed`: the caller has cleared them.
static int encode_slice_body(const uint8_t* in, uint64_t n, const gh_encode_plan* plan, uint64_t base_bit,
                             int threads, uint32_t* words, uint64_t words_cap, uint32_t* gaps, uint64_t gaps_cap,
                             bool zeroed, gh_slice* out) {
  const int nt = (int)std::min<uint64_t>(n_threads(threads), std::max<uint64_t>(1, n >> 20));
  // per-thread bit totals -> exclusive bit offsets
  std::vector<uint64_t> tbits(nt + 1, 0);
  std::atomic<bool> absent{false};
  parallel_for(nt, [&](int t) {
    const uint64_t a = n * t / nt, b = n * (t + 1) / nt;
    uint64_t s = 0;
    bool zero = false;
    for (uint64_t i = a; i < b; ++i) {
      const uint32_t l = plan->len[in[i]];
      zero |= l == 0;
      s += l;
    }
    tbits[t + 1] = s;
    if (zero) absent = true;
  });
  if (absent) return fail(GH_E_TABLE, "a byte of the input has no code in the plan");
  for (int t = 0; t < nt; ++t) tbits[t + 1] += tbits[t];
  if (gh_slice_extent(base_bit, tbits[nt], out) || base_bit + tbits[nt] > plan->bits)
    return fail(GH_E_ARG, "slice ends past the plan's bit total");
  if (words_cap < out->nwords || gaps_cap < out->ngapw) return fail(GH_E_SMALL, "slice buffer too small");
  if (!zeroed) {
    if (out->nwords) std::memset(words, 0, 4 * out->nwords);
    if (out->ngapw) std::memset(gaps, 0, 4 * out->ngapw);
  }
  const uint64_t word0 = out->word0, gapw0 = out->gapw0;
  parallel_for(nt, [&](int t) {
    const uint64_t a = n * t / nt, b = n * (t + 1) / nt;
    if (a == b) return;  // (an empty slice owns no word)
    uint64_t pos = base_bit + tbits[t];
    uint64_t acc = 0;
    int nb = (int)(pos & 31);  // placeholder zero bits already in the first word
    uint64_t widx = (pos >> 5) - word0;
    const uint64_t first_word = widx;
    auto emit = [&](uint32_t v) {
      if (widx == first_word) {
        __atomic_fetch_or(&words[widx], v, __ATOMIC_RELAXED);
      } else {
        words[widx] = v;
      }
      ++widx;
    };
    for (uint64_t i = a; i < b; ++i) {
      const uint8_t sym = in[i];
      const uint32_t l = plan->len[sym];
      const uint64_t end = pos + l;
      if ((end >> 7) != (pos >> 7)) {  // codeword crosses a 128-bit boundary
        const uint32_t gv = (uint32_t)(end & 15);
        const uint64_t j = pos >> 7;
        if (gv) __atomic_fetch_or(&gaps[(j >> 3) - gapw0], gv << (4 * (j & 7)), __ATOMIC_RELAXED);
      }
      acc = (acc << l) | plan->code[sym];
      nb += (int)l;
      if (nb >= 32) {
        nb -= 32;
        emit((uint32_t)(acc >> nb));
        acc &= (nb ? ((1ull << nb) - 1) : 0ull);
      }
      pos = end;
    }
    if (nb > 0) {  // trailing partial word, shared with the next thread
      __atomic_fetch_or(&words[widx], (uint32_t)(acc << (32 - nb)), __ATOMIC_RELAXED);
    }
  });
  return GH_OK;
}

extern "C" int gh_encode_slice(const uint8_t* in, uint64_t n, const gh_encode_plan* plan, uint64_t base_bit,
                               int threads, uint32_t* words, uint64_t words_cap, uint32_t* gapw,
                               uint64_t gaps_cap, gh_slice* out) {
  if (!plan || !out || (n && !in) || (words_cap && !words) || (gaps_cap && !gapw))
    return fail(GH_E_ARG, "null argument");
  return encode_slice_body(in, n, plan, base_bit, threads, words, words_cap, gapw, gaps_cap, false, out);
}

extern "C" int gh_encode_write(const uint8_t* in, const gh_encode_plan* plan, int threads,
                               void* out_v, uint64_t out_len) {
  if (!plan || !out_v || (plan->n && !in)) return fail(GH_E_ARG, "null argument");
  if (out_len < plan->file_bytes) return fail(GH_E_SMALL, "output buffer too small");
  uint8_t* out = (uint8_t*)out_v;
  const uint64_t W = plan->w;
  const uint64_t GW = ceil_div(plan->g, GH_GAPS_PER_WORD);
  size_t off = gh::encode_header(plan, out);
  // the whole stream is the slice at bit 0
  std::vector<uint32_t> gaps(GW + 1, 0), words(W + 1, 0);
  gh_slice sl;
  const int rc = encode_slice_body(in, plan->n, plan, 0, threads, words.data(), W, gaps.data(), GW, true, &sl);
  if (rc || sl.bits != plan->bits) return fail(GH_E_ARG, "input does not match the plan");
  std::memcpy(out + off, gaps.data(), 4 * GW);
  off += 4 * GW;
  std::memcpy(out + off, words.data(), 4 * W);
  return GH_OK;
}

// Bytes of the image before the gap words.
static uint64_t image_header_bytes(const gh_encode_plan* plan) {
  return (plan->version == 2 ? 16 : 8) + 2ull * plan->nsyms + (plan->version == 2 ? 24 : 12);
}

extern "C" int gh_encode_image_init(const gh_encode_plan* plan, void* image, uint64_t image_len) {
  if (!plan || !image) return fail(GH_E_ARG, "null argument");
  const uint64_t hdr = image_header_bytes(plan), body = 4 * ceil_div(plan->g, GH_GAPS_PER_WORD) + 4 * plan->w;
  if (plan->nsyms > GH_MAX_SYMBOLS || plan->file_bytes != hdr + body) return fail(GH_E_ARG, "inconsistent plan");
  if (image_len < plan->file_bytes) return fail(GH_E_SMALL, "image buffer too small");
  uint8_t* o = (uint8_t*)image;
  const size_t off = gh::encode_header(plan, o);
  std::memset(o + off, 0, body);
  return GH_OK;
}

// Bytewise OR: the image's word area has no alignment, and OR does not care about the
// byte order inside a word.
extern "C" int gh_slice_merge(void* image, uint64_t image_len, const gh_encode_plan* plan, const gh_slice* s,
                              const uint32_t* words, const uint32_t* gapw) {
  if (!image || !plan || !s || (s->nwords && !words) || (s->ngapw && !gapw)) return fail(GH_E_ARG, "null argument");
  const uint64_t GW = ceil_div(plan->g, GH_GAPS_PER_WORD), hdr = image_header_bytes(plan);
  if (plan->file_bytes != hdr + 4 * GW + 4 * plan->w) return fail(GH_E_ARG, "inconsistent plan");
  if (s->word0 > plan->w || s->nwords > plan->w - s->word0 || s->gapw0 > GW || s->ngapw > GW - s->gapw0)
    return fail(GH_E_ARG, "slice extents outside the stream");
  if (image_len < plan->file_bytes) return fail(GH_E_SMALL, "image buffer too small");
  uint8_t* g = (uint8_t*)image + hdr + 4 * s->gapw0;
  uint8_t* w = (uint8_t*)image + hdr + 4 * GW + 4 * s->word0;
  const uint8_t* sg = (const uint8_t*)gapw;
  const uint8_t* sw = (const uint8_t*)words;
  for (uint64_t i = 0; i < 4 * s->ngapw; ++i) g[i] |= sg[i];
  for (uint64_t i = 0; i < 4 * s->nwords; ++i) w[i] |= sw[i];
  return GH_OK;
}

// Header of a seek index image (gaphuff.h); returns its size in bytes.
size_t gh::index_header(uint32_t log2_stride, uint64_t n, uint64_t g, uint64_t nentries, uint8_t* out) {
  wr<uint64_t>(out, GH_INDEX_MAGIC);
  wr<uint32_t>(out + 8, log2_stride);
  wr<uint32_t>(out + 12, 0u);
  wr<uint64_t>(out + 16, n);
  wr<uint64_t>(out + 24, g);
  wr<uint64_t>(out + 32, nentries);
  return IDX_HEADER;
}

// Which index entries a slice owns (gaphuff.h, "the index of a sliced stream"): the
// boundaries S * k inside its bits [base_bit, base_bit + bits).
extern "C" int gh_index_slice_extent(uint64_t base_bit, uint64_t bits, uint32_t log2_stride, uint64_t* k0,
                                     uint64_t* nk) {
  if (!k0 || !nk) return fail(GH_E_ARG, "null argument");
  if (log2_stride < GH_INDEX_MIN_LOG2 || log2_stride > GH_INDEX_MAX_LOG2)
    return fail(GH_E_ARG, "index stride outside 2^8 .. 2^20 segments");
  if (base_bit + bits < base_bit) return fail(GH_E_ARG, "slice end overflows 64 bits");
  const uint32_t sh = 7 + log2_stride;  // S = 1 << sh
  auto ceil_s = [&](uint64_t x) { return (x >> sh) + ((x & ((1ull << sh) - 1)) != 0); };
  *k0 = ceil_s(base_bit);
  *nk = ceil_s(base_bit + bits) - *k0;
  return GH_OK;
}

// The host index walk's body: the entries the bytes in[0..n) own as the slice at base_bit /
// sym_base (gaphuff.h); the whole stream is the slice at bit 0 / symbol 0.  The encoder
// knows every codeword's first bit, so entry k = sym_base + the first i with start(i) >=
// S * k falls out of a walk over the code lengths.  Threaded as the encode: per-thread bit
// totals, a scan, then thread t resolves the boundaries inside its bit range
// [base_bit + tbits[t], base_bit + tbits[t + 1]); the threads' ranges partition the
// slice's bits, so every owned boundary has exactly one such thread.  ent: 8 * cap bytes
// at any alignment, entry k at ent + 8 * (k - *k0).  want_bits (may be NULL): the bit
// total the input must have, checked before anything is written.
static int index_slice_body(const uint8_t* in, uint64_t n, const gh_encode_plan* plan, uint64_t base_bit,
                            uint64_t sym_base, uint32_t log2_stride, int threads, uint8_t* ent, uint64_t cap,
                            uint64_t* k0, uint64_t* nk, const uint64_t* want_bits) {
  const uint64_t S = (uint64_t)GH_SEGMENT_BITS << log2_stride;
  const int nt = (int)std::min<uint64_t>(n_threads(threads), std::max<uint64_t>(1, n >> 20));
  std::vector<uint64_t> tbits(nt + 1, 0);
  std::atomic<bool> absent{false};
  parallel_for(nt, [&](int t) {
    const uint64_t a = n * t / nt, b = n * (t + 1) / nt;
    uint64_t s = 0;
    bool zero = false;
    for (uint64_t i = a; i < b; ++i) {
      const uint32_t l = plan->len[in[i]];
      zero |= l == 0;
      s += l;
    }
    tbits[t + 1] = s;
    if (zero) absent = true;
  });
  if (absent) return fail(GH_E_TABLE, "a byte of the input has no code in the plan");
  for (int t = 0; t < nt; ++t) tbits[t + 1] += tbits[t];
  const uint64_t bits = tbits[nt];
  if (want_bits && bits != *want_bits) return fail(GH_E_ARG, "input does not match the plan");
  if (base_bit + bits < base_bit || base_bit + bits > plan->bits)
    return fail(GH_E_ARG, "slice ends past the plan's bit total");
  if (int rc = gh_index_slice_extent(base_bit, bits, log2_stride, k0, nk)) return rc;
  if (cap < *nk) return fail(GH_E_SMALL, "entry buffer too small");
  const uint64_t kbase = *k0;
  parallel_for(nt, [&](int t) {
    const uint64_t a = n * t / nt, b = n * (t + 1) / nt;
    const uint64_t lo = base_bit + tbits[t], hi = base_bit + tbits[t + 1];
    uint64_t k = ceil_div(lo, S);  // the first boundary at or past this thread's first bit
    if (k * S >= hi) return;
    uint64_t pos = lo;
    for (uint64_t i = a; i < b; ++i) {
      if (pos >= k * S) {  // (codewords are shorter than a stride: at most one boundary)
        wr<uint64_t>(ent + 8 * (k - kbase), sym_base + i);
        if (++k * S >= hi) return;
      }
      pos += plan->len[in[i]];
    }
    // boundaries inside the thread's last codeword: the next thread's (or slice's) first symbol
    for (; k * S < hi; ++k) wr<uint64_t>(ent + 8 * (k - kbase), sym_base + b);
  });
  return GH_OK;
}

extern "C" int gh_encode_index_slice(const uint8_t* in, uint64_t n, const gh_encode_plan* plan, uint64_t base_bit,
                                     uint64_t sym_base, uint32_t log2_stride, int threads, uint64_t* entries,
                                     uint64_t cap, uint64_t* k0, uint64_t* nk) {
  if (!plan || !k0 || !nk || (n && !in) || (cap && !entries)) return fail(GH_E_ARG, "null argument");
  if (log2_stride < GH_INDEX_MIN_LOG2 || log2_stride > GH_INDEX_MAX_LOG2)
    return fail(GH_E_ARG, "index stride outside 2^8 .. 2^20 segments");
  return index_slice_body(in, n, plan, base_bit, sym_base, log2_stride, threads, (uint8_t*)entries, cap, k0, nk,
                          nullptr);
}

extern "C" int gh_index_image_init(const gh_encode_plan* plan, uint32_t log2_stride, void* image,
                                   uint64_t image_len) {
  if (!plan || !image) return fail(GH_E_ARG, "null argument");
  const uint64_t bytes = gh_index_bytes(plan->g, log2_stride);
  if (bytes == 0) return fail(GH_E_ARG, "index stride outside 2^8 .. 2^20 segments");
  if (image_len < bytes) return fail(GH_E_SMALL, "index buffer too small");
  uint8_t* out = (uint8_t*)image;
  const uint64_t nentries = (bytes - IDX_HEADER) / 8;
  uint8_t* ent = out + gh::index_header(log2_stride, plan->n, plan->g, nentries, out);
  std::memset(ent, 0, 8 * (nentries - 1));
  wr<uint64_t>(ent + 8 * (nentries - 1), plan->n);
  return GH_OK;
}

// A bounds-checked store against the image's own header: the owned entries of different
// slices are disjoint (gaphuff.h), so nothing is combined.
extern "C" int gh_index_slice_merge(void* image, uint64_t image_len, uint64_t k0, uint64_t nk,
                                    const uint64_t* entries) {
  if (!image || (nk && !entries)) return fail(GH_E_ARG, "null argument");
  uint8_t* p = (uint8_t*)image;
  if (image_len < IDX_HEADER) return fail(GH_E_SMALL, "index image shorter than its header");
  if (rd<uint64_t>(p) != GH_INDEX_MAGIC) return fail(GH_E_FORMAT, "not a seek index (magic)");
  const uint64_t bytes = gh_index_bytes(rd<uint64_t>(p + 24), rd<uint32_t>(p + 8));
  if (bytes == 0 || rd<uint64_t>(p + 32) != (bytes - IDX_HEADER) / 8)
    return fail(GH_E_FORMAT, "index: entry count does not match G and the stride");
  if (image_len < bytes) return fail(GH_E_SMALL, "index image shorter than its entries");
  const uint64_t nblocks = (bytes - IDX_HEADER) / 8 - 1;  // the terminal entry belongs to no slice
  if (k0 > nblocks || nk > nblocks - k0) return fail(GH_E_ARG, "slice entries outside the index");
  if (nk) std::memcpy(p + IDX_HEADER + 8 * k0, entries, 8 * nk);
  return GH_OK;
}

// The seek index of the stream gh_encode_write produces, from the input alone: the image
// of gh_index_image_init with the entries of the slice at bit 0 / symbol 0, which owns
// every entry k < nblocks (every boundary lies below the stream's bit total: k * stride
// < G).
extern "C" int gh_encode_index(const uint8_t* in, const gh_encode_plan* plan, uint32_t log2_stride,
                               int threads, void* out_v, uint64_t out_len) {
  if (!plan || !out_v || (plan->n && !in)) return fail(GH_E_ARG, "null argument");
  const uint64_t bytes = gh_index_bytes(plan->g, log2_stride);
  if (bytes == 0) return fail(GH_E_ARG, "index stride outside 2^8 .. 2^20 segments");
  if (out_len < bytes) return fail(GH_E_SMALL, "index buffer too small");
  if (ceil_div(plan->bits, GH_SEGMENT_BITS) != plan->g) return fail(GH_E_ARG, "input does not match the plan");
  if (int rc = gh_index_image_init(plan, log2_stride, out_v, out_len)) return rc;
  const uint64_t nblocks = (bytes - IDX_HEADER) / 8 - 1;
  uint64_t k0 = 0, nk = 0;
  const int rc = index_slice_body(in, plan->n, plan, 0, 0, log2_stride, threads, (uint8_t*)out_v + IDX_HEADER,
                                  nblocks, &k0, &nk, &plan->bits);
  if (rc) return fail(GH_E_ARG, "input does not match the plan");
  return GH_OK;
}

// ---------------------------------------------------------------------------
// Generator (generate.cpp:32-47 distribution, counter-based PRNG)
// ---------------------------------------------------------------------------
static inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

extern "C" int gh_generate(uint64_t seed, double redundancy, uint64_t offset, uint64_t n,
                           uint8_t* out, int threads) {
  if (n && !out) return fail(GH_E_ARG, "null output");
  if (!(redundancy >= 0.0)) redundancy = 0.0;  // also maps NaN to 0
  if (redundancy > 1.0) redundancy = 1.0;
  // P(u < r) with u = k * 2^-53: threshold on the 53-bit integer
  const uint64_t thr = (uint64_t)(redundancy * 9007199254740992.0);  // r * 2^53
  const uint64_t key = mix64(seed ^ 0x6A09E667F3BCC909ull);
  const int nt = (int)std::min<uint64_t>(n_threads(threads), std::max<uint64_t>(1, n >> 22));
  parallel_for(nt, [&](int t) {
    const uint64_t a = n * t / nt, b = n * (t + 1) / nt;
    for (uint64_t i = a; i < b; ++i) {
      const uint64_t z = mix64(key + (offset + i + 1) * 0x9E3779B97F4A7C15ull);
      const bool low = (z >> 11) < thr;
      out[i] = low ? (uint8_t)('A' + (z & 3)) : (uint8_t)(z & 0xFF);
    }
  });
  return GH_OK;
}

extern "C" int gh_plan_shards(uint64_t g, uint32_t nshards, uint64_t* bounds) {
  if (!bounds || nshards == 0) return fail(GH_E_ARG, "bad shard request");
  for (uint32_t k = 0; k <= nshards; ++k)
    bounds[k] = (uint64_t)((unsigned __int128)g * k / nshards);
  return GH_OK;
}

// ---------------------------------------------------------------------------
// Byte planes (gaphuff.h, "byte planes"): the layout, the CPU twins of the split and join
// kernels (the same text, csrc/gh_planes.hpp) and the container.  No device.
// ---------------------------------------------------------------------------
static int planes_item_check(const gh_planes_item& it, const std::string& who) {
  if (!planes_elem_ok(it.elem_size)) return fail(GH_E_ARG, who + "element size not 1, 2, 4 or 8");
  if (!planes_mask_ok(it.elem_size, it.coded_mask)) return fail(GH_E_ARG, who + "coded_mask names a plane >= elem_size");
  return GH_OK;
}

extern "C" int gh_planes_layout(const gh_planes_item* items, uint32_t ntensors, gh_planes_slot* slots,
                                uint32_t* nstreams, uint64_t* stored_bytes) {
  if (nstreams) *nstreams = 0;
  if (stored_bytes) *stored_bytes = 0;
  if (!nstreams || !stored_bytes || (ntensors && (!items || !slots))) return fail(GH_E_ARG, "null argument");
  uint64_t ns = 0, at = 0;
  for (uint32_t t = 0; t < ntensors; ++t) {
    const gh_planes_item& it = items[t];
    const std::string who = "tensor " + std::to_string(t) + ": ";
    if (int rc = planes_item_check(it, who)) return rc;
    uint64_t padded;
    if (!planes_padded(it.nelem, &padded)) return fail(GH_E_ARG, who + "the stored arena overflows 64 bits");
    for (uint32_t p = 0; p < PLANES_MAX_E; ++p) {
      gh_planes_slot& s = slots[(uint64_t)PLANES_MAX_E * t + p];
      s = gh_planes_slot{GH_PLANES_STORED, 0, 0};
      if (p >= it.elem_size) continue;
      if ((it.coded_mask >> p) & 1u) {
        if (ns == PLANES_MAX_CODED) return fail(GH_E_ARG, who + "more than 2^24 coded planes");
        s.stream = (uint32_t)ns++;
      } else {
        s.stored_off = at;
        if (!planes_add(at, padded, &at)) return fail(GH_E_ARG, who + "the stored arena overflows 64 bits");
      }
    }
  }
  *nstreams = (uint32_t)ns;
  *stored_bytes = at;
  return GH_OK;
}

// Whole groups of 16 elements by the vector rule, the rest by the scalar rule.
template <uint32_t E>
static void planes_split_t(const uint8_t* src, uint64_t nelem, uint8_t* const* pl) {
  uint64_t i = 0;
  for (; i + PLANES_GROUP <= nelem; i += PLANES_GROUP) {
    uint32_t w[4 * E], o[E][4];
    std::memcpy(w, src + i * E, sizeof(w));
    planes_split16<E>(w, o);
    for (uint32_t p = 0; p < E; ++p) std::memcpy(pl[p] + i, o[p], 16);
  }
  for (; i < nelem; ++i)
    for (uint32_t p = 0; p < E; ++p) pl[p][i] = src[planes_src_index(i, E, p)];
}

template <uint32_t E>
static void planes_join_t(uint8_t* dst, uint64_t nelem, const uint8_t* const* pl) {
  uint64_t i = 0;
  for (; i + PLANES_GROUP <= nelem; i += PLANES_GROUP) {
    uint32_t w[4 * E], o[E][4];
    for (uint32_t p = 0; p < E; ++p) std::memcpy(o[p], pl[p] + i, 16);
    planes_join16<E>(o, w);
    std::memcpy(dst + i * E, w, sizeof(w));
  }
  for (; i < nelem; ++i)
    for (uint32_t p = 0; p < E; ++p) dst[planes_src_index(i, E, p)] = pl[p][i];
}

static int planes_twin_check(const gh_planes_item* item, const void* const* planes) {
  if (!item || !planes) return fail(GH_E_ARG, "null argument");
  if (int rc = planes_item_check(*item, "")) return rc;
  if (item->nelem) {
    if (!item->data) return fail(GH_E_ARG, "null tensor pointer");
    for (uint32_t p = 0; p < item->elem_size; ++p)
      if (!planes[p]) return fail(GH_E_ARG, "null plane pointer");
  }
  return GH_OK;
}

extern "C" int gh_planes_split_host(const gh_planes_item* item, void* const* planes) {
  if (int rc = planes_twin_check(item, planes)) return rc;
  const uint8_t* src = (const uint8_t*)item->data;
  uint8_t* const* pl = (uint8_t* const*)planes;
  switch (item->elem_size) {
    case 1: planes_split_t<1>(src, item->nelem, pl); break;
    case 2: planes_split_t<2>(src, item->nelem, pl); break;
    case 4: planes_split_t<4>(src, item->nelem, pl); break;
    default: planes_split_t<8>(src, item->nelem, pl); break;
  }
  return GH_OK;
}

extern "C" int gh_planes_join_host(const gh_planes_item* item, const void* const* planes) {
  if (int rc = planes_twin_check(item, planes)) return rc;
  uint8_t* dst = (uint8_t*)item->data;
  const uint8_t* const* pl = (const uint8_t* const*)planes;
  switch (item->elem_size) {
    case 1: planes_join_t<1>(dst, item->nelem, pl); break;
    case 2: planes_join_t<2>(dst, item->nelem, pl); break;
    case 4: planes_join_t<4>(dst, item->nelem, pl); break;
    default: planes_join_t<8>(dst, item->nelem, pl); break;
  }
  return GH_OK;
}

// Plane choice (gaphuff.h, "plane choice"): bits and nsyms of a plane's code by the host plan,
// sizes and decisions by csrc/gh_pmask.hpp, the text the decide kernel compiles too.
// One tensor of nelem > 0 elements from its e x 256 counts.
static int pmask_tensor(const uint64_t* counts, uint64_t nelem, uint32_t e, const std::string& who, uint32_t* mask,
                        uint64_t* plane_bytes) {
  for (uint32_t p = 0; p < e; ++p) {
    const uint64_t* c = counts + 256ull * p;
    uint64_t sum = 0;
    bool ok = true;
    for (uint32_t v = 0; v < 256; ++v) ok = planes_add(sum, c[v], &sum) && ok;
    if (!ok || sum != nelem) return fail(GH_E_ARG, who + "plane " + std::to_string(p) + ": the counts do not sum to nelem");
    gh_encode_plan plan;
    if (int rc = gh_encode_plan_from_counts(c, 0, &plan)) return fail(rc, who + gh_last_error());
    const uint64_t fb = pmask_file_bytes(plan.bits, plan.nsyms, nelem);
    if (plane_bytes) plane_bytes[p] = fb;
    if (pmask_coded(fb, nelem)) *mask |= 1u << p;
  }
  return GH_OK;
}

// The checks both host entry points share; clears the outputs.
static int pmask_check(const gh_planes_item* items, uint32_t ntensors, uint32_t* masks, uint64_t* plane_bytes) {
  if (ntensors && (!items || !masks)) return fail(GH_E_ARG, "null argument");
  uint32_t q0 = 0;
  for (uint32_t t = 0; t < ntensors; ++t) {
    const std::string who = "tensor " + std::to_string(t) + ": ";
    if (!planes_elem_ok(items[t].elem_size)) return fail(GH_E_ARG, who + "element size not 1, 2, 4 or 8");
    if (!pmask_next_q0(q0, items[t].elem_size, &q0)) return fail(GH_E_ARG, who + "more than 2^24 candidate planes");
  }
  for (uint32_t t = 0; t < ntensors; ++t) masks[t] = 0;
  if (plane_bytes) std::memset(plane_bytes, 0, sizeof(uint64_t) * PLANES_MAX_E * (size_t)ntensors);
  return GH_OK;
}

extern "C" int gh_pmask_from_counts(const uint64_t* counts, const gh_planes_item* items, uint32_t ntensors,
                                    uint32_t* masks, uint64_t* plane_bytes) {
  if (ntensors && !counts) return fail(GH_E_ARG, "null argument");
  if (int rc = pmask_check(items, ntensors, masks, plane_bytes)) return rc;
  uint32_t q0 = 0;
  for (uint32_t t = 0; t < ntensors; ++t) {
    const gh_planes_item& it = items[t];
    const uint64_t* c = counts + 256ull * q0;
    pmask_next_q0(q0, it.elem_size, &q0);
    if (!it.nelem) {  // (its counts must still be empty)
      for (uint32_t k = 0; k < 256u * it.elem_size; ++k)
        if (c[k]) return fail(GH_E_ARG, "tensor " + std::to_string(t) + ": the counts do not sum to nelem");
      continue;
    }
    if (int rc = pmask_tensor(c, it.nelem, it.elem_size, "tensor " + std::to_string(t) + ": ", &masks[t],
                              plane_bytes ? plane_bytes + (size_t)PLANES_MAX_E * t : nullptr))
      return rc;
  }
  return GH_OK;
}

extern "C" int gh_pmask_host(const gh_planes_item* items, uint32_t ntensors, uint32_t* masks, uint64_t* plane_bytes) {
  if (int rc = pmask_check(items, ntensors, masks, plane_bytes)) return rc;
  std::vector<uint64_t> counts(256 * PLANES_MAX_E);
  for (uint32_t t = 0; t < ntensors; ++t) {
    const gh_planes_item& it = items[t];
    const std::string who = "tensor " + std::to_string(t) + ": ";
    if (!it.nelem) continue;
    if (!it.data) return fail(GH_E_ARG, who + "null pointer");
    const uint32_t e = it.elem_size;
    if (it.nelem > UINT64_MAX / e) return fail(GH_E_ARG, who + "nelem * elem_size overflows 64 bits");
    std::fill(counts.begin(), counts.end(), 0);
    const uint8_t* src = (const uint8_t*)it.data;
    for (uint64_t i = 0; i < it.nelem; ++i)
      for (uint32_t p = 0; p < e; ++p) ++counts[256u * p + src[planes_src_index(i, e, p)]];
    if (int rc = pmask_tensor(counts.data(), it.nelem, e, who, &masks[t],
                              plane_bytes ? plane_bytes + (size_t)PLANES_MAX_E * t : nullptr))
      return rc;
  }
  return GH_OK;
}

// Element gather: the tensors' descriptors and the host plan (gaphuff.h, "element gather"), the
// loop form of what gh_pgather_scan_kernel and gh_pgather_expand_kernel do with the same
// arithmetic (gh_planes_gather.hpp).
int gh::pgather_descs(const gh_planes_item* items, uint32_t ntensors, std::vector<PlanesTensor>& desc,
                      uint32_t* nstreams, uint64_t* stored_bytes, uint32_t* max_coded) {
  std::vector<gh_planes_slot> slots((size_t)PLANES_MAX_E * std::max(ntensors, 1u));
  if (int rc = gh_planes_layout(items, ntensors, slots.data(), nstreams, stored_bytes)) return rc;
  desc.assign(ntensors, PlanesTensor{});
  *max_coded = 0;
  for (uint32_t t = 0; t < ntensors; ++t) {
    const gh_planes_item& it = items[t];
    if (it.nelem >= PG_MAX_TENSOR_BYTES / it.elem_size)
      return fail(GH_E_ARG, "tensor " + std::to_string(t) + ": 2^40 bytes or more");
    PlanesTensor& d = desc[t];
    d.nelem = it.nelem;
    d.elem = it.elem_size;
    d.mask = it.coded_mask;
    *max_coded = std::max(*max_coded, pg_popc(d.mask));
    for (uint32_t p = 0; p < PLANES_MAX_E; ++p) {
      d.stream[p] = slots[PLANES_MAX_E * t + p].stream;
      d.off[p] = slots[PLANES_MAX_E * t + p].stored_off;
    }
  }
  return GH_OK;
}

extern "C" int gh_pgather_plan(const gh_planes_item* items, uint32_t ntensors, const uint32_t* stream_status,
                               const gh_erange* ranges, uint32_t nranges, gh_brange* branges, uint64_t cap,
                               uint64_t* nbranges, uint64_t* stage_off, uint64_t* dst_off, uint64_t* out_bytes,
                               uint32_t* bad_ranges) {
  if (nbranges) *nbranges = 0;
  if (out_bytes) *out_bytes = 0;
  if (bad_ranges) *bad_ranges = 0;
  if (!nbranges || !out_bytes || !bad_ranges || (ntensors && !items) || (nranges && (!ranges || !stage_off || !dst_off)) ||
      (cap && !branges))
    return fail(GH_E_ARG, "null argument");
  if (nranges > PG_MAX_RANGES) return fail(GH_E_ARG, "gh_pgather_plan: more than 2^21 ranges in one call");
  std::vector<PlanesTensor> desc;
  uint32_t ns = 0, maxc = 0;
  uint64_t stored_bytes = 0;
  if (int rc = pgather_descs(items, ntensors, desc, &ns, &stored_bytes, &maxc)) return rc;
  uint64_t nb = 0, stage = 0, dst = 0;
  uint32_t bad = 0;
  for (uint32_t i = 0; i < nranges; ++i) {
    const PgLoc loc = pg_locate([&](uint32_t t) -> const PlanesTensor& { return desc[t]; },
                                [&](uint32_t s) { return stream_status ? stream_status[s] : 0u; }, ntensors, ranges[i]);
    if (loc.ncoded == PG_BAD)
      return fail(GH_E_ARG, "range " + std::to_string(i) + ": no such tensor, or elements outside [0, nelem] of its tensor");
    if (nb + loc.ncoded <= cap) pg_emit(desc[ranges[i].tensor], ranges[i], branges + nb);
    stage_off[i] = stage;
    dst_off[i] = dst;
    nb += loc.ncoded;
    stage += loc.stage;
    dst += loc.dst;
    bad += loc.flagged;
  }
  *nbranges = nb;
  *out_bytes = dst;
  *bad_ranges = bad;
  if (nb > cap) return fail(GH_E_SMALL, "byte-range buffer smaller than the plan");
  return GH_OK;
}

// The container: 24 header bytes, E plane sizes, then the planes on 8-byte boundaries.
constexpr uint64_t PLANES_HEADER = 24;

extern "C" int gh_planes_image_bytes(uint32_t elem_size, const uint64_t* plane_bytes, uint64_t* total) {
  if (total) *total = 0;
  if (!plane_bytes || !total) return fail(GH_E_ARG, "null argument");
  if (!planes_elem_ok(elem_size)) return fail(GH_E_ARG, "element size not 1, 2, 4 or 8");
  uint64_t at = PLANES_HEADER + 8ull * elem_size;
  for (uint32_t p = 0; p < elem_size; ++p) {
    uint64_t start;
    if (!planes_add(at, 7, &start) || !planes_add(start & ~7ull, plane_bytes[p], &at))
      return fail(GH_E_ARG, "the container's size overflows 64 bits");
  }
  *total = at;
  return GH_OK;
}

extern "C" int gh_planes_image_write(const gh_planes_item* item, const void* const* planes, const uint64_t* plane_bytes,
                                     void* out, uint64_t out_len) {
  if (!item || !planes || !plane_bytes || !out) return fail(GH_E_ARG, "null argument");
  if (int rc = planes_item_check(*item, "")) return rc;
  const uint32_t e = item->elem_size;
  for (uint32_t p = 0; p < e; ++p) {
    if (plane_bytes[p] && !planes[p]) return fail(GH_E_ARG, "null plane pointer");
    if (!((item->coded_mask >> p) & 1u) && plane_bytes[p] != item->nelem)
      return fail(GH_E_ARG, "plane " + std::to_string(p) + ": a stored plane holds nelem bytes");
  }
  uint64_t total;
  if (int rc = gh_planes_image_bytes(e, plane_bytes, &total)) return rc;
  if (out_len < total) return fail(GH_E_SMALL, "output buffer smaller than the container");
  uint8_t* o = (uint8_t*)out;
  std::memset(o, 0, total);
  const uint64_t magic = GH_PLANES_MAGIC;
  std::memcpy(o, &magic, 8);
  std::memcpy(o + 8, &item->elem_size, 4);
  std::memcpy(o + 12, &item->coded_mask, 4);
  std::memcpy(o + 16, &item->nelem, 8);
  uint64_t at = PLANES_HEADER + 8ull * e;
  for (uint32_t p = 0; p < e; ++p) {
    std::memcpy(o + PLANES_HEADER + 8ull * p, &plane_bytes[p], 8);
    at = (at + 7) & ~7ull;
    if (plane_bytes[p]) std::memcpy(o + at, planes[p], plane_bytes[p]);
    at += plane_bytes[p];
  }
  return GH_OK;
}

extern "C" int gh_planes_parse(const void* file, size_t file_len, gh_planes_image* out) {
  if (!file || !out) return fail(GH_E_ARG, "null argument");
  *out = gh_planes_image{};
  const uint8_t* f = (const uint8_t*)file;
  const uint64_t len = file_len;
  if (len < PLANES_HEADER || rd<uint64_t>(f) != GH_PLANES_MAGIC) return fail(GH_E_FORMAT, "not a byte-plane container");
  gh_planes_image im{};
  im.elem_size = rd<uint32_t>(f + 8);
  im.coded_mask = rd<uint32_t>(f + 12);
  im.nelem = rd<uint64_t>(f + 16);
  if (!planes_elem_ok(im.elem_size)) return fail(GH_E_FORMAT, "element size not 1, 2, 4 or 8");
  if (!planes_mask_ok(im.elem_size, im.coded_mask)) return fail(GH_E_FORMAT, "coded_mask names a plane >= elem_size");
  uint64_t at = PLANES_HEADER + 8ull * im.elem_size;
  if (len < at) return fail(GH_E_FORMAT, "truncated plane sizes");
  for (uint32_t p = 0; p < im.elem_size; ++p) {
    const std::string who = "plane " + std::to_string(p) + ": ";
    const uint64_t nb = rd<uint64_t>(f + PLANES_HEADER + 8ull * p);
    at = (at + 7) & ~7ull;  // (at <= len < 2^64 - 7: a file in memory)
    if (at > len || nb > len - at) return fail(GH_E_FORMAT, who + "outside the file");
    im.plane[p] = f + at;
    im.plane_bytes[p] = nb;
    if ((im.coded_mask >> p) & 1u) {
      if (gh_stream_parse(f + at, nb, &im.stream[p])) return fail(GH_E_FORMAT, who + gh_last_error());
      if (im.stream[p].n != im.nelem) return fail(GH_E_FORMAT, who + "its stream's n is not nelem");
    } else if (nb != im.nelem) {
      return fail(GH_E_FORMAT, who + "a stored plane holds nelem bytes");
    }
    at += nb;  // (<= len)
  }
  *out = im;
  return GH_OK;
}

extern "C" const char* gh_version(void) { return "gaphuff-mi355x 0.1 (gfx950)"; }
extern "C" const char* gh_last_error(void) { return g_last_error.c_str(); }
