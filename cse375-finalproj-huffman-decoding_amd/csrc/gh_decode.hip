// gh_decode.hip — MI355X (gfx950) gap-array Huffman decoder: the decode kernels and the
// host context behind the C ABI (include/gaphuff.h).
//
// Replaces the reference hot path gpu_dec_l1_l2 (Huffman_coding_Gap_arrays/decoder/
// src/decoder.cu:454-730) and its launcher decoder_l1_l2 (decoder.cu:732-815).
// Semantics kept from the reference:
//   * segment i (128 bits = 4 payload words) starts at bit 128*i + gap[i-1], the gap
//     being a 4-bit nibble, 8 per u32 (decoder.cu:501-507);
//   * a segment decodes every codeword that starts inside it (decoder.cu:529-569);
//   * outputs are concatenated in segment order by an exclusive scan of the
//     per-segment symbol counts (decoder.cu:571-653).
// Two decode structures, chosen per code on the host:
//   * gh_tile.hip — grouped codes (complete, 4 <= len <= 12, e.g. BASELINE r = 0.1): one
//     persistent kernel, one decode pass, round-leader prefixes;
//   * gh_wsplit.hip — every other code: count, scan and write kernels in which no wave
//     waits for another, four symbols per write lookup, a canonical fallback for
//     codewords longer than the tables and for incomplete codes.
// Every output write is clamped at the shard's output capacity (the reference wrote
// past N, decoder.cu:672-728).  Tables: gh_lut.hpp; device helpers: gh_device.hpp.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "gh_batch_range.hpp"
#include "gh_device.hpp"
#include "gh_gather_range.hpp"
#include "gh_hip.hpp"
#include "gh_internal.hpp"
#include "gh_lut.hpp"
#include "gh_planes.hpp"
#include "gh_planes_gather.hpp"
#include "gh_raw_trans.hpp"
#include "gh_units.hpp"

namespace gh {

constexpr uint32_t EPOCH_MAX = (1u << 24) - 1;

#include "gh_tile.hip"
#include "gh_wsplit.hip"
#include "gh_index.hip"
#include "gh_gather.hip"
#include "gh_gather_plan.hip"
#include "gh_batch.hip"
#include "gh_batch_raw.hip"
#include "gh_batch_gather.hip"
#include "gh_planes_join.hip"
#include "gh_planes_gather.hip"
#include "gh_mtile.hip"

}  // namespace gh

using namespace gh;

// Tile kernel shapes: codes of >= 4-bit codewords (at most 32 per segment) run three
// segments per lane with 8 output words each; codes with 3-bit codewords (at most 43
// per segment, e.g. BASELINE's r = 0.5 codes) two segments per lane with 11 words (the
// registers and the staging of a third segment would halve the workgroups per CU).
static uint32_t tile_u_for(uint32_t minlen) { return minlen >= 4 ? (uint32_t)TILE_U : (uint32_t)TILE_U3; }
#ifndef GH_TILE_OW7
#define GH_TILE_OW7 1  // codes of >= 5-bit codewords: 7 output words per segment (<= 26 codewords)
#endif
// A picked kernel: its launch pointer and the name of its template instantiation
// (gh_ctx_kernel_shape, gh_kernel_shapes).  Both come from the one template argument list
// of the *_kern functions below, so the name cannot drift from the pointer.
struct Kern {
  const void* fn;
  const char* name;
  const void* fn_known = nullptr;  // tile kernel: its known-offsets instantiation (same name: a
                                   // shape names U / G / OW / MINL, not the mode of one decode)
};
template <class... A>
static std::string kern_name(const char* fmt, A... a) {
  char b[96];
  snprintf(b, sizeof(b), fmt, a...);
  return b;
}
template <int TB, int U, int G, int OW, int MINL>
static Kern tile_kern() {
  static const std::string n = kern_name("tile<%d,%d,%d,%d,%d>", TB, U, G, OW, MINL);
  return {(const void*)gh_tile_kernel<TB, U, G, OW, MINL, false>, n.c_str(),
          (const void*)gh_tile_kernel<TB, U, G, OW, MINL, true>};
}
template <int TB, int GL, int NS, bool FB, int NP = 1>
static Kern mtile_kern() {
  static const std::string n = kern_name("mtile<%d,%d,%d,fb=%d,np=%d>", TB, GL, NS, (int)FB, NP);
  return {(const void*)gh_mtile_kernel<TB, GL, NS, FB, NP>, n.c_str()};
}
template <int U, int TB, int GL, bool FB>
static Kern ws_count_kern() {
  static const std::string n = kern_name("ws_count<%d,%d,%d,fb=%d>", U, TB, GL, (int)FB);
  return {(const void*)gh_ws_count_kernel<U, TB, GL, FB>, n.c_str()};
}
template <int U, int TB, int GL, int NS, bool FB>
static Kern ws_write_kern() {
  static const std::string n = kern_name("ws_write<%d,%d,%d,%d,fb=%d>", U, TB, GL, NS, (int)FB);
  return {(const void*)gh_ws_write_kernel<U, TB, GL, NS, FB>, n.c_str()};
}

static Kern tile_kernel_for(uint32_t minlen, uint32_t g) {
  if (minlen >= 5 && GH_TILE_OW7)
    return g >= 4 ? tile_kern<TILE_TB, TILE_U, 4, 7, 5>()
         : g == 3 ? tile_kern<TILE_TB, TILE_U, 3, 7, 5>()
                  : tile_kern<TILE_TB, TILE_U, 2, 7, 5>();
  if (minlen >= 4)
    return g >= 4 ? tile_kern<TILE_TB, TILE_U, 4, 8, 4>()
         : g == 3 ? tile_kern<TILE_TB, TILE_U, 3, 8, 4>()
                  : tile_kern<TILE_TB, TILE_U, 2, 8, 4>();
  return g >= 4 ? tile_kern<TILE_TB, TILE_U3, 4, 11, 3>()
       : g == 3 ? tile_kern<TILE_TB, TILE_U3, 3, 11, 3>()
                : tile_kern<TILE_TB, TILE_U3, 2, 11, 3>();
}

// Two-pass tile kernel by lookups per window shift and 16-byte stores per copy-out.
template <int GL, bool FB>
static Kern mtile_ns(int ns) {
  return ns <= 4 ? mtile_kern<MT_TB, GL, 4, FB>()
       : ns <= 6 ? mtile_kern<MT_TB, GL, 6, FB>()
       : ns <= 8 ? mtile_kern<MT_TB, GL, 8, FB>()
                 : mtile_kern<MT_TB, GL, 5, FB, 2>();  // (10: two copy-out parts of 5 x 64 chunks)
}
// fb: codewords longer than the tables (K = 11..12, GL = 2) through the canonical fallback
static Kern mtile_kernel_for(int gl, int ns, bool fb = false) {
  if (fb) return mtile_ns<2, true>(ns);
  return gl >= 4 ? mtile_ns<4, false>(ns) : gl == 3 ? mtile_ns<3, false>(ns) : mtile_ns<2, false>(ns);
}

struct WsKernels {
  Kern count;
  Kern write;
};
template <int GL, bool FB = false>
static Kern ws_write_ns(int ns) {
  return ns <= 2 ? ws_write_kern<WS_U, WS_TB, GL, 2, FB>()
         : ns <= 3 ? ws_write_kern<WS_U, WS_TB, GL, 3, FB>()
         : ns <= 4 ? ws_write_kern<WS_U, WS_TB, GL, 4, FB>()
         : ns <= 6 ? ws_write_kern<WS_U, WS_TB, GL, 6, FB>()
                   : ws_write_kern<WS_U, WS_TB, GL, 8, FB>();
}
// The <GL, FB> member of a kernel family keyed by a table's width: GL lookups of `bits`
// bits per window shift, or the canonical fallback with two.  kern(gl, fb) receives the
// two as integral constants and returns the instantiation.
template <class F>
static auto kernel_by_width(uint32_t bits, bool fb, F kern) {
  using std::integral_constant;
  if (fb) return kern(integral_constant<int, 2>{}, std::true_type{});
  const int gl = lookups_per_shift(bits);
  return gl >= 4 ? kern(integral_constant<int, 4>{}, std::false_type{})
       : gl == 3 ? kern(integral_constant<int, 3>{}, std::false_type{})
                 : kern(integral_constant<int, 2>{}, std::false_type{});
}
// Count kernel by its LUT width Kc, write kernel by K and NS (store instructions per
// lane per piece: the typical piece's 16-byte chunks / 64).  fb: codes longer than the
// tables or incomplete codes (canonical fallback, two lookups per window shift).
static WsKernels ws_kernels(uint32_t Kc, uint32_t K, int ns, bool fb) {
  return {kernel_by_width(Kc, fb, [](auto gl, auto f) { return ws_count_kern<WS_UC, WS_TBC, decltype(gl)::value, decltype(f)::value>(); }),
          kernel_by_width(K, fb, [ns](auto gl, auto f) { return ws_write_ns<decltype(gl)::value, decltype(f)::value>(ns); })};
}

// Every name the pickers can return, one per line: the pickers enumerated over their
// argument domains (shortest codeword and codewords per shift; lookups per shift, stores
// per copy-out and fallback; table widths, stores per piece and fallback).  No device.
static std::string all_kernel_shapes() {
  std::vector<std::string> v;
  auto add = [&](const char* n) {
    if (std::find(v.begin(), v.end(), n) == v.end()) v.push_back(n);
  };
  for (uint32_t ml = 3; ml <= 12; ++ml)
    for (uint32_t g = 2; g <= 4; ++g) add(tile_kernel_for(ml, g).name);
  for (int fb = 0; fb <= 1; ++fb)
    for (int gl = 2; gl <= 4; ++gl)
      for (int ns = 4; ns <= 10; ++ns) add(mtile_kernel_for(gl, ns, fb != 0).name);
  for (int pass = 0; pass < 2; ++pass)  // the count names, then the write names
    for (int fb = 0; fb <= 1; ++fb)
      for (uint32_t kc = 2; kc <= 14; ++kc)
        for (uint32_t k = 2; k <= 12; ++k)
          for (int ns = 2; ns <= 8; ++ns) {
            const WsKernels w = ws_kernels(kc, k, ns, fb != 0);
            add(pass ? w.write.name : w.count.name);
          }
  std::string s;
  for (const std::string& n : v) s += n + "\n";
  return s;
}

// The lane-major load of the tile kernel reads U segments past the shard end (a lane
// clamped to segment nseg: words up to 4 * (nseg + U) - 1, gh_tile.hip); gh_ctx_load /
// gh_ctx_load_device allocate 4 * nseg + 16 words, the tail zeroed, which covers U <= 4
// with no word to spare.  Its gap load reads dword gwords at most of gwords + 4.
static_assert(TILE_U <= 4 && TILE_U3 <= 4, "payload padding (16 words) covers at most 4 segments per lane");

// ---- the context, by parts ---------------------------------------------------------
// Each part owns its device memory (DevBuf): resetting a part frees it.

// The loaded shard: segments [seg_begin, seg_end) of a stream of g_total.
struct Shard {
  uint64_t nseg = 0, seg_begin = 0, seg_end = 0, n_total = 0, g_total = 0;
  uint32_t gap_nib0 = 0, first_start = 0;  // nibble of local segment 0's end in `gaps`; its start bit
  uint32_t last_end = 0;  // wave split: end bit of the stream's last segment when the shard holds it
  DevBuf payload;         // words [4 b, 4 e + 1) of the stream + zero padding (16 words in all)
  DevBuf gaps;            // gap words from word b / 8
  DevBuf out;
  uint64_t out_cap = 0;
};

enum class Mode { NONE, TILE, MTILE, WSPLIT };  // (NONE: nothing loaded, or an empty shard)

// Tile kernel (grouped codes) and two-pass tile kernel (gh_mtile.hip).
struct TilePlan {
  uint32_t ntiles = 0;
  uint32_t kbits = 0;      // LUT width (two-pass: its write table's)
  uint32_t kbits_c = 0;    // two-pass: its count table's width
  uint32_t lut_lgr = 0;    // tile: log2 copies of the LUT in LDS
  uint32_t clut_lgr = 0;   // two-pass: log2 copies of the count table in LDS
  uint32_t lut_bytes = 0;  // LDS bytes of the tables (tile: the LUT's copies; two-pass: write + count + fallback)
  uint32_t stage_bytes = 0;  // one staging buffer (tile) / one wave's region (two-pass)
  uint32_t idle_block = 0xFFFFFFFFu;  // GH_TILE_IDLE experiments: a block that exits at once
  uint32_t epoch = 0;
  uint64_t gran_words = 0;
  DevBuf lut;     // the tables as they lie in LDS (one copy each)
  DevBuf gran;    // granules, within-round prefixes, round starts
  DevBuf stamps;  // GH_TILE_STAMPS builds only
  // Known piece offsets (tile kernel only, gh_tile.hip): piece_off holds 16 ntiles + 1 u64,
  // entry 16 t + w the output offset of wave w's piece of tile t, the last one the shard's
  // total.  They are a function of the loaded shard alone, so they live as long as the load:
  //   GH_OFFS_NONE      after a load (and after a decode that reported a status);
  //   GH_OFFS_RECORDED  a chained decode, which writes the table, has been launched;
  //   GH_OFFS_READY     the host has seen that decode finished with status 0 (at a wait it
  //                     makes anyway: offsets_settle): later decodes run the known-offsets
  //                     instantiation, which reads the table.
  DevBuf piece_off;
  int offs_state = GH_OFFS_NONE;
  bool offs_on = false;   // the table exists and GH_TILE_OFFS=0 is not set
  size_t lds_known = 0;   // dynamic LDS of the known-offsets instantiation
  uint32_t lgr_known = 0; // its log2 LUT copies (lut_lgr unless GH_TILE_KLGR)
};

// Wave split (every other code): count, scan and write kernels.
struct WsPlan {
  Kern count{};            // (the write kernel is Plan::kern)
  uint32_t grid_c = 0;     // workgroups of the count kernel
  size_t lds_count = 0;    // its dynamic LDS
  uint32_t k = 0, kc = 0;  // write / count LUT widths
  uint32_t lgc = 0;        // log2 count-LUT copies in LDS
  uint32_t lut_bytes = 0;  // LDS bytes of the write LUT
  uint32_t stage_bytes = 0;  // one wave's staging in the write kernel
  uint32_t nblocks = 0, nranges = 0;  // superblocks; ranges (one per wave of the write grid)
  DevBuf lut_c;    // count LUT {b | end mask << 16}
  DevBuf lut_w;    // write LUT {symbols, b | n << 8}
  DevBuf fb;       // canonical fallback tables
  DevBuf seg_cnt, junk, rng_tot, rng_off;
};

// How the loaded shard is decoded: picked once by the load, launched as stored.
struct Plan {
  Mode mode = Mode::NONE;
  Kern kern{};             // the tile / two-pass tile / wave-split write kernel
  uint32_t grid = 0, block = 0;
  size_t lds = 0;          // its dynamic LDS
  std::string shape;       // the picked kernel name(s) (gh_ctx_kernel_shape)
  TilePlan tile;           // mode TILE or MTILE
  WsPlan ws;               // mode WSPLIT
  bool tiled() const { return mode == Mode::TILE || mode == Mode::MTILE; }
};

// Range gather (gh_ctx_gather): the tables live from the first gather to the next load,
// the piece and output buffers for the life of the context (grown on demand).
struct GatherTables {
  bool ready = false;
  uint32_t kc = 0, ks = 0;  // count / symbol table widths
  uint32_t last_end = 0;
  uint32_t wgs = 0;         // workgroups the device holds at once
  size_t lds = 0;
  const void* kern = nullptr;
  DevBuf lut_c;  // count table {b | end mask << 16}
  DevBuf lut_s;  // symbol table {len | symbol << 8}
  DevBuf fb;     // canonical fallback tables
};
struct Gather {
  GatherTables tab;
  DevBuf d_pieces, d_out;
  std::vector<gh_gather_piece> pieces;
  EventPair ev;
};
// Device-planned gather (gh_ctx_gather_device): the resident index lives from
// gh_ctx_set_index to the next load, the plan's buffers for the life of the context (grown
// on demand; its pieces are not the host gather's, which may run while one is in flight).
struct DevGather {
  bool has_index = false;
  uint32_t log2_stride = 0;
  uint64_t nblocks = 0;
  DevBuf offsets, rank;  // nblocks + 1 entries as aligned u64; gh_gather_range.hpp's rank
  DevBuf loc, slot, dst0, pieces;
  Event ev_a, ev_b, ev_c;  // before the plan kernels, after them, after the gather kernel
  bool enqueued = false;   // a device gather since the load: ev_c marks the last one
  hipStream_t last_stream = nullptr;
};

struct Timing {
  std::vector<EventPair> pending, pool;  // timed decodes not yet reported; idle pairs
  double acc_ms = 0;
  uint32_t nlaunch = 0;
};

struct gh_ctx {
  int device = 0;
  int num_cu = 0;
  Stream stream;
  Event done;  // recorded after every untimed decode, on the stream it ran on
  bool done_rec = false;
  hipEvent_t done_ev = nullptr;  // marks the last decode: `done`, or the timed decode's end event
  bool loaded = false;
  Canon canon;
  DevBuf misc;  // u32 [1] status, [2..3] symbol total, [4..11] tile poll counters, [16] gather status,
                // device-planned gather: [18] status, [19] piece count, [20..21] bytes, [22..23] pieces (u64)
  Shard shard;
  Plan plan;
  Gather gather;
  DevGather dgather;
  Timing timing;
  ~gh_ctx();
  unsigned int* misc_at(int i) const { return misc.get<unsigned int>() + i; }
};

static void free_shard(gh_ctx* c) {
  (void)hipSetDevice(c->device);
  c->shard = Shard{};
  c->plan = Plan{};
  c->gather.tab = GatherTables{};
  c->dgather.has_index = false;  // (releasing device memory waits for a gather still in flight)
  c->dgather.offsets.reset();
  c->dgather.rank.reset();
  c->dgather.enqueued = false;
  c->loaded = false;
}

// Raises a kernel's dynamic LDS limit where a launch needs more than the 64 KiB default.
static int allow_lds(const void* fn, size_t lds) {
  if (lds > 64 * 1024) GH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return GH_OK;
}


// GH_TILE_GRID=n (n >= 2; tests): fewer workgroups of a persistent kernel than fit the
// device, so a small stream gives each decoding workgroup many tiles and rounds.  It only
// lowers the grid.
static uint32_t tile_grid_cap(uint32_t grid) {
  if (const char* e = getenv("GH_TILE_GRID"))
    if (grid > 2) return (uint32_t)std::clamp<long>(atol(e), 2, (long)grid);
  return grid;
}

// The part of a tile plan that both tile kernels share, once the kernel and its tables are
// known: the grid (workgroup 0 leads the rounds, up to LEAD_A aggregates per thread: D =
// grid - 1 <= LEAD_A * block, the others decode; every workgroup must be resident at once:
// `resident` is what the device holds, and decodes on one device are chained, see
// DevChain) and the per-tile aggregates and prefixes.  Leaves p.grid < 2 when the shard is
// too small for the kernel (the wave split then takes the code).
static int tile_grid_and_granules(Plan& p, uint64_t resident) {
  p.grid = (uint32_t)std::min<uint64_t>({(uint64_t)p.tile.ntiles + 1, resident, (uint64_t)LEAD_A * p.block});
  p.grid = tile_grid_cap(p.grid);
  if (p.grid < 2) return GH_OK;
  p.tile.gran_words = 2ull * p.tile.ntiles + 2;
  if (int rc = p.tile.gran.alloc(8ull * p.tile.gran_words, true)) return rc;
  // the piece-offset table of a kernel with a known-offsets instantiation (the tile kernel;
  // GH_TILE_OFFS=0 keeps every decode chained: tests, A/B timing).  The chained kernel
  // writes it in either case.
  if (p.kern.fn_known) {
    if (int rc = p.tile.piece_off.alloc(8ull * (16ull * p.tile.ntiles + 1), true)) return rc;
    const char* e = getenv("GH_TILE_OFFS");
    p.tile.offs_on = !(e && e[0] == '0');
  }
  return GH_OK;
}

// ---- tile kernel setup -----------------------------------------------------------
// LUT width K (>= maxlen), replicated 2^lgr times in LDS: the largest replication that
// keeps the best occupancy.  Returns GH_OK with the plan's mode left NONE when the kernel
// does not fit a CU (the wave split then takes the code).
static int tile_setup(gh_ctx* c, uint32_t K, double avg_seg_bytes) {
  const Canon& cn = c->canon;
  Plan p;
  TilePlan& t = p.tile;
  const uint32_t maxsyms = (128 + cn.minlen - 1) / cn.minlen;  // <= 43 (minlen >= 3)
  t.kbits = K;
  const uint32_t tile_u = tile_u_for(cn.minlen);
  t.ntiles = (uint32_t)ceil_div(c->shard.nseg, (uint64_t)tile_u * TILE_TB);
  // Staging is sized for the typical piece, not the worst case (128 / minlen bytes per
  // segment): TILE_SCAP = 20 bytes per segment for grouped codes (r = 0.1: 16.5), the
  // stream's mean + 12 % for minlen-3 codes (r = 0.5: 21.5 -> 25), so that the LUT's
  // copies and TILE_LAG regions per wave fit a CU's LDS.  A wave's piece is the sum of
  // 128-192 segments, so it stays near its mean; a larger one stores straight from
  // registers (gh_tile_kernel).  The copy-out's TILE_NS * 64 chunks cover a region.  The
  // known-offsets instantiation stages a piece up to 15 bytes further into the same region
  // (at the phase of its output offset), so its longest staged piece is 16 bytes shorter,
  // and it uses one region per wave.  GH_TILE_SCAP overrides (tests).
  double scapf = 1.12;
  if (const char* e = getenv("GH_TILE_SCAPF")) scapf = std::clamp(atof(e), 0.5, 4.0);
  uint64_t per_seg = std::min<uint64_t>(
      maxsyms, cn.minlen >= 4 ? (uint64_t)TILE_SCAP : (uint64_t)std::ceil(std::max(avg_seg_bytes, 1.0) * scapf + 1));
  if (const char* e = getenv("GH_TILE_SCAP")) per_seg = std::min<uint64_t>(maxsyms, (uint64_t)std::max(1, atoi(e)));
  const uint64_t margin = 4ull * (cn.minlen >= 4 ? 8 : 11) + 4;  // garbage past a piece's end (4 OW + 4, OW <= 8 / 11)
  const uint64_t seg_wave = 64ull * tile_u;
  per_seg = std::min<uint64_t>(per_seg, ((uint64_t)TILE_NS * 64 * 16 - 2 * STAGE_PAD - margin) / seg_wave);
  t.stage_bytes = (uint32_t)((STAGE_PAD + seg_wave * per_seg + margin + 15) & ~15ull);
  const std::vector<uint32_t> lt = grouped_lut(cn, K);
  // by the shortest codeword (>= 5 with 7 output words, >= 4, 3) and the codewords per window shift
  p.kern = tile_kernel_for(cn.minlen, std::min<uint32_t>(4, 32 / cn.maxlen));
  p.block = TILE_TB;
  if (int rc = allow_lds(p.kern.fn, 160 * 1024)) return rc;
  const char* envr = getenv("GH_LGR");
  const int lg = envr ? std::clamp(atoi(envr), 0, 14 - (int)K) : std::min(5, 14 - (int)K);
  int best = 0, best_lg = 0;
  for (int l2 = lg; l2 >= 0; --l2) {
    int pc = 0;
    GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, p.kern.fn, TILE_TB, tile_lds_bytes(4ull << (K + l2), t.stage_bytes)));
    if (pc > best) {
      best = pc;
      best_lg = l2;
    }
    if (envr) break;
  }
  // The kernel is compiled for 4 waves per SIMD: one 1024-thread workgroup per CU (two
  // of a GH_TILE_TB=512 build).  The occupancy query can answer one more than the hardware
  // admits at these SGPR counts (MI355X guide, "Occupancy API one block/CU high"); a grid
  // that is not resident at once never finishes (its bounded polls then report
  // GH_ST_TIMEOUT), so never plan more than two.
  best = std::min(best, 2);
  if (best < 1) return GH_OK;
  t.lut_lgr = (uint32_t)best_lg;
  t.lut_bytes = (uint32_t)(4ull << (K + best_lg));
  p.lds = tile_lds_bytes(t.lut_bytes, t.stage_bytes);
  // the known-offsets instantiation: same grid, LUT copies and regions (its freed LDS is
  // left free), so whatever holds the chained grid resident holds this one
  // (GH_TILE_KLGR=n, experiments: 2^n times the LUT copies in its freed LDS, where they
  // fit; measured no faster on cfg4)
  t.lgr_known = t.lut_lgr;
  if (const char* e = getenv("GH_TILE_KLGR")) {
    const uint32_t want = std::min<uint32_t>(t.lut_lgr + (uint32_t)std::clamp(atoi(e), 0, 5), 14 - K);
    if (tile_lds_bytes_known(4ull << (K + want), t.stage_bytes) <= 160 * 1024) t.lgr_known = want;
  }
  t.lds_known = tile_lds_bytes_known(4ull << (K + t.lgr_known), t.stage_bytes);
  if (int rc = allow_lds(p.kern.fn_known, 160 * 1024)) return rc;
  if (int rc = tile_grid_and_granules(p, (uint64_t)best * c->num_cu)) return rc;
  if (p.grid < 2) return GH_OK;
  if (const char* e = getenv("GH_TILE_IDLE"))  // experiment: block grid / 2 (the leader's CU partner) idles
    if (atoi(e) && p.grid == (uint32_t)best * c->num_cu && best == 2) t.idle_block = p.grid / 2;
  if (int rc = t.lut.upload(lt.data(), 4ull << K)) return rc;
  if (GH_TILE_STAMPS)
    if (int rc = t.stamps.alloc(32ull * p.grid * 2 * 128 + 8ull * (3ull * t.ntiles + 64 + 4 * 1024 + 4ull * p.grid), true))
      return rc;
  p.shape = p.kern.name;
  p.mode = Mode::TILE;
  c->plan = std::move(p);
  return GH_OK;
}

// ---- two-pass tile kernel setup (gh_mtile.hip) -------------------------------------
// Codes for it: complete, 1 <= len <= 16 (at most 128 codewords per segment), not taken
// by the single-pass tile kernel.  One LUT of width K (the wave split's write width; 11
// with a 1-bit codeword) with the codewords' start masks; one staging region per wave, sized for the stream's mean
// bytes per segment + 12 % and at least one chain's worst case (64 x 128 / minlen bytes: a larger
// piece is written and copied out chain by chain).  Returns GH_OK with the plan's mode
// left NONE when it does not fit a CU.
static uint32_t ws_write_bits(const Canon& cn);
static int mtile_setup(gh_ctx* c, double avg_seg_bytes) {
  const Canon& cn = c->canon;
  Plan p;
  TilePlan& t = p.tile;
  // codes with a 1-bit codeword: segments of up to 128 codewords, a chain's worst case
  // 8 KB, so 11-bit tables (24 KB with the count table) leave 16 regions of 8.5 KB
  const bool one = cn.minlen == 1;
  const uint32_t K = one ? std::min<uint32_t>(ws_write_bits(cn), 11) : ws_write_bits(cn);
  // codewords longer than the tables (up to 16 bits) take the canonical fallback, with
  // two lookups per window shift (2 x 12 + 16 > 32 otherwise)
  const bool fb = K < cn.maxlen;
  // (and windows that reach a 16-bit codeword's last bit: K = 12, or 11 in the kernels
  // for codes with a 1-bit codeword, gh_mtile.hip)
  if (fb && (K != (one ? 11u : 12u) || cn.maxlen > 16)) return GH_OK;
  const uint32_t maxsyms = (128 + cn.minlen - 1) / cn.minlen;  // <= 128
  double scapf = 1.12;
  if (const char* e = getenv("GH_TILE_SCAPF")) scapf = std::clamp(atof(e), 0.5, 4.0);
  uint64_t per_seg = std::min<uint64_t>(maxsyms, (uint64_t)std::ceil(std::max(avg_seg_bytes, 1.0) * scapf + 1));
  if (const char* e = getenv("GH_TILE_SCAP")) per_seg = std::min<uint64_t>(maxsyms, (uint64_t)std::max(1, atoi(e)));
  // at most what the LDS (LUT + 16 regions + slots) and the copy-out's 8 x 64 chunks hold
  // count table width: wider than the write table's (more codewords per lookup) where
  // the LDS and a window shift allow it (GL lookups of Kc bits within 31 bits)
  uint32_t Kc = K;
  if (GH_MT_CLUT && !one) {
    const int gl = lookups_per_shift(K);
    Kc = std::min<uint32_t>(13, 31 / gl);
    if (const char* e = getenv("GH_MT_KC")) Kc = (uint32_t)std::clamp(atoi(e), (int)K, (int)std::min(14, 31 / gl));
    Kc = std::max(Kc, K);
  }
  // the count table's copies (log2; GH_MT_CLGR, default 0): Kc + copies <= 14 keeps the
  // count e-window's S >= 16
  uint32_t clgr = 0;
  if (const char* e = getenv("GH_MT_CLGR")) clgr = (uint32_t)std::clamp(atoi(e), 0, 3);
  if (!GH_MT_CLUT || one) clgr = 0;
  clgr = std::min<uint32_t>(clgr, Kc + clgr > 14 ? 14 - Kc : clgr);
  const uint64_t lut_b = (GH_MT_CLUT ? (8ull << K) + (4ull << (Kc + clgr)) : 8ull << K)  // write table (+ count table)
                         + (fb ? (uint64_t)FB_BYTES : 0);                         // (+ fallback tables)
  const uint64_t lds_free = 160ull * 1024 - lut_b - mtile_lds_bytes(0, 0);
  // (the copy-out: 8 x 64 chunks, or 2 x 5 x 64 for codes with a 1-bit codeword)
  const uint64_t region_max = std::min<uint64_t>(lds_free / (MT_TB / 64), (one ? 10 : 8) * 1024 + STAGE_PAD) & ~15ull;
  per_seg = std::min<uint64_t>(per_seg, (region_max - STAGE_PAD - 16) / (64ull * MT_U));
  {  // six copy-out stores per lane (the 8-store kernel spills at lag 3) when the mean + 5 % fits
    const uint64_t ps6 = (6144 - 16) / (64ull * MT_U);
    if (per_seg > ps6 && (double)ps6 >= std::max(avg_seg_bytes, 1.0) * 1.05 + 1) per_seg = ps6;
  }
  const uint64_t cap = std::max<uint64_t>(64ull * MT_U * per_seg, 64ull * maxsyms);  // piece bytes staged at once
  if (STAGE_PAD + cap + 16 > region_max) return GH_OK;
  const int ns = cap + 16 <= 4096 ? 4 : cap + 16 <= 6144 ? 6 : cap + 16 <= 8192 ? 8 : 10;  // the copy-out's chunks cover a piece
  t.stage_bytes = (uint32_t)((STAGE_PAD + cap + 16 + 15) & ~15ull);  // + the write overrun
  p.kern = mtile_kernel_for(lookups_per_shift(K), ns, fb);
  p.block = MT_TB;
  t.lut_bytes = (uint32_t)lut_b;
  p.lds = mtile_lds_bytes(t.lut_bytes, t.stage_bytes);
  if (int rc = allow_lds(p.kern.fn, 160 * 1024)) return rc;
  int pc = 0;
  GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, p.kern.fn, MT_TB, p.lds));
  pc = std::min(pc, 2);  // (as tile_setup: the occupancy query can answer one too many)
  if (pc < 1) return GH_OK;
  t.kbits = K;
  t.kbits_c = Kc;
  t.clut_lgr = clgr;
  t.ntiles = (uint32_t)ceil_div(c->shard.nseg, (uint64_t)MT_U * MT_TB);
  if (int rc = tile_grid_and_granules(p, (uint64_t)pc * c->num_cu)) return rc;
  if (p.grid < 2) return GH_OK;
  // the tables as they lie in LDS: the write and count tables, the larger first
  // (gh_mtile.hip), then the canonical tables (the kernel reads the last FB_BYTES)
  std::vector<uint64_t> img(lut_b / 8, 0);
  const std::vector<uint64_t> lt = multi_lut(cn, K);
  const uint64_t wb = 8ull << K, cb = GH_MT_CLUT ? 4ull << (Kc + clgr) : 0;
  std::memcpy((uint8_t*)img.data() + (cb > wb ? cb : 0), lt.data(), wb);
  if (GH_MT_CLUT) {
    const std::vector<uint32_t> lc = start_count_lut(cn, Kc, clgr);
    std::memcpy((uint8_t*)img.data() + (cb > wb ? 0 : wb), lc.data(), cb);
  }
  if (fb) {
    uint32_t fbt[FB_WORDS];
    fallback_tables(cn, fbt);
    std::memcpy((uint8_t*)img.data() + lut_b - FB_BYTES, fbt, sizeof(fbt));
  }
  if (int rc = t.lut.upload(img.data(), lut_b)) return rc;
  p.shape = p.kern.name;
  p.mode = Mode::MTILE;
  c->plan = std::move(p);
  return GH_OK;
}

// ---- wave split setup ------------------------------------------------------------
// Count-LUT width Kc in [max(maxlen, 2), 13] maximising bits per VALU op of a lookup
// group: GL lookups of ~6 ops each plus ~8 ops of window shift and end upkeep per chain
// (r=0.9: Kc=13, 10.6 vs 8.5 bits per lookup at 11; r=0.5: Kc=12, 10.3 vs 7.1 at 9-10).
// Longer codes: the fallback.  GH_WS_KC overrides (tests).
static uint32_t ws_count_bits(const Canon& cn) {
  const uint32_t lo = std::min<uint32_t>(std::max<uint32_t>(cn.maxlen, 2), 13);
  if (const char* e = getenv("GH_WS_KC")) return (uint32_t)std::clamp(atoi(e), (int)lo, 14);
  uint32_t best = lo;
  double best_eff = -1;
  for (uint32_t kc = lo; kc <= 13; ++kc) {  // 14 (64 KiB) measured no faster
    const int gl = lookups_per_shift(kc);
    const double eff = gl * count_lut(cn, kc, nullptr) / (6.0 * gl + 8.0);
    if (eff > best_eff * 1.01) {  // prefer the smaller table unless clearly better
      best_eff = eff;
      best = kc;
    }
  }
  return best;
}
// Write-LUT width K in [max(maxlen, 10), 12] maximising the expected bits per lookup
// (entries hold up to four codewords, so a wider window helps only codes whose short
// codewords it can fit more of: r=0.5 codes 7.6 -> 10.4 bits at K 10 -> 12) times
// lookups per window shift over ~13 ops per lookup plus ~12 per shift; a wider table
// must win by 5 % (its LDS costs occupancy).  GH_WS_K overrides (tests).
static uint32_t ws_write_bits(const Canon& cn) {
  if (const char* ek = getenv("GH_WS_K"))  // (a width below maxlen takes the canonical fallback)
    return (uint32_t)std::clamp(atoi(ek), 2, 12);
  const uint32_t lo = std::min<uint32_t>(std::max<uint32_t>(cn.maxlen, 10), 12);
  uint32_t best = lo;
  double best_eff = -1;
  for (uint32_t K = lo; K <= 12; ++K) {
    double sum = 0;
    for (uint32_t i = 0; i < (1u << K); ++i) sum += window_codewords(cn, i, K, 4, nullptr, nullptr, nullptr);
    const int gl = lookups_per_shift(K);
    const double eff = gl * (sum / (double)(1u << K)) / (13.0 * gl + 12.0);
    if (best_eff < 0 || eff > best_eff * 1.05) {
      best_eff = eff;
      best = K;
    }
  }
  return best;
}
#ifndef GH_WS_CLUT_MAX
#define GH_WS_CLUT_MAX 0  // count-LUT bytes in LDS with its copies (0: one copy; round 5: copies at Kc 10-12
                          // measured no faster on cfg3 than one copy at Kc 13, gpurun_out/r05am)
#endif
constexpr uint64_t WS_CLUT_MAX = GH_WS_CLUT_MAX;
static int ws_ns_for(double avg_seg_bytes) {
  const double chunks = avg_seg_bytes * 64 * WS_U / 16.0 * 1.15 + 2;
  const int ns = (int)std::ceil(chunks / 64);
  return ns <= 2 ? 2 : ns <= 3 ? 3 : ns <= 4 ? 4 : ns <= 6 ? 6 : 8;
}

// A count table of width kc and the canonical fallback tables, built and uploaded: for the
// wave split's count pass, the index build and the gather.
static int upload_count_tables(const Canon& cn, uint32_t kc, DevBuf& lut_c, DevBuf& fb) {
  std::vector<uint32_t> lc;
  count_lut(cn, kc, &lc);
  uint32_t fbt[FB_WORDS];
  fallback_tables(cn, fbt);
  if (int rc = lut_c.upload(lc.data(), 4ull << kc)) return rc;
  return fb.upload(fbt, sizeof(fbt));
}

static int ws_setup(gh_ctx* c, double avg_seg_bytes) {
  const Canon& cn = c->canon;
  const uint64_t nseg = c->shard.nseg;
  Plan p;
  WsPlan& w = p.ws;
  const uint32_t K = ws_write_bits(cn), kc = ws_count_bits(cn);
  // canonical fallback: codewords longer than a table, or patterns outside an incomplete
  // code (a LUT entry with no codeword)
  const bool fb = kraft16(cn) != 65536 || cn.maxlen > std::min(K, kc);
  w.k = K;
  w.kc = kc;
  if (int rc = w.lut_w.upload(write_lut(cn, K).data(), 8ull << K)) return rc;
  if (int rc = upload_count_tables(cn, kc, w.lut_c, w.fb)) return rc;
  w.lut_bytes = 8u << K;  // >= 32 bytes: whole 16-byte chunks
  const size_t lb = w.lut_bytes + (fb ? (size_t)FB_BYTES : 0);  // write kernel: LUT + fallback tables
  constexpr int NW = WS_TB / 64;
  // codewords per segment: wholly inside [start, E), E - start <= 143
  const uint32_t maxsyms = std::min<uint32_t>(143 / std::max<uint32_t>(cn.minlen, 1) + 1, 255);
  // per-wave staging: at least one chain's worst case (64 segments x maxsyms), and a
  // typical whole block (both chains) with room to spare when the LDS allows
  const size_t chain_worst = 64ull * maxsyms + 64;
  const size_t full_worst = 64ull * WS_U * maxsyms + 64;
  const size_t typical = (size_t)(1.3 * avg_seg_bytes * 64 * WS_U) + 64;
  const size_t want = std::max(chain_worst, std::min(full_worst, typical));
  size_t stage = 0;
  for (int wg = 8; wg >= 1 && stage == 0; --wg) {
    const long avail = ((long)(163840 / wg) - (long)lb) / NW;
    if (avail >= (long)want) stage = std::min<size_t>((size_t)avail, full_worst + 15) & ~15ull;
  }
  if (stage == 0) {
    const long avail = ((long)163840 - (long)lb) / NW;
    if (avail < (long)chain_worst) return fail(GH_E_HIP, "wave-split staging does not fit");
    stage = (size_t)avail & ~15ull;
  }
  if (const char* es = getenv("GH_WS_STAGE"))  // tests: force a small staging (per-chain blocks)
    stage = std::max<size_t>((size_t)atoll(es), (chain_worst + 15) & ~15ull) & ~15ull;
  w.stage_bytes = (uint32_t)stage;
  p.lds = lb + NW * stage;
  // count LUT copies (lane l reads copy l mod 2^lgc: fewer bank conflicts on the skewed
  // lookups), up to 32 KB in LDS; GH_WS_LGC overrides (tests, experiments)
  if (!fb) {
    uint32_t lgc = 0;
    while (lgc < 5 && (4ull << (kc + lgc + 1)) <= (uint64_t)WS_CLUT_MAX && 30u - kc - (lgc + 1) >= 16u) ++lgc;
    if (const char* e = getenv("GH_WS_LGC")) lgc = (uint32_t)std::clamp(atoi(e), 0, std::max(0, 14 - (int)kc));
    w.lgc = lgc;
  }
  w.lds_count = std::max<size_t>(4ull << (kc + w.lgc), 64) + (fb ? FB_BYTES : 0);
  int ns = ws_ns_for(avg_seg_bytes);
  if (const char* en = getenv("GH_WS_NS")) ns = std::clamp(atoi(en), 2, 8);
  const WsKernels k = ws_kernels(kc, K, ns, fb);
  w.count = k.count;
  p.kern = k.write;
  p.block = WS_TB;
  if (int rc = allow_lds(w.count.fn, w.lds_count)) return rc;
  if (int rc = allow_lds(p.kern.fn, p.lds)) return rc;
  int pc_c = 0, pc_w = 0;
  GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc_c, w.count.fn, WS_TBC, w.lds_count));
  GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc_w, p.kern.fn, WS_TB, p.lds));
  if (pc_c < 1 || pc_w < 1) return fail(GH_E_HIP, "wave-split kernels do not fit on a CU");
  w.nblocks = (uint32_t)ceil_div(nseg, (uint64_t)WS_SB);  // superblocks
  const uint64_t wg_blocks = ceil_div(w.nblocks, (uint64_t)NW);  // workgroups that have a superblock
  p.grid = (uint32_t)std::min<uint64_t>((uint64_t)pc_w * c->num_cu, wg_blocks);
  w.grid_c = (uint32_t)std::min<uint64_t>((uint64_t)pc_c * c->num_cu, ceil_div(w.nblocks, (uint64_t)(WS_TBC / 64)));
  if (const char* eg = getenv("GH_WS_GRID")) {  // tests: few workgroups, many blocks per wave
    p.grid = (uint32_t)std::clamp<long>(atol(eg), 1, (long)p.grid);
    w.grid_c = (uint32_t)std::clamp<long>(atol(eg), 1, (long)w.grid_c);
  }
  w.nranges = p.grid * (uint32_t)NW;  // one contiguous range per wave of the write grid
  if (int rc = w.seg_cnt.alloc(nseg + WS_CNT_PAD + 16)) return rc;
  if (int rc = w.junk.alloc(16ull * 64 * w.nranges)) return rc;
  if (int rc = w.rng_tot.alloc(8ull * w.nranges + 16)) return rc;
  if (int rc = w.rng_off.alloc(8ull * w.nranges + 16)) return rc;
  p.shape = std::string(w.count.name) + "+" + p.kern.name;
  p.mode = Mode::WSPLIT;
  c->plan = std::move(p);
  return GH_OK;
}

// End bit of the stream's last segment (segment-relative) under the reference rule
// "codewords starting before bit 128" (decoder.cu:529-569), its zero padding
// decoded like the reference's: the end of the last codeword starting before 128.
static uint32_t last_segment_end(const Canon& cn, const uint32_t* w5, uint32_t start) {
  uint32_t pos = start;
  while (pos < 128) {
    const uint32_t wi = pos >> 5, sh = pos & 31;
    const uint32_t hi = w5[wi], lo = wi + 1 < 5 ? w5[wi + 1] : 0u;
    const uint32_t w32 = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
    uint32_t fi = 0;
    const uint32_t l = canon_decode16(cn, w32 >> 16, &fi);
    if (l == 0) break;
    pos += l;
  }
  return std::max<uint32_t>(pos, 128);
}

// Gap nibble `nib` of gap words in host memory (any alignment): 8 per u32, lowest first.
static uint32_t gap_nibble(const void* words, uint64_t nib) {
  uint32_t wv;
  std::memcpy(&wv, (const uint8_t*)words + 4 * (nib >> 3), 4);
  return (wv >> (4 * (nib & 7))) & 15u;
}

extern "C" int gh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int gh_ctx_create(int device, gh_ctx** out) {
  if (!out) return fail(GH_E_ARG, "null ctx pointer");
  *out = nullptr;
  int num_cu = 0;
  if (int rc = open_device(device, "no HIP device visible (the decoder has no CPU fallback)", &num_cu)) return rc;
  std::unique_ptr<gh_ctx> c(new gh_ctx());  // (a failure below frees what was made)
  c->device = device;
  c->num_cu = num_cu;
  if (int rc = c->stream.create()) return rc;
  if (int rc = c->done.create(hipEventDisableTiming)) return rc;
  if (int rc = c->misc.alloc(128, true)) return rc;
  *out = c.release();
  return GH_OK;
}

extern "C" int gh_ctx_kernel_shape(gh_ctx* c, char* buf, size_t cap) {
  if (!c) return fail(GH_E_ARG, "null ctx");
  if (!c->loaded) return fail(GH_E_STATE, "gh_ctx_kernel_shape before gh_ctx_load");
  return copy_name(c->plan.shape, buf, cap);
}

extern "C" int gh_ctx_offsets_state(gh_ctx* c, int* state) {
  if (!c || !state) return fail(GH_E_ARG, "null argument");
  *state = (c->loaded && c->plan.mode == Mode::TILE) ? c->plan.tile.offs_state : GH_OFFS_NONE;
  return GH_OK;
}

extern "C" int gh_kernel_shapes(char* buf, size_t cap) { return copy_name(all_kernel_shapes(), buf, cap); }

extern "C" int gh_ctx_device(gh_ctx* c, int* device) {
  if (!c || !device) return fail(GH_E_ARG, "null argument");
  *device = c->device;
  return GH_OK;
}

// The tile kernel's workgroups wait on each other (round prefixes): it assumes that the
// whole grid becomes resident.  Two of them running at once on one device (several shard
// contexts on one GPU, each on its own stream) can each hold half the CUs and wait
// forever for the rest (their bounded spins then report GH_ST_TIMEOUT).  So launches
// of such kernels on one device are chained: each waits for the previous one's
// completion event, whatever stream either was launched on.
struct DevChain {
  std::mutex mu;
  hipEvent_t last = nullptr;          // the last tile decode's done_ev, or the end event of a
                                      // device-planned gather (owned by `owner`)
  const gh_ctx* owner = nullptr;
  bool has = false;
  hipStream_t last_stream = nullptr;  // the stream the last tile kernel ran on
};
static DevChain& dev_chain(int device) {
  static std::mutex mu;
  static std::map<int, DevChain*> m;
  std::lock_guard<std::mutex> g(mu);
  DevChain*& d = m[device];
  if (!d) d = new DevChain();  // one per device, for the life of the process
  return *d;
}

gh_ctx::~gh_ctx() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  if (done_rec) (void)hipEventSynchronize(done_ev);
  if (dgather.enqueued) (void)hipEventSynchronize(dgather.ev_c);  // (it may run on a caller's stream)
  // the device chain must not keep one of this context's events
  DevChain& dc = dev_chain(device);
  std::lock_guard<std::mutex> g(dc.mu);
  if (dc.owner == this) {
    dc.has = false;
    dc.owner = nullptr;
    dc.last = nullptr;
  }
}  // (then the parts free their memory and events, the stream last)

extern "C" int gh_ctx_destroy(gh_ctx* c) {
  delete c;
  return GH_OK;
}

// Drops the loaded shard, then plans the decode of segments [b, e) of s: the code, the
// output buffer and the decode structure with its tables.
static int plan_shard(gh_ctx* c, const gh_stream* s, uint64_t b, uint64_t e, uint64_t out_cap) {
  if (b > e || e > s->g) return fail(GH_E_ARG, "shard range outside [0, G]");
  if (e - b >= (1ull << 31))  // 32-bit segment indices in the kernels: 32 GiB of payload per shard
    return fail(GH_E_ARG, "shard of 2^31 or more segments: split the stream into more shards");
  free_shard(c);
  int rc = build_canon(s->syms, s->nsyms, c->canon);
  if (rc) return rc;
  const Canon& cn = c->canon;
  Shard& sh = c->shard;
  sh.nseg = e - b;
  sh.seg_begin = b;
  sh.seg_end = e;
  sh.n_total = s->n;
  sh.g_total = s->g;
  if (sh.nseg > 0 && cn.nsyms == 0) return fail(GH_E_TABLE, "empty code");
  const uint64_t per_seg = cn.minlen ? (128 + cn.minlen - 1) / cn.minlen : 128;  // codewords per segment, at most
  if (out_cap == 0) out_cap = std::min<uint64_t>(s->n, sh.nseg * per_seg);
  sh.out_cap = out_cap;
  GH_HIP(hipSetDevice(c->device));
  if ((rc = sh.out.alloc(std::max<uint64_t>(out_cap, 16) + 64))) return rc;
  GH_HIP(hipMemset(c->misc.get(), 0, 128));
  if (sh.nseg == 0) return GH_OK;
  // Structure: the tile kernel for grouped codes, the wave split for every other code.
  // GH_MODE=tile|wsplit forces one; GH_LUT_BITS sets the tile kernel's LUT width (a
  // width below maxlen leaves the code to the wave split).
  const char* envm = getenv("GH_MODE");
  const bool force_tile = envm && !strcmp(envm, "tile"), force_ws = envm && !strcmp(envm, "wsplit");
  const bool force_mt = envm && !strcmp(envm, "mtile");
  if (envm && *envm && !force_tile && !force_ws && !force_mt) return fail(GH_E_ARG, "GH_MODE: tile, mtile or wsplit");
  const char* envk = getenv("GH_LUT_BITS");
  const uint32_t K = envk ? (uint32_t)std::clamp(atoi(envk), 1, 12) : cn.maxlen;
  const bool grouped = (grouped_code(cn) || short_code(cn)) && K >= cn.maxlen;
  if (force_tile && !grouped)
    return fail(GH_E_ARG, "GH_MODE=tile: the code is not for the tile kernel (complete, 3..12 bits)");
  const double avg = s->g ? (double)s->n / (double)s->g : 16.0;
  const Mode& mode = c->plan.mode;
  if (grouped && !force_ws && !force_mt) {
    if ((rc = tile_setup(c, K, avg))) return rc;
    if (force_tile && mode == Mode::NONE) return fail(GH_E_HIP, "GH_MODE=tile: the tile kernel does not fit a CU");
  }
  // the two-pass tile kernel: codes of 2..12-bit codewords the single-pass one does not
  // take (cfg3's r = 0.9 codes; GH_MTILE=0 leaves them to the wave split, GH_MODE=mtile
  // forces it)
  const bool multi = cn.maxlen <= 16 && kraft16(cn) == 65536;
  if (force_mt && !multi)
    return fail(GH_E_ARG, "GH_MODE=mtile: the code is not for the two-pass tile kernel (complete, 1..16 bits)");
  static const bool mt_on = [] {
    const char* e = getenv("GH_MTILE");
    return !(e && e[0] == '0');
  }();
  if (mode == Mode::NONE && multi && (force_mt || (mt_on && !force_ws && !force_tile))) {
    if ((rc = mtile_setup(c, avg))) return rc;
    if (force_mt && mode == Mode::NONE) return fail(GH_E_HIP, "GH_MODE=mtile: the two-pass tile kernel does not fit a CU");
  }
  if (mode == Mode::NONE) return ws_setup(c, avg);
  return GH_OK;
}

// Where a load reads the stream's words from: host memory (gh_ctx_load) or device memory
// (gh_ctx_load_device).
struct ShardSource {
  bool device;
  const void* payload;  // payload words, the shard's first at word `skip`
  uint64_t skip, words;
  const void* gaps;     // the stream's whole gap array
};

// End of the last loaded segment (nseg > 0) by the decode's rule (last_segment_end): its
// words and its start bit from the context's device copies.
static int loaded_last_end(gh_ctx* c, uint32_t* out) {
  const Shard& sh = c->shard;
  uint32_t w5[5] = {};
  GH_HIP(hipMemcpy(w5, sh.payload.get<uint32_t>() + 4 * (sh.nseg - 1), sizeof(w5), hipMemcpyDeviceToHost));  // (16 padding words follow)
  uint32_t st = sh.first_start;
  if (sh.nseg > 1) {
    const uint64_t nib = sh.gap_nib0 + sh.nseg - 2;
    uint32_t wv = 0;
    GH_HIP(hipMemcpy(&wv, sh.gaps.get<uint32_t>() + (nib >> 3), 4, hipMemcpyDeviceToHost));
    st = gap_nibble(&wv, nib & 7);
  }
  *out = last_segment_end(c->canon, w5, st);
  return GH_OK;
}

static int load_shard(gh_ctx* c, const gh_stream* s, uint64_t b, uint64_t e, uint64_t out_cap,
                      const ShardSource& src) {
  if (int rc = plan_shard(c, s, b, e, out_cap)) return rc;
  Shard& sh = c->shard;
  if (sh.nseg == 0) {
    c->loaded = true;
    return GH_OK;
  }
  const hipMemcpyKind kind = src.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // payload words [4b, 4e+1) (clipped at what the source holds) + zero padding
  const uint64_t have = std::min<uint64_t>(4 * sh.nseg + 1, src.skip < src.words ? src.words - src.skip : 0);
  const uint8_t* from = (const uint8_t*)src.payload + 4 * src.skip;
  const uint64_t alloc_words = 4 * sh.nseg + 16;
  if (int rc = sh.payload.alloc(4 * alloc_words)) return rc;
  // zero only the padding past the copied words: the copies below may run on the
  // staging set's non-blocking stream, which is not ordered against this memset
  GH_HIP(hipMemset(sh.payload.get<uint32_t>() + have, 0, 4 * (alloc_words - have)));
  if (have) {
    if (!src.device && use_staged(4 * have)) {  // pinned double-buffered (concurrent across shards' threads)
      if (int rc = h2d_staged(c->device, from, 4 * have, sh.payload.get())) return rc;
    } else {
      GH_HIP(hipMemcpy(sh.payload.get(), from, 4 * have, kind));
    }
  }
  // gap nibbles: starts of local segments 1..nseg-1 and ends of all: global [b-1, e)
  const uint64_t gw0 = b >> 3;
  const uint64_t gw1 = (e >= 1) ? ((e - 1) >> 3) + 1 : gw0 + 1;
  const uint64_t gwords = std::max<uint64_t>(gw1, gw0 + 1) - gw0;
  const uint64_t total_gw = ceil_div(s->g, GH_GAPS_PER_WORD);
  const uint64_t gcopy = (gw0 < total_gw) ? std::min<uint64_t>(gwords, total_gw - gw0) : 0;
  if (int rc = sh.gaps.alloc(4 * (gwords + 4), true)) return rc;
  if (gcopy) GH_HIP(hipMemcpy(sh.gaps.get(), (const uint8_t*)src.gaps + 4 * gw0, 4 * gcopy, kind));
  sh.gap_nib0 = (uint32_t)(b - 8 * gw0);
  // start bit of local segment 0: nibble b - 1, which the context's copy need not hold
  if (b > 0 && src.gaps) {
    if (src.device) {
      uint32_t wv = 0;
      GH_HIP(hipMemcpy(&wv, (const uint8_t*)src.gaps + 4 * ((b - 1) >> 3), 4, hipMemcpyDeviceToHost));
      sh.first_start = gap_nibble(&wv, (b - 1) & 7);
    } else {
      sh.first_start = gap_nibble(src.gaps, b - 1);
    }
  }
  if (c->plan.mode == Mode::WSPLIT && e == s->g)
    if (int rc = loaded_last_end(c, &sh.last_end)) return rc;
  c->loaded = true;
  return GH_OK;
}

extern "C" int gh_ctx_load(gh_ctx* c, const gh_stream* s, uint64_t b, uint64_t e,
                           uint64_t out_cap) {
  if (!c || !s) return fail(GH_E_ARG, "null argument");
  return load_shard(c, s, b, e, out_cap, {false, s->payload, 4 * b, s->w, s->gap_words});
}

extern "C" int gh_ctx_load_device(gh_ctx* c, const gh_stream* s, uint64_t b, uint64_t e,
                                  const uint32_t* d_payload, uint64_t d_words,
                                  const uint32_t* d_gap_words, uint64_t out_cap) {
  if (!d_payload || !d_gap_words) return fail(GH_E_ARG, "null device buffer");
  if (!c || !s) return fail(GH_E_ARG, "null argument");
  return load_shard(c, s, b, e, out_cap, {true, d_payload, 0, d_words, d_gap_words});
}

// The WsParams fields that every user of the resident shard fills alike (the wave split's
// decode, the index build, the gather); each adds its own tables, outputs and status word.
static WsParams shard_params(const gh_ctx* c) {
  const Shard& sh = c->shard;
  WsParams m{};
  m.payload = sh.payload.get<uint32_t>();
  m.gaps = sh.gaps.get<uint32_t>();
  m.nseg = (uint32_t)sh.nseg;
  m.gap_nib0 = sh.gap_nib0;
  m.first_start = sh.first_start;
  m.fb_lo = std::max<uint32_t>(c->canon.minlen, 1);
  m.fb_hi = std::max<uint32_t>(c->canon.maxlen, m.fb_lo);
  m.chk_pay = 4 * sh.nseg + 16;
  m.chk_gap = sh.nseg / 8 + 4;  // (at least; the allocation holds gwords + 4)
  return m;
}

extern "C" int gh_ctx_decode(gh_ctx* c, void* hip_stream, int timed) {
  if (!c) return fail(GH_E_ARG, "null ctx");
  if (!c->loaded) return fail(GH_E_STATE, "gh_ctx_decode before gh_ctx_load");
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)c->stream;
  GH_HIP(hipSetDevice(c->device));
  const Shard& sh = c->shard;
  Plan& p = c->plan;
  if (sh.nseg == 0) {
    GH_HIP(hipMemsetAsync(c->misc_at(2), 0, 8, st));
    GH_HIP(hipEventRecord(c->done, st));
    c->done_ev = c->done;
    c->done_rec = true;
    return GH_OK;
  }
  // Tile kernels are chained per device: wait for the previous one before the start
  // event, so a decode's time excludes its queueing behind other contexts' decodes.
  const bool tiled = p.tiled();
  DevChain& dc = dev_chain(c->device);
  std::unique_lock<std::mutex> chain_lock(dc.mu, std::defer_lock);
  if (tiled) {
    if (++p.tile.epoch >= EPOCH_MAX) {  // granule epochs wrap: start clean
      GH_HIP(hipMemsetAsync(p.tile.gran.get(), 0, 8ull * p.tile.gran_words, st));
      p.tile.epoch = 1;
    }
    chain_lock.lock();
    // (the context's own stream, which the last tile decode of the device ran on for this
    // same context, is ordered behind it already: no wait packet.  A caller's stream is
    // never trusted that way: it may have been destroyed and its handle reused since.)
    const bool ordered = dc.owner == c && dc.last_stream == st && st == c->stream;
    if (dc.has && !ordered) GH_HIP(hipStreamWaitEvent(st, dc.last, 0));
  }
  EventPair ev;
  if (timed) {
    if (!c->timing.pool.empty()) {
      ev = std::move(c->timing.pool.back());
      c->timing.pool.pop_back();
    } else if (int rc = ev.create()) {
      return rc;
    }
    if (!tiled) GH_HIP(hipEventRecord(ev.a, st));  // (tile: in the dispatch itself, below)
  }
  if (p.mode == Mode::WSPLIT) {
    const WsPlan& w = p.ws;
    WsParams m = shard_params(c);
    m.seg_cnt = w.seg_cnt.get<uint8_t>();
    m.rng_tot = w.rng_tot.get<unsigned long long>();
    m.rng_off = w.rng_off.get<unsigned long long>();
    m.out = sh.out.get<uint8_t>();
    m.junk = w.junk.get<uint4>();
    m.status = c->misc_at(1);
    m.total = (unsigned long long*)c->misc_at(2);
    m.out_cap = sh.out_cap;
    m.nsb = w.nblocks;
    m.nranges = w.nranges;
    m.chk_out = std::max<uint64_t>(sh.out_cap, 16) + 64;
    m.stage_bytes = w.stage_bytes;
    m.last_end = sh.last_end;
    m.fb = w.fb.get<uint32_t>();
    WsParams wc = m, ww = m;  // the count and scan kernels' / the write kernel's
    wc.lut = w.lut_c.get<uint2>();
    wc.kbits = w.kc;
    wc.lut_bytes = (uint32_t)(4u << w.kc);
    wc.lgc = w.lgc;
    ww.lut = w.lut_w.get<uint2>();
    ww.kbits = w.k;
    ww.lut_bytes = w.lut_bytes;
    void* ac[1] = {&wc};
    void* aw[1] = {&ww};
    GH_HIP(hipLaunchKernel(w.count.fn, dim3(w.grid_c), dim3(WS_TBC), ac, w.lds_count, st));
    GH_HIP(hipLaunchKernel((const void*)gh_ws_scan_kernel, dim3(1), dim3(WS_SCAN_TB), ac, 0, st));
    GH_HIP(hipLaunchKernel(p.kern.fn, dim3(p.grid), dim3(p.block), aw, p.lds, st));
  } else {
    TilePlan& tp = p.tile;
    // known piece offsets: the table of this load is READY -> the known-offsets
    // instantiation; otherwise the chained kernel, which records the table
    const bool known = p.mode == Mode::TILE && tp.offs_on && tp.offs_state == GH_OFFS_READY;
    if (p.mode == Mode::TILE && tp.offs_on && tp.offs_state == GH_OFFS_NONE) tp.offs_state = GH_OFFS_RECORDED;
    const void* fn = known ? p.kern.fn_known : p.kern.fn;
    const size_t lds = known ? tp.lds_known : p.lds;
    unsigned long long* gran = tp.gran.get<unsigned long long>();
    TileParams t{};
    t.payload = sh.payload.get<uint32_t>();
    t.gaps = sh.gaps.get<uint32_t>();
    t.lut = tp.lut.get<uint32_t>();
    t.out = sh.out.get<uint8_t>();
    t.granules = gran;
    t.prefix = gran + tp.ntiles;
    t.status = c->misc_at(1);
    t.total = (unsigned long long*)c->misc_at(2);
    t.stats = (unsigned long long*)c->misc_at(4);
    t.piece_off = tp.piece_off.get<unsigned long long>();
    t.out_cap = sh.out_cap;
    t.nseg = sh.nseg;
    t.gap_nib0 = sh.gap_nib0;
    t.first_start = sh.first_start;
    t.ntiles = tp.ntiles;
    t.kbits = tp.kbits;
    t.lgr = p.mode == Mode::MTILE ? tp.clut_lgr : tp.lut_lgr;
    t.epoch = tp.epoch;
    t.lut_bytes = tp.lut_bytes;
    t.stage_bytes = tp.stage_bytes;
    t.kbits_c = tp.kbits_c;
    t.fb_hi = c->canon.maxlen;
    t.stamps = tp.stamps.get<uint4>();
    t.tstamps = tp.stamps ? (unsigned long long*)(tp.stamps.get<uint8_t>() + 32ull * p.grid * 2 * 128) : nullptr;
    t.idle_block = tp.idle_block;
    if (known) {
      t.lgr = tp.lgr_known;
      t.lut_bytes = (uint32_t)(4ull << (tp.kbits + tp.lgr_known));
    }
    void* ta[1] = {&t};
    // timed: the start and stop timestamps are taken by the dispatch packet itself
    // (hipExtLaunchKernel), not by marker packets around it, so back-to-back decodes
    // have no extra packets between them
    if (timed)
      GH_HIP(hipExtLaunchKernel(fn, dim3(p.grid), dim3(p.block), ta, lds, st, ev.a, ev.b, 0));
    else
      GH_HIP(hipLaunchKernel(fn, dim3(p.grid), dim3(p.block), ta, lds, st));
  }
  GH_HIP(hipGetLastError());
  // one event after the kernel(s): the timed decode's end event, or `done` (each marker
  // between back-to-back decodes costs the GPU microseconds)
  if (timed) {
    if (!tiled) GH_HIP(hipEventRecord(ev.b, st));
    c->done_ev = ev.b;
    c->timing.pending.push_back(std::move(ev));
  } else {
    GH_HIP(hipEventRecord(c->done, st));
    c->done_ev = c->done;
  }
  c->done_rec = true;
  if (tiled) {  // the device chain's last decode (chain_lock held)
    dc.last = c->done_ev;
    dc.owner = c;
    dc.has = true;
    dc.last_stream = st;
  }
  return GH_OK;
}

// Waits for the context's last decode, whatever stream it was launched on.
// Known piece offsets: every decode of the context has finished (wait_decode).  A table
// that was being RECORDED is READY if the decodes left status 0, else dropped; the one
// status read per load that this costs happens only in that state.
static int offsets_settle(gh_ctx* c, const unsigned int* status_seen = nullptr) {
  TilePlan& tp = c->plan.tile;
  if (c->plan.mode != Mode::TILE || tp.offs_state == GH_OFFS_NONE) return GH_OK;
  unsigned int status = 0;
  if (status_seen) {
    status = *status_seen;
  } else {
    if (tp.offs_state != GH_OFFS_RECORDED) return GH_OK;
    GH_HIP(hipMemcpy(&status, c->misc_at(1), 4, hipMemcpyDeviceToHost));
  }
  tp.offs_state = status ? GH_OFFS_NONE : GH_OFFS_READY;
  return GH_OK;
}

static int wait_decode(gh_ctx* c) {
  GH_HIP(hipStreamSynchronize(c->stream));
  if (c->done_rec) GH_HIP(hipEventSynchronize(c->done_ev));
  return offsets_settle(c);
}

extern "C" int gh_ctx_report(gh_ctx* c, void* hip_stream, gh_report* rep) {
  if (!c) return fail(GH_E_ARG, "null ctx");
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)c->stream;
  GH_HIP(hipSetDevice(c->device));
  GH_HIP(hipStreamSynchronize(st));
  if (int rc = wait_decode(c)) return rc;
  Timing& tm = c->timing;
  for (EventPair& e : tm.pending) {
    float ms = 0;
    if (int rc = e.elapsed(&ms)) return rc;
    tm.acc_ms += ms;
    tm.nlaunch++;
    tm.pool.push_back(std::move(e));
  }
  tm.pending.clear();
  const Plan& p = c->plan;
  if (GH_TILE_STAMPS && p.tile.stamps) {  // diagnostic builds: the last decode's phase deltas
    if (const char* f = getenv("GH_STAMPS_OUT")) {
      std::vector<uint8_t> h(p.tile.stamps.capacity());
      GH_HIP(hipMemcpy(h.data(), p.tile.stamps.get(), h.size(), hipMemcpyDeviceToHost));
      if (FILE* fp = fopen(f, "wb")) {
        fwrite(h.data(), 1, h.size(), fp);
        fclose(fp);
      }
    }
  }
  unsigned int misc[6] = {};
  GH_HIP(hipMemcpy(misc, c->misc.get(), sizeof(misc), hipMemcpyDeviceToHost));
  // a decode that reports a status (GH_ST_OFFSETS: a piece disagreed with the table; any
  // other) drops the piece offsets: the next decode is chained again
  if (int rc = offsets_settle(c, &misc[1])) return rc;
  if (rep) {
    std::memset(rep, 0, sizeof(*rep));
    uint64_t tot;
    std::memcpy(&tot, misc + 2, 8);
    rep->symbols = tot;
    rep->out_bytes = std::min<uint64_t>(tot, c->shard.out_cap);
    rep->status = misc[1];
    rep->lut_bits = p.tiled() ? p.tile.kbits : p.ws.k;
    rep->grid = p.grid;
    rep->tiles = p.tiled() ? p.tile.ntiles : p.ws.nblocks;  // tiles / wave blocks
    rep->mode = p.mode == Mode::MTILE ? GH_MODE_MTILE : p.mode == Mode::TILE ? GH_MODE_TILE : GH_MODE_SPLIT;
    std::memcpy(&rep->slow_lookbacks, misc + 4, 8);
    rep->path = p.mode == Mode::MTILE ? GH_PATH_MULTI_TILE : p.mode == Mode::TILE ? GH_PATH_GROUPED : GH_PATH_MULTI_WAVE;
    rep->launches = tm.nlaunch;
    rep->kernel_ms = tm.nlaunch ? (float)(tm.acc_ms / tm.nlaunch) : 0.f;
  }
  return GH_OK;
}

extern "C" int gh_ctx_reset_timing(gh_ctx* c) {
  if (!c) return fail(GH_E_ARG, "null ctx");
  c->timing.acc_ms = 0;
  c->timing.nlaunch = 0;
  return GH_OK;
}

extern "C" int gh_ctx_download(gh_ctx* c, uint64_t off, uint8_t* dst, uint64_t nbytes) {
  if (!c || (nbytes && !dst)) return fail(GH_E_ARG, "null argument");
  if (off + nbytes > c->shard.out_cap) return fail(GH_E_ARG, "download beyond the output capacity");
  if (!nbytes) return GH_OK;
  GH_HIP(hipSetDevice(c->device));
  if (int rc = wait_decode(c)) return rc;
  const uint8_t* src = c->shard.out.get<uint8_t>() + off;
  if (use_staged(nbytes)) return d2h_staged(c->device, src, nbytes, dst);
  GH_HIP(hipMemcpy(dst, src, nbytes, hipMemcpyDeviceToHost));
  return GH_OK;
}

extern "C" int gh_ctx_output(gh_ctx* c, void** d_out, uint64_t* cap) {
  if (!c || !d_out) return fail(GH_E_ARG, "null argument");
  *d_out = c->shard.out.get();
  if (cap) *cap = c->shard.out_cap;
  return GH_OK;
}

extern "C" int gh_ctx_copy_output(gh_ctx* c, uint64_t off, void* dst, uint64_t nbytes,
                                  void* hip_stream) {
  if (!c || (nbytes && !dst)) return fail(GH_E_ARG, "null argument");
  if (off + nbytes > c->shard.out_cap) return fail(GH_E_ARG, "copy beyond the output capacity");
  if (!nbytes) return GH_OK;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)c->stream;
  GH_HIP(hipSetDevice(c->device));
  if (c->done_rec) GH_HIP(hipStreamWaitEvent(st, c->done_ev, 0));  // after the last decode
  GH_HIP(hipMemcpyAsync(dst, c->shard.out.get<uint8_t>() + off, nbytes, hipMemcpyDefault, st));
  return GH_OK;
}

// ---- seek index (gh_index.hip) ------------------------------------------------------
// The index and gather kernels are not decode shapes: no load picks them, gh_kernel_shapes
// does not list them.  Both go by their count table's width and the fallback.
extern "C" int gh_ctx_build_index(gh_ctx* c, uint32_t log2_stride, void* out, uint64_t out_len,
                                  uint64_t* symbols, float* kernel_ms) {
  if (!c || !out) return fail(GH_E_ARG, "null argument");
  if (!c->loaded) return fail(GH_E_STATE, "gh_ctx_build_index before gh_ctx_load");
  const Shard& sh = c->shard;
  const uint64_t bytes = gh_index_bytes(sh.g_total, log2_stride);
  if (bytes == 0) return fail(GH_E_ARG, "index stride outside 2^8 .. 2^20 segments");
  if (sh.seg_begin != 0 || sh.seg_end != sh.g_total)
    return fail(GH_E_ARG, "gh_ctx_build_index: the load must cover segments [0, G)");
  if (out_len < bytes) return fail(GH_E_SMALL, "index buffer smaller than gh_index_bytes");
  const uint64_t nblocks = (bytes - 40) / 8 - 1;
  std::vector<uint64_t> counts(nblocks, 0);
  float ms = 0;
  GH_HIP(hipSetDevice(c->device));
  if (int rc = wait_decode(c)) return rc;
  if (sh.nseg > 0) {
    const Canon& cn = c->canon;
    // The context's decode mode may be a tile kernel, which keeps no count table on the
    // device: the build makes its own table and fallback tables, and frees them.
    const uint32_t kc = ws_count_bits(cn);
    const bool fb = kraft16(cn) != 65536 || cn.maxlen > kc;
    DevBuf d_lut, d_fb, d_cnt, d_status;
    if (int rc = upload_count_tables(cn, kc, d_lut, d_fb)) return rc;
    if (int rc = d_cnt.alloc(8 * nblocks, true)) return rc;
    if (int rc = d_status.alloc(16, true)) return rc;
    IdxParams ip{};
    ip.w = shard_params(c);
    if (int rc = loaded_last_end(c, &ip.w.last_end)) return rc;
    ip.w.lut = d_lut.get<uint2>();
    ip.w.status = d_status.get<unsigned int>();
    ip.w.kbits = kc;
    ip.w.lut_bytes = (uint32_t)(4u << kc);
    ip.w.fb = d_fb.get<uint32_t>();
    ip.counts = d_cnt.get<unsigned long long>();
    ip.nblocks = (uint32_t)nblocks;
    ip.log2_stride = log2_stride;
    const void* kern = kernel_by_width(kc, fb, [](auto gl, auto f) {
      return (const void*)gh_index_count_kernel<IDX_U, IDX_TB, decltype(gl)::value, decltype(f)::value>;
    });
    const size_t lds = std::max<size_t>(4ull << kc, 64) + (fb ? FB_BYTES : 0);
    if (int rc = allow_lds(kern, lds)) return rc;
    int pc = 0;
    GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, kern, IDX_TB, lds));
    if (pc < 1) return fail(GH_E_HIP, "the index kernel does not fit on a CU");
    // every workgroup that has an index block, at most what the device holds at once
    uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)pc * c->num_cu, ceil_div(nblocks, (uint64_t)(IDX_TB / 64)));
    if (const char* eg = getenv("GH_INDEX_GRID"))  // tests: few workgroups, many index blocks per wave
      grid = (uint32_t)std::clamp<long>(atol(eg), 1, (long)grid);
    EventPair ev;
    if (int rc = ev.create()) return rc;
    void* args[1] = {&ip};
    {
      // Joins the device's decode chain: a persistent tile kernel assumes its whole grid
      // is resident, so the build starts after the device's last tile decode, and the
      // chain stays locked until the build has finished (no tile decode of any context
      // is launched while it runs).
      DevChain& dc = dev_chain(c->device);
      std::lock_guard<std::mutex> chain_lock(dc.mu);
      if (dc.has) GH_HIP(hipStreamWaitEvent(c->stream, dc.last, 0));
      GH_HIP(hipEventRecord(ev.a, c->stream));
      GH_HIP(hipLaunchKernel(kern, dim3(grid), dim3(IDX_TB), args, lds, c->stream));
      GH_HIP(hipGetLastError());
      GH_HIP(hipEventRecord(ev.b, c->stream));
      GH_HIP(hipStreamSynchronize(c->stream));
    }
    if (int rc = ev.elapsed(&ms)) return rc;
    unsigned int status = 0;
    GH_HIP(hipMemcpy(&status, d_status.get(), 4, hipMemcpyDeviceToHost));
    GH_HIP(hipMemcpy(counts.data(), d_cnt.get(), 8 * nblocks, hipMemcpyDeviceToHost));
    if (status & GH_ST_LAYOUT) return fail(GH_E_HIP, "index kernel: LDS layout assumption violated");
    if (status & GH_ST_BADCODE) return fail(GH_E_CORRUPT, "invalid code in stream");
  }
  // exclusive scan of the block counts on the host; the last entry is N
  uint8_t* o = (uint8_t*)out;
  auto put64 = [&](size_t at, uint64_t v) { std::memcpy(o + at, &v, 8); };
  uint64_t run = 0;
  for (uint64_t k = 0; k < nblocks; ++k) {
    if (run > sh.n_total) return fail(GH_E_CORRUPT, "stream holds more than N symbols before its last segments");
    put64(40 + 8 * k, run);
    run += counts[k];
  }
  if (run < sh.n_total) return fail(GH_E_CORRUPT, "stream holds fewer than N symbols");
  put64(40 + 8 * nblocks, sh.n_total);
  index_header(log2_stride, sh.n_total, sh.g_total, nblocks + 1, o);
  if (symbols) *symbols = run;
  if (kernel_ms) *kernel_ms = ms;
  return GH_OK;
}

// ---- batched range gather (gh_gather.hip) -------------------------------------------
// The gather's tables, built on the context's first gather after a load (free_shard drops
// them): the count table of the index build (ws_count_bits), a single-symbol table of at
// most 12 bits, the fallback tables and the end of the stream's last segment.
static int gather_setup(gh_ctx* c) {
  const Canon& cn = c->canon;
  GatherTables t;
  t.kc = ws_count_bits(cn);
  t.ks = std::min<uint32_t>(std::max<uint32_t>(cn.maxlen, 2), 12);
  const bool fb = kraft16(cn) != 65536 || cn.maxlen > std::min(t.kc, t.ks);
  if (int rc = upload_count_tables(cn, t.kc, t.lut_c, t.fb)) return rc;
  if (int rc = t.lut_s.upload(single_lut(cn, t.ks).data(), 4ull << t.ks)) return rc;
  if (int rc = loaded_last_end(c, &t.last_end)) return rc;
  t.kern = kernel_by_width(t.kc, fb, [](auto gl, auto f) {
    return (const void*)gh_gather_kernel<GA_U, GA_TB, decltype(gl)::value, decltype(f)::value>;
  });
  t.lds = (4ull << t.kc) + (4ull << t.ks) + (fb ? FB_BYTES : 0);
  if (int rc = allow_lds(t.kern, t.lds)) return rc;
  int pc = 0;
  GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, t.kern, GA_TB, t.lds));
  if (pc < 1) return fail(GH_E_HIP, "the gather kernel does not fit on a CU");
  t.wgs = (uint32_t)pc * (uint32_t)c->num_cu;
  if (int rc = c->gather.ev.create()) return rc;
  t.ready = true;
  c->gather.tab = std::move(t);
  return GH_OK;
}

extern "C" int gh_ctx_gather(gh_ctx* c, const gh_index* ix, const gh_range* ranges, uint32_t nranges,
                             void* dst, uint64_t dst_len, void* hip_stream, float* kernel_ms) {
  if (!c || !ix || !ix->offsets || (nranges && !ranges)) return fail(GH_E_ARG, "null argument");
  if (kernel_ms) *kernel_ms = 0;
  if (!c->loaded) return fail(GH_E_STATE, "gh_ctx_gather before gh_ctx_load");
  const Shard& sh = c->shard;
  Gather& ga = c->gather;
  if (sh.seg_begin != 0 || sh.seg_end != sh.g_total)
    return fail(GH_E_ARG, "gh_ctx_gather: the load must cover segments [0, G)");
  if (ix->n != sh.n_total || ix->g != sh.g_total) return fail(GH_E_ARG, "gh_ctx_gather: the index is another stream's (N, G)");
  const uint64_t ibytes = gh_index_bytes(ix->g, ix->log2_stride);
  if (ibytes == 0 || ix->nentries != (ibytes - 40) / 8) return fail(GH_E_ARG, "gh_ctx_gather: malformed index");
  // plan into the context's piece vector (sized by a first pass)
  uint64_t np = 0, total = 0;
  int rc = gh_gather_plan(ix, ranges, nranges, ga.pieces.data(), ga.pieces.size(), &np, &total);
  if (rc == GH_E_SMALL) {
    ga.pieces.resize(np);
    rc = gh_gather_plan(ix, ranges, nranges, ga.pieces.data(), ga.pieces.size(), &np, &total);
  }
  if (rc) return rc;
  if (total > dst_len) return fail(GH_E_SMALL, "gather destination smaller than the ranges' bytes");
  if (total == 0) return GH_OK;  // (no range, only empty ranges, or an empty stream)
  if (!dst) return fail(GH_E_ARG, "null argument");
  if (np >= (1ull << 31)) return fail(GH_E_ARG, "gh_ctx_gather: 2^31 or more pieces in one batch");
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)c->stream;
  GH_HIP(hipSetDevice(c->device));
  if (int rc2 = wait_decode(c)) return rc2;
  if (!ga.tab.ready)
    if (int rc2 = gather_setup(c)) return rc2;
  const GatherTables& t = ga.tab;
  if (int rc2 = ga.d_pieces.reserve(np * sizeof(gh_gather_piece))) return rc2;
  if (int rc2 = ga.d_out.reserve(total)) return rc2;
  unsigned int* d_status = c->misc_at(16);  // (a word of its own: [1] is the decode's)
  GatherParams gp{};
  gp.w = shard_params(c);
  gp.w.lut = t.lut_c.get<uint2>();
  gp.w.out = ga.d_out.get<uint8_t>();
  gp.w.status = d_status;
  gp.w.kbits = t.kc;
  gp.w.lut_bytes = (uint32_t)(4u << t.kc);
  gp.w.last_end = t.last_end;
  gp.w.fb = t.fb.get<uint32_t>();
  gp.pieces = ga.d_pieces.get<gh_gather_piece>();
  gp.sym_lut = t.lut_s.get<uint32_t>();
  gp.npieces = (uint32_t)np;
  gp.log2_stride = ix->log2_stride;
  gp.sym_bits = t.ks;
  // every workgroup that has a piece, at most what the device holds at once
  uint32_t grid = (uint32_t)std::min<uint64_t>(t.wgs, ceil_div(np, (uint64_t)(GA_TB / 64)));
  if (const char* eg = getenv("GH_GATHER_GRID"))  // tests: few workgroups, many pieces per wave
    grid = (uint32_t)std::clamp<long>(atol(eg), 1, (long)grid);
  void* args[1] = {&gp};
  unsigned int status = 0;
  float ms = 0;
  {
    // Joins the device's decode chain as gh_ctx_build_index does: the gather starts after
    // the device's last tile decode, and the chain stays locked until it has finished.
    DevChain& dc = dev_chain(c->device);
    std::lock_guard<std::mutex> chain_lock(dc.mu);
    if (dc.has) GH_HIP(hipStreamWaitEvent(st, dc.last, 0));
    GH_HIP(hipMemsetAsync(d_status, 0, 4, st));
    GH_HIP(hipMemcpyAsync(ga.d_pieces.get(), ga.pieces.data(), np * sizeof(gh_gather_piece), hipMemcpyHostToDevice, st));
    GH_HIP(hipEventRecord(ga.ev.a, st));
    GH_HIP(hipLaunchKernel(t.kern, dim3(grid), dim3(GA_TB), args, t.lds, st));
    GH_HIP(hipGetLastError());
    GH_HIP(hipEventRecord(ga.ev.b, st));
    GH_HIP(hipMemcpyAsync(dst, ga.d_out.get(), total, hipMemcpyDefault, st));
    GH_HIP(hipStreamSynchronize(st));
  }
  if (int rc2 = ga.ev.elapsed(&ms)) return rc2;
  GH_HIP(hipMemcpy(&status, d_status, 4, hipMemcpyDeviceToHost));
  if (status & GH_ST_LAYOUT) return fail(GH_E_HIP, "gather kernel: LDS layout assumption violated");
  if (status & GH_ST_BADCODE) return fail(GH_E_CORRUPT, "gather: invalid code in stream, or the index is another stream's");
  if (kernel_ms) *kernel_ms = ms;
  return GH_OK;
}

// ---- device-planned gather (gh_gather_plan.hip) ---------------------------------------
extern "C" int gh_ctx_set_index(gh_ctx* c, const gh_index* ix) {
  if (!c || !ix || !ix->offsets) return fail(GH_E_ARG, "null argument");
  if (!c->loaded) return fail(GH_E_STATE, "gh_ctx_set_index before gh_ctx_load");
  const Shard& sh = c->shard;
  DevGather& dg = c->dgather;
  if (sh.seg_begin != 0 || sh.seg_end != sh.g_total)
    return fail(GH_E_ARG, "gh_ctx_set_index: the load must cover segments [0, G)");
  if (ix->n != sh.n_total || ix->g != sh.g_total) return fail(GH_E_ARG, "gh_ctx_set_index: the index is another stream's (N, G)");
  const uint64_t ibytes = gh_index_bytes(ix->g, ix->log2_stride);
  if (ibytes == 0 || ix->nentries != (ibytes - 40) / 8) return fail(GH_E_ARG, "gh_ctx_set_index: malformed index");
  // the entries as aligned u64 (the image's may lie at any address), checked as
  // gh_index_parse checks them: the kernels' piece arithmetic relies on it
  std::vector<uint64_t> off(ix->nentries);
  std::memcpy(off.data(), ix->offsets, 8 * ix->nentries);
  const uint64_t nblocks = ix->nentries - 1;
  bool ok = off[0] == 0 && off[nblocks] == ix->n;
  for (uint64_t k = 0; k < nblocks && ok; ++k) ok = off[k + 1] >= off[k] && off[k + 1] - off[k] <= (143ull << ix->log2_stride);
  if (!ok) return fail(GH_E_ARG, "gh_ctx_set_index: the entries are not those of a parsed index");
  std::vector<uint32_t> rank(ix->nentries);  // (nblocks < 2^23: a load holds fewer than 2^31 segments)
  gr_rank(off.data(), nblocks, rank.data());
  GH_HIP(hipSetDevice(c->device));
  if (dg.enqueued) GH_HIP(hipEventSynchronize(dg.ev_c));  // a gather in flight reads the old entries
  dg.has_index = false;
  if (int rc = dg.offsets.upload(off.data(), 8 * ix->nentries)) return rc;
  if (int rc = dg.rank.upload(rank.data(), 4 * ix->nentries)) return rc;
  dg.nblocks = nblocks;
  dg.log2_stride = ix->log2_stride;
  dg.has_index = true;
  return GH_OK;
}

// Enqueues the plan kernels and the gather kernel and returns.  Device waits on this path:
// none when the tables exist and the buffers are large enough.  The exceptions: the first
// gather after a load (gather_setup reads the stream's last words back), a buffer that has
// to grow (the last gather in flight still uses the old one), and nothing else: the
// context's own decodes are not waited for, since the gather reads only the loaded stream
// and writes only its own buffers, status words and d_dst.
extern "C" int gh_ctx_gather_device(gh_ctx* c, const gh_range* d_ranges, uint32_t nranges, void* d_dst,
                                    uint64_t dst_len, void* hip_stream) {
  if (!c) return fail(GH_E_ARG, "null ctx");
  if (!c->loaded) return fail(GH_E_STATE, "gh_ctx_gather_device before gh_ctx_load");
  DevGather& dg = c->dgather;
  if (!dg.has_index) return fail(GH_E_STATE, "gh_ctx_gather_device without a resident index (gh_ctx_set_index)");
  if (nranges == 0) return GH_OK;
  if (!d_ranges || !d_dst) return fail(GH_E_ARG, "null argument");
  if (nranges > GH_GATHER_MAX_RANGES) return fail(GH_E_ARG, "gh_ctx_gather_device: more than 2^24 ranges in one batch");
  // (the gather kernel counts pieces in 32 bits)
  const uint64_t cap = std::min<uint64_t>(gh_gather_piece_bound(nranges, dst_len, dg.log2_stride), (1ull << 31) - 1);
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)c->stream;
  GH_HIP(hipSetDevice(c->device));
  Gather& ga = c->gather;
  // (a stream without segments has N = 0: the plan kernels alone run, and refuse every
  // range that is not empty)
  const bool has_segments = c->shard.nseg > 0;
  if (has_segments && !ga.tab.ready)
    if (int rc = gather_setup(c)) return rc;
  const GatherTables& t = ga.tab;
  if (int rc = dg.ev_a.create()) return rc;
  if (int rc = dg.ev_b.create()) return rc;
  if (int rc = dg.ev_c.create()) return rc;
  if (dg.loc.capacity() < nranges * sizeof(RangeLoc) || dg.pieces.capacity() < cap * sizeof(gh_gather_piece)) {
    if (dg.enqueued) GH_HIP(hipEventSynchronize(dg.ev_c));
    if (int rc = dg.loc.reserve(nranges * sizeof(RangeLoc))) return rc;
    if (int rc = dg.slot.reserve(nranges * 4ull)) return rc;
    if (int rc = dg.dst0.reserve(nranges * 8ull)) return rc;
    if (int rc = dg.pieces.reserve(cap * sizeof(gh_gather_piece))) return rc;
  }
  GplanParams pp{};
  pp.ranges = d_ranges;
  pp.offsets = dg.offsets.get<uint64_t>();
  pp.rank = dg.rank.get<uint32_t>();
  pp.loc = dg.loc.get<RangeLoc>();
  pp.slot = dg.slot.get<uint32_t>();
  pp.dst0 = dg.dst0.get<unsigned long long>();
  pp.pieces = dg.pieces.get<gh_gather_piece>();
  pp.status = c->misc_at(18);
  pp.npieces = c->misc_at(19);
  pp.totals = (unsigned long long*)c->misc_at(20);
  pp.nblocks = dg.nblocks;
  pp.n = c->shard.n_total;
  pp.cap = cap;
  pp.dst_len = dst_len;
  pp.nranges = nranges;
  GatherParams gp{};
  gp.w = shard_params(c);
  gp.w.lut = t.lut_c.get<uint2>();
  gp.w.out = (uint8_t*)d_dst;
  gp.w.status = pp.status;
  gp.w.kbits = t.kc;
  gp.w.lut_bytes = (uint32_t)(4u << t.kc);
  gp.w.last_end = t.last_end;
  gp.w.fb = t.fb.get<uint32_t>();
  gp.pieces = pp.pieces;
  gp.sym_lut = t.lut_s.get<uint32_t>();
  gp.d_npieces = pp.npieces;
  gp.log2_stride = dg.log2_stride;
  gp.sym_bits = t.ks;
  // the host knows only the bound: every workgroup that could have a piece, at most what
  // the device holds at once
  uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint32_t>(t.wgs, 1), ceil_div(cap, (uint64_t)(GA_TB / 64)));
  if (const char* eg = getenv("GH_GATHER_GRID"))  // tests: few workgroups, many pieces per wave
    grid = (uint32_t)std::clamp<long>(atol(eg), 1, (long)grid);
  const uint32_t grid_r = (uint32_t)ceil_div((uint64_t)nranges, (uint64_t)GP_TB);
  const uint32_t grid_e = (uint32_t)std::min<uint64_t>(ceil_div(cap, (uint64_t)GP_TB), 1024);
  void* pa[1] = {&pp};
  void* args[1] = {&gp};
  // A member of the device's decode chain, without holding it: the lock is taken only
  // while enqueuing.  The gather starts after the device's last tile decode (or chain
  // member), and its end event becomes the chain's last, so the next tile decode of any
  // context starts after the gather.
  DevChain& dc = dev_chain(c->device);
  std::lock_guard<std::mutex> chain_lock(dc.mu);
  const bool ordered = dc.owner == c && dc.last_stream == st && st == c->stream;
  if (dc.has && !ordered) GH_HIP(hipStreamWaitEvent(st, dc.last, 0));
  // (the context's gathers share the plan's buffers: in turn, whatever their streams)
  if (dg.enqueued && dg.last_stream != st) GH_HIP(hipStreamWaitEvent(st, dg.ev_c, 0));
  GH_HIP(hipEventRecord(dg.ev_a, st));
  GH_HIP(hipLaunchKernel((const void*)gh_gplan_locate_kernel, dim3(grid_r), dim3(GP_TB), pa, 0, st));
  GH_HIP(hipLaunchKernel((const void*)gh_gplan_scan_kernel, dim3(1), dim3(GP_SCAN_TB), pa, 0, st));
  GH_HIP(hipLaunchKernel((const void*)gh_gplan_emit_kernel, dim3(grid_e), dim3(GP_TB), pa, 0, st));
  GH_HIP(hipEventRecord(dg.ev_b, st));
  if (has_segments) GH_HIP(hipLaunchKernel(t.kern, dim3(grid), dim3(GA_TB), args, t.lds, st));
  GH_HIP(hipGetLastError());
  GH_HIP(hipEventRecord(dg.ev_c, st));
  dg.enqueued = true;
  dg.last_stream = st;
  dc.last = dg.ev_c;
  dc.owner = c;
  dc.has = true;
  dc.last_stream = st;
  return GH_OK;
}

// Waits for the last device gather and reads its words of misc: [18] status, [19] piece
// count, [20..21] bytes.
static int dgather_result(gh_ctx* c, const char* who, unsigned int* status, uint64_t* np, uint64_t* bytes) {
  if (!c) return fail(GH_E_ARG, "null ctx");
  if (!c->dgather.enqueued) return fail(GH_E_STATE, std::string(who) + ": no device gather since the load");
  GH_HIP(hipSetDevice(c->device));
  GH_HIP(hipEventSynchronize(c->dgather.ev_c));
  unsigned int m[4] = {};
  GH_HIP(hipMemcpy(m, c->misc_at(18), sizeof(m), hipMemcpyDeviceToHost));
  *status = m[0];
  *np = m[1];
  std::memcpy(bytes, m + 2, 8);
  return GH_OK;
}

// Event times of the last device gather, once it has finished: plan kernels, gather kernel.
static int dgather_times(const gh_ctx* c, float* plan_ms, float* gather_ms) {
  GH_HIP(hipEventElapsedTime(plan_ms, c->dgather.ev_a, c->dgather.ev_b));
  GH_HIP(hipEventElapsedTime(gather_ms, c->dgather.ev_b, c->dgather.ev_c));
  return GH_OK;
}

extern "C" int gh_ctx_gather_times(gh_ctx* c, float* plan_ms, float* gather_ms) {
  unsigned int status;
  uint64_t np, bytes;
  if (int rc = dgather_result(c, "gh_ctx_gather_times", &status, &np, &bytes)) return rc;
  float a = 0, b = 0;
  if (int rc = dgather_times(c, &a, &b)) return rc;
  if (plan_ms) *plan_ms = a;
  if (gather_ms) *gather_ms = b;
  return GH_OK;
}

extern "C" int gh_ctx_gather_wait(gh_ctx* c, gh_gather_report* rep) {
  if (rep) std::memset(rep, 0, sizeof(*rep));
  unsigned int status;
  uint64_t np, bytes;
  if (int rc = dgather_result(c, "gh_ctx_gather_wait", &status, &np, &bytes)) return rc;
  float a = 0, b = 0;
  if (int rc = dgather_times(c, &a, &b)) return rc;
  if (rep) {
    rep->out_bytes = bytes;
    rep->npieces = np;
    rep->status = status;
    rep->kernel_ms = a + b;
  }
  if (status & GH_ST_RANGE) return fail(GH_E_ARG, "device gather: a byte range outside [0, N]");
  if (status & GH_ST_DSTSMALL) return fail(GH_E_SMALL, "device gather: destination smaller than the ranges' bytes");
  if (status & GH_ST_PIECES) return fail(GH_E_CORRUPT, "device gather: the plan exceeds the piece bound (the index is no real stream's)");
  if (status & GH_ST_LAYOUT) return fail(GH_E_HIP, "gather kernel: LDS layout assumption violated");
  if (status & GH_ST_BADCODE) return fail(GH_E_CORRUPT, "gather: invalid code in stream, or the index is another stream's");
  return GH_OK;
}

extern "C" int gh_ctx_gather_pieces(gh_ctx* c, gh_gather_piece* pieces, uint64_t cap, uint64_t* npieces) {
  if (!npieces || (cap && !pieces)) return fail(GH_E_ARG, "null argument");
  *npieces = 0;
  unsigned int status;
  uint64_t np, bytes;
  if (int rc = dgather_result(c, "gh_ctx_gather_pieces", &status, &np, &bytes)) return rc;
  *npieces = np;
  if (np > cap) return fail(GH_E_SMALL, "piece buffer smaller than the plan");
  if (np) GH_HIP(hipMemcpy(pieces, c->dgather.pieces.get(), np * sizeof(gh_gather_piece), hipMemcpyDeviceToHost));
  return GH_OK;
}

// ---- batched decode (gaphuff.h; kernels: gh_batch.hip; host plan: gh::batch_plan) ------
// The count and write kernels of a batch share one template argument list, as the *_kern
// functions above: FB, whether a lookup can miss.
struct BatchKernels {
  const void* count;
  const void* write;
  const char* name;
};
template <bool FB>
static BatchKernels batch_kernels() {
  static const std::string n = kern_name("batch<fb=%d>", (int)FB);
  return {(const void*)gh_batch_count_kernel<FB>, (const void*)gh_batch_write_kernel<FB>, n.c_str()};
}
static BatchKernels batch_kernels_for(bool fb) { return fb ? batch_kernels<true>() : batch_kernels<false>(); }
constexpr uint32_t BATCH_LAUNCHES = 3;  // count, scan, write
constexpr uint32_t BATCH_INDEX_LAUNCHES = 2;   // count, scan (gh_batchdec_index)
constexpr uint32_t BATCH_GATHER_LAUNCHES = 5;  // memset, locate, scan, emit, gather
constexpr uint32_t BATCH_RAW_LAUNCHES = 3;     // trans, chain, apply (a raw load's gap kernels)

// The trans kernel of a raw load, picked as the decode kernels are.
template <bool FB>
static Kern batchraw_kern() {
  static const std::string n = kern_name("batchraw<fb=%d>", (int)FB);
  return {(const void*)gh_batchraw_trans_kernel<FB>, n.c_str()};
}
static Kern batchraw_kern_for(bool fb) { return fb ? batchraw_kern<true>() : batchraw_kern<false>(); }

template <bool FB>
static Kern bgather_kern() {
  static const std::string n = kern_name("bgather<fb=%d>", (int)FB);
  return {(const void*)gh_batch_gather_kernel<FB>, n.c_str()};
}
static Kern bgather_kern_for(bool fb) { return fb ? bgather_kern<true>() : bgather_kern<false>(); }

// The batched gather's state in a gh_batch (gh_batchdec_*).  words: [0] status, [1] piece
// count, [2..3] bytes, [4..5] pieces, [6] ranges on flagged streams; its own, not the
// decode's flag words, which the next decode memsets.
struct BatchGather {
  DevBuf loc, slot, dst0, pieces, words, ranges;  // (ranges: gh_batchdec_gather's upload)
  EventPair ev;
  bool enqueued = false, timed = false;
};

// The byte-plane join's state in a gh_batch (gh_planes_*).  desc: the tensors' descriptors,
// then their unit prefix; words: [0] tensors with a flagged plane.
struct BatchPlanes {
  DevBuf desc, words;
  EventPair ev;
  uint64_t out_bytes = 0;
  uint32_t ntensors = 0;
  bool enqueued = false, timed = false;
};

// The element gather's state in a gh_batch (gh_pgather_*).  desc: the tensors' descriptors, as
// uploaded (last_desc: their host copy; a call with the same list uploads nothing); per: the
// per-range arrays (loc: PgLoc; stage_off, dst_off: u64; slot, unit0: u32); words: PgatherParams's.
struct BatchPGather {
  DevBuf desc, words, branges, per, staging, ranges;  // (ranges: gh_pgather's upload)
  std::vector<uint8_t> last_desc;
  EventPair ev_x, ev_j;  // around the memset, scan and expand; around the range join
  uint64_t nslots = 0;
  bool enqueued = false, timed = false;
};

struct gh_batch {
  DevBuf payload, gaps, tables, desc, unit0, syms, items;  // the loaded batch
  DevBuf seg_cnt, unit_tot, unit_off, symbols;             // decode scratch
  DevBuf flags;                                            // 4 summary words, then a status word per stream
  DevBuf out;                                              // the batch's own output arena (on demand)
  DevBuf raw_scratch;  // raw loads: per unit 256 T_j (8 bytes each), its aggregate (8) and its entry (4)
  EventPair raw_ev;    // around the gap kernels of the last raw load
  uint64_t raw_scratch_bytes = 0;
  bool raw = false;    // the last load was a raw load
  BatchPlan plan;
  std::vector<uint64_t> n;
  uint32_t nstreams = 0, launches = 0;  // launches: of the last decode or index
  bool loaded = false, fb = false, own_out = false;
  bool indexed = false;  // seg_cnt / unit_off / status are (being) made by a decode or an index since the load
  BatchGather g;
  BatchPlanes pl;
  BatchPGather pg;
  BatchQueue q;  // (last: its destructor waits for the decode before the buffers above go)
};

extern "C" int gh_batch_create(int device, gh_batch** out) {
  if (!out) return fail(GH_E_ARG, "null batch pointer");
  *out = nullptr;
  std::unique_ptr<gh_batch> b(new gh_batch());
  if (int rc = b->q.create(device, "no HIP device visible (the decoder has no CPU fallback)")) return rc;
  *out = b.release();
  return GH_OK;
}

extern "C" int gh_batch_destroy(gh_batch* b) {
  delete b;
  return GH_OK;
}

// ss[i]: stream i's header; its word pointers are host memory (any alignment), or device
// memory when `device`.  raw: gap-less streams (g = ceil(w / 4), no gap source); their gap
// words are built in the gap arena by the three kernels of gh_batch_raw.hip.
static int batch_load(gh_batch* b, const std::vector<gh_stream>& ss, bool device, void* hip_stream, bool raw = false) {
  const uint32_t ns = (uint32_t)ss.size();
  GH_HIP(hipSetDevice(b->q.device));
  if (int rc = b->q.quiesce()) return rc;  // the previous batch's decode reads what is replaced
  b->loaded = b->own_out = b->indexed = b->g.enqueued = b->pl.enqueued = b->pg.enqueued = b->raw = false;
  b->pg.last_desc.clear();
  std::vector<uint64_t> n(ns), w(ns), g(ns);
  std::vector<BatchDesc> desc(ns);
  std::vector<gh_sym> syms;
  uint64_t tab_words = 0;
  bool fb = false;
  for (uint32_t i = 0; i < ns; ++i) {
    const gh_stream& s = ss[i];
    const std::string who = "stream " + std::to_string(i) + ": ";
    if (int rc = gh_stream_validate(&s)) return fail(rc, who + gh_last_error());
    Canon cn;
    if (int rc = build_canon(s.syms, s.nsyms, cn)) return fail(rc, who + gh_last_error());
    if (s.g > 0 && cn.nsyms == 0) return fail(GH_E_TABLE, who + "segments but an empty code");
    if ((s.w && !s.payload) || (s.g && !raw && !s.gap_words)) return fail(GH_E_ARG, who + "null word pointer");
    if (device && ((((uintptr_t)s.payload) | (raw ? 0 : (uintptr_t)s.gap_words)) & 3u))
      return fail(GH_E_ARG, who + "device words not 4-byte aligned");
    n[i] = s.n;
    w[i] = s.w;
    g[i] = s.g;
    BatchDesc& d = desc[i];
    d = BatchDesc{};
    d.n = s.n;
    d.minlen = std::max<uint32_t>(cn.minlen, 1);
    d.maxlen = std::max<uint32_t>(cn.maxlen, d.minlen);
    d.sym_off = (uint32_t)syms.size();
    d.nsyms = s.nsyms;
    d.tab_off = tab_words;
    if (s.g) {
      d.kbits = std::min<uint32_t>(cn.maxlen, BA_KMAX);
      tab_words += BA_FBW + std::max<uint32_t>(1u << d.kbits, 4u);
      fb |= cn.maxlen > BA_KMAX || kraft16(cn) != 65536;
      syms.insert(syms.end(), s.syms, s.syms + s.nsyms);
    }
  }
  BatchPlan plan;
  if (int rc = batch_plan(n.data(), w.data(), g.data(), ns, plan)) return rc;
  std::vector<uint32_t> unit0(ns + 1);
  for (uint32_t i = 0; i < ns; ++i) {
    const BatchExtent& e = plan.ext[i];
    desc[i].pay_off = e.pay_off;
    desc[i].gap_off = e.gap_off;
    desc[i].out_off = e.out_off;
    desc[i].nseg = (uint32_t)g[i];
    unit0[i] = (uint32_t)e.unit0;
  }
  unit0[ns] = (uint32_t)plan.nunits;
  if (int rc = upload_at_least(b->desc, desc.data(), sizeof(BatchDesc) * (uint64_t)ns)) return rc;
  if (int rc = upload_at_least(b->unit0, unit0.data(), 4ull * (ns + 1))) return rc;
  if (int rc = upload_at_least(b->syms, syms.data(), sizeof(gh_sym) * (uint64_t)syms.size())) return rc;
  if (int rc = b->tables.reserve(std::max<uint64_t>(4 * tab_words, 16))) return rc;
  if (int rc = b->payload.reserve(std::max<uint64_t>(4 * plan.pay_words, 16))) return rc;
  if (int rc = b->gaps.reserve(std::max<uint64_t>(4 * plan.gap_words, 16))) return rc;
  if (int rc = b->seg_cnt.reserve(std::max<uint64_t>(plan.nunits * BATCH_UNIT_SEGS, 16))) return rc;
  if (int rc = b->unit_tot.reserve(std::max<uint64_t>(4 * plan.nunits, 16))) return rc;
  if (int rc = b->unit_off.reserve(8 * (plan.nunits + 1))) return rc;
  if (int rc = b->symbols.reserve(std::max<uint64_t>(8ull * ns, 16))) return rc;
  if (int rc = b->flags.reserve(16 + 4ull * ns)) return rc;
  const uint64_t raw_bytes = (BR_T_BYTES + 8ull + 4ull) * plan.nunits;
  if (raw) {
    if (int rc = b->raw_scratch.reserve(std::max<uint64_t>(raw_bytes, 16))) return rc;
    if (int rc = b->raw_ev.create()) return rc;
  }
  if (!device) {
    // the arenas are assembled in host memory, padding included, and go up in two copies
    std::vector<uint32_t> pay(plan.pay_words, 0u), gap(plan.gap_words, 0u);
    for (uint32_t i = 0; i < ns; ++i) {
      if (w[i]) std::memcpy(pay.data() + plan.ext[i].pay_off, ss[i].payload, 4 * w[i]);
      if (g[i] && !raw) std::memcpy(gap.data() + plan.ext[i].gap_off, ss[i].gap_words, 4 * plan.ext[i].gap_words);
    }
    if (int rc = upload_arena(b->q.device, b->payload, pay.data(), 4 * pay.size())) return rc;
    if (!gap.empty() && !raw) GH_HIP(hipMemcpy(b->gaps.get(), gap.data(), 4 * gap.size(), hipMemcpyHostToDevice));
  } else {
    std::vector<BatchCopyItem> items(ns);
    for (uint32_t i = 0; i < ns; ++i) {
      const BatchExtent& e = plan.ext[i];
      items[i] = BatchCopyItem{ss[i].payload, raw ? nullptr : ss[i].gap_words, w[i], e.pay_off, e.pay_words, e.gap_off,
                               raw ? 0ull : e.gap_words};
    }
    if (int rc = upload_at_least(b->items, items.data(), sizeof(BatchCopyItem) * (uint64_t)ns)) return rc;
    // after what the producer's stream holds now, then one copy kernel on the batch's stream
    if (int rc = b->q.follow(hip_stream)) return rc;
    if (plan.pay_words) {
      hipLaunchKernelGGL(gh_batch_copy_kernel, dim3(std::min<uint32_t>(ns, 4096u), BA_COPY_Y), dim3(256), 0, b->q.stream,
                         b->items.get<BatchCopyItem>(), ns, b->payload.get<uint32_t>(), b->gaps.get<uint32_t>());
      GH_HIP(hipGetLastError());
    }
  }
  if (tab_words) {  // every stream's tables: one launch
    hipLaunchKernelGGL(gh_batch_table_kernel, dim3(std::min<uint32_t>(ns, 16u * (uint32_t)b->q.num_cu)), dim3(256), 0,
                       b->q.stream, b->desc.get<BatchDesc>(), b->syms.get<gh_sym>(), b->tables.get<uint32_t>(), ns);
    GH_HIP(hipGetLastError());
  }
  if (raw) {  // the gap arena from the payload: three launches, whatever ns is (every unit's gap words are written whole)
    GH_HIP(hipEventRecord(b->raw_ev.a, b->q.stream));
    if (plan.nunits) {
      BatchParams bp{};
      bp.desc = b->desc.get<BatchDesc>();
      bp.unit0 = b->unit0.get<uint32_t>();
      bp.payload = b->payload.get<uint32_t>();
      bp.tables = b->tables.get<uint32_t>();
      bp.nstreams = ns;
      bp.nunits = (uint32_t)plan.nunits;
      unsigned long long* trans = b->raw_scratch.get<unsigned long long>();
      unsigned long long* agg = trans + plan.nunits * BATCH_UNIT_SEGS;
      uint32_t* entry = (uint32_t*)(agg + plan.nunits);
      const uint32_t* cunit0 = bp.unit0;
      uint32_t* dgaps = b->gaps.get<uint32_t>();
      const uint32_t grid = unit_grid("GH_BATCH_GRID", plan.nunits, BA_TB / 64, b->q.num_cu);
      const uint32_t cgrid = (uint32_t)std::clamp<uint64_t>(ceil_div(ns, BR_CHAIN_TB / 64), 1, 4ull * (uint64_t)b->q.num_cu);
      uint32_t nsv = ns;
      void* targs[] = {&bp, &trans, &agg};
      GH_HIP(hipLaunchKernel(batchraw_kern_for(fb).fn, dim3(grid), dim3(BA_TB), targs, 0, b->q.stream));
      void* cargs[] = {&cunit0, &nsv, &agg, &entry};
      GH_HIP(hipLaunchKernel((const void*)gh_batchraw_chain_kernel, dim3(cgrid), dim3(BR_CHAIN_TB), cargs, 0, b->q.stream));
      void* aargs[] = {&bp, &trans, &entry, &dgaps};
      GH_HIP(hipLaunchKernel((const void*)gh_batchraw_apply_kernel, dim3(grid), dim3(BA_TB), aargs, 0, b->q.stream));
    }
    GH_HIP(hipEventRecord(b->raw_ev.b, b->q.stream));
  }
  GH_HIP(hipStreamSynchronize(b->q.stream));
  b->raw = raw;
  b->raw_scratch_bytes = raw ? raw_bytes : 0;
  b->plan = std::move(plan);
  b->n = std::move(n);
  b->nstreams = ns;
  b->fb = fb;
  b->loaded = true;
  return GH_OK;
}

extern "C" int gh_batch_load(gh_batch* b, const gh_stream* streams, uint32_t nstreams) {
  if (!b || (nstreams && !streams)) return fail(GH_E_ARG, "null argument");
  if (nstreams > BATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  return batch_load(b, std::vector<gh_stream>(streams, streams + nstreams), false, nullptr);
}

extern "C" int gh_batch_load_device(gh_batch* b, const gh_batch_item* items, uint32_t nstreams, void* hip_stream) {
  if (!b || (nstreams && !items)) return fail(GH_E_ARG, "null argument");
  if (nstreams > BATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  std::vector<gh_stream> ss(nstreams);
  for (uint32_t i = 0; i < nstreams; ++i) {
    const gh_batch_item& it = items[i];
    ss[i] = gh_stream{it.syms, it.nsyms, 2u, it.n, it.w, it.g, it.d_gap_words, it.d_payload};
  }
  return batch_load(b, ss, true, hip_stream);
}

// ---- batched gap-less load (gaphuff.h; kernels: gh_batch_raw.hip; functions: gh_raw_trans.hpp) ----
extern "C" int gh_batchraw_load(gh_batch* b, const gh_raw_stream* streams, uint32_t nstreams) {
  if (!b || (nstreams && !streams)) return fail(GH_E_ARG, "null argument");
  if (nstreams > BATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  std::vector<gh_stream> ss(nstreams);
  for (uint32_t i = 0; i < nstreams; ++i) {
    const gh_raw_stream& r = streams[i];
    ss[i] = gh_stream{r.syms, r.nsyms, 2u, r.n, r.w, r.w / 4 + (r.w % 4 != 0), nullptr, r.units};
  }
  return batch_load(b, ss, false, nullptr, true);
}

extern "C" int gh_batchraw_load_device(gh_batch* b, const gh_batch_item* items, uint32_t nstreams, void* hip_stream) {
  if (!b || (nstreams && !items)) return fail(GH_E_ARG, "null argument");
  if (nstreams > BATCH_MAX_STREAMS) return fail(GH_E_ARG, "more than 2^24 streams in a batch");
  std::vector<gh_stream> ss(nstreams);
  for (uint32_t i = 0; i < nstreams; ++i) {
    const gh_batch_item& it = items[i];
    if (it.g != it.w / 4 + (it.w % 4 != 0))
      return fail(GH_E_ARG, "stream " + std::to_string(i) + ": a raw stream has G = ceil(W / 4) segments");
    ss[i] = gh_stream{it.syms, it.nsyms, 2u, it.n, it.w, it.g, nullptr, it.d_payload};
  }
  return batch_load(b, ss, true, hip_stream, true);
}

extern "C" int gh_batchraw_gaps(gh_batch* b, uint32_t stream, uint32_t* gap_words, uint64_t cap, uint64_t* ngapw) {
  if (ngapw) *ngapw = 0;
  if (!b || !ngapw) return fail(GH_E_ARG, "null argument");
  if (!b->loaded) return fail(GH_E_STATE, "gh_batchraw_gaps before a load");
  if (stream >= b->nstreams) return fail(GH_E_ARG, "no such stream in the batch");
  const BatchExtent& e = b->plan.ext[stream];
  *ngapw = e.gap_words;
  if (cap < e.gap_words) return fail(GH_E_SMALL, "gap word buffer smaller than the stream's gap words");
  if (e.gap_words && !gap_words) return fail(GH_E_ARG, "null argument");
  GH_HIP(hipSetDevice(b->q.device));
  if (e.gap_words)
    GH_HIP(hipMemcpy(gap_words, b->gaps.get<uint32_t>() + e.gap_off, 4 * e.gap_words, hipMemcpyDeviceToHost));
  return GH_OK;
}

extern "C" int gh_batchraw_report_get(gh_batch* b, gh_batchraw_report* rep) {
  if (!b || !rep) return fail(GH_E_ARG, "null argument");
  *rep = gh_batchraw_report{};
  if (!b->loaded || !b->raw) return fail(GH_E_STATE, "gh_batchraw_report_get: the last load was not a raw load");
  GH_HIP(hipSetDevice(b->q.device));
  if (int rc = b->raw_ev.elapsed(&rep->gap_ms)) return rc;
  rep->launches = BATCH_RAW_LAUNCHES;
  rep->scratch_bytes = b->raw_scratch_bytes;
  return GH_OK;
}

extern "C" int gh_batchraw_kernel_shape(gh_batch* b, char* buf, size_t cap) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded || !b->raw) return fail(GH_E_STATE, "gh_batchraw_kernel_shape: the last load was not a raw load");
  return copy_name(b->plan.nunits ? batchraw_kern_for(b->fb).name : "", buf, cap);
}

extern "C" int gh_batchraw_kernel_shapes(char* buf, size_t cap) {
  return copy_name(std::string(batchraw_kern_for(false).name) + "\n" + batchraw_kern_for(true).name + "\n", buf, cap);
}

// The kernels' view of the loaded batch; out: where a write or gather kernel stores.
static BatchParams batch_params(const gh_batch* b, void* out) {
  BatchParams bp{};
  bp.desc = b->desc.get<BatchDesc>();
  bp.unit0 = b->unit0.get<uint32_t>();
  bp.payload = b->payload.get<uint32_t>();
  bp.gaps = b->gaps.get<uint32_t>();
  bp.tables = b->tables.get<uint32_t>();
  bp.seg_cnt = b->seg_cnt.get<uint8_t>();
  bp.unit_tot = b->unit_tot.get<uint32_t>();
  bp.unit_off = b->unit_off.get<unsigned long long>();
  bp.summary = b->flags.get<unsigned int>();
  bp.status = bp.summary + 4;
  bp.symbols = b->symbols.get<unsigned long long>();
  bp.out = (uint8_t*)out;
  bp.nstreams = b->nstreams;
  bp.nunits = (uint32_t)b->plan.nunits;
  return bp;
}

// Enqueues the count and scan kernels and, with `write`, the write kernel into d_dst.
static int batch_run(gh_batch* b, void* d_dst, void* hip_stream, int timed, bool write) {
  BatchParams bp = batch_params(b, d_dst);
  // decodes of one batch share its scratch: they run in the order they were made
  hipStream_t st;
  if (int rc = b->q.begin(hip_stream, timed != 0, &st)) return rc;
  // (the count kernel ORs status words before the scan kernel sees them)
  GH_HIP(hipMemsetAsync(b->flags.get(), 0, 16 + 4ull * b->nstreams, st));
  if (b->nstreams) {
    const BatchKernels k = batch_kernels_for(b->fb);
    // GH_BATCH_GRID=k (tests): k workgroups for the count and write kernels
    const uint32_t grid = unit_grid("GH_BATCH_GRID", b->plan.nunits, BA_TB / 64, b->q.num_cu);
    void* args[] = {&bp};
    if (bp.nunits) GH_HIP(hipLaunchKernel(k.count, dim3(grid), dim3(BA_TB), args, 0, st));
    GH_HIP(hipLaunchKernel((const void*)gh_batch_scan_kernel, dim3(1), dim3(BA_SCAN_TB), args, 0, st));
    if (bp.nunits && write) GH_HIP(hipLaunchKernel(k.write, dim3(grid), dim3(BA_TB), args, 0, st));
  }
  if (int rc = b->q.end(st)) return rc;
  b->indexed = true;
  b->launches = write ? BATCH_LAUNCHES : BATCH_INDEX_LAUNCHES;
  return GH_OK;
}

extern "C" int gh_batch_decode(gh_batch* b, void* d_dst, uint64_t dst_len, void* hip_stream, int timed) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded) return fail(GH_E_STATE, "gh_batch_decode before a load");
  GH_HIP(hipSetDevice(b->q.device));
  const bool own = d_dst == nullptr;
  if (own) {
    if (int rc = b->out.reserve(std::max<uint64_t>(b->plan.out_bytes, 16))) return rc;
    d_dst = b->out.get();
  } else {
    if ((uintptr_t)d_dst & 15u) return fail(GH_E_ARG, "destination not 16-byte aligned");
    if (dst_len < b->plan.out_bytes) return fail(GH_E_SMALL, "destination smaller than the batch's arena");
  }
  if (int rc = batch_run(b, d_dst, hip_stream, timed, true)) return rc;
  b->own_out = own;
  return GH_OK;
}

extern "C" int gh_batch_wait(gh_batch* b, gh_batch_report* rep) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (rep) *rep = gh_batch_report{};
  if (!b->loaded || !b->q.enqueued) return fail(GH_E_STATE, "gh_batch_wait without a decode since the load");
  GH_HIP(hipSetDevice(b->q.device));
  float ms = 0;
  if (int rc = b->q.wait(&ms)) return rc;
  unsigned int sum[2] = {0, 0};
  GH_HIP(hipMemcpy(sum, b->flags.get(), sizeof(sum), hipMemcpyDeviceToHost));
  if (rep) {
    for (uint64_t v : b->n) rep->out_bytes += v;
    rep->nstreams = b->nstreams;
    rep->bad_streams = sum[0];
    rep->status = sum[1];
    rep->kernel_ms = ms;
    rep->launches = b->launches;
  }
  if (sum[0])
    return fail(GH_E_CORRUPT, std::to_string(sum[0]) + " stream(s) of the batch decoded to fewer than N symbols or met "
                                                        "a pattern outside their code (gh_batch_status names them)");
  return GH_OK;
}

extern "C" int gh_batch_status(gh_batch* b, uint32_t* status, uint64_t* symbols, uint32_t cap) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded || !b->q.enqueued) return fail(GH_E_STATE, "gh_batch_status without a decode since the load");
  if (cap < b->nstreams) return fail(GH_E_SMALL, "status arrays smaller than the batch");
  GH_HIP(hipSetDevice(b->q.device));
  GH_HIP(hipEventSynchronize(b->q.done));
  if (status && b->nstreams)
    GH_HIP(hipMemcpy(status, b->flags.get<unsigned int>() + 4, 4ull * b->nstreams, hipMemcpyDeviceToHost));
  if (symbols && b->nstreams) GH_HIP(hipMemcpy(symbols, b->symbols.get(), 8ull * b->nstreams, hipMemcpyDeviceToHost));
  return GH_OK;
}

extern "C" int gh_batch_output(gh_batch* b, void** d_out, uint64_t* cap) {
  if (!b || !d_out) return fail(GH_E_ARG, "null argument");
  *d_out = b->out.get();
  if (cap) *cap = b->out.capacity();
  return GH_OK;
}

extern "C" int gh_batch_offsets(gh_batch* b, uint64_t* out_off, uint32_t cap) {
  if (!b || !out_off) return fail(GH_E_ARG, "null argument");
  if (!b->loaded) return fail(GH_E_STATE, "gh_batch_offsets before a load");
  if ((uint64_t)cap < (uint64_t)b->nstreams + 1) return fail(GH_E_SMALL, "offset array smaller than nstreams + 1");
  for (uint32_t i = 0; i < b->nstreams; ++i) out_off[i] = b->plan.ext[i].out_off;
  out_off[b->nstreams] = b->plan.out_bytes;
  return GH_OK;
}

extern "C" int gh_batch_download(gh_batch* b, uint32_t stream, uint8_t* dst, uint64_t nbytes) {
  if (!b || (nbytes && !dst)) return fail(GH_E_ARG, "null argument");
  if (!b->loaded || !b->q.enqueued || !b->own_out)
    return fail(GH_E_STATE, "gh_batch_download without a decode into the batch's own arena");
  if (stream >= b->nstreams) return fail(GH_E_ARG, "no such stream in the batch");
  if (nbytes > b->n[stream]) return fail(GH_E_ARG, "more bytes than the stream holds");
  GH_HIP(hipSetDevice(b->q.device));
  GH_HIP(hipEventSynchronize(b->q.done));
  if (nbytes)
    GH_HIP(hipMemcpy(dst, b->out.get<uint8_t>() + b->plan.ext[stream].out_off, nbytes, hipMemcpyDeviceToHost));
  return GH_OK;
}

extern "C" int gh_batch_kernel_shape(gh_batch* b, char* buf, size_t cap) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded) return fail(GH_E_STATE, "gh_batch_kernel_shape before a load");
  return copy_name(b->plan.nunits ? batch_kernels_for(b->fb).name : "", buf, cap);
}

extern "C" int gh_batch_kernel_shapes(char* buf, size_t cap) {
  return copy_name(std::string(batch_kernels_for(false).name) + "\n" + batch_kernels_for(true).name + "\n", buf, cap);
}

// ---- batched gather (gaphuff.h; kernels: gh_batch_gather.hip; arithmetic: gh_batch_range.hpp) ----
extern "C" int gh_batchdec_index(gh_batch* b, void* hip_stream, int timed) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded) return fail(GH_E_STATE, "gh_batchdec_index before a load");
  GH_HIP(hipSetDevice(b->q.device));
  return batch_run(b, nullptr, hip_stream, timed, false);
}

// A member of the batch's queue without its timing events: it starts after the queue's last
// run (decode, index or gather) and its end becomes the queue's `done`, so the next decode,
// whose memset and count kernel rewrite what the gather reads, starts after it.
extern "C" int gh_batchdec_gather_device(gh_batch* b, const gh_brange* d_ranges, uint32_t nranges, void* d_dst,
                                         uint64_t dst_len, void* hip_stream, int timed) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded || !b->indexed)
    return fail(GH_E_STATE, "gh_batchdec_gather_device without gh_batchdec_index or gh_batch_decode since the load");
  if (nranges == 0) return GH_OK;
  if (!d_ranges || !d_dst) return fail(GH_E_ARG, "null argument");
  if (nranges > GH_GATHER_MAX_RANGES) return fail(GH_E_ARG, "gh_batchdec_gather_device: more than 2^24 ranges in one batch");
  GH_HIP(hipSetDevice(b->q.device));
  BatchGather& g = b->g;
  // (the gather kernel counts pieces in 32 bits)
  const uint64_t cap = std::min<uint64_t>(gh_gather_piece_bound(nranges, dst_len, 8), (1ull << 31) - 1);
  if (int rc = g.ev.create()) return rc;
  if (g.loc.capacity() < nranges * sizeof(RangeLoc) || g.pieces.capacity() < cap * sizeof(gh_gather_piece) || !g.words) {
    if (b->q.enqueued) GH_HIP(hipEventSynchronize(b->q.done));  // the last gather in flight uses the old buffers
    if (int rc = g.loc.reserve(nranges * sizeof(RangeLoc))) return rc;
    if (int rc = g.slot.reserve(nranges * 4ull)) return rc;
    if (int rc = g.dst0.reserve(nranges * 8ull)) return rc;
    if (int rc = g.pieces.reserve(std::max<uint64_t>(cap * sizeof(gh_gather_piece), 16))) return rc;
    if (int rc = g.words.reserve(32)) return rc;
  }
  unsigned int* words = g.words.get<unsigned int>();
  GplanParams sp{};  // what gh_gplan_scan_kernel reads
  sp.loc = g.loc.get<RangeLoc>();
  sp.slot = g.slot.get<uint32_t>();
  sp.dst0 = g.dst0.get<unsigned long long>();
  sp.status = words;
  sp.npieces = words + 1;
  sp.totals = (unsigned long long*)(words + 2);
  sp.cap = cap;
  sp.dst_len = dst_len;
  sp.nranges = nranges;
  BatchGatherParams gp{};
  gp.bp = batch_params(b, d_dst);
  gp.pieces = g.pieces.get<gh_gather_piece>();
  gp.d_npieces = sp.npieces;
  BgplanParams pp{};
  pp.ranges = d_ranges;
  pp.desc = gp.bp.desc;
  pp.unit0 = gp.bp.unit0;
  pp.unit_off = gp.bp.unit_off;
  pp.stream_status = gp.bp.status;
  pp.loc = sp.loc;
  pp.slot = sp.slot;
  pp.dst0 = sp.dst0;
  pp.pieces = g.pieces.get<gh_gather_piece>();
  pp.status = sp.status;
  pp.npieces = sp.npieces;
  pp.bad_ranges = words + 6;
  pp.cap = cap;
  pp.nranges = nranges;
  pp.nstreams = b->nstreams;
  // the host knows only the bound: a wave per piece that could exist, at most what unit_grid allows
  const uint32_t grid = unit_grid("GH_BATCH_GRID", cap, BA_TB / 64, b->q.num_cu);
  const uint32_t grid_r = (uint32_t)ceil_div((uint64_t)nranges, (uint64_t)GP_TB);
  const uint32_t grid_e = (uint32_t)std::clamp<uint64_t>(ceil_div(cap, (uint64_t)GP_TB), 1, 1024);
  void* pa[1] = {&pp};
  void* sa[1] = {&sp};
  void* ga[1] = {&gp};
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)b->q.stream;
  GH_HIP(hipStreamWaitEvent(st, b->q.done, 0));  // (indexed: the queue has a run)
  if (timed) GH_HIP(hipEventRecord(g.ev.a, st));
  GH_HIP(hipMemsetAsync(words, 0, 32, st));
  GH_HIP(hipLaunchKernel((const void*)gh_bgplan_locate_kernel, dim3(grid_r), dim3(GP_TB), pa, 0, st));
  GH_HIP(hipLaunchKernel((const void*)gh_gplan_scan_kernel, dim3(1), dim3(GP_SCAN_TB), sa, 0, st));
  GH_HIP(hipLaunchKernel((const void*)gh_bgplan_emit_kernel, dim3(grid_e), dim3(GP_TB), pa, 0, st));
  // (a batch without units has no non-empty valid range: the plan kernels alone refuse or pass it)
  if (gp.bp.nunits) GH_HIP(hipLaunchKernel(bgather_kern_for(b->fb).fn, dim3(grid), dim3(BA_TB), ga, 0, st));
  GH_HIP(hipGetLastError());
  if (timed) GH_HIP(hipEventRecord(g.ev.b, st));
  GH_HIP(hipEventRecord(b->q.done, st));
  g.enqueued = true;
  g.timed = timed != 0;
  return GH_OK;
}

// Waits for the queue's last run (the last gather or something after it) and reads the
// gather's words.
static int bgather_words(gh_batch* b, const char* who, unsigned int w[8]) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded || !b->g.enqueued) return fail(GH_E_STATE, std::string(who) + ": no gather since the load");
  GH_HIP(hipSetDevice(b->q.device));
  GH_HIP(hipEventSynchronize(b->q.done));
  GH_HIP(hipMemcpy(w, b->g.words.get(), 32, hipMemcpyDeviceToHost));
  return GH_OK;
}

extern "C" int gh_batchdec_gather_wait(gh_batch* b, gh_bgather_report* rep) {
  if (rep) *rep = gh_bgather_report{};
  unsigned int w[8] = {};
  if (int rc = bgather_words(b, "gh_batchdec_gather_wait", w)) return rc;
  float ms = 0;
  if (b->g.timed)
    if (int rc = b->g.ev.elapsed(&ms)) return rc;
  const uint32_t status = w[0] | (w[6] ? (uint32_t)GH_ST_BADCODE : 0u);
  if (rep) {
    std::memcpy(&rep->out_bytes, w + 2, 8);
    rep->npieces = w[1];
    rep->bad_ranges = w[6];
    rep->status = status;
    rep->kernel_ms = ms;
    rep->launches = BATCH_GATHER_LAUNCHES;
  }
  if (status & GH_ST_RANGE) return fail(GH_E_ARG, "batched gather: a range names no stream of the batch or bytes outside [0, n] of its stream");
  if (status & GH_ST_DSTSMALL) return fail(GH_E_SMALL, "batched gather: destination smaller than the ranges' bytes");
  if (status & GH_ST_PIECES) return fail(GH_E_CORRUPT, "batched gather: the plan exceeds the piece bound");
  if (status & GH_ST_BADCODE)
    return fail(GH_E_CORRUPT, std::to_string(w[6]) + " range(s) name a stream the index pass flagged (gh_batch_status "
                                                     "names it); their bytes were left as they were");
  return GH_OK;
}

extern "C" int gh_batchdec_gather(gh_batch* b, const gh_brange* ranges, uint32_t nranges, void* d_dst, uint64_t dst_len,
                                  void* hip_stream, gh_bgather_report* rep) {
  if (rep) *rep = gh_bgather_report{};
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded || !b->indexed)
    return fail(GH_E_STATE, "gh_batchdec_gather without gh_batchdec_index or gh_batch_decode since the load");
  if (nranges == 0) {
    if (rep) rep->launches = BATCH_GATHER_LAUNCHES;
    return GH_OK;
  }
  if (!ranges) return fail(GH_E_ARG, "null argument");
  GH_HIP(hipSetDevice(b->q.device));
  if (b->g.enqueued) GH_HIP(hipEventSynchronize(b->q.done));  // (the last gather may still read the old upload)
  if (int rc = upload_at_least(b->g.ranges, ranges, sizeof(gh_brange) * (uint64_t)nranges)) return rc;
  if (int rc = gh_batchdec_gather_device(b, b->g.ranges.get<gh_brange>(), nranges, d_dst, dst_len, hip_stream, 1)) return rc;
  return gh_batchdec_gather_wait(b, rep);
}

extern "C" int gh_batchdec_gather_pieces(gh_batch* b, gh_gather_piece* pieces, uint64_t cap, uint64_t* npieces) {
  if (!npieces || (cap && !pieces)) return fail(GH_E_ARG, "null argument");
  *npieces = 0;
  unsigned int w[8] = {};
  if (int rc = bgather_words(b, "gh_batchdec_gather_pieces", w)) return rc;
  const uint64_t np = w[1];
  *npieces = np;
  if (np > cap) return fail(GH_E_SMALL, "piece buffer smaller than the plan");
  if (np) GH_HIP(hipMemcpy(pieces, b->g.pieces.get(), np * sizeof(gh_gather_piece), hipMemcpyDeviceToHost));
  return GH_OK;
}

extern "C" int gh_batchdec_kernel_shape(gh_batch* b, char* buf, size_t cap) {
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded) return fail(GH_E_STATE, "gh_batchdec_kernel_shape before a load");
  return copy_name(b->plan.nunits ? bgather_kern_for(b->fb).name : "", buf, cap);
}

extern "C" int gh_batchdec_kernel_shapes(char* buf, size_t cap) {
  return copy_name(std::string(bgather_kern_for(false).name) + "\n" + bgather_kern_for(true).name + "\n", buf, cap);
}

// ---- byte planes (gaphuff.h; kernel: gh_planes_join.hip; layout: gh_planes_layout) -----------
constexpr uint32_t PLANES_JOIN_LAUNCHES = 2;  // the counter's memset, the join kernel

// A member of the batch's queue as the gather is: after the queue's last run, its end the
// queue's `done`.
extern "C" int gh_planes_join_device(gh_batch* b, const gh_planes_item* items, uint32_t ntensors, const void* d_stored,
                                     uint64_t stored_len, void* hip_stream, int timed) {
  if (!b || (ntensors && !items)) return fail(GH_E_ARG, "null argument");
  if (!b->loaded || !b->q.enqueued || !b->own_out)
    return fail(GH_E_STATE, "gh_planes_join_device without a decode into the batch's own arena since the load");
  if ((uintptr_t)d_stored & 15u) return fail(GH_E_ARG, "stored arena not 16-byte aligned");
  std::vector<gh_planes_slot> slots((size_t)PLANES_MAX_E * std::max(ntensors, 1u));
  uint32_t ns = 0;
  uint64_t stored_bytes = 0;
  if (int rc = gh_planes_layout(items, ntensors, slots.data(), &ns, &stored_bytes)) return rc;
  if (ns != b->nstreams) return fail(GH_E_ARG, "the tensors' coded planes are not the loaded batch's streams");
  if (stored_bytes && !d_stored) return fail(GH_E_ARG, "null stored arena");
  if (stored_len < stored_bytes) return fail(GH_E_SMALL, "stored arena smaller than the stored planes");
  // the tensors' descriptors, then their unit prefix, in one upload
  const size_t dbytes = sizeof(PlanesTensor) * (size_t)ntensors;
  std::vector<uint8_t> up(dbytes + 4ull * (ntensors + 1));
  PlanesTensor* d = (PlanesTensor*)up.data();
  std::vector<uint32_t> unit0(ntensors + 1);
  uint64_t units = 0, out_bytes = 0;
  for (uint32_t t = 0; t < ntensors; ++t) {
    const gh_planes_item& it = items[t];
    const std::string who = "tensor " + std::to_string(t) + ": ";
    if (it.nelem && !it.data) return fail(GH_E_ARG, who + "null pointer");
    unit0[t] = (uint32_t)units;
    units += planes_units(it.nelem);
    if (units >= PLANES_MAX_UNITS) return fail(GH_E_ARG, who + "the list reaches 2^31 work units");
    out_bytes += it.nelem * it.elem_size;  // (every nelem is a loaded stream's n or fills a stored plane)
    d[t] = PlanesTensor{};
    d[t].data = (uint8_t*)it.data;
    d[t].nelem = it.nelem;
    d[t].elem = it.elem_size;
    d[t].mask = it.coded_mask;
    for (uint32_t p = 0; p < it.elem_size; ++p) {
      const gh_planes_slot& s = slots[PLANES_MAX_E * t + p];
      d[t].stream[p] = s.stream;
      if (s.stream == GH_PLANES_STORED) {
        d[t].off[p] = s.stored_off;
        continue;
      }
      if (b->n[s.stream] != it.nelem) return fail(GH_E_ARG, who + "nelem differs from its stream's n in the loaded batch");
      d[t].off[p] = b->plan.ext[s.stream].out_off;
    }
  }
  unit0[ntensors] = (uint32_t)units;
  std::memcpy(up.data() + dbytes, unit0.data(), 4ull * (ntensors + 1));
  GH_HIP(hipSetDevice(b->q.device));
  BatchPlanes& pl = b->pl;
  if (int rc = pl.ev.create()) return rc;
  if (pl.enqueued) GH_HIP(hipEventSynchronize(b->q.done));  // (the last join may still read the old upload)
  if (int rc = upload_at_least(pl.desc, up.data(), up.size())) return rc;
  if (int rc = pl.words.reserve(16)) return rc;
  PlanesJoinParams jp{};
  jp.desc = pl.desc.get<PlanesTensor>();
  jp.unit0 = (const uint32_t*)(pl.desc.get<uint8_t>() + dbytes);
  jp.out = b->out.get<uint8_t>();
  jp.stored = (const uint8_t*)d_stored;
  jp.status = b->flags.get<unsigned int>() + 4;
  jp.bad = pl.words.get<unsigned int>();
  jp.ntensors = ntensors;
  jp.nunits = (uint32_t)units;
  // GH_PLANES_GRID=k (tests): k workgroups, so that one wave walks many units and tensors
  const uint32_t grid = unit_grid("GH_PLANES_GRID", units, PJ_WAVES, b->q.num_cu);
  void* ja[1] = {&jp};
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)b->q.stream;
  GH_HIP(hipStreamWaitEvent(st, b->q.done, 0));
  GH_HIP(hipMemsetAsync(pl.words.get(), 0, 16, st));
  if (timed) GH_HIP(hipEventRecord(pl.ev.a, st));  // (the join alone)
  if (units) GH_HIP(hipLaunchKernel((const void*)gh_planes_join_kernel, dim3(grid), dim3(PJ_TB), ja, 0, st));
  GH_HIP(hipGetLastError());
  if (timed) GH_HIP(hipEventRecord(pl.ev.b, st));
  GH_HIP(hipEventRecord(b->q.done, st));
  pl.enqueued = true;
  pl.timed = timed != 0;
  pl.out_bytes = out_bytes;
  pl.ntensors = ntensors;
  return GH_OK;
}

extern "C" int gh_planes_wait(gh_batch* b, gh_planes_report* rep) {
  if (rep) *rep = gh_planes_report{};
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded || !b->pl.enqueued) return fail(GH_E_STATE, "gh_planes_wait without a join since the load");
  GH_HIP(hipSetDevice(b->q.device));
  GH_HIP(hipEventSynchronize(b->q.done));
  unsigned int bad = 0;
  GH_HIP(hipMemcpy(&bad, b->pl.words.get(), sizeof(bad), hipMemcpyDeviceToHost));
  float ms = 0;
  if (b->pl.timed)
    if (int rc = b->pl.ev.elapsed(&ms)) return rc;
  if (rep) {
    rep->out_bytes = b->pl.out_bytes;
    rep->ntensors = b->pl.ntensors;
    rep->bad_tensors = bad;
    rep->kernel_ms = ms;
    rep->launches = PLANES_JOIN_LAUNCHES;
  }
  if (bad)
    return fail(GH_E_CORRUPT, std::to_string(bad) + " tensor(s) have a coded plane the decode flagged (gh_batch_status "
                                                    "names its stream); their bytes were left as they were");
  return GH_OK;
}

// ---- element gather (gaphuff.h; kernels: gh_planes_gather.hip; arithmetic: gh_planes_gather.hpp) ----
// memset, locate, scan, expand; the batched gather's five; the range join
constexpr uint32_t PGATHER_LAUNCHES = 4 + BATCH_GATHER_LAUNCHES + 1;
static_assert(PGATHER_LAUNCHES == GH_PGATHER_LAUNCHES, "the header states the launch count");
constexpr uint32_t PGATHER_WORDS = 16;

// A member of the batch's queue as the batched gather is, which it runs between its own kernels.
extern "C" int gh_pgather_device(gh_batch* b, const gh_planes_item* items, uint32_t ntensors, const void* d_stored,
                                 uint64_t stored_len, const gh_erange* d_ranges, uint32_t nranges, void* d_dst,
                                 uint64_t dst_len, void* hip_stream, int timed) {
  if (!b || (ntensors && !items)) return fail(GH_E_ARG, "null argument");
  if (!b->loaded || !b->indexed)
    return fail(GH_E_STATE, "gh_pgather_device without gh_batchdec_index or gh_batch_decode since the load");
  if (nranges == 0) return GH_OK;
  if ((uintptr_t)d_stored & 15u) return fail(GH_E_ARG, "stored arena not 16-byte aligned");
  std::vector<PlanesTensor> desc;
  uint32_t ns = 0, maxc = 0;
  uint64_t stored_bytes = 0;
  if (int rc = pgather_descs(items, ntensors, desc, &ns, &stored_bytes, &maxc)) return rc;
  if (ns != b->nstreams) return fail(GH_E_ARG, "the tensors' coded planes are not the loaded batch's streams");
  if (stored_bytes && !d_stored) return fail(GH_E_ARG, "null stored arena");
  if (stored_len < stored_bytes) return fail(GH_E_SMALL, "stored arena smaller than the stored planes");
  for (uint32_t t = 0; t < ntensors; ++t)
    for (uint32_t p = 0; p < items[t].elem_size; ++p)
      if (desc[t].stream[p] != GH_PLANES_STORED && b->n[desc[t].stream[p]] != items[t].nelem)
        return fail(GH_E_ARG, "tensor " + std::to_string(t) + ": nelem differs from its stream's n in the loaded batch");
  if (!d_ranges || !d_dst) return fail(GH_E_ARG, "null argument");
  if (nranges > PG_MAX_RANGES) return fail(GH_E_ARG, "gh_pgather_device: more than 2^21 ranges in one call");
  // a plan that stands has at most this many units: every range ceil(len / 1024), the lens' bytes within dst_len
  const uint64_t unit_bound = (uint64_t)nranges + dst_len / PLANES_UNIT_ELEMS;
  if (unit_bound >= PLANES_MAX_UNITS) return fail(GH_E_ARG, "gh_pgather_device: the destination reaches 2^31 work units");
  GH_HIP(hipSetDevice(b->q.device));
  BatchPGather& pg = b->pg;
  if (int rc = pg.ev_x.create()) return rc;
  if (int rc = pg.ev_j.create()) return rc;
  // the host does not know how many byte ranges the device will cut: the inner gather gets this
  // many slots, the ones past the device's count empty
  const uint64_t nslots = (uint64_t)maxc * nranges;
  const size_t dbytes = sizeof(PlanesTensor) * (size_t)ntensors;
  const bool same_desc = pg.last_desc.size() == dbytes && (!dbytes || !std::memcmp(pg.last_desc.data(), desc.data(), dbytes));
  // The staging buffer: dst_len bytes hold every staged plane (C <= E).  No padding past it: a
  // lane loads 16 bytes only where all 16 lie inside its range's plane, every other lane byte by byte.
  const uint64_t per_bytes = (sizeof(PgLoc) + 24ull) * nranges + 8;  // loc, stage_off, dst_off (u64), slot, unit0 (u32; unit0 has nranges + 1)
  if (!same_desc || pg.staging.capacity() < std::max<uint64_t>(dst_len, 16) || pg.per.capacity() < per_bytes ||
      pg.branges.capacity() < std::max<uint64_t>(nslots * sizeof(gh_brange), 16) || !pg.words) {
    if (b->q.enqueued) GH_HIP(hipEventSynchronize(b->q.done));  // the last gather in flight uses the old buffers
    if (!same_desc) {
      pg.last_desc.clear();
      if (int rc = upload_at_least(pg.desc, desc.data(), dbytes)) return rc;
      pg.last_desc.assign((const uint8_t*)desc.data(), (const uint8_t*)desc.data() + dbytes);
    }
    if (int rc = pg.staging.reserve(std::max<uint64_t>(dst_len, 16))) return rc;
    if (int rc = pg.per.reserve(per_bytes)) return rc;
    if (int rc = pg.branges.reserve(std::max<uint64_t>(nslots * sizeof(gh_brange), 16))) return rc;
    if (int rc = pg.words.reserve(4 * PGATHER_WORDS)) return rc;
  }
  PgatherParams pp{};
  pp.ranges = d_ranges;
  pp.desc = pg.desc.get<PlanesTensor>();
  pp.stream_status = b->flags.get<unsigned int>() + 4;
  pp.branges = pg.branges.get<gh_brange>();
  pp.loc = pg.per.get<PgLoc>();
  pp.stage_off = (unsigned long long*)(pp.loc + nranges);
  pp.dst_off = pp.stage_off + nranges;
  pp.slot = (uint32_t*)(pp.dst_off + nranges);
  pp.unit0 = pp.slot + nranges;
  pp.words = pg.words.get<unsigned int>();
  pp.stage = pg.staging.get<uint8_t>();
  pp.stored = (const uint8_t*)d_stored;
  pp.dst = (uint8_t*)d_dst;
  pp.dst_len = dst_len;
  pp.nslots = nslots;
  pp.nranges = nranges;
  pp.ntensors = ntensors;
  const uint32_t grid_r = (uint32_t)ceil_div((uint64_t)nranges, (uint64_t)GP_TB);
  void* pa[1] = {&pp};
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)b->q.stream;
  GH_HIP(hipStreamWaitEvent(st, b->q.done, 0));  // (indexed: the queue has a run)
  if (timed) GH_HIP(hipEventRecord(pg.ev_x.a, st));
  GH_HIP(hipMemsetAsync(pp.words, 0, 4 * PGATHER_WORDS, st));
  GH_HIP(hipLaunchKernel((const void*)gh_pgather_locate_kernel, dim3(grid_r), dim3(GP_TB), pa, 0, st));
  GH_HIP(hipLaunchKernel((const void*)gh_pgather_scan_kernel, dim3(1), dim3(PGS_TB), pa, 0, st));
  GH_HIP(hipLaunchKernel((const void*)gh_pgather_expand_kernel, dim3(grid_r), dim3(GP_TB), pa, 0, st));
  GH_HIP(hipGetLastError());
  if (timed) GH_HIP(hipEventRecord(pg.ev_x.b, st));
  GH_HIP(hipEventRecord(b->q.done, st));
  // (a list without coded planes has no slot and no inner gather: its status word is words[8], zero)
  if (nslots)
    if (int rc = gh_batchdec_gather_device(b, pp.branges, (uint32_t)nslots, pg.staging.get(), dst_len, st, timed)) return rc;
  pp.inner_status = nslots ? b->g.words.get<unsigned int>() : pp.words + 8;
  // GH_PLANES_GRID=k (tests): k workgroups, so that one wave walks many units and ranges
  const uint32_t grid = unit_grid("GH_PLANES_GRID", unit_bound, PJ_WAVES, b->q.num_cu);
  if (timed) GH_HIP(hipEventRecord(pg.ev_j.a, st));
  GH_HIP(hipLaunchKernel((const void*)gh_pgather_join_kernel, dim3(grid), dim3(PJ_TB), pa, 0, st));
  GH_HIP(hipGetLastError());
  if (timed) GH_HIP(hipEventRecord(pg.ev_j.b, st));
  GH_HIP(hipEventRecord(b->q.done, st));
  pg.enqueued = true;
  pg.timed = timed != 0;
  pg.nslots = nslots;
  return GH_OK;
}

extern "C" int gh_pgather_wait(gh_batch* b, gh_pgather_report* rep) {
  if (rep) *rep = gh_pgather_report{};
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded || !b->pg.enqueued) return fail(GH_E_STATE, "gh_pgather_wait without an element gather since the load");
  GH_HIP(hipSetDevice(b->q.device));
  GH_HIP(hipEventSynchronize(b->q.done));
  unsigned int w[PGATHER_WORDS] = {}, iw[8] = {};
  GH_HIP(hipMemcpy(w, b->pg.words.get(), sizeof(w), hipMemcpyDeviceToHost));
  if (b->pg.nslots) GH_HIP(hipMemcpy(iw, b->g.words.get(), sizeof(iw), hipMemcpyDeviceToHost));
  float all = 0, ex = 0, jo = 0;
  if (b->pg.timed) {
    GH_HIP(hipEventElapsedTime(&all, b->pg.ev_x.a, b->pg.ev_j.b));
    if (int rc = b->pg.ev_x.elapsed(&ex)) return rc;
    if (int rc = b->pg.ev_j.elapsed(&jo)) return rc;
  }
  // (the inner gather's range and size refusals follow this gather's own: its plan is this one's)
  const uint32_t status = w[0] | (iw[0] & (uint32_t)GH_ST_PIECES) | (w[6] ? (uint32_t)GH_ST_BADCODE : 0u);
  if (rep) {
    if (!(w[0] & GH_ST_RANGE)) std::memcpy(&rep->out_bytes, w + 2, 8);
    rep->npieces = iw[1];
    rep->bad_ranges = w[6];
    rep->status = status;
    rep->kernel_ms = all;
    rep->launches = PGATHER_LAUNCHES;
    rep->expand_ms = ex;
    rep->join_ms = jo;
  }
  if (status & GH_ST_RANGE) return fail(GH_E_ARG, "element gather: a range names no tensor of the list or elements outside [0, nelem] of its tensor");
  if (status & GH_ST_DSTSMALL) return fail(GH_E_SMALL, "element gather: destination smaller than the ranges' bytes");
  if (status & GH_ST_PIECES) return fail(GH_E_CORRUPT, "element gather: the inner plan exceeds the piece bound");
  if (status & GH_ST_BADCODE)
    return fail(GH_E_CORRUPT, std::to_string(w[6]) + " range(s) name a tensor with a coded plane the index pass flagged "
                                                     "(gh_batch_status names its stream); their bytes were left as they were");
  return GH_OK;
}

extern "C" int gh_pgather(gh_batch* b, const gh_planes_item* items, uint32_t ntensors, const void* d_stored,
                          uint64_t stored_len, const gh_erange* ranges, uint32_t nranges, void* d_dst, uint64_t dst_len,
                          void* hip_stream, gh_pgather_report* rep) {
  if (rep) *rep = gh_pgather_report{};
  if (!b) return fail(GH_E_ARG, "null batch");
  if (!b->loaded || !b->indexed)
    return fail(GH_E_STATE, "gh_pgather without gh_batchdec_index or gh_batch_decode since the load");
  if (nranges && !ranges) return fail(GH_E_ARG, "null argument");
  GH_HIP(hipSetDevice(b->q.device));
  if (b->pg.enqueued) GH_HIP(hipEventSynchronize(b->q.done));  // (the last gather may still read the old upload)
  if (int rc = upload_at_least(b->pg.ranges, ranges, sizeof(gh_erange) * (uint64_t)nranges)) return rc;
  if (int rc = gh_pgather_device(b, items, ntensors, d_stored, stored_len, b->pg.ranges.get<gh_erange>(), nranges, d_dst,
                                 dst_len, hip_stream, 1))
    return rc;
  if (nranges == 0) {
    if (rep) rep->launches = PGATHER_LAUNCHES;
    return GH_OK;
  }
  return gh_pgather_wait(b, rep);
}

// Decode time of a set of shards: decodes on one device run in turn (DevChain), so a
// device's time is the sum of its shards' kernel times; devices run side by side.
static float shards_kernel_ms(const std::vector<gh_ctx*>& ctx, const std::vector<gh_report>& reps) {
  std::map<int, float> per_dev;
  for (size_t k = 0; k < ctx.size(); ++k) per_dev[ctx[k]->device] += reps[k].kernel_ms;
  float worst = 0;
  for (auto& d : per_dev) worst = std::max(worst, d.second);
  return worst;
}

// Runs f(k) for every shard k in its own host thread (one shard alone: inline);
// returns the first failure's code with its message moved to the calling thread.
template <class F>
static int for_each_shard(int n, F f) {
  if (n == 1) return f(0);
  std::vector<int> rc(n, GH_OK);
  std::vector<std::string> msg(n);
  std::vector<std::thread> th;
  for (int k = 0; k < n; ++k)
    th.emplace_back([&, k] {
      rc[k] = f(k);
      if (rc[k]) msg[k] = gh_last_error();
    });
  for (auto& t : th) t.join();
  for (int k = 0; k < n; ++k)
    if (rc[k]) {
      set_error(msg[k]);
      return rc[k];
    }
  return GH_OK;
}

extern "C" int gh_decode(const gh_stream* s, uint8_t* out, uint64_t out_len, const gh_opts* o,
                         gh_report* rep) {
  if (!s || (s->n && !out)) return fail(GH_E_ARG, "null argument");
  if (out_len < s->n) return fail(GH_E_SMALL, "output buffer smaller than N");
  int rc = gh_stream_validate(s);
  if (rc) return rc;
  const int ng = (o && o->ngpus > 1) ? o->ngpus : 1;
  const int reps = (o && o->reps > 1) ? o->reps : 1;
  std::vector<uint64_t> bounds(ng + 1);
  gh_plan_shards(s->g, (uint32_t)ng, bounds.data());
  std::vector<gh_ctx*> ctx(ng, nullptr);
  auto cleanup = [&]() {
    for (auto* c : ctx) gh_ctx_destroy(c);
  };
  // Phase 1, one host thread per shard: context, H2D of the shard's words (pinned,
  // double-buffered: the shards' PCIe transfers overlap across devices), the decodes
  // (chained per device), the report.  The reference loads, decodes and downloads one
  // device at a time (decoder.cu:759-801).
  std::vector<gh_report> reps_k(ng);
  rc = for_each_shard(ng, [&](int k) {
    const int dev = (o && o->devices) ? o->devices[k] : (ng > 1 ? k : 0);
    int r = gh_ctx_create(dev, &ctx[k]);
    if (!r) r = gh_ctx_load(ctx[k], s, bounds[k], bounds[k + 1], ng > 1 ? 0 : s->n);
    for (int i = 0; i < reps && !r; ++i) r = gh_ctx_decode(ctx[k], nullptr, 1);
    if (!r) r = gh_ctx_report(ctx[k], nullptr, &reps_k[k]);
    return r;
  });
  if (rc) {
    cleanup();
    return rc;
  }
  // output offsets: exclusive scan of the shards' symbol counts
  std::vector<uint64_t> offs(ng + 1, 0), want(ng, 0);
  uint32_t status = 0;
  for (int k = 0; k < ng; ++k) {
    status |= reps_k[k].status;
    if (k + 1 < ng && reps_k[k].symbols > reps_k[k].out_bytes) {
      cleanup();
      return fail(GH_E_CORRUPT, "shard produced more symbols than its output capacity");
    }
    want[k] = (offs[k] < s->n) ? std::min<uint64_t>(reps_k[k].symbols, s->n - offs[k]) : 0;
    offs[k + 1] = offs[k] + reps_k[k].symbols;
  }
  const uint64_t offset = offs[ng];
  // Phase 2, one host thread per shard: D2H into the caller's buffer at its offset.
  rc = for_each_shard(ng, [&](int k) { return want[k] ? gh_ctx_download(ctx[k], 0, out + offs[k], want[k]) : GH_OK; });
  const float dec_ms = shards_kernel_ms(ctx, reps_k);
  cleanup();
  if (rc) return rc;
  if (rep) {
    *rep = reps_k[0];
    rep->symbols = offset;
    rep->out_bytes = std::min<uint64_t>(offset, s->n);
    rep->status = status;
    rep->kernel_ms = dec_ms;
  }
  if (status & GH_ST_TIMEOUT) return fail(GH_E_HIP, "look-back timed out");
  if (status & GH_ST_OFFSETS) return fail(GH_E_HIP, "a piece disagreed with the recorded piece offsets");
  if (offset < s->n) return fail(GH_E_CORRUPT, "stream decoded to fewer than N symbols");
  if (status & GH_ST_BADCODE) return fail(GH_E_CORRUPT, "invalid code in stream");
  return GH_OK;
}
