/*
 * gaphuff.h — C ABI of the MI355X-native gap-array Huffman codec.
 *
 * This is the drop-in boundary for the reference's decode path
 * (dek226/CSE375-FinalProj-Huffman-Decoding, Huffman_coding_Gap_arrays/):
 *
 *   reference                                   replaced by
 *   ------------------------------------------  --------------------------------------
 *   decoder/src/huff.cpp:36-100  (header+table   gh_stream_parse()  — parses v1/v2 files
 *        parse, fread of gap words + payload)
 *   decoder/src/get_table.cpp:3-139              built inside the library from the
 *        (get_table_info / get_twolevel_table)   (symbol,length) list (see gh_ctx_load)
 *   decoder/include/decoder.cuh:4-15             gh_decode()        — one-shot decode
 *        decoder_l1_l2(input, W, output, N, G,   gh_ctx_*()         — device-resident
 *        dectable, tablesize, prefix_bit, S,                          decode (bench/CLI)
 *        TableInfo)   [decoder.cu:732-815]
 *   decoder.cu:454-730 gpu_dec_l1_l2 kernel      HIP kernel gh_decode_kernel (gfx950)
 *   parallel_cpu_prescan.cpp:423-483             gh_decode() (count+scan on the GPU)
 *   gpuhd/src/cuhd_gpu_decoder.cu:16-523         (same kernel; self-sync format: next;
 *        and its gpuhd-gapArray / gpuhd-multigpu copies)
 *   encoder/src/huff.cpp:30-220 (+encoder.cu,    gh_encode_plan()/gh_encode_write()
 *        package_merge.cpp, symbols.cpp)          (host encoder of the same format)
 *   generate.cpp:11-58                           gh_generate()      — seeded generator
 *
 * Conventions: plain C types only; every entry point returns 0 (GH_OK) or a
 * negative GH_E_* code and never exits the process (the reference calls exit()
 * via CUERROR/fatal, decoder.cu:14-20, huff.cpp:11-14).  Buffers are owned by the
 * caller unless stated.  A gh_ctx is bound to one HIP device and must be used from
 * one host thread at a time.
 */
#ifndef GAPHUFF_H_
#define GAPHUFF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GH_ABI_VERSION 1

/* ---- status codes ---------------------------------------------------------- */
#define GH_OK 0
#define GH_E_ARG -1       /* bad argument / NULL pointer / out-of-range shard      */
#define GH_E_FORMAT -2    /* malformed compressed.huff header or sizes             */
#define GH_E_TABLE -3     /* (symbol,length) list is not a valid canonical code     */
#define GH_E_HIP -4       /* HIP runtime error                                      */
#define GH_E_NODEV -5     /* no usable gfx950 device                                */
#define GH_E_NOMEM -6     /* host or device allocation failed                       */
#define GH_E_CORRUPT -7   /* stream decoded to fewer symbols than N, or bad code    */
#define GH_E_STATE -8     /* context used out of order                              */
#define GH_E_SMALL -9     /* caller buffer too small                                */

/* ---- constants of the on-disk format (reference constants.hpp) ------------- */
#define GH_SEGMENT_BITS 128   /* decoder/include/constants.hpp:9  SEGMENT_SIZE       */
#define GH_GAPS_PER_WORD 8    /* constants.hpp:22  GAP_FAC_NUM (4-bit gaps per u32)  */
#define GH_MAX_CODE_LEN 16    /* constants.hpp:5   MAX_CODEWORD_LENGTH               */
#define GH_MAX_SYMBOLS 256    /* constants.hpp:6   MAX_CODE_NUM                      */
/* v2 header magic ("GAPHUF2\0" little-endian); a v1 file starts with u64 S <= 256 */
#define GH_V2_MAGIC 0x0032465548504147ull

/* One header entry: reference struct Symbol{symbol,length} as written by
 * encoder/src/huff.cpp:189-194 (most frequent symbol first). */
typedef struct gh_sym {
  uint8_t symbol;
  uint8_t length;
} gh_sym;

/* A parsed compressed stream.  All pointers are views (no ownership). */
typedef struct gh_stream {
  const gh_sym* syms;         /* nsyms entries, file order                         */
  uint32_t nsyms;             /* S                                                 */
  uint32_t version;           /* 1 = reference v1 header, 2 = 64-bit v2 header     */
  uint64_t n;                 /* original bytes N (decoder/src/huff.cpp:83)        */
  uint64_t w;                 /* payload u32 words W (huff.cpp:85)                 */
  uint64_t g;                 /* 128-bit segments G (huff.cpp:87)                  */
  const uint32_t* gap_words;  /* ceil(G/8) words, 4-bit gaps LSB-first             */
  const uint32_t* payload;    /* W words, codewords MSB-first within each word     */
} gh_stream;

/* ---- format ----------------------------------------------------------------- */
/* Parse a whole compressed.huff image (v1 or v2).  The stream's pointers alias
 * `file`.  Validates sizes (W in [4G-3,4G], lengths 1..16, Kraft sum <= 1). */
int gh_stream_parse(const void* file, size_t file_len, gh_stream* out);
/* Validate a stream's code table (canonical order, lengths, distinct symbols). */
int gh_stream_validate(const gh_stream* s);

/* ---- encoder (host; reference encoder/src/huff.cpp:30-220) ------------------ */
typedef struct gh_encode_plan {
  uint64_t n;                       /* input bytes                                  */
  uint64_t bits;                    /* total code bits = sum len*count              */
  uint64_t w, g;                    /* payload words, segments                      */
  uint64_t file_bytes;              /* size of the compressed image                 */
  uint32_t nsyms;                   /* distinct symbols                             */
  uint32_t version;                 /* 1 or 2 (v2 when N, W or G >= 2^31)           */
  gh_sym syms[GH_MAX_SYMBOLS];      /* file order, most frequent first              */
  uint32_t code[GH_MAX_SYMBOLS];    /* canonical code per byte value                */
  uint8_t len[GH_MAX_SYMBOLS];      /* code length per byte value (0 = absent)      */
  uint64_t count[GH_MAX_SYMBOLS];   /* histogram                                    */
} gh_encode_plan;
/* Histogram + boundary package-merge (length limit 16) + canonical codes.
 * threads <= 0 selects all hardware threads.  force_version 0 = automatic. */
int gh_encode_plan_make(const uint8_t* in, uint64_t n, int threads, int force_version,
                        gh_encode_plan* plan);
/* Write the compressed image (plan->file_bytes bytes) into `out`. */
int gh_encode_write(const uint8_t* in, const gh_encode_plan* plan, int threads,
                    void* out, uint64_t out_len);
/* The plan from a histogram alone (plan->n = the sum of the counts): the same plan as
 * gh_encode_plan_make on any data with that histogram.  Counts may be sums over the
 * slices of a stream that no single caller holds. */
int gh_encode_plan_from_counts(const uint64_t counts[256], int force_version, gh_encode_plan* plan);
/* Largest file_bytes any input of n bytes can have (16-bit codes, 256 symbols, a v2
 * header): a buffer to allocate before the plan exists. */
uint64_t gh_encode_bound(uint64_t n);

/* ---- sliced encode: a stream built slice by slice ---------------------------- */
/* A codeword's bits depend only on its first bit, and a gap nibble only on the codeword
 * that crosses a 128-bit boundary, so a contiguous run of input bytes (a slice) is
 * encoded on its own once the stream-wide plan and the slice's first bit are known.
 * Under the stream's plan a slice holds code bits [base_bit, base_bit + bits), base_bit
 * being the bit total of everything before it.  Its output is slice-local: the payload
 * words [word0, word0 + nwords) and the gap words [gapw0, gapw0 + ngapw) it touches,
 * with every bit that belongs to a neighbour zero.  ORing all slices' outputs into an
 * image prepared by gh_encode_image_init gives exactly gh_encode_write's bytes for the
 * whole input.  No reference counterpart (the reference encodes whole inputs only). */
typedef struct gh_slice {
  uint64_t base_bit, bits;   /* code bits [base_bit, base_bit + bits)                   */
  uint64_t word0, nwords;    /* payload words: base_bit >> 5 up to
                                ceil((base_bit + bits) / 32); nwords = 0 when bits = 0  */
  uint64_t gapw0, ngapw;     /* gap words: base_bit >> 10 up to the word of bit
                                base_bit + bits - 1, inclusive; ngapw = 0 when bits = 0 */
} gh_slice;
/* The extents of bits [base_bit, base_bit + bits).  GH_E_ARG: null out, or the sum
 * overflows 64 bits. */
int gh_slice_extent(uint64_t base_bit, uint64_t bits, gh_slice* out);
/* Host encoder of one slice: the n bytes at `in` as the slice at base_bit of the stream
 * planned by stream_plan.  Writes out->nwords words and out->ngapw gap words, indexed
 * from out->word0 and out->gapw0 (words[0] is payload word word0).  The buffers do not
 * depend on `threads`.  GH_E_TABLE: a byte of the slice has length 0 in the plan;
 * GH_E_ARG: null pointers, base_bit + bits > plan->bits; GH_E_SMALL: words_cap <
 * nwords or gaps_cap < ngapw (counted in u32) -- *out is filled all the same, so a first
 * call with caps of 0 sizes the buffers (words and gapw may then be NULL). */
int gh_encode_slice(const uint8_t* in, uint64_t n, const gh_encode_plan* stream_plan, uint64_t base_bit,
                    int threads, uint32_t* words, uint64_t words_cap, uint32_t* gapw, uint64_t gaps_cap,
                    gh_slice* out);
/* Header of the stream into image[0 .. ), gap and payload words zeroed: the image every
 * slice is merged into.  GH_E_SMALL when image_len < plan->file_bytes. */
int gh_encode_image_init(const gh_encode_plan* plan, void* image, uint64_t image_len);
/* OR one slice's words and gap words into the image (any alignment; the word area starts
 * 8 + 2 S + 12 bytes into a v1 file).  Slices may be merged in any order, but merges
 * into one image must not run concurrently: neighbouring slices share their edge words.
 * GH_E_ARG: null pointers, extents outside the plan's W words / ceil(G / 8) gap words;
 * GH_E_SMALL: image_len < plan->file_bytes. */
int gh_slice_merge(void* image, uint64_t image_len, const gh_encode_plan* plan, const gh_slice* slice,
                   const uint32_t* words, const uint32_t* gapw);

/* Code lengths only: boundary package-merge over `nsyms` counts sorted ascending
 * (stable), restating encoder/src/package_merge.cpp:107-166; lengths written in
 * the same (ascending-count) order. */
int gh_package_merge(const uint64_t* sorted_counts, uint32_t nsyms, uint8_t* lengths);
/* gh_package_merge's lengths by the level-by-level form the GPU uses (same arguments, same
 * result for every input; tests/test_pm_flat.py).  Needs no device. */
int gh_package_merge_flat(const uint64_t* sorted_counts, uint32_t nsyms, uint8_t* lengths);

/* ---- synthetic input (reference generate.cpp:32-47, seeded) ----------------- */
/* Byte i: with probability `redundancy` 'A'+U{0..3}, else U{0..255}; counter-based
 * PRNG keyed by (seed, i) so any [offset, offset+n) slice is reproducible. */
int gh_generate(uint64_t seed, double redundancy, uint64_t offset, uint64_t n,
                uint8_t* out, int threads);

/* ---- GPU encoder ------------------------------------ */
/* Replaces the reference's GPU encoder: histogram (encoder/src/encoder.cu:118-140),
 * cuencoder (:142-355) and cu_get_gaparray (:358-379) behind encoder/src/huff.cpp:
 * 30-220.  The image is byte-identical to gh_encode_write's.  The code lengths are
 * built on the host (package-merge) from the GPU histogram.  An encoder context is
 * bound to one gfx950 device; no CPU fallback. */
typedef struct gh_ectx gh_ectx;
int gh_ectx_create(int device, gh_ectx** out);
int gh_ectx_destroy(gh_ectx* ctx);
/* Copy n input bytes to the device (kept resident across plan/encode calls). */
int gh_ectx_load(gh_ectx* ctx, const uint8_t* in, uint64_t n);
/* GPU histogram + host package-merge; fills *plan (may be NULL). */
int gh_ectx_plan(gh_ectx* ctx, int force_version, gh_encode_plan* plan);
/* Encode the loaded input on the device; kernel_ms (may be NULL): event time of the
 * encode kernels, input already resident. */
int gh_ectx_encode(gh_ectx* ctx, float* kernel_ms);
/* Header + gap words + payload words into out (plan->file_bytes bytes). */
int gh_ectx_download(gh_ectx* ctx, void* out, uint64_t out_len);
/* Sliced encode on the device (see "sliced encode" above): the loaded input is one slice
 * of a longer stream.
 * gh_ectx_counts: the GPU histogram of the loaded input, as gh_ectx_plan runs it; no plan
 * is made, and a following gh_ectx_encode needs a fresh gh_ectx_plan.  The counts of all
 * slices, summed, go to gh_encode_plan_from_counts. */
int gh_ectx_counts(gh_ectx* ctx, uint64_t counts[256]);
/* Encode the loaded input as the slice at base_bit of the stream planned by stream_plan.
 * The slice's bit total comes from its own histogram (taken here when gh_ectx_counts has
 * not run since the load).  *out (may be NULL): the extents.  kernel_ms as in
 * gh_ectx_encode.  Errors as gh_encode_slice's: GH_E_TABLE, GH_E_ARG. */
int gh_ectx_encode_slice(gh_ectx* ctx, const gh_encode_plan* stream_plan, uint64_t base_bit, gh_slice* out,
                         float* kernel_ms);
/* The slice's words and gap words to host memory, laid out as gh_encode_slice lays them
 * out.  GH_E_STATE unless the context's last encode was a slice encode; GH_E_SMALL: a cap
 * (in u32) is too small.  After a slice encode gh_ectx_download and gh_ectx_index return
 * GH_E_STATE: the context holds no whole image, and the seek index of a sliced stream is
 * made of its slices' entries (gh_ectx_index_slice below) or is gh_encode_index's. */
int gh_ectx_download_slice(gh_ectx* ctx, uint32_t* words, uint64_t words_cap, uint32_t* gapw,
                           uint64_t gaps_cap);
/* Slices from and to device memory: with gh_ectx_index_slice, a stream is encoded slice by
 * slice, merged, loaded into a gh_ctx (gh_ctx_load_device) and gathered from with no byte
 * of input, payload or gap array crossing to the host.
 * gh_ectx_load_device: gh_ectx_load with a device source (any address the context's device
 * can read).  The n bytes are copied into the context's own padded input buffer (the
 * kernels load unconditionally past n, so a borrowed pointer would need the caller to
 * pad): device to device on the context's stream, after an event recorded on hip_stream
 * (NULL: the default stream), so a producer kernel enqueued there has finished first.
 * Synchronous; the same state reset as gh_ectx_load. */
int gh_ectx_load_device(gh_ectx* ctx, const void* d_in, uint64_t n, void* hip_stream);
/* OR the context's last encode (a slice, or a whole encode: the slice at bit 0) into
 * caller-owned arrays on the context's device, laid out as gh_ctx_load_device takes them:
 * payload word w of the stream at d_payload[w] (payload_words in all), gap word j at
 * d_gap_words[j] (gap_words in all).  The caller zeroes both before the first merge.
 * gh_enc_merge_kernel stores the slice's interior words plainly and ORs its first and last
 * payload word and first and last gap word, the only words a neighbour can share, with
 * device-scope atomics: merges of different contexts of ONE device into one destination
 * may overlap on different streams, in any order.  Merges issued from DIFFERENT devices
 * into one destination must be ordered by the caller (each finished before the next
 * starts): atomicity across devices is not relied on and was not measured.  Waits for the
 * context's encode, runs on hip_stream (NULL: the context's stream) and returns when done.
 * GH_E_STATE before an encode; GH_E_ARG: a null array with a non-empty extent, the slice's
 * extents past payload_words / gap_words, d_payload or d_gap_words not 16-byte aligned. */
int gh_ectx_merge_device(gh_ectx* ctx, uint32_t* d_payload, uint64_t payload_words,
                         uint32_t* d_gap_words, uint64_t gap_words, void* hip_stream);
/* The encode's write kernel is one of 14 template instantiations, named
 * "enc_write<NSW,slice=0|1>": NSW in {1, 2, 3, 4, 5, 6, 9} payload stores per thread and
 * chunk, picked from the input's code bits per byte; slice=1 for gh_ectx_encode_slice.
 * gh_ectx_kernel_shape: the name the context's last gh_ectx_encode / gh_ectx_encode_slice
 * picked, NUL-terminated into buf[0..cap); empty for an empty input.  GH_E_SMALL when cap
 * is too small, GH_E_STATE before an encode (or after a later load or plan). */
int gh_ectx_kernel_shape(gh_ectx* ctx, char* buf, size_t cap);
/* Every name an encode can pick, one per line.  Needs no device. */
int gh_enc_kernel_shapes(char* buf, size_t cap);
/* The name the picker returns for an input of n bytes and `bits` code bits, a whole stream
 * (slice = 0) or a slice (slice = 1); empty for n = 0.  Host arithmetic only, no device.
 * GH_E_ARG: slice not 0 or 1, bits > 16 n; GH_E_SMALL when cap is too small. */
int gh_enc_kernel_shape_for(uint64_t n, uint64_t bits, int slice, char* buf, size_t cap);

/* ---- GPU decoder -------------------------------------------------------------- */
typedef struct gh_ctx gh_ctx;

typedef struct gh_report {
  uint64_t symbols;        /* symbols decoded by the loaded shard (incl. padding)  */
  uint64_t out_bytes;      /* bytes written to the shard's device output           */
  uint32_t status;         /* device status bits (GH_ST_*)                          */
  uint32_t lut_bits;       /* K of the decode lookup table (write table: wave split) */
  uint32_t grid;           /* workgroups launched (write kernel in split mode)      */
  uint32_t tiles;          /* segment tiles in the shard                            */
  float kernel_ms;         /* average time of one decode (all its kernels), events  */
  uint32_t launches;       /* decodes averaged in kernel_ms                         */
  uint32_t mode;           /* GH_MODE_SPLIT, GH_MODE_TILE or GH_MODE_MTILE          */
  uint32_t path;           /* GH_PATH_*: table / decode-loop variant                */
  uint64_t slow_lookbacks; /* tile mode: prefix reads that had to poll              */
} gh_report;

#define GH_MODE_SPLIT 1u    /* wave split: count, scan and write kernels (gh_wsplit.hip) */
#define GH_MODE_TILE 2u     /* persistent tile kernel, round-leader prefixes (gh_tile.hip) */
#define GH_MODE_FUSED 3u    /* reserved: the fused count + write tile kernel (removed)    */
#define GH_MODE_MTILE 4u    /* two-pass tile kernel: count and write over register-resident
                               words, one payload read (gh_mtile.hip) */
#define GH_PATH_GROUPED 2u  /* one codeword per lookup, grouped window shifts (tile kernel) */
#define GH_PATH_MULTI_WAVE 4u /* up to four codewords per lookup, canonical fallback for
                                 longer or incomplete codes (wave split) */
#define GH_PATH_MULTI_TILE 8u /* up to four codewords per lookup, start masks (two-pass tile) */
/* (values 0, 1, 3 were retired structures; they are no longer reported) */

#define GH_ST_BADCODE 1u    /* a bit pattern outside the code space was met       */
#define GH_ST_TIMEOUT 2u    /* look-back spin gave up (never expected)            */
#define GH_ST_LAYOUT 4u     /* kernel LDS layout assumption violated (never expected) */
#define GH_ST_OFFSETS 64u   /* a piece disagreed with the recorded piece offsets; it was
                               not written (never expected; 8, 16, 32: the gathers' bits) */

/* Create a context on HIP device `device` (ordinal among visible devices). */
int gh_ctx_create(int device, gh_ctx** out);
int gh_ctx_destroy(gh_ctx* ctx);
/* Build the decode tables from s->syms and upload segments [seg_begin, seg_end)
 * of the stream to the device (H2D, synchronous).  Allocates an output buffer of
 * out_cap bytes (0 = min(N, upper bound of the shard) rounded up). */
int gh_ctx_load(gh_ctx* ctx, const gh_stream* s, uint64_t seg_begin, uint64_t seg_end,
                uint64_t out_cap);
/* Same as gh_ctx_load but from device-resident words: `d_payload` must hold
 * words [4*seg_begin, 4*seg_end+1) (missing tail words read as zero) and
 * `d_gap_words` the whole gap array; both stay owned by the caller. */
int gh_ctx_load_device(gh_ctx* ctx, const gh_stream* s_header_only, uint64_t seg_begin,
                       uint64_t seg_end, const uint32_t* d_payload, uint64_t d_payload_words,
                       const uint32_t* d_gap_words, uint64_t out_cap);
/* Enqueue one decode of the loaded shard on `hip_stream` (NULL = the context's own
 * stream).  Asynchronous.  When `timed` != 0 the launch is bracketed by HIP events
 * whose average is reported by gh_ctx_report. */
int gh_ctx_decode(gh_ctx* ctx, void* hip_stream, int timed);
/* Wait for the context's work and fill `rep` (reads the device total + status). */
int gh_ctx_report(gh_ctx* ctx, void* hip_stream, gh_report* rep);
/* Copy the first `nbytes` bytes of the shard output to host memory. */
int gh_ctx_download(gh_ctx* ctx, uint64_t byte_offset, uint8_t* dst, uint64_t nbytes);
/* Device pointer of the shard output (for RCCL gathers / torch interop). */
int gh_ctx_output(gh_ctx* ctx, void** d_out, uint64_t* cap);
/* Asynchronously copy nbytes of the shard output (from byte_offset) to `dst`
 * (device or host memory) on `hip_stream` (NULL = the context's stream). */
int gh_ctx_copy_output(gh_ctx* ctx, uint64_t byte_offset, void* dst, uint64_t nbytes,
                       void* hip_stream);
/* Reset the accumulated kernel timing. */
int gh_ctx_reset_timing(gh_ctx* ctx);

/* HIP device ordinal the context is bound to. */
int gh_ctx_device(gh_ctx* ctx, int* device);

/* Name of the kernel template instantiation the last load picked for the shard, NUL-
 * terminated into buf[0..cap): "tile<TB,U,G,OW,MINL>" (single-pass tile kernel),
 * "mtile<TB,GL,NS,fb=F,np=P>" (two-pass tile kernel) or
 * "ws_count<U,TB,GL,fb=F>+ws_write<U,TB,GL,NS,fb=F>" (wave split); empty for an empty
 * shard.  GH_E_SMALL when cap is too small, GH_E_STATE before a load. */
int gh_ctx_kernel_shape(gh_ctx* ctx, char* buf, size_t cap);
/* Known piece offsets of the loaded shard (tile kernel).  Where every wave's piece goes
 * in the output is a function of the loaded shard alone: the first decodes after a load
 * work it out (a chain of prefixes across the workgroups) and record it; once a wait the
 * host makes anyway (gh_ctx_report, gh_ctx_download, ...) has seen such a decode finish
 * with status 0, later decodes of the same load read the offsets instead.  *state:
 * NONE after a load (always, for shards the tile kernel does not take), RECORDED once a
 * recording decode is enqueued, READY when the next decode will use the offsets.  A
 * decode that reports a status bit goes back to NONE.  GH_TILE_OFFS=0 in the environment
 * at load time keeps every decode recording (tests, A/B timing).  The name of
 * gh_ctx_kernel_shape does not change with the state. */
#define GH_OFFS_NONE 0
#define GH_OFFS_RECORDED 1
#define GH_OFFS_READY 2
int gh_ctx_offsets_state(gh_ctx* ctx, int* state);
/* Every kernel name a load can pick (the count and write kernels of the wave split
 * separately), one per line.  Needs no device. */
int gh_kernel_shapes(char* buf, size_t cap);

/* ---- streaming file I/O ------------------------------ */
/* Replaces the reference CLI's whole-file fread + synchronous copies
 * (decoder/src/huff.cpp:90-140, decoder.cu:759-768): the file's gap words and the
 * shard's payload words stream through two pinned buffers, the read of one chunk
 * overlapping the H2D of the previous one. */
typedef struct gh_file_info {
  uint64_t n, w, g;        /* stream sizes from the header                          */
  uint32_t nsyms, version;
  uint64_t bytes_read;     /* header + gap words + the shard's payload words        */
  double setup_ms;         /* open, header parse, allocations (wall)                */
  double transfer_ms;      /* overlapped file reads + H2D (wall)                    */
  double total_ms;         /* whole call (wall), including table build              */
} gh_file_info;
/* gh_ctx_load for segments [seg_begin, seg_end) of the compressed.huff at `path`
 * (seg_end = UINT64_MAX: to the end).  info may be NULL. */
int gh_ctx_load_file(gh_ctx* ctx, const char* path, uint64_t seg_begin, uint64_t seg_end,
                     uint64_t out_cap, gh_file_info* info);
/* Wait for the context's decode, then write output bytes [byte_offset,
 * byte_offset+nbytes) to `path` at file_offset (pwrite; the file is created, and
 * truncated first when `truncate`), the D2H of one chunk overlapping the write of the
 * previous one.  ms (may be NULL): wall time. */
int gh_ctx_save_file(gh_ctx* ctx, const char* path, uint64_t file_offset, uint64_t byte_offset,
                     uint64_t nbytes, int truncate, double* ms);

/* ---- random access: seek index and byte-range decode --------------------------- */
/* A shard load decodes any segment range on its own; the seek index maps an output byte
 * offset to the segment that holds it, so bytes [lo, hi) of the original data are read
 * without decoding the rest.  No reference counterpart (the reference decodes whole
 * streams only).  With stride = 1 << log2_stride segments (log2_stride in
 * GH_INDEX_MIN_LOG2..GH_INDEX_MAX_LOG2) and nblocks = ceil(G / stride), the index holds
 * nblocks + 1 entries: offsets[k], k < nblocks, is the number of codewords that start
 * before payload bit 128 * stride * k (the output offset of segment k * stride's first
 * symbol; offsets[0] = 0), and offsets[nblocks] = N.  Sidecar image, little-endian:
 *   u64 GH_INDEX_MAGIC ("GHIDX1\0\0"), u32 log2_stride, u32 0, u64 N, u64 G,
 *   u64 nentries, nentries x u64 offsets. */
#define GH_INDEX_MAGIC 0x0000315844494847ull
#define GH_INDEX_MIN_LOG2 8
#define GH_INDEX_MAX_LOG2 20
typedef struct gh_index {
  uint32_t log2_stride;
  uint64_t n, g, nentries;
  const uint64_t* offsets;   /* view into the image (any alignment: read it with memcpy) */
} gh_index;
/* Size of the image for G segments; 0 on a stride outside the range. */
uint64_t gh_index_bytes(uint64_t g, uint32_t log2_stride);
/* Parse an image (views into `file`).  GH_E_FORMAT unless: the magic and the stride are
 * right, nentries = ceil(G / stride) + 1, the image holds them, the first entry is 0
 * and the last N, the entries never decrease, and no step exceeds 143 * stride (a
 * segment holds at most 143 codewords). */
int gh_index_parse(const void* file, size_t file_len, gh_index* out);
/* Segments to load for output bytes [lo, hi): load [*seg_begin, *seg_end) with out_cap =
 * *skip + (hi - lo); the bytes start at byte *skip of that shard's output.  seg_begin =
 * k * stride for the last block k with offsets[k] <= lo, seg_end = min(m * stride, G)
 * for the first entry m with offsets[m] >= hi; an empty segment range when lo == hi.
 * GH_E_ARG when lo > hi or hi > N. */
int gh_index_locate(const gh_index* ix, uint64_t lo, uint64_t hi, uint64_t* seg_begin,
                    uint64_t* seg_end, uint64_t* skip);
/* Index of the stream loaded in ctx (the load must cover segments [0, G)); writes the
 * sidecar image (gh_index_bytes bytes) into out.  symbols (may be NULL): codewords
 * counted over all segments, the last segment's padding included (= gh_report.symbols
 * of a decode).  kernel_ms (may be NULL): HIP-event time of the kernel(s).  Synchronous.
 * GH_E_STATE before a load, GH_E_ARG when the load does not cover [0, G) or the stride
 * is bad, GH_E_SMALL when out_len is too small, GH_E_CORRUPT when the stream holds
 * fewer than N codewords. */
int gh_ctx_build_index(gh_ctx* ctx, uint32_t log2_stride, void* out, uint64_t out_len,
                       uint64_t* symbols, float* kernel_ms);
/* The same image from the encoders, which know every codeword's first bit before they
 * write a word: no decode, no decode tables, no gh_ctx.  offsets[k] is the number of i
 * with start(i) < 128 * stride * k, start(i) the exclusive prefix sum of
 * plan->len[in[i]].
 * Host: the sidecar image (gh_index_bytes(plan->g, log2_stride) bytes) of the stream that
 * gh_encode_write(in, plan, ...) produces, into out.  Threaded like gh_encode_write; the
 * image does not depend on `threads`.  No device.  GH_E_ARG: null pointers, a stride
 * outside the range, an input whose bit total differs from plan->bits; GH_E_SMALL:
 * out_len too small. */
int gh_encode_index(const uint8_t* in, const gh_encode_plan* plan, uint32_t log2_stride,
                    int threads, void* out, uint64_t out_len);
/* GPU: the sidecar image of the stream the context's last gh_ectx_encode produced, from
 * what that encode left on the device (input, code lengths, chunk bit offsets): one
 * kernel that reads only the input chunks holding an index boundary, then one copy of the
 * entries to out.  May be called repeatedly, with different strides, after one encode;
 * the encoded image (gh_ectx_download) is untouched.  Synchronous, on the context's
 * stream.  kernel_ms (may be NULL): HIP-event time of the index kernel alone.
 * GH_E_STATE before gh_ectx_encode or after a later gh_ectx_load / gh_ectx_plan;
 * GH_E_ARG: null pointers, a stride outside the range; GH_E_SMALL: out_len too small. */
int gh_ectx_index(gh_ectx* ctx, uint32_t log2_stride, void* out, uint64_t out_len, float* kernel_ms);

/* ---- the index of a sliced stream: every slice emits the entries it owns --------------- */
/* With S = 128 << log2_stride bits, entry k is the number of codewords that start before
 * stream bit S * k.  A slice ("sliced encode" above) holds code bits [base_bit, base_bit +
 * bits) and input bytes [sym_base, sym_base + n) of the stream, and it OWNS entry k when
 *   base_bit <= S * k < base_bit + bits:
 * entries [k0, k0 + nk) with k0 = ceil(base_bit / S), k1 = ceil((base_bit + bits) / S), nk =
 * k1 - k0.  The value is sym_base + the number of the slice's bytes whose first bit is
 * < S * k: every byte before the slice starts before the boundary, none after it does.  A
 * boundary exactly on a seam belongs to the later slice, with count 0; a boundary inside a
 * slice's last codeword gives sym_base + n; an empty slice owns nothing (k0 = k1).
 * Coverage: the slices' bit ranges partition [0, plan->bits), so k0 of one slice is k1 of
 * the one before (the k0 values chain from 0) and every boundary below plan->bits has
 * exactly one owner.  S * k < bits implies k * stride < G = ceil(bits / 128), and k * stride
 * < G implies S * k <= 128 * (G - 1) < bits, so the owned entries over all slices are
 * exactly k < nblocks = ceil(G / stride): the nk values sum to nblocks, no owned k reaches
 * nblocks, and the terminal entry N belongs to nobody (gh_index_image_init writes it).
 * No reference counterpart. */
/* [k0, k0 + nk) for bits [base_bit, base_bit + bits).  GH_E_ARG: nulls, a stride outside
 * the range, a sum that overflows 64 bits.  No device. */
int gh_index_slice_extent(uint64_t base_bit, uint64_t bits, uint32_t log2_stride,
                          uint64_t* k0, uint64_t* nk);
/* Host: entries [k0, k0 + nk) of the n bytes at `in` as the slice at base_bit / sym_base of
 * the stream planned by stream_plan; entries[j] is entry *k0 + j.  gh_encode_index's
 * two-pass walk with the bit origin and the symbol origin moved (gh_encode_index is the
 * slice at bit 0 / symbol 0 into gh_index_image_init's image).  The entries do not depend
 * on `threads`.  Errors as gh_encode_slice's: GH_E_TABLE: a byte of the slice has length 0
 * in the plan; GH_E_ARG: null pointers, a stride outside the range, base_bit + bits >
 * plan->bits; GH_E_SMALL: cap < nk -- *k0 and *nk are filled all the same, so a call with
 * cap = 0 sizes the buffer (entries may then be NULL). */
int gh_encode_index_slice(const uint8_t* in, uint64_t n, const gh_encode_plan* stream_plan,
                          uint64_t base_bit, uint64_t sym_base, uint32_t log2_stride, int threads,
                          uint64_t* entries, uint64_t cap, uint64_t* k0, uint64_t* nk);
/* Header, zeroed entries and the terminal entry N (gh_index_bytes(plan->g, log2_stride)
 * bytes): the image every slice's entries go into.  GH_E_ARG: nulls, a stride outside the
 * range; GH_E_SMALL: image_len too small. */
int gh_index_image_init(const gh_encode_plan* plan, uint32_t log2_stride, void* image, uint64_t image_len);
/* Store a slice's entries [k0, k0 + nk) into the image (any alignment), checked against
 * the image's own header: k0 + nk <= nentries - 1.  Slices own disjoint entries, so merges
 * may come in any order (and, unlike gh_slice_merge, share nothing).  An image with a
 * slice missing keeps that slice's zeros and fails gh_index_parse ("entries decrease": a
 * zero after a non-zero entry; only entry 0 is 0 in a stream whose every block holds a
 * codeword start): that is the intended tripwire, there is no separate completeness
 * check.  It does not cover the slice that owns entry 0: zeros after entry 0 never
 * decrease, and the parse then refuses only when the step up to the next slice's first
 * entry exceeds 143 * stride.  GH_E_ARG: nulls, entries past nentries - 1; GH_E_FORMAT: not an index image's
 * header; GH_E_SMALL: image_len shorter than the header says. */
int gh_index_slice_merge(void* image, uint64_t image_len, uint64_t k0, uint64_t nk, const uint64_t* entries);
/* GPU: the entries the context's last gh_ectx_encode_slice owns, from what that encode left
 * on the device (gh_enc_index_kernel<SLICE = true>; the slice's chunk offsets are stream
 * bit positions already), copied to entries[0 .. nk); sym_base: the stream offset of the
 * slice's first byte.  *k0, *nk as gh_encode_index_slice's, filled before cap is checked
 * (GH_E_SMALL).  nk = 0 launches nothing.  Repeatable with different strides; the slice's
 * words (gh_ectx_download_slice, gh_ectx_merge_device) are untouched.  Synchronous, on the
 * context's stream.  kernel_ms (may be NULL): HIP-event time of the index kernel alone.
 * GH_E_STATE unless the context's last encode was a slice encode (and after a later
 * load, counts, plan or encode); GH_E_ARG: nulls, a stride outside the range.
 * gh_ectx_index keeps returning GH_E_STATE after a slice encode. */
int gh_ectx_index_slice(gh_ectx* ctx, uint64_t sym_base, uint32_t log2_stride,
                        uint64_t* entries, uint64_t cap, uint64_t* k0, uint64_t* nk, float* kernel_ms);
/* Batched range gather: many byte ranges of a resident stream in one launch.  offsets[k]
 * is the output position of index block k's first symbol, so a block decodes on its own;
 * a batch is cut into pieces "decode index block k, keep the symbols at positions [a, b)
 * of the block, store them at dst".  One wave owns a piece and walks the block's segments
 * from its start, so gathers want a small stride: 2^8 .. 2^10 segments. */
typedef struct gh_range { uint64_t lo, hi; } gh_range;            /* output bytes [lo, hi) */
typedef struct gh_gather_piece {
  uint64_t dst;      /* byte offset in the gathered output                          */
  uint32_t block;    /* index block k: segments [k*stride, min((k+1)*stride, G))     */
  uint32_t a, b;     /* keep symbols at positions [a, b) counted from offsets[k]     */
  uint32_t pad;      /* 0 */
} gh_gather_piece;
/* Pieces for `nranges` ranges, in request order; range i's bytes start at
 * sum_{j<i} (hi_j - lo_j) of the output.  Ranges may be empty, overlap, repeat and
 * come in any order.  *npieces / *out_bytes are always written (so a first call with
 * cap = 0 sizes the buffers; GH_E_SMALL then).  GH_E_ARG: lo > hi or hi > N.  No device. */
int gh_gather_plan(const gh_index* ix, const gh_range* ranges, uint32_t nranges,
                   gh_gather_piece* pieces, uint64_t cap, uint64_t* npieces,
                   uint64_t* out_bytes);
/* Bytes of `nranges` ranges of the stream loaded in ctx (the load must cover [0, G)),
 * concatenated in request order, into dst (device or host memory, dst_len >= their sum).
 * Synchronous.  kernel_ms (may be NULL): HIP-event time of the gather kernel.  The tables
 * are built on the context's first gather and kept until its next load.
 * GH_E_STATE before a load; GH_E_ARG: load not covering [0, G), ix->n / ix->g differ
 * from the stream's, a bad range; GH_E_SMALL: dst_len too small; GH_E_CORRUPT on a
 * device status bit. */
int gh_ctx_gather(gh_ctx* ctx, const gh_index* ix, const gh_range* ranges, uint32_t nranges,
                  void* dst, uint64_t dst_len, void* hip_stream, float* kernel_ms);

/* Device-planned gather: the ranges and the destination are device memory, the index is
 * resident in the context, the plan (the pieces gh_gather_plan would cut, in the same
 * order) is built by kernels, and the call only enqueues: for callers that hold their row
 * ids on the GPU, on a stream that must not stall.  No reference counterpart. */
/* Keep the index's entries on the context's device.  The checks of gh_ctx_gather: the load
 * covers [0, G), ix->n / ix->g are the stream's, nentries matches gh_index_bytes (GH_E_ARG
 * otherwise, also when the entries do not start at 0, end at N and never decrease by
 * steps of at most 143 * stride); GH_E_STATE before a load.  The next load drops the
 * index; setting it again replaces it.  Synchronous (two uploads). */
int gh_ctx_set_index(gh_ctx* ctx, const gh_index* ix);
/* Status bits of a device-planned gather, beside GH_ST_BADCODE and GH_ST_LAYOUT. */
#define GH_ST_RANGE 8u       /* some range has lo > hi or hi > N                   */
#define GH_ST_DSTSMALL 16u   /* the batch's bytes exceed dst_len                   */
#define GH_ST_PIECES 32u     /* the plan would exceed the piece buffer             */
typedef struct gh_gather_report {
  uint64_t out_bytes;  /* sum of hi - lo over the batch (its valid ranges)   */
  uint64_t npieces;    /* pieces the device plan produced (0: refused)       */
  uint32_t status;     /* device status bits of the gather (GH_ST_*)         */
  float kernel_ms;     /* HIP events: plan kernels + gather kernel           */
} gh_gather_report;
/* Ranges in one device-planned batch, at most. */
#define GH_GATHER_MAX_RANGES (1u << 24)
/* Pieces a batch of nranges ranges that fits dst_len bytes can need: the host cannot know
 * the piece count of ranges it never sees, so the piece buffer is sized by this bound,
 *   2 * nranges + dst_len / (8 * stride),   stride = 1 << log2_stride segments.
 * A piece that is neither the first nor the last of its range covers a whole index block
 * that is not the stream's last; the block spans 128 * stride bits wholly inside the code
 * bits; no codeword is longer than 16 bits, so at least 8 * stride codewords start in it,
 * and the piece gives that many of the batch's bytes.  gh_index_parse enforces no minimum
 * step, so an index that belongs to no real stream can break the bound: the device plan
 * checks its piece count against the buffer and refuses (GH_ST_PIECES) instead of
 * writing.  Monotone in nranges and dst_len; 0 on a stride outside the range.  No device. */
uint64_t gh_gather_piece_bound(uint32_t nranges, uint64_t dst_len, uint32_t log2_stride);
/* Enqueue the gather of d_ranges[0 .. nranges) ({u64 lo, u64 hi} in device memory: a
 * contiguous int64[n, 2] tensor) into d_dst (device memory, dst_len bytes) on hip_stream
 * (NULL = the context's stream), and return.  Range i's bytes start at
 * sum_{j<i} (hi_j - lo_j) of d_dst, as gh_ctx_gather's, and the kernels store them there
 * directly.  d_ranges and d_dst must stay as they are until the gather has finished.
 * The call waits for the device only when it is the first gather after a load (it builds
 * the tables) or when a context buffer has to grow (the piece buffer holds
 * min(gh_gather_piece_bound, 2^31 - 1) pieces); a repeated call with the same or a smaller
 * nranges and dst_len allocates nothing.  It does not wait for the context's decodes: it
 * reads only the loaded stream.  Calls on one context run in the order they were made,
 * whatever their streams.  nranges = 0: GH_OK, nothing is launched.
 * GH_E_STATE before a load or without a resident index; GH_E_ARG: a null pointer, more
 * than GH_GATHER_MAX_RANGES ranges.  What only the device can find is returned by
 * gh_ctx_gather_wait. */
int gh_ctx_gather_device(gh_ctx* ctx, const gh_range* d_ranges, uint32_t nranges,
                         void* d_dst, uint64_t dst_len, void* hip_stream);
/* Wait for the context's last device gather and report it (rep may be NULL; it is filled
 * before an error is returned).  GH_E_ARG: some range had lo > hi or hi > N; GH_E_SMALL:
 * the batch's bytes exceed dst_len; GH_E_CORRUPT: GH_ST_BADCODE, or the plan would exceed
 * the piece buffer; GH_E_HIP: GH_ST_LAYOUT.  After GH_E_ARG, GH_E_SMALL and a piece-buffer
 * overflow not one byte of d_dst has been written.  GH_E_STATE when no device gather has
 * been enqueued since the load. */
int gh_ctx_gather_wait(gh_ctx* ctx, gh_gather_report* rep);
/* The HIP-event times of the last device gather's plan kernels and of its gather kernel
 * (their sum is gh_gather_report.kernel_ms); waits like gh_ctx_gather_wait.  Either
 * pointer may be NULL. */
int gh_ctx_gather_times(gh_ctx* ctx, float* plan_ms, float* gather_ms);
/* Pieces of the last device gather, copied to host memory (tests, diagnosis); waits for
 * it.  *npieces is always written; GH_E_SMALL when cap is smaller. */
int gh_ctx_gather_pieces(gh_ctx* ctx, gh_gather_piece* pieces, uint64_t cap, uint64_t* npieces);

/* ---- batched decode: many independent streams, one launch per batch ------------------ */
/* Many small streams, each a complete compressed.huff with its own code (a page, a column
 * chunk, a tensor, a message), decoded by one fixed set of kernel launches however many
 * they are.  No reference counterpart (the reference decodes one stream per call).  A
 * gh_batch is bound to one device and used from one host thread at a time.
 *
 * Output layout: stream i's bytes start at out_off[i] = sum_{j<i} round_up(n_j, 16) of the
 * destination arena, so every stream is 16-byte aligned; out_off[nstreams] is the arena
 * size.  Bytes in [out_off[i] + n_i, out_off[i+1]) are never written.
 *
 * Load: every stream is validated on the host (gh_stream_validate's checks, O(nsyms)); a bad
 * stream fails the whole load with that check's code, the message naming the stream's
 * index.  Payloads and gap words are packed into one library-owned device arena by a few
 * large copies (each payload 16-byte aligned and zero padded up to 4 G + 4 words, each gap
 * array 4-byte aligned), and the decode tables of ALL streams are built on the device by one
 * kernel from the uploaded (symbol, length) lists: per stream the canonical fallback tables
 * and a single-codeword lookup table {len | sym << 8} of min(maxlen, 10) bits.
 * Limits (GH_E_ARG beyond them): nstreams <= 2^24; per-stream G < 2^32 - 256; fewer than
 * 2^31 work units (a unit is 256 segments of one stream) in a batch.  Empty streams (N = 0,
 * G = 0, no symbols) decode to nothing; a stream with segments needs a code (GH_E_TABLE).
 * nstreams = 0 is GH_OK.  A load replaces the previous batch; buffers are reused when
 * large enough. */
typedef struct gh_batch gh_batch;
typedef struct gh_batch_item {
  const gh_sym* syms;           /* host memory: nsyms entries, file order                   */
  uint32_t nsyms;
  uint64_t n, w, g;             /* as gh_stream                                              */
  const uint32_t* d_payload;    /* device memory, 4-byte aligned: w words                   */
  const uint32_t* d_gap_words;  /* device memory, 4-byte aligned: ceil(g / 8) words         */
} gh_batch_item;
typedef struct gh_batch_report {
  uint64_t out_bytes;    /* sum of n_i                                                      */
  uint32_t nstreams;
  uint32_t bad_streams;  /* streams with a status bit set                                   */
  uint32_t status;       /* OR of the streams' GH_ST_* bits                                 */
  float kernel_ms;       /* HIP-event time of the last timed decode (all its kernels)       */
  uint32_t launches;     /* kernels one decode launches: a constant, whatever nstreams      */
} gh_batch_report;
/* GH_E_NODEV without a usable gfx950 device, as gh_ctx_create. */
int gh_batch_create(int device, gh_batch** out);
int gh_batch_destroy(gh_batch* b);
/* out_off[0 .. nstreams] for streams of n[i] bytes.  Host arithmetic only, no device.
 * GH_E_ARG: null pointers (n may be NULL when nstreams = 0), a sum that overflows 64 bits. */
int gh_batch_layout(const uint64_t* n, uint32_t nstreams, uint64_t* out_off);
/* Load parsed streams from host memory (gh_stream_parse output; the words may sit at any
 * alignment).  Synchronous. */
int gh_batch_load(gh_batch* b, const gh_stream* streams, uint32_t nstreams);
/* Load streams whose words are device memory (any address the batch's device can read): one
 * copy kernel reads the pointer table and copies every stream's words into the padded arena,
 * on the batch's stream, after an event recorded on hip_stream (NULL: the default stream),
 * so a producer enqueued there has finished first.  Synchronous; the caller's arrays are
 * not needed after the call.  Everything downstream is as after gh_batch_load. */
int gh_batch_load_device(gh_batch* b, const gh_batch_item* items, uint32_t nstreams, void* hip_stream);
/* Enqueue one decode of the loaded batch on hip_stream (NULL = the batch's own stream) and
 * return.  d_dst: device memory, 16-byte aligned, dst_len >= out_off[nstreams]; NULL selects
 * the batch's own output arena (allocated on demand; dst_len is ignored).  timed != 0
 * brackets the kernels with HIP events.  GH_E_STATE before a load, GH_E_SMALL when dst_len
 * is too small, GH_E_ARG on a misaligned d_dst. */
int gh_batch_decode(gh_batch* b, void* d_dst, uint64_t dst_len, void* hip_stream, int timed);
/* Wait for the last decode and report it (rep may be NULL; it is filled before an error is
 * returned).  GH_E_CORRUPT when any stream holds fewer than its N codewords or met a bit
 * pattern outside its code; GH_E_STATE when no decode has been enqueued since the load. */
int gh_batch_wait(gh_batch* b, gh_batch_report* rep);
/* Per stream, after gh_batch_wait: the GH_ST_* bits and the codewords counted over its
 * segments, the last segment's padding included (as gh_report.symbols); either array may be
 * NULL.  A bad stream never changes another stream's bytes and touches nothing outside its
 * own extents: its walk is bounded by its G segments, its stores are clipped at its N.
 * GH_E_SMALL when cap < nstreams. */
int gh_batch_status(gh_batch* b, uint32_t* status, uint64_t* symbols, uint32_t cap);
/* The batch's own output arena (NULL / 0 before a decode used it). */
int gh_batch_output(gh_batch* b, void** d_out, uint64_t* cap);
/* out_off[0 .. nstreams] of the loaded batch; GH_E_SMALL when cap < nstreams + 1. */
int gh_batch_offsets(gh_batch* b, uint64_t* out_off, uint32_t cap);
/* The first nbytes (<= n_i) of stream `stream` from the batch's own arena to host memory;
 * waits for the last decode. */
int gh_batch_download(gh_batch* b, uint32_t stream, uint8_t* dst, uint64_t nbytes);
/* The batch decode's count and write kernels are one of two instantiation pairs, named
 * "batch<fb=0>" (every stream's code is complete and no longer than the lookup table) and
 * "batch<fb=1>" (some lookup can miss: the canonical fallback is compiled in).
 * gh_batch_kernel_shape: the name the last load picked (empty for a batch without
 * segments); GH_E_STATE before a load.  gh_batch_kernel_shapes: every name, one per line;
 * needs no device.  Neither is part of gh_kernel_shapes. */
int gh_batch_kernel_shape(gh_batch* b, char* buf, size_t cap);
int gh_batch_kernel_shapes(char* buf, size_t cap);

/* ---- batched gather: byte ranges of many streams in a fixed launch count --------------- */
/* The random access of gh_ctx_gather_device for a resident batch: byte ranges (stream, lo, hi)
 * of its streams, decoded without decoding the rest.  No sidecar and no per-stream index
 * build: a decode's count and scan kernels leave one byte per segment (the codewords that
 * start in it) and the exclusive scan of the codewords per 256-segment unit on the device,
 * which is a seek index of stride 2^8 for every stream of the batch; gh_batchdec_index runs
 * those two kernels alone.  The plan is cut by three kernels and one gather kernel decodes
 * the pieces, each by one wave: a constant launch count however many ranges there are.  No
 * reference counterpart.
 *
 * Output layout: range i's bytes start at sum_{j<i} (hi_j - lo_j) of d_dst, tight and in
 * request order, as gh_ctx_gather's.  Ranges may be empty, overlap, repeat and name the
 * streams in any order (a wave reloads its tables when the stream changes from one piece to
 * the next: ranges sorted by stream cost one table load per stream and wave).
 * A piece is a gh_gather_piece whose `block` is the GLOBAL unit index of the batch and
 * whose a, b count from that unit's first symbol. */
typedef struct gh_brange { uint64_t stream, lo, hi; } gh_brange;   /* a contiguous int64[n,3] tensor */
typedef struct gh_bgather_report {
  uint64_t out_bytes;   /* sum of hi - lo over the batch's valid ranges                      */
  uint64_t npieces;     /* pieces the device plan cut (0: refused)                           */
  uint32_t bad_ranges;  /* ranges that name a stream flagged by the index pass               */
  uint32_t status;      /* GH_ST_RANGE | GH_ST_DSTSMALL | GH_ST_PIECES | GH_ST_BADCODE       */
  float kernel_ms;      /* HIP events: plan kernels + gather kernel                          */
  uint32_t launches;    /* kernels + memsets of one gather: a constant                       */
} gh_bgather_report;
/* Enqueue the count and scan kernels of the loaded batch, and nothing else: no write kernel,
 * no output arena.  Afterwards the per-segment counts, the unit scan, the per-stream status
 * words and symbol counts are valid.  It counts as a decode for gh_batch_wait and
 * gh_batch_status (which then report what the count pass found: a batch can be validated
 * without writing a byte), not for gh_batch_download.  A full gh_batch_decode leaves the same
 * state.  A load drops it.  GH_E_STATE before a load. */
int gh_batchdec_index(gh_batch* b, void* hip_stream, int timed);
/* Enqueue the gather of d_ranges[0 .. nranges) (device memory) into d_dst (device memory,
 * dst_len bytes) on hip_stream (NULL = the batch's stream), and return.  It runs after every
 * earlier decode, index or gather of the batch, whatever their streams.  d_ranges and d_dst
 * must stay untouched until the wait.  The call blocks only to grow a batch-owned buffer (the
 * piece buffer holds min(gh_gather_piece_bound(nranges, dst_len, 8), 2^31 - 1) pieces); a
 * repeated call with the same or a smaller nranges and dst_len allocates nothing.
 * timed != 0 brackets the kernels with HIP events.  nranges = 0: GH_OK, nothing is launched.
 * GH_E_STATE before an index or decode since the load; GH_E_ARG: a null pointer, more than
 * GH_GATHER_MAX_RANGES ranges. */
int gh_batchdec_gather_device(gh_batch* b, const gh_brange* d_ranges, uint32_t nranges,
                              void* d_dst, uint64_t dst_len, void* hip_stream, int timed);
/* Wait for the batch's last gather and report it (rep may be NULL; it is filled before an
 * error is returned).  GH_E_ARG: some range had stream >= nstreams, lo > hi or hi > n_stream
 * (GH_ST_RANGE); GH_E_SMALL: the batch's bytes exceed dst_len (GH_ST_DSTSMALL); GH_E_CORRUPT:
 * the plan would exceed the piece buffer (GH_ST_PIECES); after these three not one byte of
 * d_dst has been written.  GH_E_CORRUPT also when a range names a stream whose status word is
 * non-zero (GH_ST_BADCODE in the report): such a range keeps its hi - lo bytes in the layout,
 * gets no pieces and leaves its bytes as they were, every other range is gathered exactly,
 * and bad_ranges counts them.  GH_E_STATE when no gather has been enqueued since the load. */
int gh_batchdec_gather_wait(gh_batch* b, gh_bgather_report* rep);
/* The same with the ranges in host memory: uploads them, then gather_device (timed) and
 * gather_wait.  Synchronous.  rep may be NULL. */
int gh_batchdec_gather(gh_batch* b, const gh_brange* ranges /* host */, uint32_t nranges,
                       void* d_dst, uint64_t dst_len, void* hip_stream, gh_bgather_report* rep);
/* Pieces of the last gather, copied to host memory (tests, diagnosis); waits for it.
 * *npieces is always written; GH_E_SMALL when cap is smaller. */
int gh_batchdec_gather_pieces(gh_batch* b, gh_gather_piece* pieces, uint64_t cap, uint64_t* npieces);
/* The device plan from host arrays, the same pieces in the same order: unit0[0 .. nstreams]
 * the prefix of the streams' unit counts, unit_off[0 .. unit0[nstreams]] the exclusive scan
 * of the codewords per unit, n[s] the streams' output bytes, stream_status[s] their status
 * words (NULL: none is flagged).  *npieces / *out_bytes / *bad_ranges are always written (a
 * first call with cap = 0 sizes the buffer; GH_E_SMALL then).  GH_E_ARG: stream >= nstreams,
 * lo > hi or hi > n[stream] (the counts are then 0).  A range on a flagged stream adds its
 * bytes to *out_bytes, counts in *bad_ranges and gives no pieces; the return stays GH_OK.
 * No device. */
int gh_batchdec_plan(const uint32_t* unit0, const uint64_t* unit_off, const uint64_t* n,
                     const uint32_t* stream_status, uint32_t nstreams, const gh_brange* ranges,
                     uint32_t nranges, gh_gather_piece* pieces, uint64_t cap, uint64_t* npieces,
                     uint64_t* out_bytes, uint32_t* bad_ranges);
/* The gather kernel is one of two instantiations, "bgather<fb=0>" and "bgather<fb=1>", picked
 * as the batch's decode kernels are.  gh_batchdec_kernel_shape: the name for the loaded batch
 * (empty for a batch without segments); GH_E_STATE before a load.  gh_batchdec_kernel_shapes:
 * both names, one per line; needs no device.  Neither is part of another shape list. */
int gh_batchdec_kernel_shape(gh_batch* b, char* buf, size_t cap);
int gh_batchdec_kernel_shapes(char* buf, size_t cap);

/* ---- batched encode: many independent inputs, a fixed launch count per batch ---------- */
/* The other half of the batched decode: N independent inputs, each encoded with its own
 * canonical code into its own compressed.huff image, by a number of launches that does not
 * depend on N.  Every image is byte-identical to gh_encode_write's.  The payload and gap
 * words stay on the device in the form gh_batch_load_device takes (gh_ebatch_items), so a
 * batch can be encoded, decoded and checked without a payload word crossing to the host.  No
 * reference counterpart.  A gh_ebatch is bound to one device and used from one host thread
 * at a time.
 *
 * Order of calls: load (host or device memory), plan (gh_ebatch_plan: codes built on the
 * host, or gh_batchenc_plan_device: on the device; the same plans), encode, wait, then sizes /
 * download / items.  GH_E_STATE: plan before a load; encode, plan_of, plan_times, sizes or
 * items before a plan; wait or download before an encode.  A load invalidates the plan.
 *
 * Layout (host arithmetic, no device).  A work unit is GH_EBATCH_UNIT_BYTES consecutive
 * input bytes of one stream.  Input arena: stream i starts 16-byte aligned and owns
 * ceil(n_i / unit) whole units plus 32 bytes (nothing when n_i = 0), zero past n_i, so every
 * load of the kernels stays inside the stream's own extent.  Output: one payload arena and
 * one gap arena; stream i's W_i words and ceil(G_i / 8) gap words each start at a 16-byte
 * aligned offset; both arenas are zeroed at every encode.
 * Limits (GH_E_ARG beyond them): nstreams <= 2^24; fewer than 2^31 units in a batch.  Empty
 * inputs (n = 0) are legal: their image is the 20-byte header alone.  nstreams = 0 is GH_OK.
 * A load replaces the previous batch; buffers are reused when large enough. */
#define GH_EBATCH_UNIT_BYTES 1024
typedef struct gh_ebatch gh_ebatch;
typedef struct gh_ebatch_item {
  const void* d_in;  /* device memory, any byte alignment: n bytes */
  uint64_t n;
} gh_ebatch_item;
typedef struct gh_ebatch_report {
  uint64_t in_bytes, out_bytes;  /* sum n_i, sum file_bytes_i                         */
  uint32_t nstreams, status;     /* OR of the streams' GH_ST_* bits                   */
  float hist_ms, plan_host_ms;   /* plan step: histogram kernel (events), host plans  */
  float kernel_ms;               /* last timed encode, all its kernels (events)       */
  uint32_t launches;             /* kernels + memsets of one encode: a constant       */
} gh_ebatch_report;
/* GH_E_NODEV without a usable gfx950 device, as gh_ctx_create. */
int gh_ebatch_create(int device, gh_ebatch** out);
int gh_ebatch_destroy(gh_ebatch* b);
/* Load inputs from host memory: packed into one staging buffer, one upload.  Synchronous. */
int gh_ebatch_load(gh_ebatch* b, const uint8_t* const* in, const uint64_t* n, uint32_t nstreams);
/* Load inputs that are device memory (any address the batch's device can read, any byte
 * alignment): a pointer table and one copy kernel on the batch's stream, after an event
 * recorded on hip_stream (NULL: the default stream).  Exactly n_i bytes are read per stream.
 * Synchronous; the caller's memory is not needed after the call.  Stream i of a batched
 * decode's output arena, at out_off[i], is a valid source. */
int gh_ebatch_load_device(gh_ebatch* b, const gh_ebatch_item* items, uint32_t nstreams, void* hip_stream);
/* Every stream's plan (synchronous): one histogram launch, one read-back of the counts, one
 * host plan per stream (package-merge with the reference's tie-breaking and the canonical
 * code, on `threads` host threads; <= 0: all), one upload of the code tables and descriptors,
 * the sizing of the output arenas.  force_version as gh_encode_plan_make; GH_E_ARG names the
 * stream that cannot take v1. */
int gh_ebatch_plan(gh_ebatch* b, int force_version, int threads);
/* gh_ebatch_plan with the codes built on the device: histogram launch, code launch, one
 * read-back of a 528-byte record per stream (bits, nsyms, the header's symbol list), the
 * host's O(nsyms) build_canon per stream as a tripwire, the output layout, one upload of
 * the 64-byte descriptors.  No host package-merge, no read-back of counts, no upload of
 * tables.  Every plan, image and item is identical to gh_ebatch_plan's.  Synchronous.
 * GH_E_TABLE names the stream whose device-built code is not a canonical code (never
 * expected); GH_E_STATE and force_version as gh_ebatch_plan.  (The two gh_batchenc_* entry
 * points work on a gh_ebatch; the gh_ebatch_* names are a closed set that
 * tests/test_ebatch_layout.py pins, so later additions carry this prefix.) */
int gh_batchenc_plan_device(gh_ebatch* b, int force_version);
/* Times of the last plan of either kind (any pointer may be NULL): histogram kernel and code
 * kernel by HIP events (code_ms = 0 after gh_ebatch_plan), host work by wall clock.
 * GH_E_STATE before a plan. */
int gh_batchenc_plan_times(gh_ebatch* b, float* hist_ms, float* code_ms, float* host_ms);
/* Stream `stream`'s plan.  After gh_batchenc_plan_device the first call copies every stream's
 * histogram back once (the plan itself does not need it): count[] is filled as after
 * gh_ebatch_plan. */
int gh_ebatch_plan_of(gh_ebatch* b, uint32_t stream, gh_encode_plan* out);
/* Enqueue one encode of the planned batch on hip_stream (NULL = the batch's own stream) and
 * return.  timed != 0 brackets it with HIP events. */
int gh_ebatch_encode(gh_ebatch* b, void* hip_stream, int timed);
/* Wait for the last encode and report it (rep may be NULL; it is filled before an error is
 * returned).  GH_E_HIP when a stream carries GH_ST_LAYOUT: its device bit total differed
 * from its plan's (never expected). */
int gh_ebatch_wait(gh_ebatch* b, gh_ebatch_report* rep);
/* file_bytes of every stream; GH_E_SMALL when cap < nstreams. */
int gh_ebatch_sizes(gh_ebatch* b, uint64_t* file_bytes, uint32_t cap);
/* Stream `stream`'s whole image to host memory: header from the plan, gap words, payload
 * words, file_bytes in total.  Waits for the last encode.  GH_E_SMALL when out_len is short. */
int gh_ebatch_download(gh_ebatch* b, uint32_t stream, void* out, uint64_t out_len);
/* One gh_batch_item per stream, for gh_batch_load_device: syms points at the batch's own
 * host copy of the stream's table, d_payload / d_gap_words into the arenas.  Valid until the
 * batch's next load, plan or destroy.  GH_E_SMALL when cap < nstreams. */
int gh_ebatch_items(gh_ebatch* b, gh_batch_item* items, uint32_t cap);
/* The batched encode's per-unit kernels are compiled in one shape, "ebatch<lut=1>" (one copy
 * of the stream's code table per wave).  gh_ebatch_kernel_shape: the name the last plan
 * picked (empty for a batch without units); GH_E_STATE before a plan.
 * gh_ebatch_kernel_shapes: every name, one per line; needs no device.  Neither is part of
 * gh_kernel_shapes, gh_enc_kernel_shapes or gh_batch_kernel_shapes. */
int gh_ebatch_kernel_shape(gh_ebatch* b, char* buf, size_t cap);
int gh_ebatch_kernel_shapes(char* buf, size_t cap);

/* ---- self-synchronising decode of gap-less streams ---- */
/* Replaces CUHD's decoder for raw Huffman streams without a gap array
 * (gpuhd/src/cuhd_gpu_decoder.cu:145-523, CUHDGPUDecoder::decode declared at
 * gpuhd/include/cuhd_gpu_decoder.h:24-32; stream = u32 units, codewords MSB-first,
 * llhuffman_encoder.cc:200-238).  The GPU finds every 128-bit segment's first
 * codeword start by decoding from arbitrary bits and verifying that neighbouring
 * walks agree (repairing where they do not), which yields the gap array; the stream
 * is then decoded by the gap-array kernels.  Codes: the canonical (symbol,length)
 * list in file order (lengths 1..16, non-decreasing), as in gh_stream. */
typedef struct gh_sync_report {
  uint64_t g;           /* 128-bit segments = ceil(w / 4)                          */
  uint64_t mismatches;  /* segment boundaries the first walk got wrong (repaired)  */
  uint32_t passes;      /* verify/repair passes (1 when the first walk was right)  */
  float kernel_ms;      /* walk kernel to the last verify pass (HIP events; includes
                           the host turnaround between passes)                     */
  float host_ms;        /* the halo estimate before the walk (stream sample copied
                           back + host walks; 0 when GH_SYNC_HALO is set), wall time,
                           not inside kernel_ms: the whole call is host_ms + kernel_ms */
  uint32_t halo;        /* warm-up segments per lane the walk used                 */
} gh_sync_report;
/* Gap words (ceil(ceil(w/4)/8) u32, the gap-array file's layout) of the raw stream
 * d_words[0..w) (device memory, 16-byte aligned) into d_gap_words on `hip_stream`
 * (NULL = default stream) of `device`.  Synchronous (the verify loop reads a
 * counter back).  rep may be NULL. */
int gh_sync_gaps(int device, const gh_sym* syms, uint32_t nsyms, const uint32_t* d_words,
                 uint64_t w, uint32_t* d_gap_words, void* hip_stream, gh_sync_report* rep);
/* Prefix bits of gh_sync_gaps's length table: a code whose longest codeword has more bits
 * runs the kernels' long-codeword path.  Needs no device. */
int gh_sync_lut_bits(void);
/* Raw-stream file container (this repo's; gpuhd keeps its streams in memory,
 * demo.cc:100-160): u64 GH_RAW_MAGIC ("GHRAW1\0\0"), u64 nsyms, nsyms x {u8 symbol,
 * u8 length} in code order, u64 N, u64 W, W x u32 units (codewords MSB-first). */
#define GH_RAW_MAGIC 0x0000315741524847ull
typedef struct gh_raw_stream {
  const gh_sym* syms;
  uint32_t nsyms;
  uint64_t n, w;
  const uint32_t* units;   /* view into the file image                             */
} gh_raw_stream;
int gh_raw_parse(const void* file, size_t file_len, gh_raw_stream* out);
/* gh_ctx_load for a raw stream held in host memory: uploads words[0..w), builds its
 * gap array with gh_sync_gaps and loads the whole stream (n output bytes) into ctx;
 * gh_ctx_decode / gh_ctx_report / gh_ctx_download then work as for a gap-array file. */
int gh_ctx_load_raw(gh_ctx* ctx, const gh_sym* syms, uint32_t nsyms, uint64_t n,
                    const uint32_t* words, uint64_t w, uint64_t out_cap, gh_sync_report* rep);

/* ---- batched gap-less decode: raw streams into a gh_batch, gap arrays built on the GPU ---- */
/* The batch treatment for raw streams: any number of gap-less streams, each with its own code,
 * loaded into a gh_batch by a fixed number of launches, with no read-back and no host loop.
 * gh_batch_decode, gh_batchdec_index, the gathers and gh_batch_status then run unchanged.
 *
 * The method is exact.  A codeword has at most 16 bits, so a segment's entry (its first
 * codeword start minus 128 j) lies in 0..15 and segment j is a total function T_j on 16
 * states, one u64 of 16 nibbles.  e_0 = 0, e_{j+1} = T_j(e_j); composition is associative, so
 * all entries come from a prefix scan of composed functions, segmented by stream.  Gap nibble
 * j is e_{j+1} for j < G - 1 and 0 for j = G - 1 and the tail of the last gap word: what the
 * encoders write.  Three kernels: T_j and the aggregate of every 256-segment unit; the units'
 * entries, stream by stream; the gap words of every unit.  G = ceil(W / 4).  (The gh_batch_*,
 * gh_batchdec_* and gh_ebatch_* names are closed sets pinned by tests; these carry gh_batchraw_.) */
/* gh_batch_load for raw streams in host memory (any alignment); synchronous.  Runs the checks
 * of gh_raw_parse (a canonical code; N symbols fit the 32 W bits) and the batch limits; an
 * error names the stream as gh_batch_load's do. */
int gh_batchraw_load(gh_batch* b, const gh_raw_stream* streams, uint32_t nstreams);
/* gh_batch_load_device for raw streams: d_gap_words is not read; g must equal ceil(w / 4)
 * (GH_E_ARG otherwise).  Follows hip_stream as gh_batch_load_device.  gh_ebatch_items output
 * is a valid source: a batch can be encoded and decoded on the device without its gap words
 * ever being read. */
int gh_batchraw_load_device(gh_batch* b, const gh_batch_item* items, uint32_t nstreams, void* hip_stream);
/* The resident gap words of one stream (ceil(G / 8) u32) to host memory, after either kind of
 * load.  *ngapw is always written; GH_E_SMALL when cap is smaller. */
int gh_batchraw_gaps(gh_batch* b, uint32_t stream, uint32_t* gap_words, uint64_t cap, uint64_t* ngapw);
typedef struct gh_batchraw_report {
  float gap_ms;            /* HIP events around the gap kernels of the last raw load        */
  uint32_t launches;       /* their count: a constant                                       */
  uint64_t scratch_bytes;  /* 8 * 256 + 8 + 4 bytes per work unit                           */
} gh_batchraw_report;
/* GH_E_STATE when the last load was not a raw load. */
int gh_batchraw_report_get(gh_batch* b, gh_batchraw_report* rep);
/* The host twin: the same gap words (ceil(ceil(w / 4) / 8) u32; GH_E_SMALL when cap is
 * smaller) from the same functions (csrc/gh_raw_trans.hpp) under the batch's lookup rule (a
 * pattern outside an incomplete code advances maxlen bits), composed per 256-segment unit and
 * chained, as the kernels are cut.  Any words are accepted, valid streams or not.  GH_E_TABLE
 * for a non-canonical code, or an empty one with w > 0.  Needs no device. */
int gh_batchraw_gaps_host(const gh_sym* syms, uint32_t nsyms, const uint32_t* words, uint64_t w,
                          uint32_t* gap_words, uint64_t cap);
/* The T_j kernel is one of two instantiations, "batchraw<fb=0>" and "batchraw<fb=1>", picked as
 * the batch's decode kernels are.  gh_batchraw_kernel_shape: the name the last raw load picked
 * (empty for a batch without segments); GH_E_STATE when the last load was not a raw load.
 * gh_batchraw_kernel_shapes: both names, one per line; needs no device.  Neither is part of
 * another shape list. */
int gh_batchraw_kernel_shape(gh_batch* b, char* buf, size_t cap);
int gh_batchraw_kernel_shapes(char* buf, size_t cap);

/* ---- byte planes: typed tensors split, coded and joined on the GPU ---------------------- */
/* The batch family for tensors of E-byte elements, E in {1, 2, 4, 8}.  Plane p of a tensor of
 * nelem elements is the nelem bytes src[i * E + p]; the bytes of a float interleave one
 * compressible plane (sign and exponent) with mantissa planes a byte code only enlarges.  A
 * tensor's coded_mask says which planes are Huffman-coded: each is one ordinary stream of a
 * gh_ebatch / gh_batch with its own canonical code; the other planes are stored as they are.
 * One split kernel stands where gh_ebatch_load_device's copy kernel stands, one join kernel
 * after gh_batch_decode; everything between is the batched encode and decode unchanged.  No
 * reference counterpart.  (The gh_batch_*, gh_batchdec_*, gh_batchraw_* and gh_ebatch_* names
 * are closed sets pinned by tests; these carry gh_planes_.)
 *
 * Layout of a tensor list: coded planes are numbered in tensor order, then plane order, and
 * stream s has n = nelem of its tensor.  Stored planes lie in one "stored arena" by
 * gh_batch_layout's rule: each starts on a 16-byte boundary and owns round_up(nelem, 16)
 * bytes, zero past nelem. */
#define GH_PLANES_STORED 0xFFFFFFFFu
#define GH_PLANES_MAX_ELEM 8
/* "GHPLN1\0\0" little-endian */
#define GH_PLANES_MAGIC 0x0000314E4C504847ull
typedef struct gh_planes_item {
  void* data;           /* nelem * elem_size bytes, any byte alignment; host or device as the call says */
  uint64_t nelem;
  uint32_t elem_size;   /* 1, 2, 4, 8 */
  uint32_t coded_mask;  /* bit p: plane p is a coded stream; clear: stored */
} gh_planes_item;
typedef struct gh_planes_slot { uint32_t stream, pad; uint64_t stored_off; } gh_planes_slot;
typedef struct gh_planes_report {
  uint64_t out_bytes;    /* sum of nelem * elem_size                                        */
  uint32_t ntensors;
  uint32_t bad_tensors;  /* tensors with a flagged coded plane: not one byte of them written */
  float kernel_ms;       /* HIP-event time of the last timed join (the join alone)           */
  uint32_t launches;     /* what one join enqueues: a constant                               */
} gh_planes_report;
/* slots[8 * t + p] for plane p of tensor t: a coded plane's stream number and stored_off 0; a
 * stored plane's GH_PLANES_STORED and its offset in the stored arena; planes >= elem_size:
 * GH_PLANES_STORED and 0.  *nstreams: coded planes; *stored_bytes: the stored arena's size.
 * Host arithmetic only, no device.  GH_E_ARG: null pointers (items and slots may be NULL when
 * ntensors = 0), an elem_size outside {1, 2, 4, 8}, a mask >= 1 << elem_size, more than 2^24
 * coded planes, a sum that overflows 64 bits. */
int gh_planes_layout(const gh_planes_item* items, uint32_t ntensors, gh_planes_slot* slots, uint32_t* nstreams,
                     uint64_t* stored_bytes);
/* The CPU twins of the kernels: item->data is host memory, planes[p] (p < elem_size) a buffer
 * of nelem bytes.  Split reads the tensor and writes the planes, join the reverse.  GH_E_ARG:
 * null pointers (with nelem > 0), a bad elem_size.  No device. */
int gh_planes_split_host(const gh_planes_item* item, void* const* planes);
int gh_planes_join_host(const gh_planes_item* item, const void* const* planes);
/* gh_ebatch_load for tensors in host memory: a host split, then the host load of the coded
 * planes as nstreams streams; the stored planes go to `stored` (host memory, stored_len >=
 * stored_bytes: GH_E_SMALL otherwise) by the layout, zero padded.  Synchronous. */
int gh_planes_load(gh_ebatch* b, const gh_planes_item* items, uint32_t ntensors, void* stored, uint64_t stored_len);
/* gh_ebatch_load_device for tensors in device memory: one launch of the split kernel writes
 * every coded plane into the batch's padded input arena (zero past nelem, as the copy kernel
 * leaves it) and every stored plane into d_stored (device memory, 16-byte aligned: GH_E_ARG
 * otherwise; stored_len >= stored_bytes: GH_E_SMALL otherwise), zero in [nelem,
 * round_up(nelem, 16)); it reads exactly nelem * elem_size bytes per tensor.  Follows
 * hip_stream as gh_ebatch_load_device.  Synchronous.  After either load gh_ebatch_plan,
 * gh_batchenc_plan_device, encode, wait, download and items run unchanged on nstreams
 * streams.  GH_E_ARG also when the tensors have 2^31 or more work units (1024 elements). */
int gh_planes_load_device(gh_ebatch* b, const gh_planes_item* items, uint32_t ntensors, void* d_stored,
                          uint64_t stored_len, void* hip_stream);
/* HIP-event time of the split kernel of the last load when it was gh_planes_load_device (0
 * after any other load, or when the tensors had no elements).  GH_E_STATE before a load. */
int gh_planes_load_times(gh_ebatch* b, float* kernel_ms);
/* Enqueue one join kernel on hip_stream (NULL = the batch's stream) and return: it runs after
 * every earlier decode of the batch, reads the coded planes from the batch's own output arena
 * and the stored planes from d_stored, and writes exactly nelem * elem_size bytes at every
 * item's data (device memory, any alignment).  A tensor with a flagged coded plane (a nonzero
 * gh_batch_status word) is not written at all and counted; every other tensor is exact.
 * items, d_stored and the destinations must stay untouched until the wait.  GH_E_STATE unless
 * the last decode since the load wrote the batch's own arena (d_dst == NULL); GH_E_ARG: null
 * pointers, a layout whose nstreams or any n differs from the loaded batch's, a misaligned
 * d_stored; GH_E_SMALL: stored_len < stored_bytes. */
int gh_planes_join_device(gh_batch* b, const gh_planes_item* items, uint32_t ntensors, const void* d_stored,
                          uint64_t stored_len, void* hip_stream, int timed);
/* Wait for the decode and the join and report (rep may be NULL; it is filled before an error
 * is returned).  GH_E_CORRUPT when bad_tensors > 0; GH_E_STATE when no join was enqueued
 * since the load. */
int gh_planes_wait(gh_batch* b, gh_planes_report* rep);

/* ---- element gather: element ranges of compressed tensors in a fixed launch count -------- */
/* The batched gather for byte planes: element ranges (tensor, lo, hi) of a resident gh_batch
 * that holds the coded planes of a tensor list, interleaved as in the original tensors, without
 * a full decode and without the batch's output arena: gh_batch_load -> gh_batchdec_index ->
 * element gather works with no write kernel ever having run.  No reference counterpart.  (The
 * gh_planes_*, gh_batch_*, gh_batchdec_*, gh_batchraw_* and gh_ebatch_* names are closed sets
 * pinned by tests; these carry gh_pgather_.)
 *
 * items / ntensors / d_stored / stored_len are gh_planes_join_device's (items[t].data is
 * ignored).  Output layout: range i's (hi_i - lo_i) * E_i bytes start at sum_{j<i} (hi_j - lo_j)
 * * E_j of d_dst, E_j the elem_size of the tensor range j names: tight, in request order, any
 * byte alignment of d_dst.  Ranges may be empty, overlap, repeat, mix element sizes and name the
 * tensors in any order.
 *
 * One call is GH_PGATHER_LAUNCHES launches however many ranges there are: a memset, a locate
 * kernel, a one-workgroup scan and an expand kernel turn every element range into one byte range
 * (stream, lo, hi) per coded plane of its tensor; the batched gather (gh_batchdec_gather_device,
 * its memset and four kernels, as it is) decodes those into a batch-owned staging buffer; one
 * range-join kernel interleaves the staged planes with the stored planes' bytes into d_dst.
 * The call runs the batched gather inside: a later gh_batchdec_gather_wait reports that inner
 * gather.  Limits (GH_E_ARG beyond them): GH_PGATHER_MAX_RANGES ranges per call (8 byte ranges
 * per element range at the most, GH_GATHER_MAX_RANGES in all); tensors below 2^40 bytes; fewer
 * than 2^31 - nranges KiB of destination. */
#define GH_PGATHER_MAX_RANGES (GH_GATHER_MAX_RANGES / 8)
#define GH_PGATHER_LAUNCHES 10u
typedef struct gh_erange { uint64_t tensor, lo, hi; } gh_erange;   /* a contiguous int64[n,3] tensor, element units */
typedef struct gh_pgather_report {
  uint64_t out_bytes;   /* sum of (hi - lo) * elem_size over the valid ranges                */
  uint64_t npieces;     /* pieces of the inner batched gather                                */
  uint32_t bad_ranges;  /* element ranges whose tensor has a flagged coded plane             */
  uint32_t status;      /* GH_ST_RANGE | GH_ST_DSTSMALL | GH_ST_PIECES | GH_ST_BADCODE       */
  float kernel_ms;      /* HIP events: all kernels of the call                               */
  uint32_t launches;    /* kernels + memsets of one call: GH_PGATHER_LAUNCHES                */
  float expand_ms;      /* of kernel_ms: the memset and the three plan kernels               */
  float join_ms;        /* of kernel_ms: the range join (the rest is the batched gather)     */
} gh_pgather_report;
/* The device's plan from host arrays, with no device: the byte ranges in range-major, then plane
 * order into branges[0 .. cap), stage_off[i] / dst_off[i] (nranges entries each) the byte offset
 * of range i in the staging buffer (the prefix of (hi - lo) * C, C the tensor's coded planes: the
 * dst0 gh_batchdec_plan gives range i's first byte range) and in d_dst.  stream_status[s]: the
 * batch's status words (NULL: none is flagged).  *nbranges / *out_bytes / *bad_ranges are always
 * written (a first call with cap = 0 sizes the buffer; GH_E_SMALL then).  GH_E_ARG: null
 * pointers, what gh_planes_layout refuses, tensor >= ntensors, lo > hi or hi > nelem (the counts
 * are then 0).  A range whose tensor has a flagged coded plane keeps its bytes in both layouts
 * and its byte ranges and counts once in *bad_ranges; the return stays GH_OK.  A tensor without
 * coded planes gives no byte ranges. */
int gh_pgather_plan(const gh_planes_item* items, uint32_t ntensors, const uint32_t* stream_status,
                    const gh_erange* ranges, uint32_t nranges, gh_brange* branges, uint64_t cap,
                    uint64_t* nbranges, uint64_t* stage_off, uint64_t* dst_off, uint64_t* out_bytes,
                    uint32_t* bad_ranges);
/* Enqueue the gather of d_ranges[0 .. nranges) (device memory) into d_dst (device memory,
 * dst_len bytes) on hip_stream (NULL = the batch's stream), and return.  It runs after every
 * earlier decode, index or gather of the batch, whatever their streams.  d_ranges, d_stored and
 * d_dst must stay untouched until the wait.  The staging buffer (dst_len bytes: C <= E), the
 * byte ranges and the per-range offsets are the batch's; the call blocks only to grow them or to
 * upload a tensor list that differs from the previous call's: a repeated call with the same
 * items and the same or a smaller nranges and dst_len allocates nothing and only enqueues.
 * timed != 0 brackets the kernels with HIP events.  nranges = 0: GH_OK, nothing is launched.
 * GH_E_STATE before an index or decode since the load; GH_E_ARG: null pointers, more than
 * GH_PGATHER_MAX_RANGES ranges, a layout whose nstreams or any n differs from the loaded
 * batch's, a misaligned d_stored; GH_E_SMALL: stored_len < stored_bytes. */
int gh_pgather_device(gh_batch* b, const gh_planes_item* items, uint32_t ntensors, const void* d_stored,
                      uint64_t stored_len, const gh_erange* d_ranges, uint32_t nranges, void* d_dst,
                      uint64_t dst_len, void* hip_stream, int timed);
/* Wait for the batch's last element gather and report it (rep may be NULL; it is filled before
 * an error is returned).  GH_E_ARG: some range had tensor >= ntensors, lo > hi or hi > nelem
 * (GH_ST_RANGE); GH_E_SMALL: the ranges' bytes exceed dst_len (GH_ST_DSTSMALL); GH_E_CORRUPT:
 * the inner plan would exceed its piece buffer (GH_ST_PIECES); after these three not one byte of
 * d_dst has been written.  GH_E_CORRUPT also when a range's tensor has a coded plane whose
 * stream status word is non-zero (GH_ST_BADCODE in the report): such a range keeps its bytes in
 * the layout and leaves them as they were, every other range is exact, and bad_ranges counts
 * them, once per element range.  GH_E_STATE when no element gather was enqueued since the load. */
int gh_pgather_wait(gh_batch* b, gh_pgather_report* rep);
/* The same with the ranges in host memory: uploads them, then gh_pgather_device (timed) and
 * gh_pgather_wait.  Synchronous.  rep may be NULL. */
int gh_pgather(gh_batch* b, const gh_planes_item* items, uint32_t ntensors, const void* d_stored,
               uint64_t stored_len, const gh_erange* ranges /* host */, uint32_t nranges, void* d_dst,
               uint64_t dst_len, void* hip_stream, gh_pgather_report* rep);

/* ---- plane choice: every tensor's coded planes from its own bytes ----------------------- */
/* Which planes of a tensor are worth coding, by exact size.  For plane p < E of tensor t with
 * nelem > 0, fb(t, p) is gh_encode_plan_from_counts(counts of the plane's bytes, 0).file_bytes:
 * the size of the compressed.huff image gh_encode_write makes of the plane.  The plane is coded
 * iff fb(t, p) < nelem; a tie is stored; a tensor with nelem = 0 gets mask 0.  Containers align
 * planes to 8 bytes and fb < nelem implies round_up8(fb) <= round_up8(nelem), so the chosen
 * mask gives a container no larger than any other mask's and never larger than the all-stored
 * one.  One definition for CPU and GPU (csrc/gh_pmask.hpp).  No reference counterpart.  (The
 * gh_planes_*, gh_pgather_*, gh_batch*_ and gh_ebatch_* names are closed sets pinned by tests;
 * these carry gh_pmask_.)
 *
 * Candidate planes are numbered in tensor order, then plane order, over ALL E planes of every
 * tensor: q = q0[t] + p, q0[t] the sum of E_j for j < t.  items[t].coded_mask and, where the
 * call takes counts, items[t].data are ignored.  masks[t]: the chosen mask; plane_bytes[8 t + p]
 * (may be NULL): fb(t, p) of every candidate, chosen or not, 0 for p >= E and for nelem = 0. */
#define GH_PMASK_LAUNCHES 4u   /* memset of the counts, histogram, code, decide */
typedef struct gh_pmask_report {
  uint64_t raw_bytes, chosen_bytes;   /* sum nelem*E; sum over planes of min-by-rule size */
  uint32_t ntensors, coded_planes;    /* planes the rule codes */
  float hist_ms, code_ms, decide_ms;  /* HIP events */
  uint32_t launches;                  /* GH_PMASK_LAUNCHES */
} gh_pmask_report;
/* The masks from byte counts, counts[q][256] in candidate order.  No device.  GH_E_ARG: null
 * pointers (all may be NULL when ntensors = 0), an elem_size outside {1, 2, 4, 8}, a plane whose
 * counts do not sum to nelem, more than 2^24 candidate planes. */
int gh_pmask_from_counts(const uint64_t* counts, const gh_planes_item* items, uint32_t ntensors, uint32_t* masks,
                         uint64_t* plane_bytes);
/* The same from tensors in host memory: scalar histograms of exactly nelem * elem_size bytes
 * per tensor, at any alignment, then the function above.  No device. */
int gh_pmask_host(const gh_planes_item* items, uint32_t ntensors, uint32_t* masks, uint64_t* plane_bytes);
/* The same from tensors in device memory (any alignment; exactly nelem * elem_size bytes of
 * each are read), in GH_PMASK_LAUNCHES launches however many tensors there are: a memset of
 * the counts, one histogram kernel over units of 1024 elements, the batched encode's code kernel
 * on the nplanes histograms, one decide kernel; then one read-back of the masks and sizes (4 +
 * 64 bytes per tensor) into masks / plane_bytes (host memory).  Synchronous; follows hip_stream
 * as gh_ebatch_load_device does (the kernels run on the batch's stream after what hip_stream
 * holds now).  It works in buffers of its own inside the batch and leaves the batch's load,
 * plan and encode state untouched: legal before any load, and between a plan and an encode.
 * ntensors = 0: GH_OK, nothing is launched.  GH_E_ARG: null pointers, what gh_pmask_from_counts
 * refuses, 2^31 or more units of 1024 elements.  rep may be NULL. */
int gh_pmask_device(gh_ebatch* b, const gh_planes_item* items, uint32_t ntensors, uint32_t* masks,
                    uint64_t* plane_bytes, void* hip_stream, gh_pmask_report* rep);
/* The byte counts of candidate plane `plane` as the last gh_pmask_device left them.
 * GH_E_STATE before one; GH_E_ARG: no such candidate. */
int gh_pmask_counts(gh_ebatch* b, uint32_t plane, uint64_t counts[256]);

/* The container, one tensor per image, little-endian: u64 GH_PLANES_MAGIC, u32 elem_size, u32
 * coded_mask, u64 nelem, elem_size x u64 plane_bytes; then the planes in order, each at the
 * next 8-byte aligned offset.  A coded plane is a whole compressed.huff image, a stored plane
 * nelem raw bytes. */
typedef struct gh_planes_image {
  uint64_t nelem;
  uint32_t elem_size, coded_mask;
  const void* plane[GH_PLANES_MAX_ELEM];        /* views into the file                        */
  uint64_t plane_bytes[GH_PLANES_MAX_ELEM];
  gh_stream stream[GH_PLANES_MAX_ELEM];         /* coded planes: gh_stream_parse's output     */
} gh_planes_image;
/* *total: the container's size for planes of plane_bytes[0 .. elem_size).  GH_E_ARG: nulls, a
 * bad elem_size, a sum that overflows. */
int gh_planes_image_bytes(uint32_t elem_size, const uint64_t* plane_bytes, uint64_t* total);
/* Write the container of item (nelem, elem_size, coded_mask; data is not read) from
 * planes[p] / plane_bytes[p]; gaps between planes are zero.  GH_E_ARG: nulls, a bad elem_size
 * or mask, a stored plane whose plane_bytes is not nelem; GH_E_SMALL: out_len too small. */
int gh_planes_image_write(const gh_planes_item* item, const void* const* planes, const uint64_t* plane_bytes,
                          void* out, uint64_t out_len);
/* Parse a container (views into `file`).  GH_E_FORMAT unless: the magic, elem_size and the
 * mask are right, every plane lies inside the file, a stored plane has exactly nelem bytes
 * and every coded plane passes gh_stream_parse with n == nelem. */
int gh_planes_parse(const void* file, size_t file_len, gh_planes_image* out);

/* One-shot decode of a whole stream into host memory `out` (out_len >= N):
 * mirrors decoder_l1_l2 (decoder.cu:732-815) without its 200-iteration loop.
 * ngpus <= 0 or 1: device `devices ? devices[0] : 0`; ngpus > 1 shards the
 * segments evenly over `devices` (or 0..ngpus-1; a device may repeat), decodes each
 * shard on its own device, and places shard outputs at the scanned offsets.  Each
 * shard is loaded, decoded and downloaded from its own host thread through pinned
 * double-buffered copies, so the shards' PCIe transfers overlap across devices (the
 * reference's launcher runs one device after another, decoder.cu:759-801).
 * rep->kernel_ms: per device the SUM of its shards' average decode times (decodes on
 * one device run in turn), the maximum over devices. */
typedef struct gh_opts {
  int ngpus;
  const int* devices;
  int reps;          /* decode repetitions (timing); <= 1 means one             */
} gh_opts;
int gh_decode(const gh_stream* s, uint8_t* out, uint64_t out_len, const gh_opts* opts,
              gh_report* rep);

/* One-shot sliced encode of host memory: the input is cut evenly into nslices byte ranges,
 * slice i goes to device opts->devices[i % ngpus] (or i % ngpus; ngpus <= 1: device
 * `devices ? devices[0] : 0`; a device may repeat, as in gh_decode), one host thread per
 * device and one gh_ectx per slice: load and gh_ectx_counts, then the plan from the summed
 * counts, then gh_ectx_encode_slice at the scanned bit offsets, and the slices merged in
 * order into out.  The image is byte-identical to gh_encode_write's.  *plan (may be NULL)
 * is filled before out_len is checked (GH_E_SMALL when out_len < plan->file_bytes;
 * gh_encode_bound(n) always suffices).  kernel_ms (may be NULL): per device the sum of its
 * slices' encode times, the maximum over devices (gh_decode's convention). */
int gh_encode_sharded(const uint8_t* in, uint64_t n, const gh_opts* opts, uint32_t nslices,
                      int force_version, void* out, uint64_t out_len, gh_encode_plan* plan,
                      float* kernel_ms);
/* gh_encode_sharded plus the stream's seek index (gh_index_bytes(plan->g, log2_stride)
 * bytes into index_out; byte-identical to gh_encode_index's): the same two passes, each
 * slice's context also running gh_ectx_index_slice (sym_base = the slice's first byte)
 * right after its slice encode, and the calling thread gh_index_image_init and the
 * gh_index_slice_merge calls.  No host pass over the input.  index_ms (may be NULL): the
 * index kernels' time, by kernel_ms's convention (per device the sum over its slices, the
 * maximum over devices).  GH_E_ARG also for a stride outside the range (before any device
 * work); GH_E_SMALL also when index_len is too small (checked once the plan is known:
 * gh_index_bytes(ceil(n / 8), log2_stride) always suffices). */
int gh_encode_sharded_index(const uint8_t* in, uint64_t n, const gh_opts* opts, uint32_t nslices,
                            int force_version, void* out, uint64_t out_len, gh_encode_plan* plan,
                            float* kernel_ms, uint32_t log2_stride, void* index_out, uint64_t index_len,
                            float* index_ms);

/* Evenly split G segments into `nshards` contiguous ranges: bounds[0..nshards]. */
int gh_plan_shards(uint64_t g, uint32_t nshards, uint64_t* bounds);

/* Device memory for FFI callers without a HIP binding (buffers for gh_sync_gaps /
 * gh_ctx_load_device).  gh_dev_copy: any direction (unified addressing). */
int gh_dev_alloc(int device, uint64_t bytes, void** out);
int gh_dev_free(void* p);
int gh_dev_copy(void* dst, const void* src, uint64_t bytes);

/* Diagnostic yardstick: one streaming copy of `bytes` (multiple of
 * 16, 16-byte aligned device buffers) on `hip_stream` (NULL = default stream) of the
 * current device, repeated `reps` times after one warm-up pass; *ms_avg = HIP-event
 * time per pass.  The decode's roofline is quoted as a fraction of this rate.  No
 * reference counterpart (the reference measures nothing on the device). */
int gh_bw_copy(void* dst, const void* src, uint64_t bytes, void* hip_stream, int reps, float* ms_avg);

/* Number of visible HIP devices (0 when none / no driver). */
int gh_device_count(void);
/* Library version string. */
const char* gh_version(void);
/* Last error message of the calling thread (empty when none). */
const char* gh_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GAPHUFF_H_ */
