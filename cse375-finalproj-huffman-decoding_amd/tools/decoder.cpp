// bin/decoder <compressed.huff | raw container> <output> [--gpus N] [--shards S] [--reps R] [--json]
//             [--verify FILE] [--write-index FILE [--index-stride K]] [--index FILE --range LO:HI]
//             [--index FILE --ranges FILE]
// bin/decoder --batch LIST [--ranges FILE OUT | --elements FILE OUT]
// --batch LIST (a text file, one input<TAB>output per line) decodes all inputs as one batch
// (gh_batch_*: one fixed set of launches however many streams) and writes every output.
// When every input is a raw container the batch is loaded by gh_batchraw_load (the gap arrays
// are built on the GPU); a list that mixes the two kinds is refused.
// When every input is a byte-plane container (bin/encoder --batch LIST --planes E, GH_PLANES_MAGIC)
// the coded planes of all tensors are the batch's streams and one join kernel after the decode
// interleaves them with the stored planes (gh_planes_join_device); every output is a tensor's bytes.
// --batch LIST --ranges FILE OUT (FILE: one `STREAM LO:HI` per line, STREAM the 0-based line
// of LIST, blank lines not counted) indexes the batch without decoding it and gathers only the
// named byte ranges (gh_batchdec_*); their concatenation in file order goes to OUT and the
// per-input outputs of LIST are not written (its lines may then omit <TAB>output).
// --batch LIST --elements FILE OUT (every input a byte-plane container; FILE: one `TENSOR LO:HI`
// per line, TENSOR the 0-based line of LIST, LO:HI in elements) indexes the batch without decoding
// it and gathers only the named element ranges (gh_pgather_*), interleaved as in the tensors;
// their concatenation in file order goes to OUT.  --ranges stays refused for containers.
// --shards S (default: one per GPU) splits the gap segments into S shards, shard k on
// device k mod N, each streaming its own payload range and writing at its offset.
// A raw-stream container (bin/encoder --raw, GH_RAW_MAGIC) is decoded by the
// self-synchronising path (gh_ctx_load_raw) on one GPU.
// --write-index FILE (single-shard runs) builds the stream's seek index on the GPU after
// the load, one entry per 2^K segments (--index-stride K, 8..20, default 8), and writes
// the sidecar image.  --index FILE --range LO:HI decodes only the segments that hold
// output bytes [LO, HI) and writes just those bytes to the output.
// --index FILE --ranges FILE (a text file, one LO:HI per line) loads the whole stream once
// and decodes every range in one launch (gh_ctx_gather); the output is their
// concatenation in file order.
//
// Drop-in for the reference decoder CLI (Huffman_coding_Gap_arrays/decoder/src/
// huff.cpp:22-142, used as `./bin/decoder in out` by run_huffman.sh:38), decoding on
// MI355X through the gaphuff C ABI.  Differences from the reference, on purpose:
//   * the output goes to argv[2] (the reference always wrote "decodedfile", :32);
//   * malformed input exits non-zero with a message instead of decoding garbage;
//   * the decode kernel is timed per launch (hipEvents) instead of a wall-clock
//     span over 200 iterations + allocations (:106-129, decoder.cu:760).
// The reference's stdout lines are kept so existing log parsers keep working.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "gaphuff.h"

static double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// Runs f(k) for every shard in its own host thread; the first failure's code, with its
// message re-raised on the calling thread (gh_last_error is per thread).
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
      std::fprintf(stderr, "decoder: shard %d: %s\n", k, msg[k].c_str());
      return rc[k];
    }
  return GH_OK;
}

static int die(const char* what, int rc) {
  std::fprintf(stderr, "decoder: %s (code %d): %s\n", what, rc, gh_last_error());
  return 1;
}

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  out.resize((size_t)std::max(std::ftell(f), 0L));
  std::fseek(f, 0, SEEK_SET);
  const bool ok = std::fread(out.data(), 1, out.size(), f) == out.size();
  std::fclose(f);
  return ok;
}

// --index FILE --ranges FILE: the whole stream loaded once, every range of the text file
// (one LO:HI per line; blank lines skipped) decoded in one launch, the concatenation
// written to `output`.
static int gather_main(const char* input, const char* output, const char* index_file, const char* ranges_file) {
  std::vector<uint8_t> ix_img, text;
  gh_index ix{};
  if (!read_file(index_file, ix_img)) { std::fprintf(stderr, "decoder: Could not open index file %s\n", index_file); return 1; }
  int rc = gh_index_parse(ix_img.data(), ix_img.size(), &ix);
  if (rc) return die("bad index", rc);
  if (!read_file(ranges_file, text)) { std::fprintf(stderr, "decoder: Could not open ranges file %s\n", ranges_file); return 1; }
  text.push_back(0);
  std::vector<gh_range> ranges;
  for (const char* p = (const char*)text.data(); *p;) {
    while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
    if (!*p) break;
    char* end = nullptr;
    gh_range r{};
    bool ok = *p >= '0' && *p <= '9';
    if (ok) r.lo = std::strtoull(p, &end, 10);
    ok = ok && *end == ':' && end[1] >= '0' && end[1] <= '9';
    if (ok) {
      p = end + 1;
      r.hi = std::strtoull(p, &end, 10);
      ok = *end == 0 || *end == ' ' || *end == '\t' || *end == '\r' || *end == '\n';
    }
    if (!ok || ranges.size() >= 0xFFFFFFFFull) {
      std::fprintf(stderr, "decoder: %s: range %zu: expected LO:HI\n", ranges_file, ranges.size() + 1);
      return 1;
    }
    ranges.push_back(r);
    p = end;
  }
  uint64_t npieces = 0, total = 0;
  rc = gh_gather_plan(&ix, ranges.data(), (uint32_t)ranges.size(), nullptr, 0, &npieces, &total);
  if (rc && rc != GH_E_SMALL) return die("bad range", rc);
  if (gh_device_count() < 1) return die("no HIP device", GH_E_NODEV);
  gh_ctx* ctx = nullptr;
  gh_file_info info{};
  const double t0 = now_ms();
  if ((rc = gh_ctx_create(0, &ctx))) return die("device init", rc);
  if ((rc = gh_ctx_load_file(ctx, input, 0, UINT64_MAX, 0, &info))) { gh_ctx_destroy(ctx); return die("bad compressed stream / upload", rc); }
  if (info.n != ix.n || info.g != ix.g) {
    gh_ctx_destroy(ctx);
    std::fprintf(stderr, "decoder: the index is for another stream (N or G differ)\n");
    return 1;
  }
  std::vector<uint8_t> out((size_t)total);
  float ms = 0;
  const double t1 = now_ms();
  rc = gh_ctx_gather(ctx, &ix, ranges.data(), (uint32_t)ranges.size(), out.data(), out.size(), nullptr, &ms);
  const double t2 = now_ms();
  gh_ctx_destroy(ctx);
  if (rc) return die("gather", rc);
  FILE* f = std::fopen(output, "wb");
  bool okw = f && std::fwrite(out.data(), 1, out.size(), f) == out.size();
  if (f) okw = std::fclose(f) == 0 && okw;
  if (!okw) { std::fprintf(stderr, "decoder: cannot write %s\n", output); return 1; }
  std::printf("Input file: %s\n", input);
  std::printf("Original size: %llu bytes\n", (unsigned long long)info.n);
  std::printf("Gather: %zu ranges, %llu pieces, %llu bytes; load %.3f ms, kernel %.3f ms, call %.3f ms\n", ranges.size(),
              (unsigned long long)npieces, (unsigned long long)total, t1 - t0, ms, t2 - t1);
  return 0;
}

// A list of byte-plane containers (img[i], all read): their coded planes decoded as one batch,
// joined with the stored planes on the device, every tensor written to out[i].  A corrupt
// plane: exit code 1, its tensor's line named, no output written for it.
static int planes_batch_main(const char* list_file, const std::vector<std::string>& in, const std::vector<std::string>& out,
                             const std::vector<size_t>& line_of, const std::vector<std::vector<uint8_t>>& img) {
  const size_t nt = in.size();
  std::vector<gh_planes_image> im(nt);
  std::vector<gh_planes_item> items(nt);
  std::vector<gh_planes_slot> slots(8 * std::max<size_t>(nt, 1));
  int rc;
  for (size_t i = 0; i < nt; ++i) {
    if ((rc = gh_planes_parse(img[i].data(), img[i].size(), &im[i]))) {
      std::fprintf(stderr, "decoder: %s: line %zu: %s: ", list_file, line_of[i], in[i].c_str());
      return die("bad byte-plane container", rc);
    }
    items[i] = gh_planes_item{nullptr, im[i].nelem, im[i].elem_size, im[i].coded_mask};
  }
  uint32_t ns = 0;
  uint64_t stored_bytes = 0;
  if ((rc = gh_planes_layout(items.data(), (uint32_t)nt, slots.data(), &ns, &stored_bytes))) return die("layout", rc);
  std::vector<gh_stream> streams(ns);
  std::vector<uint8_t> stored((size_t)stored_bytes, 0);
  std::vector<uint64_t> dst_off(nt + 1, 0);
  for (size_t i = 0; i < nt; ++i) {
    for (uint32_t p = 0; p < im[i].elem_size; ++p) {
      const gh_planes_slot& sl = slots[8 * i + p];
      if (sl.stream != GH_PLANES_STORED) streams[sl.stream] = im[i].stream[p];
      else if (im[i].nelem) std::memcpy(stored.data() + sl.stored_off, im[i].plane[p], (size_t)im[i].nelem);
    }
    dst_off[i + 1] = dst_off[i] + ((im[i].nelem * im[i].elem_size + 15) & ~15ull);
  }
  if (gh_device_count() < 1) return die("no HIP device", GH_E_NODEV);
  gh_batch* b = nullptr;
  void *d_dst = nullptr, *d_stored = nullptr;
  auto done = [&](int r) {
    if (d_dst) gh_dev_free(d_dst);
    if (d_stored) gh_dev_free(d_stored);
    gh_batch_destroy(b);
    return r;
  };
  if ((rc = gh_batch_create(0, &b))) return die("device init", rc);
  const double t0 = now_ms();
  if ((rc = gh_batch_load(b, streams.data(), ns))) return done(die("batch load", rc));
  const double t1 = now_ms();
  if ((rc = gh_dev_alloc(0, std::max<uint64_t>(dst_off[nt], 16), &d_dst)) ||
      (rc = gh_dev_alloc(0, std::max<uint64_t>(stored_bytes, 16), &d_stored)) ||
      (stored_bytes && (rc = gh_dev_copy(d_stored, stored.data(), stored_bytes))))
    return done(die("device allocation", rc));
  for (size_t i = 0; i < nt; ++i) items[i].data = (uint8_t*)d_dst + dst_off[i];
  gh_planes_report rep{};
  if ((rc = gh_batch_decode(b, nullptr, 0, nullptr, 1)) ||
      (rc = gh_planes_join_device(b, items.data(), (uint32_t)nt, d_stored, stored_bytes, nullptr, 1)))
    return done(die("batch decode", rc));
  rc = gh_planes_wait(b, &rep);
  const double t2 = now_ms();
  std::vector<uint32_t> status(std::max<uint32_t>(ns, 1), 0);
  std::vector<bool> bad(nt, false);
  if (rc == GH_E_CORRUPT && gh_batch_status(b, status.data(), nullptr, ns) == GH_OK) {
    for (size_t i = 0; i < nt; ++i)
      for (uint32_t p = 0; p < im[i].elem_size; ++p) {
        const uint32_t sidx = slots[8 * i + p].stream;
        if (sidx == GH_PLANES_STORED || !status[sidx]) continue;
        bad[i] = true;
        std::fprintf(stderr, "decoder: %s: line %zu: %s: plane %u: corrupt stream (status 0x%x)\n", list_file, line_of[i],
                     in[i].c_str(), p, status[sidx]);
      }
  } else if (rc) {
    return done(die("byte-plane join", rc));
  }
  std::vector<uint8_t> bytes;
  for (size_t i = 0; i < nt; ++i) {
    if (bad[i]) continue;
    bytes.resize((size_t)(im[i].nelem * im[i].elem_size));
    int r = bytes.empty() ? GH_OK : gh_dev_copy(bytes.data(), items[i].data, bytes.size());
    if (r) return done(die("download", r));
    FILE* f = std::fopen(out[i].c_str(), "wb");
    bool okw = f && std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (f) okw = std::fclose(f) == 0 && okw;
    if (!okw) { std::fprintf(stderr, "decoder: cannot write %s\n", out[i].c_str()); return done(1); }
  }
  std::printf("Planes batch: %u tensors, %u coded planes, %llu bytes; load %.3f ms, join kernel %.3f ms, call %.3f ms, %u bad\n",
              rep.ntensors, ns, (unsigned long long)rep.out_bytes, t1 - t0, rep.kernel_ms, t2 - t1, rep.bad_tensors);
  return done(rc ? 1 : 0);
}

// --batch LIST --elements FILE OUT on a list of byte-plane containers (img[i], all read): the
// coded planes loaded and indexed, the stored planes uploaded, the element ranges of FILE (one
// `TENSOR LO:HI` per line) gathered by one gh_pgather call, their bytes written to OUT.
static int planes_elements_main(const char* list_file, const std::vector<std::string>& in, const std::vector<size_t>& line_of,
                                const std::vector<std::vector<uint8_t>>& img, const char* ranges_file, const char* range_out) {
  const size_t nt = in.size();
  std::vector<gh_planes_image> im(nt);
  std::vector<gh_planes_item> items(nt);
  std::vector<gh_planes_slot> slots(8 * std::max<size_t>(nt, 1));
  int rc;
  for (size_t i = 0; i < nt; ++i) {
    if ((rc = gh_planes_parse(img[i].data(), img[i].size(), &im[i]))) {
      std::fprintf(stderr, "decoder: %s: line %zu: %s: ", list_file, line_of[i], in[i].c_str());
      return die("bad byte-plane container", rc);
    }
    items[i] = gh_planes_item{nullptr, im[i].nelem, im[i].elem_size, im[i].coded_mask};
  }
  uint32_t ns = 0;
  uint64_t stored_bytes = 0;
  if ((rc = gh_planes_layout(items.data(), (uint32_t)nt, slots.data(), &ns, &stored_bytes))) return die("layout", rc);
  std::vector<gh_stream> streams(ns);
  std::vector<uint8_t> stored((size_t)stored_bytes, 0);
  for (size_t i = 0; i < nt; ++i)
    for (uint32_t p = 0; p < im[i].elem_size; ++p) {
      const gh_planes_slot& sl = slots[8 * i + p];
      if (sl.stream != GH_PLANES_STORED) streams[sl.stream] = im[i].stream[p];
      else if (im[i].nelem) std::memcpy(stored.data() + sl.stored_off, im[i].plane[p], (size_t)im[i].nelem);
    }
  std::vector<gh_erange> ranges;
  std::vector<uint8_t> rtext;
  if (!read_file(ranges_file, rtext)) { std::fprintf(stderr, "decoder: Could not open ranges file %s\n", ranges_file); return 1; }
  rtext.push_back(0);
  uint64_t total = 0;
  for (const char* p = (const char*)rtext.data(); *p;) {
    while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
    if (!*p) break;
    char* end = nullptr;
    gh_erange r{};
    bool ok = *p >= '0' && *p <= '9';
    if (ok) r.tensor = std::strtoull(p, &end, 10);
    ok = ok && (*end == ' ' || *end == '\t');
    if (ok) {
      p = end;
      while (*p == ' ' || *p == '\t') ++p;
      ok = *p >= '0' && *p <= '9';
    }
    if (ok) r.lo = std::strtoull(p, &end, 10);
    ok = ok && *end == ':' && end[1] >= '0' && end[1] <= '9';
    if (ok) {
      p = end + 1;
      r.hi = std::strtoull(p, &end, 10);
      ok = *end == 0 || *end == ' ' || *end == '\t' || *end == '\r' || *end == '\n';
    }
    if (!ok || ranges.size() >= GH_PGATHER_MAX_RANGES) {
      std::fprintf(stderr, "decoder: %s: range %zu: expected TENSOR LO:HI\n", ranges_file, ranges.size() + 1);
      return 1;
    }
    if (r.tensor >= nt || r.lo > r.hi || r.hi > im[r.tensor].nelem) {
      std::fprintf(stderr, "decoder: %s: range %zu: no such tensor, or elements outside [0, nelem] of it\n", ranges_file, ranges.size() + 1);
      return 1;
    }
    total += (r.hi - r.lo) * im[r.tensor].elem_size;
    ranges.push_back(r);
    p = end;
  }
  if (gh_device_count() < 1) return die("no HIP device", GH_E_NODEV);
  gh_batch* b = nullptr;
  void *d_dst = nullptr, *d_stored = nullptr;
  auto done = [&](int r) {
    if (d_dst) gh_dev_free(d_dst);
    if (d_stored) gh_dev_free(d_stored);
    gh_batch_destroy(b);
    return r;
  };
  if ((rc = gh_batch_create(0, &b))) return die("device init", rc);
  const double t0 = now_ms();
  if ((rc = gh_batch_load(b, streams.data(), ns))) return done(die("batch load", rc));
  const double t1 = now_ms();
  if ((rc = gh_dev_alloc(0, std::max<uint64_t>(total, 16), &d_dst)) ||
      (rc = gh_dev_alloc(0, std::max<uint64_t>(stored_bytes, 16), &d_stored)) ||
      (stored_bytes && (rc = gh_dev_copy(d_stored, stored.data(), stored_bytes))))
    return done(die("device allocation", rc));
  gh_pgather_report rep{};
  if ((rc = gh_batchdec_index(b, nullptr, 1)) == GH_OK)
    rc = gh_pgather(b, items.data(), (uint32_t)nt, d_stored, stored_bytes, ranges.data(), (uint32_t)ranges.size(), d_dst, total,
                    nullptr, &rep);
  const double t2 = now_ms();
  if (rc == GH_E_CORRUPT && rep.bad_ranges) {
    std::vector<uint32_t> status(std::max<uint32_t>(ns, 1), 0);
    if (gh_batch_status(b, status.data(), nullptr, ns) == GH_OK)
      for (size_t i = 0; i < nt; ++i)
        for (uint32_t p = 0; p < im[i].elem_size; ++p) {
          const uint32_t sidx = slots[8 * i + p].stream;
          if (sidx != GH_PLANES_STORED && status[sidx])
            std::fprintf(stderr, "decoder: %s: line %zu: %s: plane %u: corrupt stream (status 0x%x)\n", list_file, line_of[i],
                         in[i].c_str(), p, status[sidx]);
        }
  }
  std::vector<uint8_t> bytes((size_t)total);
  if (rc == GH_OK && total) rc = gh_dev_copy(bytes.data(), d_dst, total);
  if (rc) return done(die("element gather", rc));
  FILE* f = std::fopen(range_out, "wb");
  bool okw = f && std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
  if (f) okw = std::fclose(f) == 0 && okw;
  if (!okw) { std::fprintf(stderr, "decoder: cannot write %s\n", range_out); return done(1); }
  std::printf("Element gather: %zu tensors, %zu ranges, %llu pieces, %llu bytes; load %.3f ms, kernels %.3f ms, call %.3f ms\n", nt,
              ranges.size(), (unsigned long long)rep.npieces, (unsigned long long)total, t1 - t0, rep.kernel_ms, t2 - t1);
  return done(0);
}

// --batch LIST: every line of the text file is `input<TAB>output`; all inputs are decoded as
// one batch (gh_batch_*) and every output file is written.  A corrupt stream: exit code 1,
// its line named, no output written for it.
// With ranges_file / range_out: --batch LIST --ranges FILE OUT, the byte ranges alone; with
// `elements` as well: --batch LIST --elements FILE OUT, element ranges of byte-plane containers.
static int batch_main(const char* list_file, const char* ranges_file = nullptr, const char* range_out = nullptr,
                      bool elements = false) {
  std::vector<uint8_t> text;
  if (!read_file(list_file, text)) { std::fprintf(stderr, "decoder: Could not open batch list %s\n", list_file); return 1; }
  std::vector<std::string> in, out;
  std::vector<size_t> line_of;
  {
    const std::string t(text.begin(), text.end());
    size_t at = 0, line = 0;
    while (at < t.size()) {
      size_t nl = t.find('\n', at);
      if (nl == std::string::npos) nl = t.size();
      std::string ln = t.substr(at, nl - at);
      at = nl + 1;
      ++line;
      if (!ln.empty() && ln.back() == '\r') ln.pop_back();
      if (ln.empty()) continue;
      const size_t tab = ln.find('\t');
      if (ranges_file && tab == std::string::npos) {  // (no per-input output is written)
        in.push_back(ln);
        out.push_back("");
        line_of.push_back(line);
        continue;
      }
      if (tab == std::string::npos || tab == 0 || tab + 1 == ln.size()) {
        std::fprintf(stderr, "decoder: %s: line %zu: expected input<TAB>output\n", list_file, line);
        return 1;
      }
      in.push_back(ln.substr(0, tab));
      out.push_back(ln.substr(tab + 1));
      line_of.push_back(line);
    }
  }
  const size_t ns = in.size();
  std::vector<std::vector<uint8_t>> img(ns);
  std::vector<gh_stream> streams(ns);
  std::vector<gh_raw_stream> raws;  // a list of raw containers: the batch's gap arrays are built on the GPU
  bool raw = false, planes = false;
  int rc;
  for (size_t i = 0; i < ns; ++i) {
    if (!read_file(in[i].c_str(), img[i])) {
      std::fprintf(stderr, "decoder: %s: line %zu: Could not open input file %s\n", list_file, line_of[i], in[i].c_str());
      return 1;
    }
    uint64_t magic = 0;
    if (img[i].size() >= 8) std::memcpy(&magic, img[i].data(), 8);
    const bool is_raw = magic == GH_RAW_MAGIC, is_planes = magic == GH_PLANES_MAGIC;
    if (i == 0) raw = is_raw, planes = is_planes;
    if (is_planes != planes) {
      std::fprintf(stderr, "decoder: %s: line %zu: %s is %s, the lines before it are %s: a batch is all byte-plane "
                           "containers or none\n", list_file, line_of[i], in[i].c_str(),
                   is_planes ? "a byte-plane container" : "no byte-plane container",
                   planes ? "byte-plane containers" : "compressed streams");
      return 1;
    }
    if (planes) continue;
    if (is_raw != raw) {
      std::fprintf(stderr, "decoder: %s: line %zu: %s is %s, the lines before it are %s: a batch is all raw containers or all "
                           "compressed.huff files\n", list_file, line_of[i], in[i].c_str(), is_raw ? "a raw container" : "a compressed.huff file",
                   raw ? "raw containers" : "compressed.huff files");
      return 1;
    }
    if (raw) {
      gh_raw_stream r;
      if ((rc = gh_raw_parse(img[i].data(), img[i].size(), &r))) {
        std::fprintf(stderr, "decoder: %s: line %zu: %s: ", list_file, line_of[i], in[i].c_str());
        return die("bad raw stream", rc);
      }
      raws.push_back(r);
      streams[i].n = r.n;  // (what the ranges and the downloads below read)
    } else if ((rc = gh_stream_parse(img[i].data(), img[i].size(), &streams[i]))) {
      std::fprintf(stderr, "decoder: %s: line %zu: %s: ", list_file, line_of[i], in[i].c_str());
      return die("bad compressed stream", rc);
    }
  }
  if (elements) {
    if (!planes) {
      std::fprintf(stderr, "decoder: %s: --elements takes byte-plane containers only (--ranges gathers bytes of compressed streams)\n", list_file);
      return 1;
    }
    return planes_elements_main(list_file, in, line_of, img, ranges_file, range_out);
  }
  if (planes) {
    if (ranges_file) {
      std::fprintf(stderr, "decoder: %s: --ranges takes no byte-plane containers (gather a plane's stream instead)\n", list_file);
      return 1;
    }
    return planes_batch_main(list_file, in, out, line_of, img);
  }
  if (gh_device_count() < 1) return die("no HIP device", GH_E_NODEV);
  gh_batch* b = nullptr;
  if ((rc = gh_batch_create(0, &b))) return die("device init", rc);
  const double t0 = now_ms();
  if ((rc = raw ? gh_batchraw_load(b, raws.data(), (uint32_t)ns) : gh_batch_load(b, streams.data(), (uint32_t)ns))) {
    gh_batch_destroy(b);
    return die("batch load", rc);
  }
  const double t1 = now_ms();
  if (ranges_file) {
    std::vector<gh_brange> ranges;
    std::vector<uint8_t> rtext;
    if (!read_file(ranges_file, rtext)) { gh_batch_destroy(b); std::fprintf(stderr, "decoder: Could not open ranges file %s\n", ranges_file); return 1; }
    rtext.push_back(0);
    uint64_t total = 0;
    for (const char* p = (const char*)rtext.data(); *p;) {
      while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
      if (!*p) break;
      char* end = nullptr;
      gh_brange r{};
      bool ok = *p >= '0' && *p <= '9';
      if (ok) r.stream = std::strtoull(p, &end, 10);
      ok = ok && (*end == ' ' || *end == '\t');
      if (ok) {
        p = end;
        while (*p == ' ' || *p == '\t') ++p;
        ok = *p >= '0' && *p <= '9';
      }
      if (ok) r.lo = std::strtoull(p, &end, 10);
      ok = ok && *end == ':' && end[1] >= '0' && end[1] <= '9';
      if (ok) {
        p = end + 1;
        r.hi = std::strtoull(p, &end, 10);
        ok = *end == 0 || *end == ' ' || *end == '\t' || *end == '\r' || *end == '\n';
      }
      if (!ok || ranges.size() >= GH_GATHER_MAX_RANGES) {
        gh_batch_destroy(b);
        std::fprintf(stderr, "decoder: %s: range %zu: expected STREAM LO:HI\n", ranges_file, ranges.size() + 1);
        return 1;
      }
      if (r.stream >= ns || r.lo > r.hi || r.hi > streams[r.stream].n) {
        gh_batch_destroy(b);
        std::fprintf(stderr, "decoder: %s: range %zu: no such stream, or bytes outside [0, N] of it\n", ranges_file, ranges.size() + 1);
        return 1;
      }
      total += r.hi - r.lo;
      ranges.push_back(r);
      p = end;
    }
    void* d_dst = nullptr;
    if ((rc = gh_dev_alloc(0, total ? total : 16, &d_dst))) { gh_batch_destroy(b); return die("device allocation", rc); }
    gh_bgather_report grep{};
    std::vector<uint8_t> bytes((size_t)total);
    if ((rc = gh_batchdec_index(b, nullptr, 1)) == GH_OK)
      rc = gh_batchdec_gather(b, ranges.data(), (uint32_t)ranges.size(), d_dst, total, nullptr, &grep);
    const double t2 = now_ms();
    if (rc == GH_E_CORRUPT && grep.bad_ranges) {
      std::vector<uint32_t> status(ns, 0);
      if (gh_batch_status(b, status.data(), nullptr, (uint32_t)ns) == GH_OK)
        for (size_t i = 0; i < ns; ++i)
          if (status[i])
            std::fprintf(stderr, "decoder: %s: line %zu: %s: corrupt stream (status 0x%x)\n", list_file, line_of[i],
                         in[i].c_str(), status[i]);
    }
    if (rc == GH_OK && total) rc = gh_dev_copy(bytes.data(), d_dst, total);
    if (rc) {
      const int r = die("batched gather", rc);
      gh_dev_free(d_dst);
      gh_batch_destroy(b);
      return r;
    }
    gh_dev_free(d_dst);
    gh_batch_destroy(b);
    FILE* f = std::fopen(range_out, "wb");
    bool okw = f && std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (f) okw = std::fclose(f) == 0 && okw;
    if (!okw) { std::fprintf(stderr, "decoder: cannot write %s\n", range_out); return 1; }
    std::printf("Batch gather: %zu streams, %zu ranges, %llu pieces, %llu bytes; load %.3f ms, kernel %.3f ms, call %.3f ms\n",
                ns, ranges.size(), (unsigned long long)grep.npieces, (unsigned long long)total, t1 - t0, grep.kernel_ms, t2 - t1);
    return 0;
  }
  gh_batch_report rep{};
  if ((rc = gh_batch_decode(b, nullptr, 0, nullptr, 1))) { gh_batch_destroy(b); return die("batch decode", rc); }
  rc = gh_batch_wait(b, &rep);
  const double t2 = now_ms();
  std::vector<uint32_t> status(ns, 0);
  if (rc == GH_E_CORRUPT && gh_batch_status(b, status.data(), nullptr, (uint32_t)ns) == GH_OK) {
    for (size_t i = 0; i < ns; ++i)
      if (status[i])
        std::fprintf(stderr, "decoder: %s: line %zu: %s: corrupt stream (status 0x%x)\n", list_file, line_of[i],
                     in[i].c_str(), status[i]);
  } else if (rc) {
    gh_batch_destroy(b);
    return die("batch decode", rc);
  }
  std::vector<uint8_t> bytes;
  for (size_t i = 0; i < ns; ++i) {
    if (status[i]) continue;
    bytes.resize((size_t)streams[i].n);
    int r = gh_batch_download(b, (uint32_t)i, bytes.data(), bytes.size());
    if (r) { gh_batch_destroy(b); return die("download", r); }
    FILE* f = std::fopen(out[i].c_str(), "wb");
    bool okw = f && std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (f) okw = std::fclose(f) == 0 && okw;
    if (!okw) { gh_batch_destroy(b); std::fprintf(stderr, "decoder: cannot write %s\n", out[i].c_str()); return 1; }
  }
  gh_batch_destroy(b);
  std::printf("Batch: %u streams, %llu bytes; load %.3f ms, kernel %.3f ms, call %.3f ms, %u bad\n", rep.nstreams,
              (unsigned long long)rep.out_bytes, t1 - t0, rep.kernel_ms, t2 - t1, rep.bad_streams);
  return rc ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--batch")) return batch_main(argv[2]);
  if (argc == 6 && !std::strcmp(argv[1], "--batch") && !std::strcmp(argv[3], "--ranges"))
    return batch_main(argv[2], argv[4], argv[5]);
  if (argc == 6 && !std::strcmp(argv[1], "--batch") && !std::strcmp(argv[3], "--elements"))
    return batch_main(argv[2], argv[4], argv[5], true);
  if (argc < 3) {
    std::fprintf(stderr,
                 "Usage: bin/decoder input output [--gpus N] [--shards S] [--reps R] [--json] [--verify FILE]\n"
                 "       [--write-index FILE [--index-stride K]] [--index FILE --range LO:HI]\n"
                 "       [--index FILE --ranges FILE]\n"
                 "       bin/decoder --batch LIST   (LIST: one input<TAB>output per line)\n"
                 "       bin/decoder --batch LIST --ranges FILE OUT   (FILE: one STREAM LO:HI per line)\n"
                 "       bin/decoder --batch LIST --elements FILE OUT   (byte-plane containers; FILE: one TENSOR LO:HI per line)\n");
    return 2;
  }
  int ngpus = 1, reps = 1, nshards = 0;
  bool json = false;
  const char* verify = nullptr;
  const char* write_index = nullptr;
  const char* index_file = nullptr;
  const char* range = nullptr;
  const char* ranges_file = nullptr;
  int index_stride = GH_INDEX_MIN_LOG2;
  for (int i = 3; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) ngpus = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--shards") && i + 1 < argc) nshards = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--reps") && i + 1 < argc) reps = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--json")) json = true;
    else if (!std::strcmp(argv[i], "--verify") && i + 1 < argc) verify = argv[++i];
    else if (!std::strcmp(argv[i], "--write-index") && i + 1 < argc) write_index = argv[++i];
    else if (!std::strcmp(argv[i], "--index-stride") && i + 1 < argc) index_stride = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--index") && i + 1 < argc) index_file = argv[++i];
    else if (!std::strcmp(argv[i], "--range") && i + 1 < argc) range = argv[++i];
    else if (!std::strcmp(argv[i], "--ranges") && i + 1 < argc) ranges_file = argv[++i];
    else {
      std::fprintf(stderr, "decoder: unknown option %s\n", argv[i]);
      return 2;
    }
  }
  if (ngpus < 1) ngpus = 1;
  if (reps < 1) reps = 1;
  if (ranges_file) {
    if (!index_file || range || write_index) {
      std::fprintf(stderr, "decoder: --ranges FILE goes with --index FILE (and not with --range or --write-index)\n");
      return 2;
    }
    return gather_main(argv[1], argv[2], index_file, ranges_file);
  }
  // --index FILE --range LO:HI: the segments to load, from the sidecar alone
  const bool ranged = index_file || range;
  uint64_t lo = 0, hi = 0, rb = 0, re = 0, skip = 0;
  gh_index ix{};
  std::vector<uint8_t> ix_img;
  if (ranged) {
    char* end = nullptr;
    if (!index_file || !range || write_index) {
      std::fprintf(stderr, "decoder: --index FILE and --range LO:HI go together (and not with --write-index)\n");
      return 2;
    }
    lo = std::strtoull(range, &end, 10);
    if (end == range || *end != ':') { std::fprintf(stderr, "decoder: --range LO:HI\n"); return 2; }
    const char* h = end + 1;
    hi = std::strtoull(h, &end, 10);
    if (end == h || *end) { std::fprintf(stderr, "decoder: --range LO:HI\n"); return 2; }
    FILE* f = std::fopen(index_file, "rb");
    if (!f) { std::fprintf(stderr, "decoder: Could not open index file %s\n", index_file); return 1; }
    std::fseek(f, 0, SEEK_END);
    ix_img.resize((size_t)std::max(std::ftell(f), 0L));
    std::fseek(f, 0, SEEK_SET);
    const bool okr = std::fread(ix_img.data(), 1, ix_img.size(), f) == ix_img.size();
    std::fclose(f);
    int r = okr ? gh_index_parse(ix_img.data(), ix_img.size(), &ix) : GH_E_FORMAT;
    if (!r) r = gh_index_locate(&ix, lo, hi, &rb, &re, &skip);
    if (r) return die("bad index / range", r);
    ngpus = nshards = 1;
  }

  // Header first (sizes for the shard plan); each shard then streams its own payload
  // range from the file (gh_ctx_load_file: pinned double-buffered read -> H2D).
  gh_stream s{};
  bool is_raw = false;  // gap-less raw-stream container (gh_ctx_load_raw, self-sync)
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
      std::fprintf(stderr, "decoder: Could not open input file %s\n", argv[1]);
      return 1;
    }
    uint64_t magic = 0;
    is_raw = std::fread(&magic, 1, 8, f) == 8 && magic == GH_RAW_MAGIC;
    std::fclose(f);
  }
  if (is_raw) ngpus = nshards = 1;  // a raw stream's segment entries are found on one device
  if (is_raw && ranged) {
    std::fprintf(stderr, "decoder: --range needs a gap-array file\n");
    return 2;
  }
  const int ndev = gh_device_count();
  if (ndev < 1) return die("no HIP device", GH_E_NODEV);
  if (ngpus > ndev) ngpus = ndev;
  if (nshards < 1) nshards = ngpus;
  std::vector<gh_ctx*> ctx(nshards, nullptr);
  auto cleanup = [&]() {
    for (auto* c : ctx) gh_ctx_destroy(c);
  };
  int rc;
  const double t0 = now_ms();
  gh_file_info info{};
  if ((rc = gh_ctx_create(0, &ctx[0]))) { cleanup(); return die("device init", rc); }
  std::vector<uint64_t> bounds(nshards + 1, 0);
  if (is_raw) {
    std::vector<uint8_t> file;
    FILE* f = std::fopen(argv[1], "rb");
    std::fseek(f, 0, SEEK_END);
    file.resize((size_t)std::max(std::ftell(f), 0L));
    std::fseek(f, 0, SEEK_SET);
    const bool okr = std::fread(file.data(), 1, file.size(), f) == file.size();
    std::fclose(f);
    gh_raw_stream r;
    gh_sync_report sr;
    if (!okr || (rc = gh_raw_parse(file.data(), file.size(), &r)) ||
        (rc = gh_ctx_load_raw(ctx[0], r.syms, r.nsyms, r.n, r.units, r.w, 0, &sr))) {
      cleanup();
      return die("bad raw stream / upload", okr ? rc : GH_E_FORMAT);
    }
    info.n = r.n;
    info.w = r.w;
    info.g = (r.w + 3) / 4;
    bounds[1] = info.g;
    std::printf("Raw stream: gap array built on the GPU in %.3f ms (%llu boundaries repaired)\n",
                sr.kernel_ms, (unsigned long long)sr.mismatches);
  } else if (ranged) {
    if ((rc = gh_ctx_load_file(ctx[0], argv[1], rb, re, skip + (hi - lo), &info))) {
      cleanup();
      return die("bad compressed stream / upload", rc);
    }
    if (info.n != ix.n || info.g != ix.g) {
      cleanup();
      std::fprintf(stderr, "decoder: the index is for another stream (N or G differ)\n");
      return 1;
    }
    bounds[0] = rb;
    bounds[1] = re;
  } else if (nshards == 1) {
    if ((rc = gh_ctx_load_file(ctx[0], argv[1], 0, UINT64_MAX, 0, &info))) {
      cleanup();
      return die("bad compressed stream / upload", rc);
    }
    bounds[1] = info.g;
  } else {
    // a zero-segment load reads just the header
    if ((rc = gh_ctx_load_file(ctx[0], argv[1], 0, 0, 0, &info))) {
      cleanup();
      return die("bad compressed stream / upload", rc);
    }
    gh_plan_shards(info.g, (uint32_t)nshards, bounds.data());
    // one host thread per shard: each streams its own payload range through its own
    // pinned buffers, so the shards' file reads and H2D transfers overlap
    if ((rc = for_each_shard(nshards, [&](int k) {
           int r = k ? gh_ctx_create(k % ngpus, &ctx[k]) : GH_OK;
           return r ? r : gh_ctx_load_file(ctx[k], argv[1], bounds[k], bounds[k + 1], 0, nullptr);
         }))) {
      cleanup();
      return die("upload", rc);
    }
  }
  s.n = info.n;
  s.w = info.w;
  s.g = info.g;
  std::printf("Input file: %s\n", argv[1]);
  std::printf("Original size: %llu bytes\n", (unsigned long long)s.n);
  std::printf("Compressed size: %llu bytes\n", (unsigned long long)s.w);  // reference prints W
  if (write_index) {
    if (nshards != 1) {
      cleanup();
      std::fprintf(stderr, "decoder: --write-index needs a single-shard run\n");
      return 2;
    }
    std::vector<uint8_t> img((size_t)gh_index_bytes(info.g, (uint32_t)index_stride));
    float ims = 0;
    if (img.empty()) { cleanup(); std::fprintf(stderr, "decoder: --index-stride 8..20\n"); return 2; }
    if ((rc = gh_ctx_build_index(ctx[0], (uint32_t)index_stride, img.data(), img.size(), nullptr, &ims))) {
      cleanup();
      return die("index build", rc);
    }
    FILE* f = std::fopen(write_index, "wb");
    bool okw = f && std::fwrite(img.data(), 1, img.size(), f) == img.size();
    if (f) okw = std::fclose(f) == 0 && okw;
    if (!okw) { cleanup(); std::fprintf(stderr, "decoder: cannot write %s\n", write_index); return 1; }
    std::printf("Index: %zu bytes (one entry per %u segments), built in %.3f ms\n", img.size(), 1u << index_stride, ims);
  }
  const double t1 = now_ms();
  for (int r = 0; r < reps; ++r)
    for (int k = 0; k < nshards; ++k)
      if ((rc = gh_ctx_decode(ctx[k], nullptr, 1))) { cleanup(); return die("decode", rc); }
  std::vector<gh_report> rep(nshards);
  uint32_t status = 0;
  uint64_t total = 0;
  std::map<int, float> dev_ms;  // decodes on one device run in turn: their times add up
  for (int k = 0; k < nshards; ++k) {
    if ((rc = gh_ctx_report(ctx[k], nullptr, &rep[k]))) { cleanup(); return die("decode", rc); }
    int dev = 0;
    gh_ctx_device(ctx[k], &dev);
    dev_ms[dev] += rep[k].kernel_ms;
    status |= rep[k].status;
    total += rep[k].symbols;
  }
  float dec_ms = 0;  // devices run side by side
  for (auto& d : dev_ms) dec_ms = std::max(dec_ms, d.second);
  if (status) {
    cleanup();
    std::fprintf(stderr, "decoder: device reported status 0x%x (corrupted stream?)\n", status);
    return 1;
  }
  // bytes to write: the whole stream, or the range's (at byte `skip` of the shard's output)
  const uint64_t need = ranged ? skip + (hi - lo) : s.n;
  if (total < need) {
    cleanup();
    std::fprintf(stderr, "decoder: stream decoded to %llu < N symbols\n", (unsigned long long)total);
    return 1;
  }
  // each shard writes its bytes at its offset of argv[2] (pinned double-buffered
  // D2H -> pwrite); the reference always wrote "decodedfile" (huff.cpp:32)
  const double t2 = now_ms();
  std::vector<uint64_t> off(nshards + 1, 0), want(nshards, 0);
  for (int k = 0; k < nshards; ++k) {
    if (k + 1 < nshards && rep[k].symbols > rep[k].out_bytes) {
      cleanup();
      std::fprintf(stderr, "decoder: shard %d overflowed its output (corrupted stream?)\n", k);
      return 1;
    }
    want[k] = ranged ? hi - lo : off[k] < s.n ? std::min<uint64_t>(rep[k].symbols, s.n - off[k]) : 0;
    off[k + 1] = off[k] + rep[k].symbols;
  }
  {  // create / truncate the output once, then every shard writes its range concurrently
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) {
      cleanup();
      std::fprintf(stderr, "decoder: cannot create %s\n", argv[2]);
      return 1;
    }
    std::fclose(f);
  }
  if ((rc = for_each_shard(nshards, [&](int k) {
         return gh_ctx_save_file(ctx[k], argv[2], off[k], ranged ? skip : 0, want[k], 0, nullptr);
       }))) {
    cleanup();
    return die("write output", rc);
  }
  const double t3 = now_ms();
  cleanup();
  std::printf("HtoD,%f, dec,%f, DtoH,%f,SEGMENTSIZE,%d,THREAD_NUM,%d,LOCAL_SEGMENT_NUM,%d\n",
              t1 - t0, dec_ms, t3 - t2, GH_SEGMENT_BITS, 256, 1);
  const double total_ms = (t1 - t0) + dec_ms + (t3 - t2);
  std::printf("Decode time: %.3f ms\n", total_ms);
  std::printf("Throughput: %.2f MB/s\n", (double)s.n / (1024.0 * 1024.0) / (total_ms / 1000.0));

  int ok = -1;
  if (verify) {
    // compare the written file with the reference bytes, chunk by chunk
    FILE* v = std::fopen(verify, "rb");
    FILE* o = std::fopen(argv[2], "rb");
    ok = 0;
    if (v && o) {
      std::vector<uint8_t> x(1 << 24), y(1 << 24);
      ok = 1;
      uint64_t seen = 0;
      for (;;) {
        const size_t a = std::fread(x.data(), 1, x.size(), v), b = std::fread(y.data(), 1, y.size(), o);
        if (a != b || std::memcmp(x.data(), y.data(), a)) { ok = 0; break; }
        seen += a;
        if (a == 0) break;
      }
      if (seen != (ranged ? hi - lo : s.n)) ok = 0;
    }
    if (v) std::fclose(v);
    if (o) std::fclose(o);
    std::printf("Verification: %s\n", ok ? "PASS" : "FAIL");
  }
  if (json) {
    const double kbytes = 4.0 * s.w + 4.0 * ((s.g + 7) / 8) + (double)s.n;
    std::printf(
        "{\"N\": %llu, \"W\": %llu, \"G\": %llu, \"gpus\": %d, \"reps\": %d, \"kernel_ms\": %.6f, "
        "\"load_ms\": %.3f, \"save_ms\": %.3f, \"decoded_GBps\": %.3f, \"alg_bytes\": %.0f, "
        "\"alg_GBps\": %.3f, \"lut_bits\": %u, \"bitexact\": %s}\n",
        (unsigned long long)s.n, (unsigned long long)s.w, (unsigned long long)s.g, ngpus, reps,
        dec_ms, t1 - t0, t3 - t2, dec_ms > 0 ? s.n / (dec_ms * 1e6) : 0.0, kbytes,
        dec_ms > 0 ? kbytes / (dec_ms * 1e6) : 0.0, rep[0].lut_bits,
        ok < 0 ? "null" : (ok ? "true" : "false"));
  }
  if (verify && !ok) return 3;
  return 0;
}
