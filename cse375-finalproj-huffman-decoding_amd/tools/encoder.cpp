// bin/encoder <input> <compressed.huff> [--threads T] [--v2] [--gpu [DEVICE]] [--raw]
//             [--write-index FILE [--index-stride K]] [--slices K [--devices a,b,c]]
//
// Drop-in for the reference encoder CLI (Huffman_coding_Gap_arrays/encoder/src/
// huff.cpp:30-220): same positional arguments, same output format (v1 header when
// the sizes fit the reference's 32-bit fields, the 64-bit v2 header otherwise), and
// the same stdout lines (:176-181).  Encoding runs on the host through the gaphuff C
// ABI, or with --gpu on a gfx950 device (gh_ectx_*, byte-identical output; the
// reference's own encoder is a GPU one, encoder.cu:382-457).  --write-index also writes
// the stream's seek index (gaphuff.h "random access"; K = log2 of the stride in segments,
// default 8) from the encoder itself: gh_encode_index on the host, gh_ectx_index with
// --gpu; the same index with --raw (G is the same).  --gpu --slices K encodes the input
// in K slices (gh_encode_sharded), slice i on the i-th of --devices (round robin; default:
// the --gpu device); the same file, and the index then from the slices' own entries
// (gh_encode_sharded_index: gh_ectx_index_slice per slice, no host pass over the input).
// bin/encoder --batch LIST [--gpu D] [--device-plan]
// --batch LIST (a text file, one input<TAB>output per line) encodes all inputs as one batch
// on the GPU (gh_ebatch_*: each input with its own code, a fixed set of launches however
// many inputs) and writes every output.  --device-plan builds the codes on the GPU too
// (gh_batchenc_plan_device): the same files.
// bin/encoder --batch LIST --planes E[:MASK|:auto] [--gpu D] [--device-plan]
// --planes E[:MASK] treats every input as a tensor of E-byte elements (E = 1, 2, 4, 8): the
// byte planes MASK names (default: the top plane alone) are the batch's streams, the others
// are stored, and every output is a byte-plane container (gaphuff.h "byte planes").
// --planes E:auto gives every input its own mask: the planes whose image is smaller than their
// raw bytes (gh_pmask_host, gaphuff.h "plane choice").
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gaphuff.h"

static double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out.resize((size_t)std::max(n, 0L));
  const bool ok = n <= 0 || std::fread(out.data(), 1, (size_t)n, f) == (size_t)n;
  std::fclose(f);
  return ok;
}

// --batch LIST [--gpu D] [--device-plan]: every line of the text file is `input<TAB>output` (as bin/decoder
// --batch reads it); all inputs are encoded as one batch (gh_ebatch_*), each with its own
// code, and every output file is written.  device_plan: gh_batchenc_plan_device instead of
// gh_ebatch_plan.  planes_e != 0: every input is a tensor of planes_e-byte elements whose planes
// in planes_mask are coded (gh_planes_load), and every output a byte-plane container;
// planes_auto: every tensor's own mask by gh_pmask_host.
static int batch_main(const char* list_file, int device, bool device_plan, uint32_t planes_e, uint32_t planes_mask,
                      bool planes_auto) {
  std::vector<uint8_t> text;
  if (!read_file(list_file, text)) {
    std::fprintf(stderr, "encoder: Could not open batch list %s\n", list_file);
    return 1;
  }
  std::vector<std::string> in, out;
  std::vector<size_t> lines;
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
      if (tab == std::string::npos || tab == 0 || tab + 1 == ln.size()) {
        std::fprintf(stderr, "encoder: %s: line %zu: expected input<TAB>output\n", list_file, line);
        return 1;
      }
      in.push_back(ln.substr(0, tab));
      out.push_back(ln.substr(tab + 1));
      lines.push_back(line);
    }
  }
  const size_t ns = in.size();
  std::vector<std::vector<uint8_t>> data(ns);
  std::vector<const uint8_t*> ptr(ns);
  std::vector<uint64_t> n(ns);
  for (size_t i = 0; i < ns; ++i) {
    if (!read_file(in[i].c_str(), data[i])) {
      std::fprintf(stderr, "encoder: %s: Could not open input file %s\n", list_file, in[i].c_str());
      return 1;
    }
    ptr[i] = data[i].data();
    n[i] = data[i].size();
    if (planes_e && n[i] % planes_e) {
      std::fprintf(stderr, "encoder: %s: line %zu: %s holds %llu bytes, no multiple of the element size %u\n", list_file,
                   lines[i], in[i].c_str(), (unsigned long long)n[i], planes_e);
      return 1;
    }
  }
  // --planes: the tensors, their layout and the stored planes
  std::vector<gh_planes_item> items(planes_e ? ns : 0);
  std::vector<gh_planes_slot> slots(planes_e ? 8 * std::max<size_t>(ns, 1) : 0);
  std::vector<uint8_t> stored;
  uint32_t nstreams = (uint32_t)ns;
  if (planes_e) {
    for (size_t i = 0; i < ns; ++i) items[i] = gh_planes_item{data[i].data(), n[i] / planes_e, planes_e, planes_mask};
    if (planes_auto) {
      std::vector<uint32_t> masks(std::max<size_t>(ns, 1));
      if (gh_pmask_host(items.data(), (uint32_t)ns, masks.data(), nullptr)) {
        std::fprintf(stderr, "encoder: --planes: %s\n", gh_last_error());
        return 1;
      }
      for (size_t i = 0; i < ns; ++i) items[i].coded_mask = masks[i];
    }
    uint64_t stored_bytes = 0;
    if (gh_planes_layout(items.data(), (uint32_t)ns, slots.data(), &nstreams, &stored_bytes)) {
      std::fprintf(stderr, "encoder: --planes: %s\n", gh_last_error());
      return 1;
    }
    stored.resize((size_t)stored_bytes);
  }
  auto die = [](const char* what, gh_ebatch* b) {
    std::fprintf(stderr, "encoder: %s: %s\n", what, gh_last_error());
    gh_ebatch_destroy(b);
    return 1;
  };
  gh_ebatch* b = nullptr;
  if (gh_ebatch_create(device, &b)) return die("device init", nullptr);
  const double t0 = now_ms();
  if (planes_e ? gh_planes_load(b, items.data(), (uint32_t)ns, stored.data(), stored.size())
               : gh_ebatch_load(b, ptr.data(), n.data(), (uint32_t)ns))
    return die("batch load", b);
  const double t1 = now_ms();
  if (device_plan ? gh_batchenc_plan_device(b, 0) : gh_ebatch_plan(b, 0, 0)) return die("batch plan", b);
  const double t2 = now_ms();
  float code_ms = 0;
  if (gh_batchenc_plan_times(b, nullptr, &code_ms, nullptr)) return die("plan times", b);
  gh_ebatch_report rep{};
  if (gh_ebatch_encode(b, nullptr, 1) || gh_ebatch_wait(b, &rep)) return die("batch encode", b);
  const double t3 = now_ms();
  std::vector<uint64_t> sizes(nstreams);
  if (gh_ebatch_sizes(b, sizes.data(), nstreams)) return die("sizes", b);
  std::vector<uint8_t> img;
  std::vector<std::vector<uint8_t>> coded(planes_e);
  uint64_t out_total = 0;
  for (size_t i = 0; i < ns; ++i) {
    if (!planes_e) {
      img.resize((size_t)sizes[i]);
      if (gh_ebatch_download(b, (uint32_t)i, img.data(), img.size())) return die("download", b);
    } else {
      // the tensor's container: its coded planes' images and its stored planes' bytes
      const void* planes[8] = {};
      uint64_t plane_bytes[8] = {};
      for (uint32_t p = 0; p < planes_e; ++p) {
        const gh_planes_slot& sl = slots[8 * i + p];
        if (sl.stream == GH_PLANES_STORED) {
          planes[p] = stored.data() + sl.stored_off;
          plane_bytes[p] = items[i].nelem;
          continue;
        }
        coded[p].resize((size_t)sizes[sl.stream]);
        if (gh_ebatch_download(b, sl.stream, coded[p].data(), coded[p].size())) return die("download", b);
        planes[p] = coded[p].data();
        plane_bytes[p] = coded[p].size();
      }
      uint64_t total = 0;
      if (gh_planes_image_bytes(planes_e, plane_bytes, &total)) return die("container", b);
      img.resize((size_t)total);
      if (gh_planes_image_write(&items[i], planes, plane_bytes, img.data(), img.size())) return die("container", b);
    }
    out_total += img.size();
    FILE* f = std::fopen(out[i].c_str(), "wb");
    bool okw = f && std::fwrite(img.data(), 1, img.size(), f) == img.size();
    if (f) okw = std::fclose(f) == 0 && okw;
    if (!okw) {
      gh_ebatch_destroy(b);
      std::fprintf(stderr, "encoder: cannot write %s\n", out[i].c_str());
      return 1;
    }
  }
  gh_ebatch_destroy(b);
  char code[48] = "";
  if (device_plan) std::snprintf(code, sizeof(code), "code kernel %.3f, ", code_ms);
  if (planes_e) {
    char mask[24] = "auto";
    if (!planes_auto) std::snprintf(mask, sizeof(mask), "0x%x", planes_mask);
    std::printf("Planes: %zu tensors of %u-byte elements, mask %s: %u coded planes, %zu stored bytes, %llu container "
                "bytes\n", ns, planes_e, mask, nstreams, stored.size(), (unsigned long long)out_total);
  }
  std::printf("Batch: %u streams, %llu bytes -> %llu bytes; load %.3f ms, plan %.3f ms (histogram %.3f, %shost %.3f), "
              "kernel %.3f ms, call %.3f ms\n",
              rep.nstreams, (unsigned long long)rep.in_bytes, (unsigned long long)rep.out_bytes, t1 - t0, t2 - t1,
              rep.hist_ms, code, rep.plan_host_ms, rep.kernel_ms, t3 - t2);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !std::strcmp(argv[1], "--batch")) {
    int device = 0;
    bool device_plan = false, bad = false, planes_auto = false;
    uint32_t planes_e = 0, planes_mask = 0;
    for (int i = 3; i < argc; ++i) {
      if (!std::strcmp(argv[i], "--gpu") && i + 1 < argc) device = std::atoi(argv[++i]);
      else if (!std::strcmp(argv[i], "--device-plan")) device_plan = true;
      else if (!std::strcmp(argv[i], "--planes") && i + 1 < argc) {
        char* end = nullptr;
        planes_e = (uint32_t)std::strtoul(argv[++i], &end, 0);
        planes_mask = planes_e >= 1 && planes_e <= 8 ? 1u << (planes_e - 1) : 0u;
        if (!std::strcmp(end, ":auto")) {
          planes_auto = true;
          end += 5;
        } else if (*end == ':') {
          planes_mask = (uint32_t)std::strtoul(end + 1, &end, 0);
        }
        if (*end || (planes_e != 1 && planes_e != 2 && planes_e != 4 && planes_e != 8) || planes_mask >> planes_e) bad = true;
      } else bad = true;
    }
    if (bad) {
      std::fprintf(stderr, "Usage: bin/encoder --batch LIST [--planes E[:MASK|:auto]] [--gpu D] [--device-plan]   (LIST: "
                           "one input<TAB>output per line; E: 1, 2, 4 or 8; MASK < 1 << E)\n");
      return 2;
    }
    return batch_main(argv[2], device, device_plan, planes_e, planes_mask, planes_auto);
  }
  if (argc < 3) {
    std::printf("Usage: bin/encoder input output\n");
    return 1;
  }
  int threads = 0, force = 0, gpu = -1;
  bool raw = false;  // write the gap-less raw-stream container (GH_RAW_MAGIC) instead
  const char* index_path = nullptr;
  uint32_t index_k = 8, slices = 0;
  std::vector<int> devices;
  for (int i = 3; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--threads") && i + 1 < argc) threads = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--v2")) force = 2;
    else if (!std::strcmp(argv[i], "--raw")) raw = true;
    else if (!std::strcmp(argv[i], "--write-index") && i + 1 < argc) index_path = argv[++i];
    else if (!std::strcmp(argv[i], "--index-stride") && i + 1 < argc) index_k = (uint32_t)std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--slices") && i + 1 < argc) slices = (uint32_t)std::max(std::atoi(argv[++i]), 0);
    else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) {
      for (const char* s = argv[++i]; *s;) {
        char* end = nullptr;
        devices.push_back((int)std::strtol(s, &end, 10));
        if (end == s) {
          std::fprintf(stderr, "encoder: bad --devices list\n");
          return 2;
        }
        s = *end == ',' ? end + 1 : end;
      }
    }
    else if (!std::strcmp(argv[i], "--gpu")) gpu = (i + 1 < argc && argv[i + 1][0] != '-') ? std::atoi(argv[++i]) : 0;
    else {
      std::fprintf(stderr, "encoder: unknown option %s\n", argv[i]);
      return 2;
    }
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::fprintf(stderr, "Could not open input file\n");
    return 1;
  }
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> in((size_t)std::max(n, 0L));
  if (n > 0 && std::fread(in.data(), 1, (size_t)n, f) != (size_t)n) {
    std::fclose(f);
    std::fprintf(stderr, "File read error\n");
    return 1;
  }
  std::fclose(f);
  gh_encode_plan* plan = new gh_encode_plan;
  std::vector<uint8_t> out, index;
  double t0, t1, t2;
  int rc;
  if (slices && gpu < 0) {
    std::fprintf(stderr, "encoder: --slices needs --gpu\n");
    return 2;
  }
  if (gpu >= 0 && slices) {
    if (devices.empty()) devices.push_back(gpu);
    const gh_opts opts{(int)devices.size(), devices.data(), 1};
    float ms = 0.f;
    out.resize(gh_encode_bound(in.size()));
    t0 = now_ms();
    if (index_path) {  // the index of a sliced stream: every slice's entries, from its GPU
      // (G <= ceil(n / 8): 16-bit codes; a bad stride: size 0, and the library's refusal)
      index.resize(std::max<uint64_t>(gh_index_bytes((in.size() + 7) / 8, index_k), 1));
      rc = gh_encode_sharded_index(in.data(), in.size(), &opts, slices, force, out.data(), out.size(), plan, &ms,
                                   index_k, index.data(), index.size(), nullptr);
      t2 = now_ms();
      if (!rc) index.resize(gh_index_bytes(plan->g, index_k));
    } else {
      rc = gh_encode_sharded(in.data(), in.size(), &opts, slices, force, out.data(), out.size(), plan, &ms);
      t2 = now_ms();
    }
    t1 = t2 - ms;
    if (!rc) out.resize(plan->file_bytes);
    if (rc) {
      std::fprintf(stderr, "encoder: %s\n", gh_last_error());
      return 1;
    }
  } else if (gpu >= 0) {
    gh_ectx* e = nullptr;
    float ms = 0.f;
    rc = gh_ectx_create(gpu, &e);
    if (!rc) rc = gh_ectx_load(e, in.data(), in.size());
    t0 = now_ms();
    if (!rc) rc = gh_ectx_plan(e, force, plan);
    if (!rc) rc = gh_ectx_encode(e, &ms);
    t2 = now_ms();
    t1 = t2 - ms;  // "kernel time": the device encode's event time
    if (!rc) {
      out.resize(plan->file_bytes);
      rc = gh_ectx_download(e, out.data(), out.size());
    }
    if (!rc && index_path) {  // (a bad stride: size 0, and the library's refusal)
      index.resize(std::max<uint64_t>(gh_index_bytes(plan->g, index_k), 1));
      rc = gh_ectx_index(e, index_k, index.data(), index.size(), nullptr);
    }
    if (rc) {
      std::fprintf(stderr, "encoder: %s\n", gh_last_error());
      return 1;
    }
    gh_ectx_destroy(e);
  } else {
    t0 = now_ms();
    rc = gh_encode_plan_make(in.data(), in.size(), threads, force, plan);
    if (rc) {
      std::fprintf(stderr, "encoder: %s\n", gh_last_error());
      return 1;
    }
    out.resize(plan->file_bytes);
    t1 = now_ms();
    rc = gh_encode_write(in.data(), plan, threads, out.data(), out.size());
    if (rc) {
      std::fprintf(stderr, "encoder: %s\n", gh_last_error());
      return 1;
    }
    t2 = now_ms();
    if (index_path) {  // (a bad stride: size 0, and the library's refusal)
      index.resize(std::max<uint64_t>(gh_index_bytes(plan->g, index_k), 1));
      rc = gh_encode_index(in.data(), plan, index_k, threads, index.data(), index.size());
      if (rc) {
        std::fprintf(stderr, "encoder: %s\n", gh_last_error());
        return 1;
      }
    }
  }
  if (raw) {  // same code and payload words, no gap array
    gh_stream st;
    if (gh_stream_parse(out.data(), out.size(), &st)) {
      std::fprintf(stderr, "encoder: %s\n", gh_last_error());
      return 1;
    }
    std::vector<uint8_t> r;
    auto put = [&](uint64_t x) {
      for (int i = 0; i < 8; ++i) r.push_back((uint8_t)(x >> (8 * i)));
    };
    put(GH_RAW_MAGIC);
    put(st.nsyms);
    for (uint32_t i = 0; i < st.nsyms; ++i) {
      r.push_back(st.syms[i].symbol);
      r.push_back(st.syms[i].length);
    }
    put(st.n);
    put(st.w);
    const uint8_t* pw = (const uint8_t*)st.payload;
    r.insert(r.end(), pw, pw + 4 * st.w);
    out.swap(r);
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) {
    std::fprintf(stderr, "Could not open output file\n");
    return 1;
  }
  if (!out.empty() && std::fwrite(out.data(), 1, out.size(), o) != out.size()) {
    std::fclose(o);
    std::fprintf(stderr, "write error\n");
    return 1;
  }
  std::fclose(o);
  if (index_path) {
    FILE* x = std::fopen(index_path, "wb");
    if (!x) {
      std::fprintf(stderr, "Could not open index file\n");
      return 1;
    }
    if (std::fwrite(index.data(), 1, index.size(), x) != index.size()) {
      std::fclose(x);
      std::fprintf(stderr, "write error\n");
      return 1;
    }
    std::fclose(x);
  }
  std::printf("Input file: %s\n", argv[1]);
  std::printf("Original size: %llu bytes\n", (unsigned long long)plan->n);
  std::printf("Compressed size: %llu bytes\n", (unsigned long long)(plan->w * 4));
  std::printf("Encode kernel time: %.3f ms\n", t2 - t1);
  std::printf("Total encode time: %.3f ms\n", t2 - t0);
  std::printf("Throughput: %.2f MB/s\n",
              (double)plan->n / (1024.0 * 1024.0) / std::max(1e-9, (t2 - t0) / 1000.0));
  if (index_path)
    std::printf("Index: %llu entries, stride 2^%u, %llu bytes\n", (unsigned long long)((index.size() - 40) / 8),
                index_k, (unsigned long long)index.size());
  delete plan;
  return 0;
}
