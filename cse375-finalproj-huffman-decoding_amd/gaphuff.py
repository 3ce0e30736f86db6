"""Python host mirror of the gaphuff C ABI (include/gaphuff.h) for tests and bench.

This is plumbing over ``lib/libgaphuff.so`` (ctypes, no torch types).  The product
path is the HIP kernel behind the C ABI; there is no CPU decode fallback here: if
the shared library or a gfx950 device is missing, the decode entry points raise.

Reference interfaces mirrored (paths relative to the reference repo):

* :func:`decoder_l1_l2` — ``void decoder_l1_l2(unsigned *input, int inputfilesize,
  unsigned *output, int outputfilesize, int gap_element_num, void *dectable, int
  tablesize, unsigned prefix_bit, unsigned symbol_count, TableInfo)``
  (Huffman_coding_Gap_arrays/decoder/include/decoder.cuh:4-15, decoder.cu:732-815):
  same argument meaning (``input`` = gap words followed by payload words,
  huff.cpp:90-100); the decode table is built inside the library from the
  (symbol, length) list instead of being passed pre-built (get_table.cpp:48-139),
  and errors raise :class:`GapHuffError` instead of ``exit()`` (decoder.cu:14-20).
* :func:`encode` — the encoder CLI pipeline (encoder/src/huff.cpp:30-220).
* :func:`generate` — generate.cpp:32-47 with an explicit seed.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GAPHUFF_LIB", os.path.join(_HERE, "lib", "libgaphuff.so"))

GH_OK = 0
GH_ERRORS = {
    -1: "GH_E_ARG", -2: "GH_E_FORMAT", -3: "GH_E_TABLE", -4: "GH_E_HIP", -5: "GH_E_NODEV",
    -6: "GH_E_NOMEM", -7: "GH_E_CORRUPT", -8: "GH_E_STATE", -9: "GH_E_SMALL",
}
GH_V2_MAGIC = 0x0032465548504147
GH_ST_BADCODE = 1
GH_ST_TIMEOUT = 2
GH_ST_LAYOUT = 4
GH_ST_RANGE, GH_ST_DSTSMALL, GH_ST_PIECES = 8, 16, 32  # device-planned gather
GH_ST_OFFSETS = 64  # a piece disagreed with the recorded piece offsets
GH_OFFS_NONE, GH_OFFS_RECORDED, GH_OFFS_READY = 0, 1, 2  # gh_ctx_offsets_state
GH_GATHER_MAX_RANGES = 1 << 24
GH_PGATHER_MAX_RANGES = GH_GATHER_MAX_RANGES // 8
GH_PGATHER_LAUNCHES = 10
GH_PMASK_LAUNCHES = 4

# Every symbol include/gaphuff.h declares (checked by tests/test_abi.py).
EXPORTED = (
    "gh_stream_parse", "gh_stream_validate", "gh_encode_plan_make", "gh_encode_write",
    "gh_package_merge", "gh_generate", "gh_ctx_create", "gh_ctx_destroy", "gh_ctx_load",
    "gh_ctx_load_device", "gh_ctx_decode", "gh_ctx_report", "gh_ctx_download",
    "gh_ctx_output", "gh_ctx_copy_output", "gh_ctx_reset_timing", "gh_decode", "gh_plan_shards",
    "gh_device_count", "gh_version", "gh_last_error",
    "gh_ectx_create", "gh_ectx_destroy", "gh_ectx_load", "gh_ectx_plan", "gh_ectx_encode",
    "gh_ectx_download", "gh_ctx_device", "gh_sync_gaps", "gh_ctx_load_raw",
    "gh_ctx_load_file", "gh_ctx_save_file", "gh_dev_alloc", "gh_dev_free", "gh_dev_copy",
    "gh_raw_parse", "gh_bw_copy", "gh_ctx_kernel_shape", "gh_kernel_shapes", "gh_ctx_offsets_state",
    "gh_index_bytes", "gh_index_parse", "gh_index_locate", "gh_ctx_build_index",
    "gh_gather_plan", "gh_ctx_gather", "gh_encode_index", "gh_ectx_index",
    "gh_encode_plan_from_counts", "gh_encode_bound", "gh_slice_extent", "gh_encode_slice",
    "gh_encode_image_init", "gh_slice_merge", "gh_ectx_counts", "gh_ectx_encode_slice",
    "gh_ectx_download_slice", "gh_encode_sharded",
    "gh_ctx_set_index", "gh_gather_piece_bound", "gh_ctx_gather_device", "gh_ctx_gather_wait",
    "gh_ctx_gather_times", "gh_ctx_gather_pieces",
    "gh_index_slice_extent", "gh_encode_index_slice", "gh_index_image_init", "gh_index_slice_merge",
    "gh_ectx_index_slice", "gh_ectx_load_device", "gh_ectx_merge_device", "gh_encode_sharded_index",
    "gh_ectx_kernel_shape", "gh_enc_kernel_shapes", "gh_enc_kernel_shape_for", "gh_sync_lut_bits",
    "gh_batch_create", "gh_batch_destroy", "gh_batch_layout", "gh_batch_load", "gh_batch_load_device",
    "gh_batch_decode", "gh_batch_wait", "gh_batch_status", "gh_batch_output", "gh_batch_offsets",
    "gh_batch_download", "gh_batch_kernel_shape", "gh_batch_kernel_shapes",
    "gh_ebatch_create", "gh_ebatch_destroy", "gh_ebatch_load", "gh_ebatch_load_device", "gh_ebatch_plan",
    "gh_ebatch_plan_of", "gh_ebatch_encode", "gh_ebatch_wait", "gh_ebatch_sizes", "gh_ebatch_download",
    "gh_ebatch_items", "gh_ebatch_kernel_shape", "gh_ebatch_kernel_shapes",
    "gh_package_merge_flat", "gh_batchenc_plan_device", "gh_batchenc_plan_times",
    "gh_batchdec_index", "gh_batchdec_gather_device", "gh_batchdec_gather_wait", "gh_batchdec_gather",
    "gh_batchdec_gather_pieces", "gh_batchdec_plan", "gh_batchdec_kernel_shape", "gh_batchdec_kernel_shapes",
    "gh_batchraw_load", "gh_batchraw_load_device", "gh_batchraw_gaps", "gh_batchraw_report_get",
    "gh_batchraw_gaps_host", "gh_batchraw_kernel_shape", "gh_batchraw_kernel_shapes",
    "gh_planes_layout", "gh_planes_split_host", "gh_planes_join_host", "gh_planes_load", "gh_planes_load_device",
    "gh_planes_load_times", "gh_planes_join_device", "gh_planes_wait", "gh_planes_image_bytes", "gh_planes_image_write", "gh_planes_parse",
    "gh_pgather_plan", "gh_pgather_device", "gh_pgather_wait", "gh_pgather",
    "gh_pmask_from_counts", "gh_pmask_host", "gh_pmask_device", "gh_pmask_counts",
)
GH_EBATCH_UNIT_BYTES = 1024
GH_PLANES_STORED = 0xFFFFFFFF
GH_PLANES_MAGIC = 0x0000314E4C504847


class GapHuffError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{GH_ERRORS.get(code, code)}: {msg}")
        self.code = code


class gh_sym(ctypes.Structure):
    _fields_ = [("symbol", ctypes.c_uint8), ("length", ctypes.c_uint8)]


class gh_stream(ctypes.Structure):
    _fields_ = [
        ("syms", ctypes.POINTER(gh_sym)), ("nsyms", ctypes.c_uint32), ("version", ctypes.c_uint32),
        ("n", ctypes.c_uint64), ("w", ctypes.c_uint64), ("g", ctypes.c_uint64),
        ("gap_words", ctypes.c_void_p), ("payload", ctypes.c_void_p),
    ]


class gh_encode_plan(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64), ("bits", ctypes.c_uint64), ("w", ctypes.c_uint64),
        ("g", ctypes.c_uint64), ("file_bytes", ctypes.c_uint64), ("nsyms", ctypes.c_uint32),
        ("version", ctypes.c_uint32), ("syms", gh_sym * 256), ("code", ctypes.c_uint32 * 256),
        ("len", ctypes.c_uint8 * 256), ("count", ctypes.c_uint64 * 256),
    ]


class gh_slice(ctypes.Structure):
    _fields_ = [("base_bit", ctypes.c_uint64), ("bits", ctypes.c_uint64), ("word0", ctypes.c_uint64),
                ("nwords", ctypes.c_uint64), ("gapw0", ctypes.c_uint64), ("ngapw", ctypes.c_uint64)]


class gh_report(ctypes.Structure):
    _fields_ = [
        ("symbols", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64), ("status", ctypes.c_uint32),
        ("lut_bits", ctypes.c_uint32), ("grid", ctypes.c_uint32), ("tiles", ctypes.c_uint32),
        ("kernel_ms", ctypes.c_float), ("launches", ctypes.c_uint32),
        ("mode", ctypes.c_uint32), ("path", ctypes.c_uint32),
        ("slow_lookbacks", ctypes.c_uint64),
    ]


class gh_file_info(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("w", ctypes.c_uint64), ("g", ctypes.c_uint64),
                ("nsyms", ctypes.c_uint32), ("version", ctypes.c_uint32), ("bytes_read", ctypes.c_uint64),
                ("setup_ms", ctypes.c_double), ("transfer_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class gh_raw_stream(ctypes.Structure):
    _fields_ = [("syms", ctypes.POINTER(gh_sym)), ("nsyms", ctypes.c_uint32), ("n", ctypes.c_uint64),
                ("w", ctypes.c_uint64), ("units", ctypes.c_void_p)]


class gh_index(ctypes.Structure):
    _fields_ = [("log2_stride", ctypes.c_uint32), ("n", ctypes.c_uint64), ("g", ctypes.c_uint64),
                ("nentries", ctypes.c_uint64), ("offsets", ctypes.c_void_p)]


class gh_range(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64)]


class gh_gather_piece(ctypes.Structure):
    _fields_ = [("dst", ctypes.c_uint64), ("block", ctypes.c_uint32), ("a", ctypes.c_uint32),
                ("b", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class gh_gather_report(ctypes.Structure):
    _fields_ = [("out_bytes", ctypes.c_uint64), ("npieces", ctypes.c_uint64), ("status", ctypes.c_uint32),
                ("kernel_ms", ctypes.c_float)]


class gh_batch_item(ctypes.Structure):
    _fields_ = [("syms", ctypes.POINTER(gh_sym)), ("nsyms", ctypes.c_uint32), ("n", ctypes.c_uint64),
                ("w", ctypes.c_uint64), ("g", ctypes.c_uint64), ("d_payload", ctypes.c_void_p),
                ("d_gap_words", ctypes.c_void_p)]


class gh_batch_report(ctypes.Structure):
    _fields_ = [("out_bytes", ctypes.c_uint64), ("nstreams", ctypes.c_uint32), ("bad_streams", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("kernel_ms", ctypes.c_float), ("launches", ctypes.c_uint32)]


class gh_brange(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_uint64), ("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64)]


class gh_bgather_report(ctypes.Structure):
    _fields_ = [("out_bytes", ctypes.c_uint64), ("npieces", ctypes.c_uint64), ("bad_ranges", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("kernel_ms", ctypes.c_float), ("launches", ctypes.c_uint32)]


class gh_batchraw_report(ctypes.Structure):
    _fields_ = [("gap_ms", ctypes.c_float), ("launches", ctypes.c_uint32), ("scratch_bytes", ctypes.c_uint64)]


class gh_ebatch_item(ctypes.Structure):
    _fields_ = [("d_in", ctypes.c_void_p), ("n", ctypes.c_uint64)]


class gh_ebatch_report(ctypes.Structure):
    _fields_ = [("in_bytes", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64), ("nstreams", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("hist_ms", ctypes.c_float), ("plan_host_ms", ctypes.c_float),
                ("kernel_ms", ctypes.c_float), ("launches", ctypes.c_uint32)]


class gh_planes_item(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("nelem", ctypes.c_uint64), ("elem_size", ctypes.c_uint32),
                ("coded_mask", ctypes.c_uint32)]


class gh_planes_slot(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("stored_off", ctypes.c_uint64)]


class gh_planes_report(ctypes.Structure):
    _fields_ = [("out_bytes", ctypes.c_uint64), ("ntensors", ctypes.c_uint32), ("bad_tensors", ctypes.c_uint32),
                ("kernel_ms", ctypes.c_float), ("launches", ctypes.c_uint32)]


class gh_erange(ctypes.Structure):
    _fields_ = [("tensor", ctypes.c_uint64), ("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64)]


class gh_pgather_report(ctypes.Structure):
    _fields_ = [("out_bytes", ctypes.c_uint64), ("npieces", ctypes.c_uint64), ("bad_ranges", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("kernel_ms", ctypes.c_float), ("launches", ctypes.c_uint32),
                ("expand_ms", ctypes.c_float), ("join_ms", ctypes.c_float)]


class gh_pmask_report(ctypes.Structure):
    _fields_ = [("raw_bytes", ctypes.c_uint64), ("chosen_bytes", ctypes.c_uint64), ("ntensors", ctypes.c_uint32),
                ("coded_planes", ctypes.c_uint32), ("hist_ms", ctypes.c_float), ("code_ms", ctypes.c_float),
                ("decide_ms", ctypes.c_float), ("launches", ctypes.c_uint32)]


class gh_planes_image(ctypes.Structure):
    _fields_ = [("nelem", ctypes.c_uint64), ("elem_size", ctypes.c_uint32), ("coded_mask", ctypes.c_uint32),
                ("plane", ctypes.c_void_p * 8), ("plane_bytes", ctypes.c_uint64 * 8), ("stream", gh_stream * 8)]


class gh_sync_report(ctypes.Structure):
    _fields_ = [("g", ctypes.c_uint64), ("mismatches", ctypes.c_uint64), ("passes", ctypes.c_uint32),
                ("kernel_ms", ctypes.c_float), ("host_ms", ctypes.c_float), ("halo", ctypes.c_uint32)]


MODE_NAMES = {1: "split", 2: "tile", 3: "fused", 4: "mtile"}
PATH_NAMES = {2: "grouped", 4: "multi_wave", 8: "multi_tile"}


class gh_opts(ctypes.Structure):
    _fields_ = [("ngpus", ctypes.c_int), ("devices", ctypes.POINTER(ctypes.c_int)),
                ("reps", ctypes.c_int)]


_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load libgaphuff.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GapHuffError(-5, f"{LIB_PATH} missing: run `make -C {_HERE}` (or build())")
        L = ctypes.CDLL(LIB_PATH)
        P, U8, U32, U64, I = ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        sig = {
            "gh_stream_parse": ([P, ctypes.c_size_t, ctypes.POINTER(gh_stream)], I),
            "gh_stream_validate": ([ctypes.POINTER(gh_stream)], I),
            "gh_encode_plan_make": ([P, U64, I, I, ctypes.POINTER(gh_encode_plan)], I),
            "gh_encode_write": ([P, ctypes.POINTER(gh_encode_plan), I, P, U64], I),
            "gh_package_merge": ([P, U32, P], I),
            "gh_package_merge_flat": ([P, U32, P], I),
            "gh_generate": ([U64, ctypes.c_double, U64, U64, P, I], I),
            "gh_ctx_create": ([I, ctypes.POINTER(P)], I),
            "gh_ctx_destroy": ([P], I),
            "gh_ctx_load": ([P, ctypes.POINTER(gh_stream), U64, U64, U64], I),
            "gh_ctx_load_device": ([P, ctypes.POINTER(gh_stream), U64, U64, P, U64, P, U64], I),
            "gh_ctx_decode": ([P, P, I], I),
            "gh_ctx_report": ([P, P, ctypes.POINTER(gh_report)], I),
            "gh_ctx_download": ([P, U64, P, U64], I),
            "gh_ctx_output": ([P, ctypes.POINTER(P), ctypes.POINTER(U64)], I),
            "gh_ctx_copy_output": ([P, U64, P, U64, P], I),
            "gh_ctx_reset_timing": ([P], I),
            "gh_decode": ([ctypes.POINTER(gh_stream), P, U64, ctypes.POINTER(gh_opts),
                           ctypes.POINTER(gh_report)], I),
            "gh_plan_shards": ([U64, U32, P], I),
            "gh_device_count": ([], I),
            "gh_ectx_create": ([I, ctypes.POINTER(P)], I),
            "gh_ectx_destroy": ([P], I),
            "gh_ectx_load": ([P, P, U64], I),
            "gh_ectx_plan": ([P, I, ctypes.POINTER(gh_encode_plan)], I),
            "gh_ectx_encode": ([P, ctypes.POINTER(ctypes.c_float)], I),
            "gh_ectx_download": ([P, P, U64], I),
            "gh_ctx_device": ([P, ctypes.POINTER(I)], I),
            "gh_ctx_kernel_shape": ([P, ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_ctx_offsets_state": ([P, ctypes.POINTER(ctypes.c_int)], I),
            "gh_kernel_shapes": ([ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_sync_gaps": ([I, P, U32, P, U64, P, P, ctypes.POINTER(gh_sync_report)], I),
            "gh_ctx_load_raw": ([P, P, U32, U64, P, U64, U64, ctypes.POINTER(gh_sync_report)], I),
            "gh_ctx_load_file": ([P, ctypes.c_char_p, U64, U64, U64, ctypes.POINTER(gh_file_info)], I),
            "gh_ctx_save_file": ([P, ctypes.c_char_p, U64, U64, U64, I, ctypes.POINTER(ctypes.c_double)], I),
            "gh_raw_parse": ([P, ctypes.c_size_t, ctypes.POINTER(gh_raw_stream)], I),
            "gh_dev_alloc": ([I, U64, ctypes.POINTER(P)], I),
            "gh_dev_free": ([P], I),
            "gh_dev_copy": ([P, P, U64], I),
            "gh_bw_copy": ([P, P, U64, P, I, ctypes.POINTER(ctypes.c_float)], I),
            "gh_index_bytes": ([U64, U32], U64),
            "gh_index_parse": ([P, ctypes.c_size_t, ctypes.POINTER(gh_index)], I),
            "gh_index_locate": ([ctypes.POINTER(gh_index), U64, U64, ctypes.POINTER(U64), ctypes.POINTER(U64),
                                 ctypes.POINTER(U64)], I),
            "gh_ctx_build_index": ([P, U32, P, U64, ctypes.POINTER(U64), ctypes.POINTER(ctypes.c_float)], I),
            "gh_gather_plan": ([ctypes.POINTER(gh_index), P, U32, P, U64, ctypes.POINTER(U64), ctypes.POINTER(U64)], I),
            "gh_ctx_gather": ([P, ctypes.POINTER(gh_index), P, U32, P, U64, P, ctypes.POINTER(ctypes.c_float)], I),
            "gh_ctx_set_index": ([P, ctypes.POINTER(gh_index)], I),
            "gh_gather_piece_bound": ([U32, U64, U32], U64),
            "gh_ctx_gather_device": ([P, P, U32, P, U64, P], I),
            "gh_ctx_gather_wait": ([P, ctypes.POINTER(gh_gather_report)], I),
            "gh_ctx_gather_times": ([P, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)], I),
            "gh_ctx_gather_pieces": ([P, P, U64, ctypes.POINTER(U64)], I),
            "gh_encode_index": ([P, ctypes.POINTER(gh_encode_plan), U32, I, P, U64], I),
            "gh_ectx_index": ([P, U32, P, U64, ctypes.POINTER(ctypes.c_float)], I),
            "gh_encode_plan_from_counts": ([P, I, ctypes.POINTER(gh_encode_plan)], I),
            "gh_encode_bound": ([U64], U64),
            "gh_slice_extent": ([U64, U64, ctypes.POINTER(gh_slice)], I),
            "gh_encode_slice": ([P, U64, ctypes.POINTER(gh_encode_plan), U64, I, P, U64, P, U64,
                                 ctypes.POINTER(gh_slice)], I),
            "gh_encode_image_init": ([ctypes.POINTER(gh_encode_plan), P, U64], I),
            "gh_slice_merge": ([P, U64, ctypes.POINTER(gh_encode_plan), ctypes.POINTER(gh_slice), P, P], I),
            "gh_ectx_counts": ([P, P], I),
            "gh_ectx_encode_slice": ([P, ctypes.POINTER(gh_encode_plan), U64, ctypes.POINTER(gh_slice),
                                      ctypes.POINTER(ctypes.c_float)], I),
            "gh_ectx_download_slice": ([P, P, U64, P, U64], I),
            "gh_encode_sharded": ([P, U64, ctypes.POINTER(gh_opts), U32, I, P, U64, ctypes.POINTER(gh_encode_plan),
                                   ctypes.POINTER(ctypes.c_float)], I),
            "gh_index_slice_extent": ([U64, U64, U32, ctypes.POINTER(U64), ctypes.POINTER(U64)], I),
            "gh_encode_index_slice": ([P, U64, ctypes.POINTER(gh_encode_plan), U64, U64, U32, I, P, U64,
                                       ctypes.POINTER(U64), ctypes.POINTER(U64)], I),
            "gh_index_image_init": ([ctypes.POINTER(gh_encode_plan), U32, P, U64], I),
            "gh_index_slice_merge": ([P, U64, U64, U64, P], I),
            "gh_ectx_index_slice": ([P, U64, U32, P, U64, ctypes.POINTER(U64), ctypes.POINTER(U64),
                                     ctypes.POINTER(ctypes.c_float)], I),
            "gh_ectx_load_device": ([P, P, U64, P], I),
            "gh_ectx_merge_device": ([P, P, U64, P, U64, P], I),
            "gh_encode_sharded_index": ([P, U64, ctypes.POINTER(gh_opts), U32, I, P, U64,
                                         ctypes.POINTER(gh_encode_plan), ctypes.POINTER(ctypes.c_float), U32, P, U64,
                                         ctypes.POINTER(ctypes.c_float)], I),
            "gh_ectx_kernel_shape": ([P, ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_enc_kernel_shapes": ([ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_enc_kernel_shape_for": ([U64, U64, I, ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_sync_lut_bits": ([], I),
            "gh_batch_create": ([I, ctypes.POINTER(P)], I),
            "gh_batch_destroy": ([P], I),
            "gh_batch_layout": ([P, U32, P], I),
            "gh_batch_load": ([P, ctypes.POINTER(gh_stream), U32], I),
            "gh_batch_load_device": ([P, ctypes.POINTER(gh_batch_item), U32, P], I),
            "gh_batch_decode": ([P, P, U64, P, I], I),
            "gh_batch_wait": ([P, ctypes.POINTER(gh_batch_report)], I),
            "gh_batch_status": ([P, P, P, U32], I),
            "gh_batch_output": ([P, ctypes.POINTER(P), ctypes.POINTER(U64)], I),
            "gh_batch_offsets": ([P, P, U32], I),
            "gh_batch_download": ([P, U32, P, U64], I),
            "gh_batch_kernel_shape": ([P, ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_batch_kernel_shapes": ([ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_batchdec_index": ([P, P, I], I),
            "gh_batchdec_gather_device": ([P, P, U32, P, U64, P, I], I),
            "gh_batchdec_gather_wait": ([P, ctypes.POINTER(gh_bgather_report)], I),
            "gh_batchdec_gather": ([P, P, U32, P, U64, P, ctypes.POINTER(gh_bgather_report)], I),
            "gh_batchdec_gather_pieces": ([P, P, U64, ctypes.POINTER(U64)], I),
            "gh_batchdec_plan": ([P, P, P, P, U32, P, U32, P, U64, ctypes.POINTER(U64), ctypes.POINTER(U64),
                                  ctypes.POINTER(U32)], I),
            "gh_batchdec_kernel_shape": ([P, ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_batchdec_kernel_shapes": ([ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_batchraw_load": ([P, ctypes.POINTER(gh_raw_stream), U32], I),
            "gh_batchraw_load_device": ([P, ctypes.POINTER(gh_batch_item), U32, P], I),
            "gh_batchraw_gaps": ([P, U32, P, U64, ctypes.POINTER(U64)], I),
            "gh_batchraw_report_get": ([P, ctypes.POINTER(gh_batchraw_report)], I),
            "gh_batchraw_gaps_host": ([P, U32, P, U64, P, U64], I),
            "gh_batchraw_kernel_shape": ([P, ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_batchraw_kernel_shapes": ([ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_ebatch_create": ([I, ctypes.POINTER(P)], I),
            "gh_ebatch_destroy": ([P], I),
            "gh_ebatch_load": ([P, P, P, U32], I),
            "gh_ebatch_load_device": ([P, ctypes.POINTER(gh_ebatch_item), U32, P], I),
            "gh_ebatch_plan": ([P, I, I], I),
            "gh_batchenc_plan_device": ([P, I], I),
            "gh_batchenc_plan_times": ([P, P, P, P], I),
            "gh_ebatch_plan_of": ([P, U32, ctypes.POINTER(gh_encode_plan)], I),
            "gh_ebatch_encode": ([P, P, I], I),
            "gh_ebatch_wait": ([P, ctypes.POINTER(gh_ebatch_report)], I),
            "gh_ebatch_sizes": ([P, P, U32], I),
            "gh_ebatch_download": ([P, U32, P, U64], I),
            "gh_ebatch_items": ([P, ctypes.POINTER(gh_batch_item), U32], I),
            "gh_ebatch_kernel_shape": ([P, ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_ebatch_kernel_shapes": ([ctypes.c_char_p, ctypes.c_size_t], I),
            "gh_planes_layout": ([ctypes.POINTER(gh_planes_item), U32, ctypes.POINTER(gh_planes_slot),
                                  ctypes.POINTER(U32), ctypes.POINTER(U64)], I),
            "gh_planes_split_host": ([ctypes.POINTER(gh_planes_item), ctypes.POINTER(P)], I),
            "gh_planes_join_host": ([ctypes.POINTER(gh_planes_item), ctypes.POINTER(P)], I),
            "gh_planes_load": ([P, ctypes.POINTER(gh_planes_item), U32, P, U64], I),
            "gh_planes_load_device": ([P, ctypes.POINTER(gh_planes_item), U32, P, U64, P], I),
            "gh_planes_load_times": ([P, ctypes.POINTER(ctypes.c_float)], I),
            "gh_planes_join_device": ([P, ctypes.POINTER(gh_planes_item), U32, P, U64, P, I], I),
            "gh_planes_wait": ([P, ctypes.POINTER(gh_planes_report)], I),
            "gh_planes_image_bytes": ([U32, P, ctypes.POINTER(U64)], I),
            "gh_planes_image_write": ([ctypes.POINTER(gh_planes_item), ctypes.POINTER(P), P, P, U64], I),
            "gh_planes_parse": ([P, ctypes.c_size_t, ctypes.POINTER(gh_planes_image)], I),
            "gh_pgather_plan": ([ctypes.POINTER(gh_planes_item), U32, P, P, U32, P, U64, ctypes.POINTER(U64), P, P,
                                 ctypes.POINTER(U64), ctypes.POINTER(U32)], I),
            "gh_pgather_device": ([P, ctypes.POINTER(gh_planes_item), U32, P, U64, P, U32, P, U64, P, I], I),
            "gh_pgather_wait": ([P, ctypes.POINTER(gh_pgather_report)], I),
            "gh_pgather": ([P, ctypes.POINTER(gh_planes_item), U32, P, U64, P, U32, P, U64, P,
                            ctypes.POINTER(gh_pgather_report)], I),
            "gh_pmask_from_counts": ([P, ctypes.POINTER(gh_planes_item), U32, P, P], I),
            "gh_pmask_host": ([ctypes.POINTER(gh_planes_item), U32, P, P], I),
            "gh_pmask_device": ([P, ctypes.POINTER(gh_planes_item), U32, P, P, P, ctypes.POINTER(gh_pmask_report)], I),
            "gh_pmask_counts": ([P, U32, P], I),
            "gh_version": ([], ctypes.c_char_p),
            "gh_last_error": ([], ctypes.c_char_p),
        }
        for name, (args, res) in sig.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        del U8
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc != GH_OK:
        raise GapHuffError(rc, lib().gh_last_error().decode(errors="replace"))


def _u8(a) -> np.ndarray:
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(a, dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def _ptr(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


def _name(fn, *args, cap: int = 64) -> str:
    """A kernel-name query: ``fn(*args, buf, cap)`` fills a NUL-terminated string."""
    buf = ctypes.create_string_buffer(cap)
    _check(fn(*args, buf, len(buf)))
    return buf.value.decode()


class _Handle:
    """Owner of one library object on one device: ``create_fn(device, &h)`` makes it,
    ``destroy_fn(h)`` releases it, on :meth:`close`, at the end of a ``with`` block or when
    the object is collected."""

    def __init__(self, create_fn, destroy_fn, device: int):
        self._h = ctypes.c_void_p()
        self._destroy = destroy_fn
        self.device = device
        _check(create_fn(device, ctypes.byref(self._h)))

    def close(self) -> None:
        if self._h:
            self._destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _wait(self, fn, report):
        """``fn(h, &report)``; raises :class:`GapHuffError` with the report as ``.report``."""
        rc = fn(self._h, ctypes.byref(report))
        if rc != GH_OK:
            e = GapHuffError(rc, lib().gh_last_error().decode(errors="replace"))
            e.report = report
            raise e
        return report


# --------------------------------------------------------------------------- format
@dataclass
class Stream:
    """A parsed compressed.huff (keeps the file bytes alive)."""

    raw: np.ndarray
    c: gh_stream

    @property
    def n(self) -> int:
        return int(self.c.n)

    @property
    def w(self) -> int:
        return int(self.c.w)

    @property
    def g(self) -> int:
        return int(self.c.g)

    @property
    def version(self) -> int:
        return int(self.c.version)

    @property
    def symbols(self) -> list:
        return [(self.c.syms[i].symbol, self.c.syms[i].length) for i in range(self.c.nsyms)]

    @classmethod
    def from_plan(cls, plan: "gh_encode_plan") -> "Stream":
        """A header-only stream of the plan's sizes and code, for :meth:`Decoder.load_device`:
        ``syms`` point into (a kept copy of) the plan, the word pointers are null."""
        keep = gh_encode_plan.from_buffer_copy(plan)
        s = gh_stream()
        s.syms = ctypes.cast(ctypes.byref(keep, gh_encode_plan.syms.offset), ctypes.POINTER(gh_sym))
        s.nsyms, s.version = keep.nsyms, keep.version
        s.n, s.w, s.g = keep.n, keep.w, keep.g
        s.gap_words = s.payload = None
        st = cls(np.zeros(0, dtype=np.uint8), s)
        st._plan = keep  # (syms point into it)
        return st


def parse(file_bytes) -> Stream:
    raw = _u8(file_bytes)
    s = gh_stream()
    _check(lib().gh_stream_parse(_ptr(raw), raw.size, ctypes.byref(s)))
    return Stream(raw, s)


# --------------------------------------------------------------------------- encoder
def encode_plan(data, threads: int = 0, force_version: int = 0) -> gh_encode_plan:
    d = _u8(data)
    plan = gh_encode_plan()
    _check(lib().gh_encode_plan_make(_ptr(d), d.size, threads, force_version, ctypes.byref(plan)))
    return plan


def encode(data, threads: int = 0, force_version: int = 0) -> np.ndarray:
    """Compress bytes into a compressed.huff image (np.uint8)."""
    d = _u8(data)
    plan = encode_plan(d, threads, force_version)
    out = np.empty(plan.file_bytes, dtype=np.uint8)
    _check(lib().gh_encode_write(_ptr(d), ctypes.byref(plan), threads, _ptr(out), out.size))
    return out


def encode_index(data, log2_stride: int = 8, threads: int = 0, force_version: int = 0) -> np.ndarray:
    """Seek index (sidecar image, np.uint8) of the stream ``encode(data)`` produces, from
    the data alone (gh_encode_index): no decode, no device."""
    d = _u8(data)
    plan = encode_plan(d, threads, force_version)
    nbytes = int(lib().gh_index_bytes(plan.g, log2_stride))
    if nbytes == 0:
        raise GapHuffError(-1, "index stride outside 2^8 .. 2^20 segments")
    img = np.zeros(nbytes, dtype=np.uint8)
    _check(lib().gh_encode_index(_ptr(d), ctypes.byref(plan), log2_stride, threads, _ptr(img), img.size))
    return img


# ---- sliced encode (include/gaphuff.h, "sliced encode") ----
def plan_from_counts(counts, force_version: int = 0) -> gh_encode_plan:
    """The stream-wide plan from a 256-entry histogram (e.g. the sum of the slices')."""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    if c.size != 256:
        raise GapHuffError(-1, "a histogram has 256 counts")
    plan = gh_encode_plan()
    _check(lib().gh_encode_plan_from_counts(_ptr(c), force_version, ctypes.byref(plan)))
    return plan


def slice_extent(base_bit: int, bits: int) -> gh_slice:
    s = gh_slice()
    _check(lib().gh_slice_extent(base_bit, bits, ctypes.byref(s)))
    return s


def encode_slice(data, plan: gh_encode_plan, base_bit: int, threads: int = 0):
    """Host encoder of one slice of the stream planned by ``plan``: ``data`` as the code
    bits from ``base_bit`` on.  Returns (gh_slice, words, gapw): the slice-local payload
    and gap words (np.uint32), indexed from slice.word0 / slice.gapw0."""
    d = _u8(data)
    s = gh_slice()
    rc = lib().gh_encode_slice(_ptr(d), d.size, ctypes.byref(plan), base_bit, threads, None, 0, None, 0,
                               ctypes.byref(s))
    if rc not in (GH_OK, -9):
        _check(rc)
    words = np.zeros(int(s.nwords), dtype=np.uint32)
    gapw = np.zeros(int(s.ngapw), dtype=np.uint32)
    _check(lib().gh_encode_slice(_ptr(d), d.size, ctypes.byref(plan), base_bit, threads, _ptr(words), words.size,
                                 _ptr(gapw), gapw.size, ctypes.byref(s)))
    return s, words, gapw


def merge_slices(plan: gh_encode_plan, parts) -> np.ndarray:
    """The compressed.huff image (np.uint8) of the (gh_slice, words, gapw) ``parts``, in
    any order (gh_encode_image_init + gh_slice_merge, one after the other)."""
    img = np.empty(plan.file_bytes, dtype=np.uint8)
    _check(lib().gh_encode_image_init(ctypes.byref(plan), _ptr(img), img.size))
    for s, words, gapw in parts:
        w = np.ascontiguousarray(words, dtype=np.uint32)
        g = np.ascontiguousarray(gapw, dtype=np.uint32)
        if w.size < s.nwords or g.size < s.ngapw:
            raise GapHuffError(-1, "slice buffers shorter than the slice's extents")
        _check(lib().gh_slice_merge(_ptr(img), img.size, ctypes.byref(plan), ctypes.byref(s), _ptr(w), _ptr(g)))
    return img


# ---- the index of a sliced stream (include/gaphuff.h) ----
def index_slice_extent(base_bit: int, bits: int, log2_stride: int = 8):
    """(k0, nk): the index entries the slice holding code bits [base_bit, base_bit + bits)
    owns (gh_index_slice_extent)."""
    k0, nk = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().gh_index_slice_extent(base_bit, bits, log2_stride, ctypes.byref(k0), ctypes.byref(nk)))
    return int(k0.value), int(nk.value)


def encode_index_slice(data, plan: gh_encode_plan, base_bit: int, sym_base: int, log2_stride: int = 8,
                       threads: int = 0):
    """Host: (entries as np.uint64, k0) of ``data`` as the slice at ``base_bit`` /
    ``sym_base`` of the stream planned by ``plan`` (gh_encode_index_slice); the buffer
    holds exactly the slice's nk entries."""
    d = _u8(data)
    k0, nk = ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib().gh_encode_index_slice(_ptr(d), d.size, ctypes.byref(plan), base_bit, sym_base, log2_stride, threads,
                                     None, 0, ctypes.byref(k0), ctypes.byref(nk))
    if rc not in (GH_OK, -9):
        _check(rc)
    ent = np.zeros(int(nk.value), dtype=np.uint64)
    _check(lib().gh_encode_index_slice(_ptr(d), d.size, ctypes.byref(plan), base_bit, sym_base, log2_stride, threads,
                                       _ptr(ent), ent.size, ctypes.byref(k0), ctypes.byref(nk)))
    return ent, int(k0.value)


def merge_index_slices(plan: gh_encode_plan, log2_stride: int, parts) -> np.ndarray:
    """The seek index image (np.uint8) of the (entries, k0) ``parts``, in any order
    (gh_index_image_init + gh_index_slice_merge).  With a slice missing the image does not
    parse."""
    nbytes = int(lib().gh_index_bytes(plan.g, log2_stride))
    if nbytes == 0:
        raise GapHuffError(-1, "index stride outside 2^8 .. 2^20 segments")
    img = np.empty(nbytes, dtype=np.uint8)
    _check(lib().gh_index_image_init(ctypes.byref(plan), log2_stride, _ptr(img), img.size))
    for part in parts:
        ent = np.ascontiguousarray(part[0], dtype=np.uint64)
        _check(lib().gh_index_slice_merge(_ptr(img), img.size, int(part[1]), ent.size, _ptr(ent)))
    return img


class Encoder(_Handle):
    """One gh_ectx: the GPU encoder on one gfx950 device.

    Mirrors the reference encoder CLI's steps (encoder/src/huff.cpp:30-220): load the
    input, plan (histogram on the GPU, package-merge on the host), encode, download
    the compressed.huff image -- byte-identical to ``encode()``."""

    def __init__(self, device: int = 0):
        super().__init__(lib().gh_ectx_create, lib().gh_ectx_destroy, device)
        self.plan: Optional[gh_encode_plan] = None
        self._slice: Optional[gh_slice] = None  # extents of the last slice encode

    def load(self, data) -> None:
        d = _u8(data)
        _check(lib().gh_ectx_load(self._h, _ptr(d), d.size))

    def load_device(self, ptr: int, n: int, hip_stream: int = 0) -> None:
        """Load ``n`` input bytes from device memory at address ``ptr`` (gh_ectx_load_device):
        copied on the device after what ``hip_stream`` (0: the default stream) holds now."""
        _check(lib().gh_ectx_load_device(self._h, ctypes.c_void_p(ptr or None), n, ctypes.c_void_p(hip_stream or None)))

    def make_plan(self, force_version: int = 0) -> gh_encode_plan:
        p = gh_encode_plan()
        _check(lib().gh_ectx_plan(self._h, force_version, ctypes.byref(p)))
        self.plan = p
        return p

    def encode(self) -> float:
        """Encode on the device; returns the kernels' event time in ms."""
        ms = ctypes.c_float()
        _check(lib().gh_ectx_encode(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def download(self) -> np.ndarray:
        if self.plan is None:
            raise GapHuffError(-8, "download before make_plan/encode")
        out = np.empty(self.plan.file_bytes, dtype=np.uint8)
        _check(lib().gh_ectx_download(self._h, _ptr(out), out.size))
        return out

    def kernel_shape(self) -> str:
        """Name of the write kernel instantiation the last encode or slice encode picked
        (gh_ectx_kernel_shape)."""
        return _name(lib().gh_ectx_kernel_shape, self._h)

    def counts(self) -> np.ndarray:
        """GPU histogram of the loaded input (256 x np.uint64); makes no plan."""
        c = np.zeros(256, dtype=np.uint64)
        _check(lib().gh_ectx_counts(self._h, _ptr(c)))
        self.plan = None
        return c

    def encode_slice(self, plan: gh_encode_plan, base_bit: int):
        """Encode the loaded input as the slice at ``base_bit`` of the stream planned by
        ``plan`` (gh_ectx_encode_slice): (gh_slice, kernel ms)."""
        s = gh_slice()
        ms = ctypes.c_float()
        _check(lib().gh_ectx_encode_slice(self._h, ctypes.byref(plan), base_bit, ctypes.byref(s), ctypes.byref(ms)))
        self._slice = s
        return s, float(ms.value)

    def download_slice(self):
        """(words, gapw) of the last slice encode, laid out as :func:`encode_slice`'s."""
        s = self._slice or gh_slice()
        words = np.zeros(int(s.nwords), dtype=np.uint32)
        gapw = np.zeros(int(s.ngapw), dtype=np.uint32)
        _check(lib().gh_ectx_download_slice(self._h, _ptr(words), words.size, _ptr(gapw), gapw.size))
        return words, gapw

    def index_slice(self, sym_base: int, log2_stride: int = 8):
        """The index entries the last slice encode owns, built on the device
        (gh_ectx_index_slice): (entries as np.uint64, k0, kernel ms).  ``sym_base``: the
        stream offset of the slice's first byte."""
        k0, nk, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_float()
        rc = lib().gh_ectx_index_slice(self._h, sym_base, log2_stride, None, 0, ctypes.byref(k0), ctypes.byref(nk), None)
        if rc not in (GH_OK, -9):
            _check(rc)
        ent = np.zeros(int(nk.value), dtype=np.uint64)
        _check(lib().gh_ectx_index_slice(self._h, sym_base, log2_stride, _ptr(ent), ent.size, ctypes.byref(k0),
                                         ctypes.byref(nk), ctypes.byref(ms)))
        return ent, int(k0.value), float(ms.value)

    def merge_device(self, payload_ptr: int, payload_words: int, gap_ptr: int, gap_words: int,
                     hip_stream: int = 0) -> None:
        """OR the last encode (a slice, or a whole encode) into the stream's zeroed device
        arrays: ``payload_words`` u32 at ``payload_ptr``, ``gap_words`` u32 at ``gap_ptr``,
        both 16-byte aligned (gh_ectx_merge_device)."""
        _check(lib().gh_ectx_merge_device(self._h, ctypes.c_void_p(payload_ptr or None), payload_words,
                                          ctypes.c_void_p(gap_ptr or None), gap_words,
                                          ctypes.c_void_p(hip_stream or None)))

    def index(self, log2_stride: int = 8):
        """Seek index of the encoded stream, built on the device from what the encode left
        there (gh_ectx_index): (sidecar image as np.uint8, kernel ms)."""
        g = self.plan.g if self.plan is not None else 0
        nbytes = int(lib().gh_index_bytes(g, log2_stride))
        if nbytes == 0:
            raise GapHuffError(-1, "index stride outside 2^8 .. 2^20 segments")
        img = np.zeros(nbytes, dtype=np.uint8)
        ms = ctypes.c_float()
        _check(lib().gh_ectx_index(self._h, log2_stride, _ptr(img), img.size, ctypes.byref(ms)))
        return img, float(ms.value)


def encode_gpu(data, device: int = 0, force_version: int = 0) -> np.ndarray:
    """Compress bytes on the GPU into a compressed.huff image (== ``encode(data)``)."""
    with Encoder(device) as e:
        e.load(data)
        e.make_plan(force_version)
        e.encode()
        return e.download()


def encode_sharded(data, nslices: int, devices: Optional[Sequence[int]] = None, force_version: int = 0,
                   return_ms: bool = False, index_log2_stride: Optional[int] = None):
    """Compress bytes on the GPU(s) slice by slice (gh_encode_sharded): ``nslices`` even
    cuts, slice i on ``devices[i % len(devices)]`` (default: device 0).  The image equals
    ``encode(data)``; with ``return_ms`` also the encode kernels' time (the slowest
    device's sum).  With ``index_log2_stride`` (gh_encode_sharded_index) the stream's seek
    index image, from the slices' own entries, is added to the tuple: (image, index) or
    (image, ms, index)."""
    d = _u8(data)
    o = gh_opts()
    o.ngpus, o.reps = 1, 1
    if devices is not None:
        arr = (ctypes.c_int * len(devices))(*devices)
        o.devices = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int))
        o.ngpus = len(devices)
    out = np.empty(int(lib().gh_encode_bound(d.size)), dtype=np.uint8)
    plan = gh_encode_plan()
    ms = ctypes.c_float()
    if index_log2_stride is None:
        _check(lib().gh_encode_sharded(_ptr(d), d.size, ctypes.byref(o), nslices, force_version, _ptr(out), out.size,
                                       ctypes.byref(plan), ctypes.byref(ms)))
        img = out[: plan.file_bytes]
        return (img, float(ms.value)) if return_ms else img
    # (G <= ceil(n / 8); a bad stride: one byte, and the library's refusal)
    idx = np.zeros(max(1, int(lib().gh_index_bytes((d.size + 7) // 8, index_log2_stride))), dtype=np.uint8)
    _check(lib().gh_encode_sharded_index(_ptr(d), d.size, ctypes.byref(o), nslices, force_version, _ptr(out), out.size,
                                         ctypes.byref(plan), ctypes.byref(ms), index_log2_stride, _ptr(idx), idx.size,
                                         None))
    img, idx = out[: plan.file_bytes], idx[: int(lib().gh_index_bytes(plan.g, index_log2_stride))]
    return (img, float(ms.value), idx) if return_ms else (img, idx)


def package_merge(sorted_counts: Sequence[int]) -> list:
    c = np.ascontiguousarray(sorted_counts, dtype=np.uint64)
    out = np.zeros(max(1, c.size), dtype=np.uint8)
    _check(lib().gh_package_merge(_ptr(c), c.size, _ptr(out)))
    return out[: c.size].tolist()


def package_merge_flat(sorted_counts: Sequence[int]) -> list:
    """:func:`package_merge` by the level-by-level form the batched encoder's code kernel runs
    (gh_package_merge_flat): the same lengths for every input."""
    c = np.ascontiguousarray(sorted_counts, dtype=np.uint64)
    out = np.zeros(max(1, c.size), dtype=np.uint8)
    _check(lib().gh_package_merge_flat(_ptr(c), c.size, _ptr(out)))
    return out[: c.size].tolist()


def generate(seed: int, redundancy: float, n: int, offset: int = 0, threads: int = 0) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    _check(lib().gh_generate(seed, float(redundancy), offset, n, _ptr(out), threads))
    return out


def plan_shards(g: int, nshards: int) -> list:
    b = np.zeros(nshards + 1, dtype=np.uint64)
    _check(lib().gh_plan_shards(g, nshards, _ptr(b)))
    return [int(x) for x in b]


def kernel_shapes() -> list:
    """Every kernel name a load can pick (gh_kernel_shapes); needs no device."""
    return _name(lib().gh_kernel_shapes, cap=1 << 14).split()


def enc_kernel_shapes() -> list:
    """Every write kernel name an encode can pick (gh_enc_kernel_shapes); needs no device."""
    return _name(lib().gh_enc_kernel_shapes, cap=1 << 10).split()


def enc_kernel_shape_for(n: int, bits: int, slice: bool = False) -> str:
    """The write kernel an encode picks for ``n`` input bytes of ``bits`` code bits
    (gh_enc_kernel_shape_for); needs no device."""
    return _name(lib().gh_enc_kernel_shape_for, n, bits, int(slice))


def sync_lut_bits() -> int:
    """Prefix bits of the self-synchronising decode's length table (gh_sync_lut_bits)."""
    return int(lib().gh_sync_lut_bits())


def device_count() -> int:
    return int(lib().gh_device_count())


# --------------------------------------------------------------------------- decoder
class Decoder(_Handle):
    """One gh_ctx: a shard of a stream resident on one GPU."""

    def __init__(self, device: int = 0):
        super().__init__(lib().gh_ctx_create, lib().gh_ctx_destroy, device)
        self._stream: Optional[Stream] = None
        self._file_g: Optional[int] = None  # G of the last load_file / load_raw

    def load(self, stream: Stream, seg_begin: int = 0, seg_end: Optional[int] = None,
             out_cap: int = 0) -> None:
        seg_end = stream.g if seg_end is None else seg_end
        self._stream = stream
        _check(lib().gh_ctx_load(self._h, ctypes.byref(stream.c), seg_begin, seg_end, out_cap))

    def load_device(self, stream: Stream, payload_ptr: int, payload_words: int, gap_ptr: int, seg_begin: int = 0,
                    seg_end: Optional[int] = None, out_cap: int = 0) -> None:
        """Load from device-resident words (gh_ctx_load_device): ``stream`` supplies the sizes
        and the code (e.g. :meth:`Stream.from_plan`); ``payload_words`` u32 at ``payload_ptr``
        and the whole gap array at ``gap_ptr`` stay owned by the caller."""
        seg_end = stream.g if seg_end is None else seg_end
        self._stream = stream
        _check(lib().gh_ctx_load_device(self._h, ctypes.byref(stream.c), seg_begin, seg_end,
                                        ctypes.c_void_p(payload_ptr or None), payload_words,
                                        ctypes.c_void_p(gap_ptr or None), out_cap))

    def load_file(self, path: str, seg_begin: int = 0, seg_end: Optional[int] = None,
                  out_cap: int = 0) -> gh_file_info:
        """Stream segments [seg_begin, seg_end) of a compressed.huff file to the device
        (pinned double-buffered read -> H2D); returns the header sizes and timings."""
        info = gh_file_info()
        _check(lib().gh_ctx_load_file(self._h, os.fsencode(path), seg_begin,
                                      (1 << 64) - 1 if seg_end is None else seg_end, out_cap,
                                      ctypes.byref(info)))
        self._stream = None
        self._file_g = int(info.g)
        return info

    def save_file(self, path: str, nbytes: int, file_offset: int = 0, offset: int = 0,
                  truncate: bool = True) -> float:
        """Write decoded bytes [offset, offset+nbytes) to `path` at file_offset; wall ms."""
        ms = ctypes.c_double()
        _check(lib().gh_ctx_save_file(self._h, os.fsencode(path), file_offset, offset, nbytes,
                                      int(truncate), ctypes.byref(ms)))
        return ms.value

    def load_raw(self, symbols: Sequence[tuple], n: int, units, out_cap: int = 0) -> gh_sync_report:
        """Load a raw (gap-less) stream: u32 ``units``, canonical ``symbols`` list
        [(symbol, length)] in code order, ``n`` output bytes.  The gap array is
        built on the GPU (gh_sync_gaps); returns its report."""
        u = np.ascontiguousarray(units, dtype=np.uint32)
        sy = _syms(symbols)
        r = gh_sync_report()
        _check(lib().gh_ctx_load_raw(self._h, ctypes.byref(sy), len(symbols), n, _ptr(u), u.size, out_cap,
                                     ctypes.byref(r)))
        self._stream = None
        self._file_g = int(r.g)
        return r

    def decode(self, hip_stream: int = 0, timed: bool = True) -> None:
        _check(lib().gh_ctx_decode(self._h, ctypes.c_void_p(hip_stream or None), int(timed)))

    def report(self, hip_stream: int = 0) -> gh_report:
        r = gh_report()
        _check(lib().gh_ctx_report(self._h, ctypes.c_void_p(hip_stream or None), ctypes.byref(r)))
        return r

    def kernel_shape(self) -> str:
        """Name of the kernel instantiation(s) the last load picked (gh_ctx_kernel_shape)."""
        return _name(lib().gh_ctx_kernel_shape, self._h, cap=256)

    def offsets_state(self) -> int:
        """State of the loaded shard's known piece offsets (gh_ctx_offsets_state):
        GH_OFFS_NONE, GH_OFFS_RECORDED, or GH_OFFS_READY when the next decode reads them."""
        st = ctypes.c_int()
        _check(lib().gh_ctx_offsets_state(self._h, ctypes.byref(st)))
        return int(st.value)

    def build_index(self, log2_stride: int = 8):
        """Seek index of the loaded stream (the load must cover all its segments), built on
        the GPU: (sidecar image as np.uint8, codewords counted, kernel ms)."""
        g = self._stream.g if self._stream is not None else (self._file_g or 0)
        nbytes = int(lib().gh_index_bytes(g, log2_stride))
        if nbytes == 0:
            raise GapHuffError(-1, "index stride outside 2^8 .. 2^20 segments")
        img = np.zeros(nbytes, dtype=np.uint8)
        symbols = ctypes.c_uint64()
        ms = ctypes.c_float()
        _check(lib().gh_ctx_build_index(self._h, log2_stride, _ptr(img), img.size, ctypes.byref(symbols),
                                        ctypes.byref(ms)))
        return img, int(symbols.value), float(ms.value)

    def gather(self, index, ranges, dst_ptr: int = 0, dst_len: int = 0, hip_stream: int = 0):
        """Bytes of the (lo, hi) ``ranges`` of the loaded stream (the load must cover all
        its segments), concatenated in request order, in one launch (gh_ctx_gather):
        (np.uint8 array, kernel ms).  With ``dst_ptr`` (a device or host address with room
        for ``dst_len`` bytes) the bytes go there and the first item is their count."""
        ix = index if isinstance(index, Index) else parse_index(index)
        r = _ranges(ranges)
        total = int((r[:, 1] - r[:, 0]).sum()) if r.size and (r[:, 1] >= r[:, 0]).all() else 0
        ms = ctypes.c_float()
        if dst_ptr:
            out, dst, cap = None, ctypes.c_void_p(dst_ptr), dst_len
        else:
            out = np.empty(total, dtype=np.uint8)
            dst, cap = _ptr(out), out.size
        _check(lib().gh_ctx_gather(self._h, ctypes.byref(ix.c), _ptr(r), r.shape[0], dst, cap,
                                   ctypes.c_void_p(hip_stream or None), ctypes.byref(ms)))
        return (total if out is None else out), float(ms.value)

    def set_index(self, index) -> None:
        """Keep the entries of ``index`` (an :class:`Index` or a sidecar image) on the device
        for :meth:`gather_device` (gh_ctx_set_index); the next load drops them."""
        ix = index if isinstance(index, Index) else parse_index(index)
        _check(lib().gh_ctx_set_index(self._h, ctypes.byref(ix.c)))

    def gather_device(self, ranges_ptr: int, nranges: int, dst_ptr: int, dst_len: int, hip_stream: int = 0) -> None:
        """Enqueue the gather of ``nranges`` (lo, hi) pairs held in device memory at
        ``ranges_ptr`` (a contiguous int64/uint64 [n, 2] array) into the ``dst_len`` device
        bytes at ``dst_ptr``, planned on the GPU, and return without waiting
        (gh_ctx_gather_device).  Addresses are integers (``tensor.data_ptr()``,
        ``DeviceBuffer.addr``).  What only the device finds is raised by :meth:`gather_wait`."""
        _check(lib().gh_ctx_gather_device(self._h, ctypes.c_void_p(ranges_ptr or None), nranges,
                                          ctypes.c_void_p(dst_ptr or None), dst_len,
                                          ctypes.c_void_p(hip_stream or None)))

    def gather_wait(self) -> gh_gather_report:
        """Wait for the last :meth:`gather_device` and return its report; raises
        :class:`GapHuffError` (with the report as ``.report``) on a device-side refusal."""
        r = gh_gather_report()
        rc = lib().gh_ctx_gather_wait(self._h, ctypes.byref(r))
        if rc != GH_OK:
            e = GapHuffError(rc, lib().gh_last_error().decode(errors="replace"))
            e.report = r
            raise e
        return r

    def gather_times(self):
        """(plan kernels ms, gather kernel ms) of the last :meth:`gather_device`."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(lib().gh_ctx_gather_times(self._h, ctypes.byref(a), ctypes.byref(b)))
        return float(a.value), float(b.value)

    def gather_pieces(self) -> np.ndarray:
        """The pieces of the last :meth:`gather_device` as the record array
        :meth:`Index.plan` returns (gh_ctx_gather_pieces)."""
        n = ctypes.c_uint64()
        rc = lib().gh_ctx_gather_pieces(self._h, None, 0, ctypes.byref(n))
        if rc not in (GH_OK, -9):
            _check(rc)
        pieces = np.zeros(int(n.value), dtype=PIECE_DTYPE)
        _check(lib().gh_ctx_gather_pieces(self._h, _ptr(pieces), pieces.size, ctypes.byref(n)))
        return pieces

    def reset_timing(self) -> None:
        _check(lib().gh_ctx_reset_timing(self._h))

    def download(self, nbytes: int, offset: int = 0) -> np.ndarray:
        out = np.empty(nbytes, dtype=np.uint8)
        _check(lib().gh_ctx_download(self._h, offset, _ptr(out), nbytes))
        return out

    def copy_output(self, dst_ptr: int, nbytes: int, offset: int = 0, hip_stream: int = 0) -> None:
        """Async copy of shard output bytes to a device/host address (e.g. a torch tensor)."""
        _check(lib().gh_ctx_copy_output(self._h, offset, ctypes.c_void_p(dst_ptr), nbytes,
                                        ctypes.c_void_p(hip_stream or None)))

    def output(self):
        p = ctypes.c_void_p()
        cap = ctypes.c_uint64()
        _check(lib().gh_ctx_output(self._h, ctypes.byref(p), ctypes.byref(cap)))
        return int(p.value or 0), int(cap.value)


def decode(file_bytes, ngpus: int = 1, devices: Optional[Sequence[int]] = None,
           reps: int = 1) -> np.ndarray:
    """Decode a whole compressed.huff image on the GPU(s); returns the N bytes."""
    s = parse(file_bytes)
    out = np.empty(max(1, s.n), dtype=np.uint8)
    o = gh_opts()
    o.ngpus = ngpus
    o.reps = reps
    if devices is not None:
        arr = (ctypes.c_int * len(devices))(*devices)
        o.devices = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int))
    r = gh_report()
    _check(lib().gh_decode(ctypes.byref(s.c), _ptr(out), out.size, ctypes.byref(o), ctypes.byref(r)))
    return out[: s.n]


# --------------------------------------------------------------------------- batched decode
def batch_layout(ns) -> np.ndarray:
    """Output offsets of a batch of streams of ``ns`` bytes (gh_batch_layout): ``len(ns) + 1``
    uint64, every stream 16-byte aligned, the last entry the arena size.  Needs no device."""
    n = np.ascontiguousarray(ns, dtype=np.uint64)
    off = np.zeros(n.size + 1, dtype=np.uint64)
    _check(lib().gh_batch_layout(_ptr(n) if n.size else None, n.size, _ptr(off)))
    return off


def batch_kernel_shapes() -> list:
    """Every kernel name a batch load can pick (gh_batch_kernel_shapes); needs no device."""
    return _name(lib().gh_batch_kernel_shapes, cap=1 << 10).split()


def batchraw_kernel_shapes() -> list:
    """Every kernel name a raw batch load can pick (gh_batchraw_kernel_shapes); needs no device."""
    return _name(lib().gh_batchraw_kernel_shapes, cap=1 << 10).split()


def raw_gaps_host(units, symbols: Sequence[tuple]) -> np.ndarray:
    """Gap words of the raw stream ``units`` (u32) under the canonical ``symbols`` list, by the
    host twin of the batched raw load's kernels (gh_batchraw_gaps_host); needs no device."""
    u = np.ascontiguousarray(units, dtype=np.uint32)
    sy = _syms(symbols)
    g = -(-u.size // 4)
    out = np.zeros(-(-g // 8), dtype=np.uint32)
    _check(lib().gh_batchraw_gaps_host(ctypes.byref(sy) if len(symbols) else None, len(symbols),
                                       _ptr(u) if u.size else None, u.size, _ptr(out) if out.size else None, out.size))
    return out


def batchdec_kernel_shapes() -> list:
    """Every kernel name a batched gather can pick (gh_batchdec_kernel_shapes); needs no device."""
    return _name(lib().gh_batchdec_kernel_shapes, cap=1 << 10).split()


def _branges(ranges) -> np.ndarray:
    """(stream, lo, hi) triples as the C array of gh_brange: a contiguous (n, 3) uint64 array."""
    if not isinstance(ranges, np.ndarray):
        ranges = list(ranges)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 3))
    if r.shape[0] >= 1 << 32:
        raise GapHuffError(-1, "2^32 or more ranges in one batch")
    return r


def batch_gather_plan(unit0, unit_off, n, status, ranges):
    """The batched gather's plan from host arrays (gh_batchdec_plan; needs no device):
    ``(pieces, out_bytes, bad_ranges)`` with the pieces as a :data:`PIECE_DTYPE` record array
    whose ``block`` is the global unit index.  ``unit0``: ``nstreams + 1`` prefix of the
    streams' unit counts; ``unit_off``: ``unit0[-1] + 1`` exclusive scan of the codewords per
    unit; ``n``: the streams' bytes; ``status``: their status words, or None."""
    u0 = np.ascontiguousarray(unit0, dtype=np.uint32)
    uo = np.ascontiguousarray(unit_off, dtype=np.uint64)
    nn = np.ascontiguousarray(n, dtype=np.uint64)
    st = None if status is None else np.ascontiguousarray(status, dtype=np.uint32)
    r = _branges(ranges)
    ns = nn.size
    if u0.size != ns + 1 or uo.size != int(u0[-1]) + 1 or (st is not None and st.size != ns):
        raise GapHuffError(-1, "batch_gather_plan: array sizes disagree")
    np_, total, bad = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
    args = (_ptr(u0), _ptr(uo), _ptr(nn) if ns else None, _ptr(st) if st is not None and ns else None, ns,
            _ptr(r) if r.size else None, r.shape[0])
    tail = (ctypes.byref(np_), ctypes.byref(total), ctypes.byref(bad))
    rc = lib().gh_batchdec_plan(*args, None, 0, *tail)
    if rc not in (GH_OK, -9):
        _check(rc)
    pieces = np.zeros(int(np_.value), dtype=PIECE_DTYPE)
    _check(lib().gh_batchdec_plan(*args, _ptr(pieces) if pieces.size else None, pieces.size, *tail))
    return pieces, int(total.value), int(bad.value)


class BatchDecoder(_Handle):
    """One gh_batch: many independent streams resident on one GPU, decoded by one fixed set
    of kernel launches per batch."""

    def __init__(self, device: int = 0):
        super().__init__(lib().gh_batch_create, lib().gh_batch_destroy, device)
        self.ns: list = []  # output bytes of every loaded stream
        self._indexed = False  # an index() or decode() since the load

    def load(self, images_or_streams) -> None:
        """Load a batch from host memory: compressed.huff images (bytes / np.uint8) or parsed
        :class:`Stream` objects, in batch order (gh_batch_load)."""
        streams = [s if isinstance(s, Stream) else parse(s) for s in images_or_streams]
        arr = (gh_stream * max(1, len(streams)))()
        for i, s in enumerate(streams):
            arr[i] = s.c
        self._indexed = False
        _check(lib().gh_batch_load(self._h, arr, len(streams)))
        self.ns = [s.n for s in streams]

    def load_device(self, items, hip_stream: int = 0) -> None:
        """Load a batch whose words are device memory (gh_batch_load_device): ``items`` are
        ``(stream, payload_ptr, gap_ptr)`` with a :class:`Stream` for the sizes and the code
        (e.g. a parsed image or :meth:`Stream.from_plan`) and two 4-byte-aligned device
        addresses as integers."""
        items = list(items)
        arr = (gh_batch_item * max(1, len(items)))()
        for i, (s, pay, gap) in enumerate(items):
            arr[i].syms, arr[i].nsyms = s.c.syms, s.c.nsyms
            arr[i].n, arr[i].w, arr[i].g = s.c.n, s.c.w, s.c.g
            arr[i].d_payload, arr[i].d_gap_words = pay or None, gap or None
        self._indexed = False
        _check(lib().gh_batch_load_device(self._h, arr, len(items), ctypes.c_void_p(hip_stream or None)))
        self.ns = [s.n for s, _, _ in items]

    def load_raw(self, raws) -> None:
        """Load a batch of gap-less (raw) streams from host memory (gh_batchraw_load): each item
        is a raw-stream container image (bytes / np.uint8) or a ``(symbols, n, units)`` triple
        as :func:`parse_raw` returns.  Their gap arrays are built on the GPU."""
        triples = [r if isinstance(r, tuple) else parse_raw(r) for r in raws]
        arr = (gh_raw_stream * max(1, len(triples)))()
        keep = []
        for i, (symbols, n, units) in enumerate(triples):
            # (symbol, length) byte pairs are gh_sym's layout; a batch holds thousands of tables
            sy = np.ascontiguousarray(np.asarray(symbols, dtype=np.uint8).reshape(-1, 2))
            u = np.ascontiguousarray(units, dtype=np.uint32)
            keep.append((sy, u))
            arr[i].syms = ctypes.cast(_ptr(sy), ctypes.POINTER(gh_sym)) if sy.size else None
            arr[i].nsyms, arr[i].n, arr[i].w = len(symbols), n, u.size
            arr[i].units = _ptr(u) if u.size else None
        self._indexed = False
        _check(lib().gh_batchraw_load(self._h, arr, len(triples)))
        self.ns = [int(n) for _, n, _ in triples]

    def load_raw_device(self, items, hip_stream: int = 0) -> None:
        """:meth:`load_device` for gap-less streams (gh_batchraw_load_device): the same
        ``(stream, payload_ptr, gap_ptr)`` items, ``gap_ptr`` ignored, ``stream.g`` equal to
        ceil(w / 4).  :meth:`BatchEncoder.items` output is a valid source."""
        items = list(items)
        arr = (gh_batch_item * max(1, len(items)))()
        for i, (s, pay, _) in enumerate(items):
            arr[i].syms, arr[i].nsyms = s.c.syms, s.c.nsyms
            arr[i].n, arr[i].w, arr[i].g = s.c.n, s.c.w, s.c.g
            arr[i].d_payload, arr[i].d_gap_words = pay or None, None
        self._indexed = False
        _check(lib().gh_batchraw_load_device(self._h, arr, len(items), ctypes.c_void_p(hip_stream or None)))
        self.ns = [s.n for s, _, _ in items]

    def raw_gaps(self, i: int) -> np.ndarray:
        """The resident gap words of stream ``i`` (gh_batchraw_gaps), after either kind of load."""
        n = ctypes.c_uint64()
        rc = lib().gh_batchraw_gaps(self._h, i, None, 0, ctypes.byref(n))
        if rc not in (GH_OK, -9):
            _check(rc)
        out = np.zeros(int(n.value), dtype=np.uint32)
        _check(lib().gh_batchraw_gaps(self._h, i, _ptr(out) if out.size else None, out.size, ctypes.byref(n)))
        return out

    def raw_report(self) -> gh_batchraw_report:
        """Event time, launch count and scratch of the last raw load's gap kernels
        (gh_batchraw_report_get); GH_E_STATE when the last load was not raw."""
        rep = gh_batchraw_report()
        _check(lib().gh_batchraw_report_get(self._h, ctypes.byref(rep)))
        return rep

    def raw_kernel_shape(self) -> str:
        """Name of the T_j kernel instantiation the last raw load picked (gh_batchraw_kernel_shape)."""
        return _name(lib().gh_batchraw_kernel_shape, self._h)

    def decode(self, dst_ptr: int = 0, dst_len: int = 0, hip_stream: int = 0, timed: bool = True) -> None:
        """Enqueue one decode of the batch into the device memory at ``dst_ptr`` (16-byte
        aligned, ``dst_len`` bytes), or into the batch's own arena, and return."""
        _check(lib().gh_batch_decode(self._h, ctypes.c_void_p(dst_ptr or None), dst_len,
                                     ctypes.c_void_p(hip_stream or None), int(timed)))
        self._indexed = True

    def index(self, hip_stream: int = 0, timed: bool = True) -> None:
        """Enqueue the count and scan kernels alone (gh_batchdec_index): the seek index the
        gathers read, and the per-stream status :meth:`wait` and :meth:`status` report,
        without writing an output byte."""
        _check(lib().gh_batchdec_index(self._h, ctypes.c_void_p(hip_stream or None), int(timed)))
        self._indexed = True

    def gather(self, ranges) -> list:
        """The bytes of each ``(stream, lo, hi)`` range of the loaded batch, as a list of
        np.uint8 arrays in request order (gh_batchdec_gather).  ``ranges``: an iterable of
        triples or an int64 / uint64 ``[n, 3]`` array.  Runs :meth:`index` first when the batch
        is neither indexed nor decoded."""
        r = _branges(ranges)
        if not self._indexed:
            self.index()
        lens = (r[:, 2] - r[:, 1]).astype(np.int64) if r.size and (r[:, 2] >= r[:, 1]).all() else np.zeros(0, np.int64)
        total = int(lens.sum())
        out = np.zeros(total, dtype=np.uint8)
        with DeviceBuffer(max(total, 16), self.device) as buf:
            rep = gh_bgather_report()
            rc = lib().gh_batchdec_gather(self._h, _ptr(r) if r.size else None, r.shape[0], buf.ptr, total, None,
                                          ctypes.byref(rep))
            if rc != GH_OK:
                e = GapHuffError(rc, lib().gh_last_error().decode(errors="replace"))
                e.report = rep
                raise e
            if total:
                buf.download(out)
        ends = np.cumsum(lens)
        return [out[int(e - l): int(e)] for e, l in zip(ends, lens)]

    def gather_device(self, ranges_ptr: int, nranges: int, dst_ptr: int, dst_len: int, hip_stream: int = 0,
                      timed: bool = True) -> None:
        """Enqueue the gather of ``nranges`` (stream, lo, hi) triples held in device memory at
        ``ranges_ptr`` (a contiguous int64 / uint64 [n, 3] array) into the ``dst_len`` device
        bytes at ``dst_ptr`` and return without waiting (gh_batchdec_gather_device).  What only
        the device finds is raised by :meth:`gather_wait`."""
        _check(lib().gh_batchdec_gather_device(self._h, ctypes.c_void_p(ranges_ptr or None), nranges,
                                               ctypes.c_void_p(dst_ptr or None), dst_len,
                                               ctypes.c_void_p(hip_stream or None), int(timed)))

    def gather_wait(self) -> gh_bgather_report:
        """Wait for the last gather and return its report; raises :class:`GapHuffError` (with
        the report as ``.report``) on a device-side refusal or a range on a flagged stream."""
        return self._wait(lib().gh_batchdec_gather_wait, gh_bgather_report())

    def gather_pieces(self) -> np.ndarray:
        """The pieces of the last gather as a :data:`PIECE_DTYPE` record array
        (gh_batchdec_gather_pieces); ``block`` is the global unit index."""
        n = ctypes.c_uint64()
        rc = lib().gh_batchdec_gather_pieces(self._h, None, 0, ctypes.byref(n))
        if rc not in (GH_OK, -9):
            _check(rc)
        pieces = np.zeros(int(n.value), dtype=PIECE_DTYPE)
        _check(lib().gh_batchdec_gather_pieces(self._h, _ptr(pieces) if pieces.size else None, pieces.size,
                                               ctypes.byref(n)))
        return pieces

    def gather_kernel_shape(self) -> str:
        """Name of the gather kernel instantiation for the loaded batch (gh_batchdec_kernel_shape)."""
        return _name(lib().gh_batchdec_kernel_shape, self._h)

    def wait(self) -> gh_batch_report:
        """Wait for the last :meth:`decode` and return its report; raises
        :class:`GapHuffError` (with the report as ``.report``) when a stream was bad."""
        return self._wait(lib().gh_batch_wait, gh_batch_report())

    def status(self):
        """(GH_ST_* bits, codewords counted) per stream, as uint32 / uint64 arrays."""
        st = np.zeros(len(self.ns), dtype=np.uint32)
        sy = np.zeros(len(self.ns), dtype=np.uint64)
        _check(lib().gh_batch_status(self._h, _ptr(st) if st.size else None, _ptr(sy) if sy.size else None, st.size))
        return st, sy

    def offsets(self) -> np.ndarray:
        off = np.zeros(len(self.ns) + 1, dtype=np.uint64)
        _check(lib().gh_batch_offsets(self._h, _ptr(off), off.size))
        return off

    def output(self):
        """(device address, capacity) of the batch's own output arena."""
        p = ctypes.c_void_p()
        cap = ctypes.c_uint64()
        _check(lib().gh_batch_output(self._h, ctypes.byref(p), ctypes.byref(cap)))
        return int(p.value or 0), int(cap.value)

    def download(self, i: int) -> np.ndarray:
        """Stream ``i``'s bytes from the batch's own arena."""
        out = np.empty(self.ns[i], dtype=np.uint8)
        _check(lib().gh_batch_download(self._h, i, _ptr(out) if out.size else None, out.size))
        return out

    def download_all(self) -> list:
        return [self.download(i) for i in range(len(self.ns))]

    def kernel_shape(self) -> str:
        """Name of the kernel instantiations the last load picked (gh_batch_kernel_shape)."""
        return _name(lib().gh_batch_kernel_shape, self._h)

    def join_planes_device(self, items, stored_ptr: int = 0, stored_len: int = 0, hip_stream: int = 0,
                           timed: bool = True) -> None:
        """Enqueue the byte-plane join after a :meth:`decode` into the batch's own arena
        (gh_planes_join_device): ``items`` are ``(device address, nelem, elem_size, coded_mask)``
        destinations whose coded planes are the loaded streams in order; the stored planes are
        read from the 16-byte-aligned device arena at ``stored_ptr``.  Returns without waiting."""
        arr, n = _planes_items(items)
        _check(lib().gh_planes_join_device(self._h, arr, n, ctypes.c_void_p(stored_ptr or None), stored_len,
                                           ctypes.c_void_p(hip_stream or None), int(timed)))

    def planes_wait(self) -> gh_planes_report:
        """Wait for the decode and the join and return the join's report; raises
        :class:`GapHuffError` (with the report as ``.report``) when a tensor was skipped."""
        return self._wait(lib().gh_planes_wait, gh_planes_report())

    def gather_elements_device(self, items, stored_ptr: int, stored_len: int, ranges_ptr: int, nranges: int,
                               dst_ptr: int, dst_len: int, hip_stream: int = 0, timed: bool = True) -> None:
        """Enqueue the gather of ``nranges`` (tensor, lo, hi) ELEMENT ranges held in device memory
        at ``ranges_ptr`` (a contiguous int64 / uint64 [n, 3] array) into the ``dst_len`` device
        bytes at ``dst_ptr`` and return without waiting (gh_pgather_device).  ``items`` are
        :meth:`join_planes_device`'s (the address is ignored), ``stored_ptr`` the stored arena.
        Needs an :meth:`index` or a :meth:`decode` since the load, no output arena.  What only
        the device finds is raised by :meth:`elements_wait`."""
        arr, n = _planes_items(items)
        _check(lib().gh_pgather_device(self._h, arr, n, ctypes.c_void_p(stored_ptr or None), stored_len,
                                       ctypes.c_void_p(ranges_ptr or None), nranges, ctypes.c_void_p(dst_ptr or None),
                                       dst_len, ctypes.c_void_p(hip_stream or None), int(timed)))

    def elements_wait(self) -> gh_pgather_report:
        """Wait for the last element gather and return its report; raises :class:`GapHuffError`
        (with the report as ``.report``) on a device-side refusal or a range on a flagged tensor."""
        return self._wait(lib().gh_pgather_wait, gh_pgather_report())

    def gather_elements(self, items, stored, ranges) -> list:
        """The elements of each ``(tensor, lo, hi)`` range, one numpy array per range in request
        order, viewed as unsigned integers of the tensor's element size (gh_pgather).  ``items``:
        ``(address, nelem, elem_size, coded_mask)`` of the loaded tensor list; ``stored``: its
        stored arena in host memory (np.uint8, as :func:`planes_layout` lays it out).  Runs
        :meth:`index` first when the batch is neither indexed nor decoded."""
        items = list(items)
        r = _branges(ranges)
        if not self._indexed:
            self.index()
        ok = bool(r.size) and (r[:, 0] < len(items)).all() and (r[:, 2] >= r[:, 1]).all()
        es = np.asarray([items[int(t)][2] for t in r[:, 0]], dtype=np.int64) if ok else np.zeros(0, np.int64)
        lens = (r[:, 2] - r[:, 1]).astype(np.int64) * es if ok else np.zeros(0, np.int64)
        total = int(lens.sum())
        out = np.zeros(total, dtype=np.uint8)
        stored = _u8(stored)
        with DeviceBuffer(max(total, 16), self.device) as buf, DeviceBuffer(max(stored.size, 16), self.device) as st:
            if stored.size:
                st.upload(stored)
            arr, n = _planes_items(items)
            rep = gh_pgather_report()
            rc = lib().gh_pgather(self._h, arr, n, st.ptr, stored.size, _ptr(r) if r.size else None, r.shape[0],
                                  buf.ptr, total, None, ctypes.byref(rep))
            if rc != GH_OK:
                e = GapHuffError(rc, lib().gh_last_error().decode(errors="replace"))
                e.report = rep
                raise e
            if total:
                buf.download(out)
        ends = np.cumsum(lens)
        return [out[int(e - l): int(e)].view(_UINT_OF[int(k)]) for e, l, k in zip(ends, lens, es)]


_UINT_OF = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def decode_batch(images, device: int = 0) -> list:
    """Decode many compressed.huff images as one batch; returns their bytes in order."""
    with BatchDecoder(device) as b:
        b.load(images)
        b.decode()
        b.wait()
        return b.download_all()


def decode_batch_raw(raws, device: int = 0) -> list:
    """Decode many gap-less streams (container images or ``(symbols, n, units)`` triples) as one
    batch; returns their bytes in order."""
    with BatchDecoder(device) as b:
        b.load_raw(raws)
        b.decode()
        b.wait()
        return b.download_all()


def decode_batch_ranges(images, ranges, device: int = 0) -> list:
    """The bytes of each ``(stream, lo, hi)`` range of many compressed.huff images loaded as
    one batch: indexed, never decoded in full (BatchDecoder.gather)."""
    with BatchDecoder(device) as b:
        b.load(images)
        return b.gather(ranges)


# --------------------------------------------------------------------------- batched encode
def ebatch_kernel_shapes() -> list:
    """Every kernel name a batched encode can pick (gh_ebatch_kernel_shapes); needs no device."""
    return _name(lib().gh_ebatch_kernel_shapes, cap=1 << 10).split()


class BatchEncoder(_Handle):
    """One gh_ebatch: many independent inputs resident on one GPU, each encoded with its own
    code by one fixed set of launches per batch.  load / load_device, plan, encode, wait, then
    sizes / download / items."""

    def __init__(self, device: int = 0):
        super().__init__(lib().gh_ebatch_create, lib().gh_ebatch_destroy, device)
        self.ns: list = []  # input bytes of every loaded stream

    def load(self, datas) -> None:
        """Load a batch of inputs (bytes / np.uint8) from host memory (gh_ebatch_load)."""
        arrs = [_u8(d) for d in datas]
        ptrs = (ctypes.c_void_p * max(1, len(arrs)))(*[a.ctypes.data if a.size else None for a in arrs])
        n = np.asarray([a.size for a in arrs], dtype=np.uint64)
        _check(lib().gh_ebatch_load(self._h, ptrs, _ptr(n) if n.size else None, len(arrs)))
        self.ns = [a.size for a in arrs]

    def load_device(self, items, hip_stream: int = 0) -> None:
        """Load a batch whose inputs are device memory (gh_ebatch_load_device): ``items`` are
        ``(device address, nbytes)``, any byte alignment."""
        items = list(items)
        arr = (gh_ebatch_item * max(1, len(items)))()
        for i, (ptr, n) in enumerate(items):
            arr[i].d_in, arr[i].n = ptr or None, n
        _check(lib().gh_ebatch_load_device(self._h, arr, len(items), ctypes.c_void_p(hip_stream or None)))
        self.ns = [int(n) for _, n in items]

    def load_planes(self, arrays, coded_masks=None) -> np.ndarray:
        """Load typed tensors from host memory (gh_planes_load): ``arrays`` are numpy arrays of
        1-, 2-, 4- or 8-byte elements, ``coded_masks`` one mask per tensor (default: the top
        plane).  The coded planes are the batch's streams; returns the stored arena (np.uint8,
        laid out by :func:`planes_layout`)."""
        arrs, items = _planes_host_items(arrays, coded_masks)
        arr, n = _planes_items(items)
        _, nstreams, stored_bytes = planes_layout(items)
        stored = np.zeros(stored_bytes, dtype=np.uint8)
        _check(lib().gh_planes_load(self._h, arr, n, _ptr(stored) if stored.size else None, stored.size))
        self.ns = [int(it[1]) for it in items for p in range(it[2]) if (it[3] >> p) & 1]
        return stored

    def load_planes_device(self, items, stored_ptr: int = 0, stored_len: int = 0, hip_stream: int = 0) -> None:
        """Load typed tensors from device memory (gh_planes_load_device): ``items`` are
        ``(device address, nelem, elem_size, coded_mask)``, any byte alignment; one split kernel
        writes the coded planes into the batch and the stored planes into the 16-byte-aligned
        device arena at ``stored_ptr`` (``stored_len`` >= :func:`planes_layout`'s size)."""
        items = list(items)
        arr, n = _planes_items(items)
        _check(lib().gh_planes_load_device(self._h, arr, n, ctypes.c_void_p(stored_ptr or None), stored_len,
                                           ctypes.c_void_p(hip_stream or None)))
        self.ns = [int(it[1]) for it in items for p in range(it[2]) if (it[3] >> p) & 1]

    def planes_load_ms(self) -> float:
        """HIP-event time of the last :meth:`load_planes_device`'s split kernel (gh_planes_load_times)."""
        ms = ctypes.c_float(0)
        _check(lib().gh_planes_load_times(self._h, ctypes.byref(ms)))
        return ms.value

    def choose_masks_device(self, items, hip_stream: int = 0):
        """Every tensor's coded planes from its own bytes, on the GPU (gh_pmask_device): ``items``
        are ``(device address, nelem, elem_size[, coded_mask])``, any byte alignment (a mask is
        ignored).  Returns ``(masks, plane_bytes)`` as :func:`choose_planes_masks` does.
        Synchronous; the batch's load, plan and encode state stay as they are."""
        arr, n = _planes_items([(it[0], it[1], it[2], 0) for it in items])
        masks, pb = np.zeros(n, dtype=np.uint32), np.zeros((n, 8), dtype=np.uint64)
        self._pmask_rep = gh_pmask_report()
        _check(lib().gh_pmask_device(self._h, arr, n, _ptr(masks) if n else None, _ptr(pb) if n else None,
                                     ctypes.c_void_p(hip_stream or None), ctypes.byref(self._pmask_rep)))
        return masks, pb

    def pmask_report(self) -> gh_pmask_report:
        """The report of the last :meth:`choose_masks_device`."""
        rep = getattr(self, "_pmask_rep", None)
        if rep is None:
            raise GapHuffError(-8, "pmask_report before a choose_masks_device")
        return rep

    def pmask_counts(self, q: int) -> np.ndarray:
        """The 256 byte counts of candidate plane ``q`` (tensor order, then plane order, over all
        planes of every tensor) as the last :meth:`choose_masks_device` left them (gh_pmask_counts)."""
        out = np.zeros(256, dtype=np.uint64)
        _check(lib().gh_pmask_counts(self._h, q, _ptr(out)))
        return out

    def plan(self, force_version: int = 0, threads: int = 0) -> None:
        """Every stream's histogram (one launch) and host plan (gh_ebatch_plan); synchronous."""
        _check(lib().gh_ebatch_plan(self._h, force_version, threads))

    def plan_device(self, force_version: int = 0) -> None:
        """:meth:`plan` with every stream's code built on the GPU (gh_batchenc_plan_device): no
        host package-merge; the same plans and images.  Synchronous."""
        _check(lib().gh_batchenc_plan_device(self._h, force_version))

    def plan_times(self) -> dict:
        """Times of the last plan of either kind in ms (gh_batchenc_plan_times): ``hist_ms`` and
        ``code_ms`` by HIP events (``code_ms`` is 0 after :meth:`plan`), ``host_ms`` by wall clock."""
        t = [ctypes.c_float(0) for _ in range(3)]
        _check(lib().gh_batchenc_plan_times(self._h, *[ctypes.byref(x) for x in t]))
        return {"hist_ms": t[0].value, "code_ms": t[1].value, "host_ms": t[2].value}

    def encode(self, hip_stream: int = 0, timed: bool = True) -> None:
        """Enqueue one encode of the planned batch and return."""
        _check(lib().gh_ebatch_encode(self._h, ctypes.c_void_p(hip_stream or None), int(timed)))

    def wait(self) -> gh_ebatch_report:
        """Wait for the last :meth:`encode` and return its report; raises
        :class:`GapHuffError` (with the report as ``.report``) on a layout tripwire."""
        return self._wait(lib().gh_ebatch_wait, gh_ebatch_report())

    def sizes(self) -> np.ndarray:
        """file_bytes of every stream's image."""
        out = np.zeros(len(self.ns), dtype=np.uint64)
        _check(lib().gh_ebatch_sizes(self._h, _ptr(out) if out.size else None, out.size))
        return out

    def plan_of(self, i: int) -> gh_encode_plan:
        plan = gh_encode_plan()
        _check(lib().gh_ebatch_plan_of(self._h, i, ctypes.byref(plan)))
        return plan

    def download(self, i: int) -> np.ndarray:
        """Stream ``i``'s whole compressed.huff image."""
        out = np.empty(int(self.plan_of(i).file_bytes), dtype=np.uint8)
        _check(lib().gh_ebatch_download(self._h, i, _ptr(out), out.size))
        return out

    def download_all(self) -> list:
        return [self.download(i) for i in range(len(self.ns))]

    def items(self) -> list:
        """What :meth:`BatchDecoder.load_device` takes: ``(stream, payload_ptr, gap_ptr)`` per
        stream, pointing into this batch's device arenas (valid until its next load or plan)."""
        arr = (gh_batch_item * max(1, len(self.ns)))()
        _check(lib().gh_ebatch_items(self._h, arr, len(self.ns)))
        return [(Stream.from_plan(self.plan_of(i)), int(arr[i].d_payload or 0), int(arr[i].d_gap_words or 0))
                for i in range(len(self.ns))]

    def kernel_shape(self) -> str:
        """Name of the per-unit kernels' shape the last plan picked (gh_ebatch_kernel_shape)."""
        return _name(lib().gh_ebatch_kernel_shape, self._h)


def encode_batch(datas, device: int = 0, device_plan: bool = False) -> list:
    """Encode many inputs as one batch, each with its own code; returns their images in order.
    ``device_plan``: build the codes on the GPU (:meth:`BatchEncoder.plan_device`)."""
    with BatchEncoder(device) as b:
        b.load(datas)
        if device_plan:
            b.plan_device()
        else:
            b.plan()
        b.encode()
        b.wait()
        return b.download_all()


# --------------------------------------------------------------------------- byte planes
def _planes_items(items):
    """``(address, nelem, elem_size, coded_mask)`` tuples as the C array of gh_planes_item."""
    items = list(items)
    arr = (gh_planes_item * max(1, len(items)))()
    for i, (ptr, nelem, e, mask) in enumerate(items):
        arr[i].data, arr[i].nelem, arr[i].elem_size, arr[i].coded_mask = ptr or None, nelem, e, mask
    return arr, len(items)


def default_planes_mask(elem_size: int) -> int:
    """The top plane alone (sign and exponent of a float); the one plane of 1-byte elements."""
    return 1 << (elem_size - 1)


def _planes_host_items(arrays, coded_masks=None):
    """Contiguous copies of ``arrays`` (kept alive by the caller) and their item tuples."""
    arrs = [np.ascontiguousarray(a) for a in arrays]
    masks = [None] * len(arrs) if coded_masks is None else list(coded_masks)
    if len(masks) != len(arrs):
        raise GapHuffError(-1, "one coded mask per tensor")
    items = []
    for a, m in zip(arrs, masks):
        e = a.dtype.itemsize
        items.append((a.ctypes.data if a.size else 0, a.size, e, default_planes_mask(e) if m is None else int(m)))
    return arrs, items


def planes_layout(items):
    """The layout of a tensor list (gh_planes_layout; needs no device): ``items`` are
    ``(address, nelem, elem_size, coded_mask)``; returns ``(slots, nstreams, stored_bytes)``
    with ``slots[t][p] = (stream, stored_off)`` for all 8 plane slots of every tensor
    (``stream == GH_PLANES_STORED`` for a stored or absent plane)."""
    arr, n = _planes_items(items)
    slots = (gh_planes_slot * max(1, 8 * n))()
    ns, sb = ctypes.c_uint32(), ctypes.c_uint64()
    _check(lib().gh_planes_layout(arr, n, slots, ctypes.byref(ns), ctypes.byref(sb)))
    out = [[(int(slots[8 * t + p].stream), int(slots[8 * t + p].stored_off)) for p in range(8)] for t in range(n)]
    return out, int(ns.value), int(sb.value)


def choose_planes_masks(arrays):
    """Every tensor's coded planes from its own bytes, on the CPU (gh_pmask_host; needs no
    device): plane ``p`` is coded iff its compressed.huff image is smaller than its ``nelem`` raw
    bytes.  Returns ``(masks, plane_bytes)``: ``masks[t]`` (np.uint32) is what ``coded_masks``
    takes, ``plane_bytes[t][p]`` (np.uint64 ``[n, 8]``) the image size of every plane, chosen or
    not (0 for ``p >= elem_size`` and for an empty tensor)."""
    arrs, items = _planes_host_items(arrays, [0] * len(arrays))
    arr, n = _planes_items(items)
    masks, pb = np.zeros(n, dtype=np.uint32), np.zeros((n, 8), dtype=np.uint64)
    _check(lib().gh_pmask_host(arr, n, _ptr(masks) if n else None, _ptr(pb) if n else None))
    return masks, pb


def planes_masks_from_counts(counts, shapes):
    """:func:`choose_planes_masks` from byte counts (gh_pmask_from_counts; needs no device):
    ``counts`` is a uint64 ``[nplanes, 256]`` array in candidate order (tensor order, then plane
    order, over all planes of every tensor), ``shapes`` one ``(nelem, elem_size)`` per tensor."""
    shapes = list(shapes)
    c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1, 256)
    # (a bad elem_size is the library's to refuse; the rows it would read must exist)
    if all(e in (1, 2, 4, 8) for _, e in shapes) and c.shape[0] != sum(e for _, e in shapes):
        raise GapHuffError(-1, "one row of 256 counts per plane of every tensor")
    arr, n = _planes_items([(0, nelem, e, 0) for nelem, e in shapes])
    masks, pb = np.zeros(n, dtype=np.uint32), np.zeros((n, 8), dtype=np.uint64)
    _check(lib().gh_pmask_from_counts(_ptr(c) if c.size else None, arr, n, _ptr(masks) if n else None,
                                      _ptr(pb) if n else None))
    return masks, pb


def planes_gather_plan(items, ranges, status=None):
    """The element gather's plan from host arrays (gh_pgather_plan; needs no device): ``items``
    are ``(address, nelem, elem_size, coded_mask)``, ``ranges`` (tensor, lo, hi) element triples,
    ``status`` the batch's per-stream status words or None.  Returns ``(branges, stage_off,
    dst_off, out_bytes, bad_ranges)``: the (stream, lo, hi) byte ranges of the inner batched
    gather as a uint64 ``[m, 3]`` array and every range's byte offset in the staging buffer and in
    the destination."""
    arr, n = _planes_items(items)
    r = _branges(ranges)
    st = None if status is None else np.ascontiguousarray(status, dtype=np.uint32)
    nr = r.shape[0]
    so, do = np.zeros(nr, dtype=np.uint64), np.zeros(nr, dtype=np.uint64)
    nb, ob, bad = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()

    def call(br):
        return lib().gh_pgather_plan(arr, n, _ptr(st) if st is not None and st.size else None,
                                     _ptr(r) if nr else None, nr, _ptr(br) if br.size else None, br.shape[0],
                                     ctypes.byref(nb), _ptr(so) if nr else None, _ptr(do) if nr else None,
                                     ctypes.byref(ob), ctypes.byref(bad))
    rc = call(np.zeros((0, 3), dtype=np.uint64))
    if rc not in (GH_OK, -9):
        _check(rc)
    br = np.zeros((int(nb.value), 3), dtype=np.uint64)
    _check(call(br))
    return br, so, do, int(ob.value), int(bad.value)


def planes_split_host(a, elem_size: Optional[int] = None) -> list:
    """The byte planes of ``a`` by the CPU twin of the split kernel (gh_planes_split_host): a
    list of ``elem_size`` np.uint8 arrays.  ``a``: a numpy array of 1/2/4/8-byte elements, or
    bytes with ``elem_size`` given."""
    raw = _u8(a) if elem_size is not None else np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    e = elem_size if elem_size is not None else np.asarray(a).dtype.itemsize
    if e < 1 or raw.size % e:
        raise GapHuffError(-1, "the tensor's bytes are no multiple of elem_size")
    nelem = raw.size // e
    planes = [np.empty(nelem, dtype=np.uint8) for _ in range(e)]
    it = gh_planes_item(raw.ctypes.data if raw.size else None, nelem, e, 0)
    ptrs = (ctypes.c_void_p * 8)(*[p.ctypes.data if p.size else None for p in planes])
    _check(lib().gh_planes_split_host(ctypes.byref(it), ptrs))
    return planes


def planes_join_host(planes) -> np.ndarray:
    """The tensor's bytes (np.uint8, ``nelem * len(planes)``) from its byte planes, by the CPU
    twin of the join kernel (gh_planes_join_host)."""
    pl = [_u8(p) for p in planes]
    e, nelem = len(pl), (pl[0].size if pl else 0)
    if any(p.size != nelem for p in pl):
        raise GapHuffError(-1, "planes of different sizes")
    out = np.empty(nelem * e, dtype=np.uint8)
    it = gh_planes_item(out.ctypes.data if out.size else None, nelem, e, 0)
    ptrs = (ctypes.c_void_p * 8)(*[p.ctypes.data if p.size else None for p in pl])
    _check(lib().gh_planes_join_host(ctypes.byref(it), ptrs))
    return out


def planes_image(nelem: int, elem_size: int, coded_mask: int, planes) -> np.ndarray:
    """The container of one tensor (gh_planes_image_write): ``planes[p]`` is a compressed.huff
    image for a coded plane and the ``nelem`` raw bytes of a stored one."""
    pl = [_u8(p) for p in planes]
    if len(pl) != elem_size:
        raise GapHuffError(-1, "one plane per byte of the element")
    nb = np.asarray([p.size for p in pl], dtype=np.uint64)
    total = ctypes.c_uint64()
    _check(lib().gh_planes_image_bytes(elem_size, _ptr(nb), ctypes.byref(total)))
    out = np.zeros(int(total.value), dtype=np.uint8)
    it = gh_planes_item(None, nelem, elem_size, coded_mask)
    ptrs = (ctypes.c_void_p * 8)(*[p.ctypes.data if p.size else None for p in pl])
    _check(lib().gh_planes_image_write(ctypes.byref(it), ptrs, _ptr(nb), _ptr(out), out.size))
    return out


@dataclass
class PlanesImage:
    """A parsed byte-plane container (keeps the file bytes alive).  ``planes[p]``: a
    :class:`Stream` for a coded plane, the raw bytes (np.uint8 view) for a stored one."""

    raw: np.ndarray
    nelem: int
    elem_size: int
    coded_mask: int
    planes: list


def parse_planes(image) -> PlanesImage:
    """Parse a byte-plane container (gh_planes_parse); GH_E_FORMAT when it is not one."""
    raw = _u8(image)
    im = gh_planes_image()
    _check(lib().gh_planes_parse(_ptr(raw), raw.size, ctypes.byref(im)))
    planes = []
    for p in range(im.elem_size):
        off, nb = int(im.plane[p] or raw.ctypes.data) - raw.ctypes.data, int(im.plane_bytes[p])
        view = raw[off: off + nb]
        planes.append(parse(view) if (im.coded_mask >> p) & 1 else view)
    return PlanesImage(raw, int(im.nelem), int(im.elem_size), int(im.coded_mask), planes)


def encode_tensors(arrays, coded_masks=None, device: int = 0, device_plan: bool = False) -> list:
    """Encode typed tensors (numpy arrays of 1/2/4/8-byte elements) as one batch on the GPU and
    return their containers.  ``coded_masks``: one mask per tensor; default the top plane alone
    (the one plane for 1-byte elements); ``"auto"``: every tensor's own best mask, chosen on the
    GPU from the uploaded tensors (:meth:`BatchEncoder.choose_masks_device`).  ``device_plan``:
    build the codes on the GPU."""
    auto = isinstance(coded_masks, str)
    if auto and coded_masks != "auto":
        raise GapHuffError(-1, "coded_masks: a list of masks, None or \"auto\"")
    arrs, items = _planes_host_items(arrays, None if auto else coded_masks)
    with BatchEncoder(device) as b:
        bufs = [DeviceBuffer(max(a.nbytes, 16), device).upload(a.reshape(-1).view(np.uint8)) if a.size
                else DeviceBuffer(16, device) for a in arrs]
        try:
            if auto:
                masks, _ = b.choose_masks_device([(buf.addr, it[1], it[2]) for buf, it in zip(bufs, items)])
                items = [(it[0], it[1], it[2], int(m)) for it, m in zip(items, masks)]
            slots, _, stored_bytes = planes_layout(items)
        except BaseException:
            for buf in bufs:
                buf.close()
            raise
        with DeviceBuffer(max(stored_bytes, 16), device) as st:
            try:
                b.load_planes_device([(buf.addr, it[1], it[2], it[3]) for buf, it in zip(bufs, items)], st.addr,
                                     stored_bytes)
            finally:
                for buf in bufs:
                    buf.close()
            stored = st.download(np.empty(stored_bytes, dtype=np.uint8)) if stored_bytes else np.zeros(0, np.uint8)
        if device_plan:
            b.plan_device()
        else:
            b.plan()
        b.encode()
        b.wait()
        images = b.download_all()
    out = []
    for (_, nelem, e, mask), sl in zip(items, slots):
        planes = [images[s] if s != GH_PLANES_STORED else stored[off: off + nelem] for s, off in sl[:e]]
        out.append(planes_image(nelem, e, mask, planes))
    return out


def decode_tensors(images, device: int = 0) -> list:
    """Decode byte-plane containers as one batch on the GPU; returns every tensor's bytes
    (np.uint8, ``nelem * elem_size``)."""
    with BatchDecoder(device) as b:
        parsed = [im if isinstance(im, PlanesImage) else parse_planes(im) for im in images]
        shapes = [(0, im.nelem, im.elem_size, im.coded_mask) for im in parsed]
        slots, _, stored_bytes = planes_layout(shapes)
        stored = np.zeros(stored_bytes, dtype=np.uint8)
        streams = []
        for im, sl in zip(parsed, slots):
            for p in range(im.elem_size):
                if sl[p][0] != GH_PLANES_STORED:
                    streams.append(im.planes[p])
                else:
                    stored[sl[p][1]: sl[p][1] + im.nelem] = im.planes[p]
        b.load(streams)
        b.decode()
        sizes = [im.nelem * im.elem_size for im in parsed]
        offs = np.concatenate([[0], np.cumsum([-(-n // 16) * 16 for n in sizes])]).astype(np.int64)
        with DeviceBuffer(max(int(offs[-1]), 16), device) as dst, DeviceBuffer(max(stored_bytes, 16), device) as st:
            if stored_bytes:
                st.upload(stored)
            b.join_planes_device([(dst.addr + int(o), s[1], s[2], s[3]) for o, s in zip(offs, shapes)], st.addr, stored_bytes)
            b.planes_wait()
            whole = dst.download(np.empty(int(offs[-1]), dtype=np.uint8)) if offs[-1] else np.zeros(0, np.uint8)
        return [whole[int(o): int(o) + n].copy() for o, n in zip(offs, sizes)]


def _planes_streams(parsed):
    """(shapes, streams, stored arena) of parsed containers, by :func:`planes_layout`."""
    shapes = [(0, im.nelem, im.elem_size, im.coded_mask) for im in parsed]
    slots, _, stored_bytes = planes_layout(shapes)
    stored = np.zeros(stored_bytes, dtype=np.uint8)
    streams = []
    for im, sl in zip(parsed, slots):
        for p in range(im.elem_size):
            if sl[p][0] != GH_PLANES_STORED:
                streams.append(im.planes[p])
            else:
                stored[sl[p][1]: sl[p][1] + im.nelem] = im.planes[p]
    return shapes, streams, stored


def decode_tensor_ranges(images, ranges, device: int = 0) -> list:
    """The elements of each ``(tensor, lo, hi)`` range of byte-plane containers, one numpy array
    per range (unsigned integers of the tensor's element size), without decoding the tensors:
    loads the coded planes, uploads the stored planes, runs the index pass and one element gather
    (:meth:`BatchDecoder.gather_elements`)."""
    with BatchDecoder(device) as b:
        parsed = [im if isinstance(im, PlanesImage) else parse_planes(im) for im in images]
        shapes, streams, stored = _planes_streams(parsed)
        b.load(streams)
        b.index()
        return [a.copy() for a in b.gather_elements(shapes, stored, ranges)]


# --------------------------------------------------------------------------- random access
@dataclass
class Index:
    """A parsed seek index (keeps the image bytes alive)."""

    raw: np.ndarray
    c: gh_index

    @property
    def log2_stride(self) -> int:
        return int(self.c.log2_stride)

    @property
    def n(self) -> int:
        return int(self.c.n)

    @property
    def g(self) -> int:
        return int(self.c.g)

    @property
    def offsets(self) -> np.ndarray:
        """The nentries output offsets (a view of the image)."""
        return self.raw[40: 40 + 8 * int(self.c.nentries)].view("<u8")

    def locate(self, lo: int, hi: int):
        """(seg_begin, seg_end, skip) for output bytes [lo, hi) (gh_index_locate)."""
        b, e, skip = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().gh_index_locate(ctypes.byref(self.c), lo, hi, ctypes.byref(b), ctypes.byref(e),
                                     ctypes.byref(skip)))
        return int(b.value), int(e.value), int(skip.value)

    def plan(self, ranges):
        """The gather plan of the (lo, hi) ``ranges`` (gh_gather_plan): (pieces as a
        structured array with fields dst, block, a, b, pad; the ranges' byte total)."""
        r = _ranges(ranges)
        np_, total = ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib().gh_gather_plan(ctypes.byref(self.c), _ptr(r), r.shape[0], None, 0, ctypes.byref(np_),
                                  ctypes.byref(total))
        if rc not in (GH_OK, -9):
            _check(rc)
        pieces = np.zeros(int(np_.value), dtype=PIECE_DTYPE)
        _check(lib().gh_gather_plan(ctypes.byref(self.c), _ptr(r), r.shape[0], _ptr(pieces), pieces.size,
                                    ctypes.byref(np_), ctypes.byref(total)))
        return pieces, int(total.value)


# gh_gather_piece as a numpy record
PIECE_DTYPE = np.dtype([("dst", "<u8"), ("block", "<u4"), ("a", "<u4"), ("b", "<u4"), ("pad", "<u4")])


def _ranges(ranges) -> np.ndarray:
    """(lo, hi) pairs as the C array of gh_range: a contiguous (n, 2) uint64 array."""
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
    if r.shape[0] >= 1 << 32:
        raise GapHuffError(-1, "2^32 or more ranges in one batch")
    return r


def gather_piece_bound(nranges: int, dst_len: int, log2_stride: int) -> int:
    """Pieces a device-planned batch can need (gh_gather_piece_bound); 0 on a bad stride."""
    return int(lib().gh_gather_piece_bound(nranges, dst_len, log2_stride))


def parse_index(image) -> Index:
    raw = _u8(image)
    ix = gh_index()
    _check(lib().gh_index_parse(_ptr(raw), raw.size, ctypes.byref(ix)))
    return Index(raw, ix)


def decode_range(src, index, lo: int, hi: int, device: int = 0) -> np.ndarray:
    """Bytes [lo, hi) of the original data: loads and decodes only the segments the
    index names for them.  ``src``: a :class:`Stream`, the file's bytes, or a path (then
    only the header, the gap array and those segments' payload are read,
    gh_ctx_load_file).  ``index``: an :class:`Index` or a sidecar image."""
    ix = index if isinstance(index, Index) else parse_index(index)
    b, e, skip = ix.locate(lo, hi)
    cap = skip + (hi - lo)
    with Decoder(device) as d:
        if isinstance(src, (str, os.PathLike)):
            # (segments past the file's G are refused by the load itself, with GH_E_ARG too)
            info = d.load_file(os.fspath(src), b, e, cap)
            n, g = int(info.n), int(info.g)
        else:
            s = src if isinstance(src, Stream) else parse(src)
            n, g = s.n, s.g
            if (n, g) == (ix.n, ix.g):
                d.load(s, b, e, cap)
        if (n, g) != (ix.n, ix.g):
            raise GapHuffError(-1, f"the index is for N = {ix.n}, G = {ix.g}; the stream has N = {n}, G = {g}")
        if hi == lo:
            return np.zeros(0, dtype=np.uint8)
        d.decode(timed=False)
        rep = d.report()
        if rep.status:
            raise GapHuffError(-7, f"device status {rep.status}")
        if rep.symbols < cap:  # never hand back undecoded (uninitialised) output bytes
            raise GapHuffError(-7, f"segments [{b}, {e}) decoded to {rep.symbols} of {cap} symbols")
        return d.download(hi - lo, offset=skip)


def decode_ranges(src, index, ranges, device: int = 0) -> list:
    """The bytes of each (lo, hi) range of the original data, as a list of arrays: the
    whole stream is loaded once and every range decoded in one launch (Decoder.gather).
    ``src`` and ``index`` as for :func:`decode_range`."""
    ix = index if isinstance(index, Index) else parse_index(index)
    r = _ranges(ranges)
    with Decoder(device) as d:
        if isinstance(src, (str, os.PathLike)):
            d.load_file(os.fspath(src))
        else:
            d.load(src if isinstance(src, Stream) else parse(src))
        out, _ = d.gather(ix, r)
    ends = np.cumsum(r[:, 1] - r[:, 0]).astype(np.int64) if r.size else np.zeros(0, dtype=np.int64)
    return [out[int(e - (h - l)): int(e)] for e, (l, h) in zip(ends, r)]


def _syms(symbols: Sequence[tuple]):
    arr = (gh_sym * max(1, len(symbols)))()
    for i, (sy, ln) in enumerate(symbols):
        arr[i].symbol, arr[i].length = sy, ln
    return arr


class DeviceBuffer:
    """Device memory through the library's own HIP runtime (gh_dev_*)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.ptr = ctypes.c_void_p()
        self.nbytes = nbytes
        _check(lib().gh_dev_alloc(device, nbytes, ctypes.byref(self.ptr)))

    @property
    def addr(self) -> int:
        return int(self.ptr.value or 0)

    def upload(self, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        _check(lib().gh_dev_copy(self.ptr, _ptr(a), a.nbytes))
        return self

    def download(self, a: np.ndarray) -> np.ndarray:
        assert a.flags.c_contiguous and a.nbytes <= self.nbytes
        _check(lib().gh_dev_copy(_ptr(a), self.ptr, a.nbytes))
        return a

    def close(self) -> None:
        if self.ptr:
            lib().gh_dev_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sync_gaps(symbols: Sequence[tuple], d_words: int, w: int, d_gap_words: int, device: int = 0,
              hip_stream: int = 0) -> gh_sync_report:
    """Gap words of a device-resident raw stream (device addresses as ints, e.g. a
    torch tensor's data_ptr()); see gh_sync_gaps in include/gaphuff.h."""
    sy = _syms(symbols)
    r = gh_sync_report()
    _check(lib().gh_sync_gaps(device, ctypes.byref(sy), len(symbols), ctypes.c_void_p(d_words), w,
                              ctypes.c_void_p(d_gap_words), ctypes.c_void_p(hip_stream or None),
                              ctypes.byref(r)))
    return r


def bw_copy(dst_ptr: int, src_ptr: int, nbytes: int, hip_stream: int = 0, reps: int = 10) -> float:
    """Streaming-copy yardstick: ms per pass of a 16-B-lane copy of `nbytes` device
    bytes (gh_bw_copy, include/gaphuff.h)."""
    ms = ctypes.c_float()
    _check(lib().gh_bw_copy(ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src_ptr), nbytes,
                            ctypes.c_void_p(hip_stream or None), reps, ctypes.byref(ms)))
    return float(ms.value)


def parse_raw(file_bytes):
    """Parse a raw-stream container (bin/encoder --raw): (symbols, n, units)."""
    raw = _u8(file_bytes)
    r = gh_raw_stream()
    _check(lib().gh_raw_parse(_ptr(raw), raw.size, ctypes.byref(r)))
    syms = [(r.syms[i].symbol, r.syms[i].length) for i in range(r.nsyms)]
    off = 16 + 2 * r.nsyms + 16
    units = raw[off: off + 4 * r.w].view(np.uint32).copy()
    return syms, int(r.n), units


def decode_raw(units, symbols: Sequence[tuple], n: int, device: int = 0) -> np.ndarray:
    """Self-synchronising decode of a raw stream: the role of CUHD's
    CUHDGPUDecoder::decode (gpuhd/include/cuhd_gpu_decoder.h:24-32) for u32 units
    packed MSB-first (llhuffman_encoder.cc:200-238).  Returns the n decoded bytes."""
    with Decoder(device) as d:
        d.load_raw(symbols, n, units)
        d.decode(timed=False)
        rep = d.report()
        if rep.status:
            raise GapHuffError(-7, f"device status {rep.status}")
        if rep.symbols < n:  # never hand back undecoded (uninitialised) output bytes
            raise GapHuffError(-7, f"raw stream decoded to {rep.symbols} of {n} symbols")
        return d.download(n) if n else np.zeros(0, dtype=np.uint8)


def decoder_l1_l2(input_words, inputfilesize: int, outputfilesize: int, gap_element_num: int,
                  symbols: Sequence[tuple], gpus: int = 1) -> np.ndarray:
    """Mirror of the reference launcher (decoder.cu:732-815).

    ``input_words``: u32 array holding ceil(G/8) gap words followed by W payload words
    (the reference's pinned ``input``, huff.cpp:90-100); ``inputfilesize`` = W,
    ``outputfilesize`` = N, ``gap_element_num`` = G, ``symbols`` = [(symbol, length)]
    in file order.  Returns the N decoded bytes.
    """
    words = np.ascontiguousarray(input_words, dtype=np.uint32)
    gw = (gap_element_num + 7) // 8
    if words.size < gw + inputfilesize:
        raise GapHuffError(-1, "input shorter than gap words + payload")
    hdr = np.zeros(8 + 2 * len(symbols) + 12, dtype=np.uint8)
    hdr[:8] = np.frombuffer(np.uint64(len(symbols)).tobytes(), dtype=np.uint8)
    for i, (sy, ln) in enumerate(symbols):
        hdr[8 + 2 * i] = sy
        hdr[9 + 2 * i] = ln
    o = 8 + 2 * len(symbols)
    hdr[o:o + 12] = np.frombuffer(np.array([outputfilesize, inputfilesize, gap_element_num],
                                           dtype=np.uint32).tobytes(), dtype=np.uint8)
    image = np.concatenate([hdr, words[: gw + inputfilesize].view(np.uint8)])
    return decode(image, ngpus=gpus)
