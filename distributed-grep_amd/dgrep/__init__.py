"""dgrep — host-side mirror of distributed-grep's grep plugin over libdgrep.so.

The reference plugin (application/grep.go) exports

    func Map(filename string, contents string) []mapreduce.KeyValue   // grep.go:13-36
    func Reduce(key string, values []string) string                   // grep.go:38-40

with the pattern held in the package variable `pattern` (grep.go:11, default
""). This module keeps those names, argument meanings and error behaviour:

* ``Map(filename, contents)`` returns ``[KeyValue(Key, Value), ...]`` in line
  order, Key = ``"%s (line number #%d)" % (filename, n)`` (grep.go:25), Value =
  the line without its '\\n'. A pattern that Go's regexp.Compile rejects gives
  an empty list (grep.go:21 discards the error). Any device failure raises
  (the Go plugin would panic, and the coordinator re-assigns the task after
  its 10 s timeout, map_reduce/coordinator.go:105).
* ``Reduce(key, values)`` returns ``values[0]``.
* ``pattern`` defaults to "" (every line matches) and can be overridden with
  the DGREP_PATTERN environment variable or :func:`set_pattern`.

The matching itself runs on the GPU through the C ABI in include/dgrep.h; there
is no CPU fallback: if libdgrep.so or a GPU is missing, calls raise.
"""
from __future__ import annotations

import ctypes
import os
import threading
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DGREP_LIB") or os.path.join(os.path.dirname(_HERE), "libdgrep.so")

DGREP_OK = 0
DGREP_E_INVALID = 1
DGREP_E_UNSUPPORTED = 2
DGREP_E_TOO_LARGE = 3
DGREP_E_HIP = 4
DGREP_E_NOMEM = 5
DGREP_E_NO_DFA = 6

DFA_GO_SYNTAX_ERROR = 1
DFA_MATCH_NONE = 2
DFA_MATCH_ALL = 4
DFA_PARTIAL = 8

# Symbols declared in include/dgrep.h (tests check the library exports all).
EXPORTS = (
    "dgrep_compile", "dgrep_compile_budget", "dgrep_blob_free", "dgrep_blob_info_get", "dgrep_open", "dgrep_close",
    "dgrep_last_error", "dgrep_pick_device", "dgrep_set_stream", "dgrep_load_dfa", "dgrep_scan", "dgrep_result_free",
    "dgrep_scan_device", "dgrep_synth_corpus", "dgrep_synth_corpus_host", "dgrep_synth_keyword",
    "dgrep_last_kernel_ms", "dgrep_take_kernel_ms", "dgrep_set_stepper", "dgrep_set_lane_chunk", "dgrep_set_ingest", "dgrep_last_ingest_ms",
    "dgrep_map_partitions", "dgrep_partitions_free", "dgrep_encode_device", "dgrep_last_encode_ms",
    "dgrep_reduce", "dgrep_reduce_free", "dgrep_last_scan_stats", "dgrep_build_info",
    "dgrep_comm_unique_id", "dgrep_comm_open", "dgrep_comm_close", "dgrep_gather_records_device",
    "dgrep_gather_records", "dgrep_gathered_free", "dgrep_comm_last_error",
    "dgrep_scan_batch", "dgrep_batch_result_free", "dgrep_scan_batch_device", "dgrep_last_batch_ms",
    "dgrep_map_partitions_batch", "dgrep_batch_partitions_free", "dgrep_encode_batch_device",
    "dgrep_reduce_batch", "dgrep_reduce_batch_free", "dgrep_reduce_batch_device", "dgrep_grep_job",
    "dgrep_last_reduce_ms",
    "dgrep_scan_windowed", "dgrep_stream_open", "dgrep_stream_feed", "dgrep_stream_finish",
    "dgrep_stream_result_free", "dgrep_stream_close", "dgrep_stream_stats",
    "dgrep_scan_bounded", "dgrep_stream_carry_stats",
    "dgrep_stream_open_partitions", "dgrep_stream_feed_partitions", "dgrep_stream_finish_partitions",
    "dgrep_map_partitions_windowed", "dgrep_stream_partition_stats", "dgrep_set_long_value",
    "dgrep_job_open", "dgrep_job_add", "dgrep_job_file_begin", "dgrep_job_file_feed", "dgrep_job_file_end",
    "dgrep_job_finish", "dgrep_job_close", "dgrep_job_stats_get", "dgrep_grep_job_windowed",
    "dgrep_last_encode_stats",
)
# csrc/kernels/encode_window.h: a long escaped value is cut into chunks of this
# many bytes, one workgroup each; the default of set_long_value
LONG_CHUNK = 16384
LONG_VALUE_DEFAULT = 256
LONG_VALUE_RESIDENT_DEFAULT = 768  # kLongValueResidentDefault: the resident and the batch writer
STREAM_VALUES = 1
STREAM_BOUNDED = 2
COMM_ID_BYTES = 128

STEPPERS = {0: "table", 1: "sheng", 3: "pair", 4: "filter"}

KeyValue = namedtuple("KeyValue", ["Key", "Value"])  # map_reduce/helper_types.go:8-11


class DgrepError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("dgrep error %d: %s" % (code, msg))
        self.code = code


class UnsupportedPattern(DgrepError):
    pass


class _Result(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64), ("line_no", ctypes.POINTER(ctypes.c_uint64)),
                ("start", ctypes.POINTER(ctypes.c_uint64)), ("len", ctypes.POINTER(ctypes.c_uint64))]


class _StreamResult(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64), ("line_no", ctypes.POINTER(ctypes.c_uint64)),
                ("start", ctypes.POINTER(ctypes.c_uint64)), ("len", ctypes.POINTER(ctypes.c_uint64)),
                ("value_off", ctypes.POINTER(ctypes.c_uint64)), ("values", ctypes.c_void_p)]


class _Partitions(ctypes.Structure):
    _fields_ = [("nreduce", ctypes.c_uint32), ("total", ctypes.c_uint64), ("begin", ctypes.POINTER(ctypes.c_uint64)),
                ("end", ctypes.POINTER(ctypes.c_uint64)), ("bytes", ctypes.c_void_p)]


class _ReduceOut(ctypes.Structure):
    _fields_ = [("lines_in", ctypes.c_uint64), ("total", ctypes.c_uint64), ("bytes", ctypes.c_void_p)]


class _ScanStats(ctypes.Structure):
    _fields_ = [("stepper", ctypes.c_uint32), ("lane_chunk", ctypes.c_uint32), ("lane_slots", ctypes.c_uint32),
                ("scan_attempts", ctypes.c_uint32), ("tiles", ctypes.c_uint64), ("overflow_lanes", ctypes.c_uint64),
                ("matches", ctypes.c_uint64), ("scan_ms", ctypes.c_float), ("overflow_ms", ctypes.c_float),
                ("verify_ms", ctypes.c_float), ("candidates", ctypes.c_uint64), ("pending", ctypes.c_uint64),
                ("long_guess_misses", ctypes.c_uint32), ("long_segments", ctypes.c_uint32)]


class _Gathered(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64), ("line_no", ctypes.POINTER(ctypes.c_uint64)),
                ("start", ctypes.POINTER(ctypes.c_uint64)), ("len", ctypes.POINTER(ctypes.c_uint64)),
                ("split", ctypes.POINTER(ctypes.c_uint32))]


class _BatchResult(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64), ("line_no", ctypes.POINTER(ctypes.c_uint64)),
                ("start", ctypes.POINTER(ctypes.c_uint64)), ("len", ctypes.POINTER(ctypes.c_uint64)),
                ("split", ctypes.POINTER(ctypes.c_uint32)), ("nsplits", ctypes.c_uint64),
                ("split_begin", ctypes.POINTER(ctypes.c_uint64))]


class _BatchPartitions(ctypes.Structure):
    _fields_ = [("nsplits", ctypes.c_uint64), ("nreduce", ctypes.c_uint32), ("total", ctypes.c_uint64),
                ("cell_off", ctypes.POINTER(ctypes.c_uint64)), ("bytes", ctypes.c_void_p)]


class _ReduceBatchOut(ctypes.Structure):
    _fields_ = [("nparts", ctypes.c_uint32), ("total", ctypes.c_uint64),
                ("part_off", ctypes.POINTER(ctypes.c_uint64)), ("lines_in", ctypes.POINTER(ctypes.c_uint64)),
                ("bytes", ctypes.c_void_p)]


class _JobStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in (
        "files", "packs", "files_packed", "files_windowed", "windows", "rows", "segments", "arena_bytes",
        "arena_device_bytes", "window_device_bytes", "long_values", "arena_growths")] + [
        (f, ctypes.c_float) for f in ("scan_ms", "encode_ms", "append_ms", "reduce_ms")]


class _EncodeStats(ctypes.Structure):
    _fields_ = [("records", ctypes.c_uint64), ("long_values", ctypes.c_uint64), ("long_chunks", ctypes.c_uint64),
                ("encode_ms", ctypes.c_float)]


class _BlobInfo(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_uint32), ("nstates", ctypes.c_uint32), ("nclasses", ctypes.c_uint32),
                ("start", ctypes.c_uint32), ("start_m", ctypes.c_uint32)]


_lib = None
_lib_lock = threading.Lock()


def lib() -> ctypes.CDLL:
    """Load libdgrep.so (fails loudly if it was not built)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError("libdgrep.so not built (run __graft_entry__.build() or `make`): " + LIB_PATH)
            L = ctypes.CDLL(LIB_PATH)
            vp, sz, u64, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int
            L.dgrep_compile.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.c_char_p, sz]
            L.dgrep_compile.restype = i
            L.dgrep_compile_budget.argtypes = [ctypes.c_char_p, sz, ctypes.c_uint32, ctypes.POINTER(vp),
                                               ctypes.POINTER(sz), ctypes.c_char_p, sz]
            L.dgrep_compile_budget.restype = i
            L.dgrep_blob_free.argtypes = [vp]
            L.dgrep_blob_free.restype = None
            L.dgrep_blob_info_get.argtypes = [vp, sz, ctypes.POINTER(_BlobInfo)]
            L.dgrep_blob_info_get.restype = i
            L.dgrep_pick_device.argtypes = [i, ctypes.POINTER(i)]
            L.dgrep_pick_device.restype = i
            L.dgrep_open.argtypes = [i, ctypes.POINTER(vp)]
            L.dgrep_open.restype = i
            L.dgrep_close.argtypes = [vp]
            L.dgrep_close.restype = None
            L.dgrep_last_error.argtypes = [vp]
            L.dgrep_last_error.restype = ctypes.c_char_p
            L.dgrep_set_stream.argtypes = [vp, vp]
            L.dgrep_set_stream.restype = i
            L.dgrep_load_dfa.argtypes = [vp, vp, sz]
            L.dgrep_load_dfa.restype = i
            L.dgrep_set_stepper.argtypes = [vp, i, ctypes.c_uint32]
            L.dgrep_set_stepper.restype = i
            L.dgrep_set_lane_chunk.argtypes = [vp, ctypes.c_uint32]
            L.dgrep_set_lane_chunk.restype = i
            L.dgrep_scan.argtypes = [vp, vp, sz, ctypes.POINTER(_Result)]
            L.dgrep_scan.restype = i
            L.dgrep_result_free.argtypes = [ctypes.POINTER(_Result)]
            L.dgrep_result_free.restype = None
            L.dgrep_scan_device.argtypes = [vp, vp, sz, vp, vp, vp, u64, ctypes.POINTER(u64)]
            L.dgrep_scan_device.restype = i
            L.dgrep_synth_corpus.argtypes = [vp, vp, sz, u64, i]
            L.dgrep_synth_corpus.restype = i
            L.dgrep_synth_corpus_host.argtypes = [vp, sz, u64, i]
            L.dgrep_synth_corpus_host.restype = i
            L.dgrep_synth_keyword.argtypes = [u64, i, ctypes.c_char_p]
            L.dgrep_synth_keyword.restype = i
            L.dgrep_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
            L.dgrep_last_kernel_ms.restype = i
            L.dgrep_take_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
            L.dgrep_take_kernel_ms.restype = i
            L.dgrep_set_ingest.argtypes = [vp, sz, i, i]
            L.dgrep_set_ingest.restype = i
            L.dgrep_last_ingest_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
            L.dgrep_last_ingest_ms.restype = i
            L.dgrep_map_partitions.argtypes = [vp, vp, sz, ctypes.c_char_p, sz, ctypes.c_uint32,
                                               ctypes.POINTER(_Partitions)]
            L.dgrep_map_partitions.restype = i
            L.dgrep_partitions_free.argtypes = [ctypes.POINTER(_Partitions)]
            L.dgrep_partitions_free.restype = None
            L.dgrep_encode_device.argtypes = [vp, vp, sz, vp, vp, vp, u64, ctypes.c_char_p, sz, ctypes.c_uint32, vp,
                                              u64, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
            L.dgrep_encode_device.restype = i
            L.dgrep_last_encode_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
            L.dgrep_last_encode_ms.restype = i
            L.dgrep_last_encode_stats.argtypes = [vp, ctypes.POINTER(_EncodeStats), sz]
            L.dgrep_last_encode_stats.restype = i
            L.dgrep_reduce.argtypes = [vp, vp, sz, ctypes.POINTER(_ReduceOut)]
            L.dgrep_reduce.restype = i
            L.dgrep_reduce_free.argtypes = [ctypes.POINTER(_ReduceOut)]
            L.dgrep_reduce_free.restype = None
            L.dgrep_last_scan_stats.argtypes = [vp, ctypes.POINTER(_ScanStats), sz]
            L.dgrep_last_scan_stats.restype = i
            L.dgrep_build_info.argtypes = []
            L.dgrep_build_info.restype = ctypes.c_char_p
            L.dgrep_comm_unique_id.argtypes = [vp]
            L.dgrep_comm_unique_id.restype = i
            L.dgrep_comm_open.argtypes = [vp, vp, i, i, ctypes.POINTER(vp)]
            L.dgrep_comm_open.restype = i
            L.dgrep_comm_close.argtypes = [vp]
            L.dgrep_comm_close.restype = None
            L.dgrep_gather_records_device.argtypes = [vp, vp, vp, vp, u64, ctypes.c_uint32, i, ctypes.POINTER(vp),
                                                      ctypes.POINTER(u64), vp]
            L.dgrep_gather_records_device.restype = i
            L.dgrep_gather_records.argtypes = [vp, vp, vp, vp, u64, ctypes.c_uint32, i, ctypes.POINTER(_Gathered)]
            L.dgrep_gather_records.restype = i
            L.dgrep_gathered_free.argtypes = [ctypes.POINTER(_Gathered)]
            L.dgrep_gathered_free.restype = None
            L.dgrep_comm_last_error.argtypes = [vp]
            L.dgrep_comm_last_error.restype = ctypes.c_char_p
            L.dgrep_scan_batch.argtypes = [vp, vp, vp, sz, ctypes.POINTER(_BatchResult)]
            L.dgrep_scan_batch.restype = i
            L.dgrep_batch_result_free.argtypes = [ctypes.POINTER(_BatchResult)]
            L.dgrep_batch_result_free.restype = None
            L.dgrep_scan_batch_device.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, u64, ctypes.POINTER(u64)]
            L.dgrep_scan_batch_device.restype = i
            L.dgrep_last_batch_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
            L.dgrep_last_batch_ms.restype = i
            L.dgrep_map_partitions_batch.argtypes = [vp, vp, vp, vp, vp, sz, ctypes.c_uint32,
                                                     ctypes.POINTER(_BatchPartitions)]
            L.dgrep_map_partitions_batch.restype = i
            L.dgrep_batch_partitions_free.argtypes = [ctypes.POINTER(_BatchPartitions)]
            L.dgrep_batch_partitions_free.restype = None
            L.dgrep_encode_batch_device.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, vp, u64, vp, vp, ctypes.c_uint32,
                                                    vp, u64, vp, ctypes.POINTER(u64)]
            L.dgrep_encode_batch_device.restype = i
            L.dgrep_reduce_batch.argtypes = [vp, vp, vp, sz, ctypes.POINTER(_ReduceBatchOut)]
            L.dgrep_reduce_batch.restype = i
            L.dgrep_reduce_batch_free.argtypes = [ctypes.POINTER(_ReduceBatchOut)]
            L.dgrep_reduce_batch_free.restype = None
            L.dgrep_reduce_batch_device.argtypes = [vp, vp, sz, vp, sz, ctypes.c_uint32, vp, u64, vp, vp,
                                                    ctypes.POINTER(u64)]
            L.dgrep_reduce_batch_device.restype = i
            L.dgrep_grep_job.argtypes = [vp, vp, vp, vp, vp, sz, ctypes.c_uint32, ctypes.POINTER(_ReduceBatchOut)]
            L.dgrep_grep_job.restype = i
            L.dgrep_last_reduce_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
            L.dgrep_last_reduce_ms.restype = i
            L.dgrep_scan_windowed.argtypes = [vp, vp, sz, sz, ctypes.POINTER(_Result)]
            L.dgrep_scan_windowed.restype = i
            L.dgrep_stream_open.argtypes = [vp, sz, ctypes.c_uint32, ctypes.POINTER(vp)]
            L.dgrep_stream_open.restype = i
            L.dgrep_stream_feed.argtypes = [vp, vp, sz, ctypes.POINTER(_StreamResult)]
            L.dgrep_stream_feed.restype = i
            L.dgrep_stream_finish.argtypes = [vp, ctypes.POINTER(_StreamResult)]
            L.dgrep_stream_finish.restype = i
            L.dgrep_stream_result_free.argtypes = [ctypes.POINTER(_StreamResult)]
            L.dgrep_stream_result_free.restype = None
            L.dgrep_stream_close.argtypes = [vp]
            L.dgrep_stream_close.restype = None
            L.dgrep_stream_stats.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64),
                                             ctypes.POINTER(ctypes.c_float)]
            L.dgrep_stream_stats.restype = i
            L.dgrep_scan_bounded.argtypes = [vp, vp, sz, sz, ctypes.POINTER(_Result)]
            L.dgrep_scan_bounded.restype = i
            L.dgrep_stream_carry_stats.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                   ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_float)]
            L.dgrep_stream_carry_stats.restype = i
            L.dgrep_stream_open_partitions.argtypes = [vp, sz, ctypes.c_char_p, sz, ctypes.c_uint32,
                                                       ctypes.POINTER(vp)]
            L.dgrep_stream_open_partitions.restype = i
            L.dgrep_stream_feed_partitions.argtypes = [vp, vp, sz, ctypes.POINTER(_BatchPartitions)]
            L.dgrep_stream_feed_partitions.restype = i
            L.dgrep_stream_finish_partitions.argtypes = [vp, ctypes.POINTER(_BatchPartitions)]
            L.dgrep_stream_finish_partitions.restype = i
            L.dgrep_map_partitions_windowed.argtypes = [vp, vp, sz, sz, ctypes.c_char_p, sz, ctypes.c_uint32,
                                                        ctypes.POINTER(_BatchPartitions)]
            L.dgrep_map_partitions_windowed.restype = i
            L.dgrep_stream_partition_stats.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                       ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                       ctypes.POINTER(ctypes.c_float)]
            L.dgrep_stream_partition_stats.restype = i
            L.dgrep_set_long_value.argtypes = [vp, ctypes.c_uint32]
            L.dgrep_set_long_value.restype = i
            L.dgrep_job_open.argtypes = [vp, sz, ctypes.c_uint32, ctypes.POINTER(vp)]
            L.dgrep_job_open.restype = i
            L.dgrep_job_add.argtypes = [vp, vp, sz, ctypes.c_char_p, sz]
            L.dgrep_job_add.restype = i
            L.dgrep_job_file_begin.argtypes = [vp, ctypes.c_char_p, sz]
            L.dgrep_job_file_begin.restype = i
            L.dgrep_job_file_feed.argtypes = [vp, vp, sz]
            L.dgrep_job_file_feed.restype = i
            L.dgrep_job_file_end.argtypes = [vp]
            L.dgrep_job_file_end.restype = i
            L.dgrep_job_finish.argtypes = [vp, ctypes.POINTER(_ReduceBatchOut)]
            L.dgrep_job_finish.restype = i
            L.dgrep_job_close.argtypes = [vp]
            L.dgrep_job_close.restype = None
            L.dgrep_job_stats_get.argtypes = [vp, ctypes.POINTER(_JobStats), sz]
            L.dgrep_job_stats_get.restype = i
            L.dgrep_grep_job_windowed.argtypes = [vp, vp, vp, vp, vp, sz, ctypes.c_uint32, sz,
                                                  ctypes.POINTER(_ReduceBatchOut)]
            L.dgrep_grep_job_windowed.restype = i
            _lib = L
    return _lib


class CompiledPattern:
    """A pattern compiled by dgrep_compile (Go regexp/syntax semantics)."""

    def __init__(self, pattern, state_budget: int = 0):
        """state_budget (tests only): a lowered DFA state budget, so that small
        patterns compile to partial blobs (dgrep_compile_budget)."""
        if isinstance(pattern, str):
            pattern = pattern.encode("utf-8", "surrogateescape")
        self.pattern = bytes(pattern)
        L = lib()
        blob = ctypes.c_void_p()
        n = ctypes.c_size_t()
        err = ctypes.create_string_buffer(512)
        rc = L.dgrep_compile_budget(self.pattern, len(self.pattern), state_budget, ctypes.byref(blob),
                                    ctypes.byref(n), err, 512)
        msg = err.value.decode(errors="replace")
        if rc == DGREP_E_UNSUPPORTED:
            raise UnsupportedPattern(rc, msg)
        if rc != DGREP_OK:
            raise DgrepError(rc, msg)
        self.blob = ctypes.string_at(blob, n.value)
        L.dgrep_blob_free(blob)
        info = _BlobInfo()
        rc = L.dgrep_blob_info_get(self.blob, len(self.blob), ctypes.byref(info))
        if rc != DGREP_OK:
            raise DgrepError(rc, "malformed blob")
        self.flags = info.flags
        self.nstates = info.nstates
        self.nclasses = info.nclasses
        self.start = info.start
        self.start_m = info.start_m
        self.message = msg

    @property
    def partial(self) -> bool:
        """DFA over the state budget: first states + CAND, lines that reach CAND
        are decided by the blob's NFA program (dgrep_blob.h)."""
        return bool(self.flags & DFA_PARTIAL)

    def nfa_program(self) -> np.ndarray:
        """The NFA program (u32 words) of a partial blob -- for tests."""
        ne = self.nstates * self.nclasses
        return np.frombuffer(self.blob[288 + 4 * ne:], dtype=np.uint32)

    @property
    def nfa_positions(self) -> int:
        """Rune-set positions (npos) of a partial blob's NFA program, 0 for any
        other blob. Up to 1024 a candidate line is decided by one lane, above
        that (up to 8192, DGREP_NFA_MAX_POS) by one wave."""
        if not self.partial:
            return 0
        at = 288 + 4 * self.nstates * self.nclasses + 4  # the program's second word
        return int.from_bytes(self.blob[at:at + 4], "little")

    @property
    def go_syntax_error(self) -> bool:
        return bool(self.flags & DFA_GO_SYNTAX_ERROR)

    def tables(self) -> Tuple[np.ndarray, np.ndarray]:
        """(byte_class[256] u8, trans[nstates, nclasses] u32) — for tests/inspection."""
        bc = np.frombuffer(self.blob[32:288], dtype=np.uint8)
        ne = self.nstates * self.nclasses
        tr = np.frombuffer(self.blob[288:288 + 4 * ne], dtype=np.uint32).reshape(self.nstates, self.nclasses)
        return bc, tr


class Context:
    """One device context (a HIP device + stream) — dgrep_open/close."""

    def __init__(self, device: int = 0):
        self._L = lib()
        h = ctypes.c_void_p()
        rc = self._L.dgrep_open(device, ctypes.byref(h))
        self._h = h
        if rc != DGREP_OK:
            msg = self._err()
            self.close()
            raise DgrepError(rc, msg)
        self.device = device
        self.pattern: Optional[CompiledPattern] = None

    def _err(self) -> str:
        m = self._L.dgrep_last_error(self._h)
        return m.decode(errors="replace") if m else ""

    def _check(self, rc: int):
        if rc != DGREP_OK:
            if rc == DGREP_E_UNSUPPORTED:
                raise UnsupportedPattern(rc, self._err())
            raise DgrepError(rc, self._err())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.dgrep_close(self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: int):
        self._check(self._L.dgrep_set_stream(self._h, ctypes.c_void_p(hip_stream or None)))

    def set_lane_chunk(self, chunk_bytes: int = 0):
        """Testing/tuning: the Sheng / pair / filter lane chunk for later scans
        (dgrep_set_lane_chunk; 0 = adaptive, else a multiple of 128 in [4096, 65536])."""
        self._check(self._L.dgrep_set_lane_chunk(self._h, chunk_bytes))

    _FORCE = {"auto": 0, "table": 2, "pair": 3, "filter": 4}

    def set_stepper(self, force="auto", filter_rows: int = 0):
        """Testing/tuning: the stepper the next load() uses (dgrep_set_stepper):
        "auto" (default: by DFA size), "table" (u8, <= 256 states), "pair" (fails
        at load if its two-byte table does not fit) or "filter"; filter_rows caps
        the filter's LDS rows (nearly every line then becomes a candidate)."""
        self._check(self._L.dgrep_set_stepper(self._h, self._FORCE[force], filter_rows))

    def load(self, pattern) -> CompiledPattern:
        cp = pattern if isinstance(pattern, CompiledPattern) else CompiledPattern(pattern)
        self._check(self._L.dgrep_load_dfa(self._h, cp.blob, len(cp.blob)))
        self.pattern = cp
        return cp

    def scan(self, contents) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Host split -> (line_no u64[], start u64[], len u64[]) of matching lines."""
        if isinstance(contents, str):
            contents = contents.encode("utf-8", "surrogateescape")
        buf = np.frombuffer(contents, dtype=np.uint8) if len(contents) else np.zeros(1, np.uint8)
        res = _Result()
        self._check(self._L.dgrep_scan(self._h, ctypes.c_void_p(buf.ctypes.data), len(contents), ctypes.byref(res)))
        try:
            n = int(res.count)
            if n == 0:
                return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64)
            ln = np.ctypeslib.as_array(res.line_no, shape=(n,)).copy()
            st = np.ctypeslib.as_array(res.start, shape=(n,)).copy()
            le = np.ctypeslib.as_array(res.len, shape=(n,)).copy()
            return ln, st, le
        finally:
            self._L.dgrep_result_free(ctypes.byref(res))

    def scan_windowed(self, contents, window: int, bounded: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """scan() with the split never resident as a whole (dgrep_scan_windowed):
        the same three arrays, from windows of `window` bytes (a multiple of 4096).
        bounded=True (dgrep_scan_bounded): a line longer than the window is folded
        into its DFA state instead of growing the window buffers."""
        if isinstance(contents, str):
            contents = contents.encode("utf-8", "surrogateescape")
        buf = np.frombuffer(contents, dtype=np.uint8) if len(contents) else np.zeros(1, np.uint8)
        res = _Result()
        call = self._L.dgrep_scan_bounded if bounded else self._L.dgrep_scan_windowed
        self._check(call(self._h, ctypes.c_void_p(buf.ctypes.data), len(contents), window, ctypes.byref(res)))
        try:
            n = int(res.count)
            if n == 0:
                return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64)
            return (np.ctypeslib.as_array(res.line_no, shape=(n,)).copy(),
                    np.ctypeslib.as_array(res.start, shape=(n,)).copy(),
                    np.ctypeslib.as_array(res.len, shape=(n,)).copy())
        finally:
            self._L.dgrep_result_free(ctypes.byref(res))

    def stream(self, window: int, values: bool = False, bounded: bool = False) -> "Stream":
        """A stream over this context's loaded pattern (dgrep_stream_open): feed
        it a split piece by piece. Close it before the context. bounded=True
        (DGREP_STREAM_BOUNDED) keeps the device footprint fixed whatever the
        lines' lengths; it returns no values."""
        return Stream(self, window, values, bounded)

    def scan_device(self, d_data: int, n: int, d_line: int, d_start: int, d_len: int, capacity: int) -> int:
        """HBM-resident split at device pointer d_data; returns the match count."""
        cnt = ctypes.c_uint64()
        self._check(self._L.dgrep_scan_device(self._h, ctypes.c_void_p(d_data), n, ctypes.c_void_p(d_line),
                                              ctypes.c_void_p(d_start), ctypes.c_void_p(d_len), capacity,
                                              ctypes.byref(cnt)))
        return int(cnt.value)

    def scan_batch(self, splits) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Many host splits in one scan (dgrep_scan_batch): (line_no u64[], start
        u64[], len u64[], split u32[], split_begin u64[len(splits) + 1]); line_no
        and start are relative to the record's split, and split s owns records
        [split_begin[s], split_begin[s+1])."""
        raws = [x.encode("utf-8", "surrogateescape") if isinstance(x, str) else bytes(x) for x in splits]
        k = len(raws)
        bufs = [np.frombuffer(r, dtype=np.uint8) for r in raws]  # keep the bytes alive over the call
        ptrs = (ctypes.c_void_p * max(k, 1))(*[b.ctypes.data if len(b) else None for b in bufs])
        lens = (ctypes.c_size_t * max(k, 1))(*[len(r) for r in raws])
        res = _BatchResult()
        self._check(self._L.dgrep_scan_batch(self._h, ptrs, lens, k, ctypes.byref(res)))
        try:
            n = int(res.count)
            sb = np.ctypeslib.as_array(res.split_begin, shape=(k + 1,)).copy()
            if n == 0:
                return (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64),
                        np.zeros(0, np.uint32), sb)
            return (np.ctypeslib.as_array(res.line_no, shape=(n,)).copy(),
                    np.ctypeslib.as_array(res.start, shape=(n,)).copy(),
                    np.ctypeslib.as_array(res.len, shape=(n,)).copy(),
                    np.ctypeslib.as_array(res.split, shape=(n,)).copy(), sb)
        finally:
            self._L.dgrep_batch_result_free(ctypes.byref(res))

    def scan_batch_device(self, d_packed: int, n_packed: int, split_len, d_line: int, d_start: int, d_len: int,
                          d_split: int, d_split_begin: int, capacity: int) -> int:
        """HBM-resident packed splits (dgrep_scan_batch_device): split_len = the
        splits' byte lengths (host), d_split_begin may be 0 (NULL); returns the
        match count over all splits."""
        lens = np.ascontiguousarray(split_len, dtype=np.uint64)
        cnt = ctypes.c_uint64()
        self._check(self._L.dgrep_scan_batch_device(
            self._h, ctypes.c_void_p(d_packed), n_packed, ctypes.c_void_p(lens.ctypes.data if len(lens) else None),
            len(lens), ctypes.c_void_p(d_line), ctypes.c_void_p(d_start), ctypes.c_void_p(d_len),
            ctypes.c_void_p(d_split), ctypes.c_void_p(d_split_begin or None), capacity, ctypes.byref(cnt)))
        return int(cnt.value)

    def last_batch_ms(self) -> Tuple[float, float]:
        """(newline_ms, rebase_ms) of the last batch call's own kernels (dgrep_last_batch_ms)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        self._check(self._L.dgrep_last_batch_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return float(a.value), float(b.value)

    def synth(self, d_out: int, n: int, seed: int, kind: int = 0):
        self._check(self._L.dgrep_synth_corpus(self._h, ctypes.c_void_p(d_out), n, seed, kind))

    def set_ingest(self, chunk_bytes: int, nbufs: int = 0, threads: int = 0):
        """Ingest pipeline of scan(): pinned staging pieces of chunk_bytes (0 =
        one direct pageable copy), nbufs buffers, threads host-copy threads
        (dgrep_set_ingest; 0 keeps the current value)."""
        self._check(self._L.dgrep_set_ingest(self._h, chunk_bytes, nbufs, threads))

    def last_ingest_ms(self) -> float:
        ms = ctypes.c_float()
        self._check(self._L.dgrep_last_ingest_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def map_partitions(self, filename, contents, nreduce: int) -> List[bytes]:
        """Map + writeMapOutput of one split on the GPU (dgrep_map_partitions):
        element p is the byte content of mr-<task>-<p> (map_reduce/worker.go:78-109)."""
        if isinstance(contents, str):
            contents = contents.encode("utf-8", "surrogateescape")
        fname = filename.encode("utf-8", "surrogateescape") if isinstance(filename, str) else bytes(filename)
        buf = np.frombuffer(contents, dtype=np.uint8) if len(contents) else np.zeros(1, np.uint8)
        res = _Partitions()
        self._check(self._L.dgrep_map_partitions(self._h, ctypes.c_void_p(buf.ctypes.data), len(contents), fname,
                                                 len(fname), nreduce, ctypes.byref(res)))
        try:
            raw = ctypes.string_at(res.bytes, res.total) if res.total else b""
            return [raw[res.begin[p]:res.end[p]] for p in range(nreduce)]
        finally:
            self._L.dgrep_partitions_free(ctypes.byref(res))

    def set_long_value(self, n: int = 0):
        """Testing/tuning: the value length from which an escaped value takes the
        partition writers' parallel path (dgrep_set_long_value; 0 = each writer's
        default, 256 for the window writer and 768 for the resident and batch ones,
        else a multiple of 64 in [256, 2^30]). All three writers (resident,
        batch, window) read it; 2^30 forces the one-lane path everywhere."""
        self._check(self._L.dgrep_set_long_value(self._h, n))

    def map_partitions_windowed(self, filename, contents, nreduce: int, window: int) -> List[bytes]:
        """map_partitions() with the split never resident as a whole
        (dgrep_map_partitions_windowed): element p is the byte content of
        mr-<task>-<p>, the rows of the windowed result joined per partition."""
        if isinstance(contents, str):
            contents = contents.encode("utf-8", "surrogateescape")
        fname = filename.encode("utf-8", "surrogateescape") if isinstance(filename, str) else bytes(filename)
        buf = np.frombuffer(contents, dtype=np.uint8) if len(contents) else np.zeros(1, np.uint8)
        res = _BatchPartitions()
        self._check(self._L.dgrep_map_partitions_windowed(self._h, ctypes.c_void_p(buf.ctypes.data), len(contents),
                                                          window, fname, len(fname), nreduce, ctypes.byref(res)))
        rows = _take_rows(self._L, res)
        return [b"".join(r[p] for r in rows) for p in range(nreduce)]

    def partition_stream(self, window: int, filename, nreduce: int) -> "PartitionStream":
        """A stream that returns partition cells (dgrep_stream_open_partitions):
        feed it a split piece by piece, append cell [w][p] to mr-<task>-<p>.
        Close it before the context."""
        return PartitionStream(self, window, filename, nreduce)

    def encode_device(self, d_data: int, n: int, d_line: int, d_start: int, d_len: int, count: int, filename,
                      nreduce: int, d_out: int, out_cap: int):
        """dgrep_encode_device: returns (begin[], end[], total)."""
        fname = filename.encode("utf-8", "surrogateescape") if isinstance(filename, str) else bytes(filename)
        b = (ctypes.c_uint64 * nreduce)()
        e = (ctypes.c_uint64 * nreduce)()
        tot = ctypes.c_uint64()
        self._check(self._L.dgrep_encode_device(self._h, ctypes.c_void_p(d_data), n, ctypes.c_void_p(d_line),
                                                ctypes.c_void_p(d_start), ctypes.c_void_p(d_len), count, fname,
                                                len(fname), nreduce, ctypes.c_void_p(d_out), out_cap, b, e,
                                                ctypes.byref(tot)))
        return list(b), list(e), int(tot.value)

    def map_partitions_batch(self, files, nreduce: int) -> List[List[bytes]]:
        """Map + writeMapOutput of many splits in one scan and one encode
        (dgrep_map_partitions_batch): files = [(filename, contents), ...];
        element [s][p] is the byte content of mr-<s>-<p>. No file: [] without a
        C call."""
        files = list(files)
        if not files:
            return []
        as_bytes = lambda x: x.encode("utf-8", "surrogateescape") if isinstance(x, str) else bytes(x)
        names = [as_bytes(f) for f, _ in files]
        raws = [as_bytes(c) for _, c in files]
        k = len(files)
        bufs = [np.frombuffer(r, dtype=np.uint8) for r in raws]  # keep the bytes alive over the call
        ptrs = (ctypes.c_void_p * k)(*[b.ctypes.data if len(b) else None for b in bufs])
        lens = (ctypes.c_size_t * k)(*[len(r) for r in raws])
        fptrs = (ctypes.c_char_p * k)(*names)
        flens = (ctypes.c_size_t * k)(*[len(f) for f in names])
        res = _BatchPartitions()
        self._check(self._L.dgrep_map_partitions_batch(self._h, ptrs, lens, fptrs, flens, k, nreduce,
                                                       ctypes.byref(res)))
        try:
            raw = ctypes.string_at(res.bytes, res.total) if res.total else b""
            off = np.ctypeslib.as_array(res.cell_off, shape=(k * nreduce + 1,)).tolist()
            return [[raw[off[s * nreduce + p]:off[s * nreduce + p + 1]] for p in range(nreduce)] for s in range(k)]
        finally:
            self._L.dgrep_batch_partitions_free(ctypes.byref(res))

    def encode_batch_device(self, d_packed: int, n_packed: int, split_len, d_line: int, d_start: int, d_len: int,
                            d_split: int, count: int, filenames, nreduce: int, d_out: int, out_cap: int):
        """dgrep_encode_batch_device over the records dgrep_scan_batch_device
        returned for the same packed buffer: returns (cell_off list of
        len(split_len) * nreduce + 1 entries, total)."""
        lens = np.ascontiguousarray(split_len, dtype=np.uint64)
        k = len(lens)
        names = [f.encode("utf-8", "surrogateescape") if isinstance(f, str) else bytes(f) for f in filenames]
        assert len(names) == k, "one filename per split"
        fptrs = (ctypes.c_char_p * max(k, 1))(*names)
        flens = (ctypes.c_size_t * max(k, 1))(*[len(f) for f in names])
        off = np.zeros(k * nreduce + 1, np.uint64)
        tot = ctypes.c_uint64()
        self._check(self._L.dgrep_encode_batch_device(
            self._h, ctypes.c_void_p(d_packed), n_packed, ctypes.c_void_p(lens.ctypes.data if k else None), k,
            ctypes.c_void_p(d_line), ctypes.c_void_p(d_start), ctypes.c_void_p(d_len), ctypes.c_void_p(d_split),
            count, fptrs, flens, nreduce, ctypes.c_void_p(d_out or None), out_cap, ctypes.c_void_p(off.ctypes.data),
            ctypes.byref(tot)))
        return off.tolist(), int(tot.value)

    def reduce(self, data: bytes) -> bytes:
        """One grep reduce task on the GPU (dgrep_reduce): data = the
        concatenated mr-<map>-<r> files; returns the content of mr-out-<r>."""
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        res = _ReduceOut()
        self._check(self._L.dgrep_reduce(self._h, ctypes.c_void_p(buf.ctypes.data), len(data), ctypes.byref(res)))
        try:
            return ctypes.string_at(res.bytes, res.total) if res.total else b""
        finally:
            self._L.dgrep_reduce_free(ctypes.byref(res))

    def _reduce_batch_parts(self, res: "_ReduceBatchOut") -> List[bytes]:
        try:
            k = int(res.nparts)
            raw = ctypes.string_at(res.bytes, res.total) if res.total else b""
            off = np.ctypeslib.as_array(res.part_off, shape=(k + 1,)).tolist()
            self.last_lines_in = np.ctypeslib.as_array(res.lines_in, shape=(k,)).tolist()
            return [raw[off[p]:off[p + 1]] for p in range(k)]
        finally:
            self._L.dgrep_reduce_batch_free(ctypes.byref(res))

    def reduce_batch(self, inputs) -> List[bytes]:
        """Every reduce task of a job in one pass (dgrep_reduce_batch):
        inputs[p] = the concatenated mr-<map>-<p> files; element p of the result
        is the content of mr-out-<p>, equal to reduce(inputs[p]). The lines read
        per partition are left in self.last_lines_in. No input: [] without a C
        call."""
        raws = [bytes(x) for x in inputs]
        if not raws:
            return []
        k = len(raws)
        bufs = [np.frombuffer(r, dtype=np.uint8) for r in raws]  # keep the bytes alive over the call
        ptrs = (ctypes.c_void_p * k)(*[b.ctypes.data if len(b) else None for b in bufs])
        lens = (ctypes.c_size_t * k)(*[len(r) for r in raws])
        res = _ReduceBatchOut()
        self._check(self._L.dgrep_reduce_batch(self._h, ptrs, lens, k, ctypes.byref(res)))
        return self._reduce_batch_parts(res)

    def reduce_batch_device(self, d_data: int, n: int, seg_off, nparts: int, d_out: int, out_cap: int):
        """dgrep_reduce_batch_device over the segments seg_off (host, nseg + 1
        entries) of the device buffer d_data: returns (part_off list of nparts + 1
        entries, lines_in list of nparts entries, total)."""
        seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
        off = np.zeros(nparts + 1, np.uint64)
        lin = np.zeros(max(nparts, 1), np.uint64)
        tot = ctypes.c_uint64()
        self._check(self._L.dgrep_reduce_batch_device(
            self._h, ctypes.c_void_p(d_data or None), n, ctypes.c_void_p(seg.ctypes.data if len(seg) else None),
            max(len(seg), 1) - 1, nparts, ctypes.c_void_p(d_out or None), out_cap, ctypes.c_void_p(off.ctypes.data),
            ctypes.c_void_p(lin.ctypes.data), ctypes.byref(tot)))
        return off.tolist(), lin[:nparts].tolist(), int(tot.value)

    def grep_job(self, files, nreduce: int) -> List[bytes]:
        """The whole grep job of one worker in one call (dgrep_grep_job): files
        = [(filename, contents), ...] as map_partitions_batch takes them; element
        r of the result is the content of mr-out-<r>. The intermediate bytes
        stay on the device. No file: [] without a C call."""
        files = list(files)
        if not files:
            return []
        as_bytes = lambda x: x.encode("utf-8", "surrogateescape") if isinstance(x, str) else bytes(x)
        names = [as_bytes(f) for f, _ in files]
        raws = [as_bytes(c) for _, c in files]
        k = len(files)
        bufs = [np.frombuffer(r, dtype=np.uint8) for r in raws]  # keep the bytes alive over the call
        ptrs = (ctypes.c_void_p * k)(*[b.ctypes.data if len(b) else None for b in bufs])
        lens = (ctypes.c_size_t * k)(*[len(r) for r in raws])
        fptrs = (ctypes.c_char_p * k)(*names)
        flens = (ctypes.c_size_t * k)(*[len(f) for f in names])
        res = _ReduceBatchOut()
        self._check(self._L.dgrep_grep_job(self._h, ptrs, lens, fptrs, flens, k, nreduce, ctypes.byref(res)))
        return self._reduce_batch_parts(res)

    def job(self, window: int, nreduce: int) -> "Job":
        """A windowed whole job (dgrep_job_*): add files of any size in task
        order, finish() returns every mr-out-<r>."""
        return Job(self, window, nreduce)

    def grep_job_windowed(self, files, nreduce: int, window: int) -> List[bytes]:
        """grep_job with no input resident as a whole (dgrep_grep_job_windowed):
        the same result byte for byte, last_lines_in included, whatever the
        window. No file: [] without a C call."""
        files = list(files)
        if not files:
            return []
        as_bytes = lambda x: x.encode("utf-8", "surrogateescape") if isinstance(x, str) else bytes(x)
        names = [as_bytes(f) for f, _ in files]
        raws = [as_bytes(c) for _, c in files]
        k = len(files)
        bufs = [np.frombuffer(r, dtype=np.uint8) for r in raws]  # keep the bytes alive over the call
        ptrs = (ctypes.c_void_p * k)(*[b.ctypes.data if len(b) else None for b in bufs])
        lens = (ctypes.c_size_t * k)(*[len(r) for r in raws])
        fptrs = (ctypes.c_char_p * k)(*names)
        flens = (ctypes.c_size_t * k)(*[len(f) for f in names])
        res = _ReduceBatchOut()
        self._check(self._L.dgrep_grep_job_windowed(self._h, ptrs, lens, fptrs, flens, k, nreduce, window,
                                                    ctypes.byref(res)))
        return self._reduce_batch_parts(res)

    def last_reduce_ms(self) -> float:
        """Device time of the last batch reduce (dgrep_last_reduce_ms)."""
        ms = ctypes.c_float()
        self._check(self._L.dgrep_last_reduce_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def last_encode_ms(self) -> float:
        ms = ctypes.c_float()
        self._check(self._L.dgrep_last_encode_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def encode_stats(self) -> dict:
        """dgrep_last_encode_stats: records, long_values and long_chunks of the
        last resident or batch encode (after a job: the sums over its packs),
        and its device ms. A window-route encode does not touch it."""
        st = _EncodeStats()
        self._check(self._L.dgrep_last_encode_stats(self._h, ctypes.byref(st), ctypes.sizeof(st)))
        return {f: getattr(st, f) for f, _ in _EncodeStats._fields_}

    def last_kernel_ms(self) -> float:
        ms = ctypes.c_float()
        self._check(self._L.dgrep_last_kernel_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def take_kernel_ms(self):
        """(sum of the scans' device ms, number of scans) since the previous take (dgrep_take_kernel_ms)."""
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        self._check(self._L.dgrep_take_kernel_ms(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def scan_stats(self) -> dict:
        """dgrep_last_scan_stats of the last scan (stepper, lane chunk, overflow lanes, times)."""
        st = _ScanStats()
        self._check(self._L.dgrep_last_scan_stats(self._h, ctypes.byref(st), ctypes.sizeof(st)))
        d = {f: getattr(st, f) for f, _ in _ScanStats._fields_}
        d["stepper"] = STEPPERS.get(d["stepper"], d["stepper"])
        return d


class Stream:
    """dgrep_stream_*: a split fed in pieces of any length. feed(piece) and
    finish() return (line_no u64[], start u64[], len u64[]) of the matching
    lines the call completed, numbered and placed in the whole stream, plus --
    with values=True -- a list of those lines' bytes (gathered on the device)."""

    def __init__(self, ctx: "Context", window: int, values: bool = False, bounded: bool = False):
        self._L = lib()
        self.ctx = ctx
        self.values = bool(values)
        self.bounded = bool(bounded)
        h = ctypes.c_void_p()
        self._h = h
        flags = (STREAM_VALUES if values else 0) | (STREAM_BOUNDED if bounded else 0)
        ctx._check(self._L.dgrep_stream_open(ctx._h, window, flags, ctypes.byref(h)))

    def _take(self, res: "_StreamResult"):
        try:
            n = int(res.count)
            arr = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            out = (arr(res.line_no), arr(res.start), arr(res.len))
            if not self.values:
                return out
            off = np.ctypeslib.as_array(res.value_off, shape=(n + 1,)).tolist()
            raw = ctypes.string_at(res.values, off[n]) if off[n] else b""
            return out + ([raw[off[r]:off[r + 1]] for r in range(n)],)
        finally:
            self._L.dgrep_stream_result_free(ctypes.byref(res))

    def feed(self, piece):
        piece = piece.encode("utf-8", "surrogateescape") if isinstance(piece, str) else piece
        buf = np.frombuffer(piece, dtype=np.uint8) if len(piece) else np.zeros(1, np.uint8)
        res = _StreamResult()
        self.ctx._check(self._L.dgrep_stream_feed(self._h, ctypes.c_void_p(buf.ctypes.data), len(piece),
                                                  ctypes.byref(res)))
        return self._take(res)

    def finish(self):
        res = _StreamResult()
        self.ctx._check(self._L.dgrep_stream_finish(self._h, ctypes.byref(res)))
        return self._take(res)

    def stats(self) -> dict:
        """dgrep_stream_stats: windows scanned, device bytes of the two window
        buffers now, the longest carried tail, the cut passes' device ms."""
        w, d, m, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_float()
        self.ctx._check(self._L.dgrep_stream_stats(self._h, ctypes.byref(w), ctypes.byref(d), ctypes.byref(m),
                                                   ctypes.byref(ms)))
        return {"windows": int(w.value), "data_bytes": int(d.value), "max_carry": int(m.value),
                "cut_ms": float(ms.value)}

    def carry_stats(self) -> dict:
        """dgrep_stream_carry_stats: a bounded stream's folds, their bytes, the
        chunks its walks covered, the chunks whose guesses missed, the walks'
        device ms (all 0 on a stream that is not bounded)."""
        f, b, ch, gm, ms = (ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(),
                            ctypes.c_float())
        self.ctx._check(self._L.dgrep_stream_carry_stats(self._h, ctypes.byref(f), ctypes.byref(b), ctypes.byref(ch),
                                                         ctypes.byref(gm), ctypes.byref(ms)))
        return {"folds": int(f.value), "folded_bytes": int(b.value), "chunks": int(ch.value),
                "guess_misses": int(gm.value), "walk_ms": float(ms.value)}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value and self.ctx._h.value:
            self._L.dgrep_stream_close(self._h)
        self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _take_rows(L, res: "_BatchPartitions") -> List[List[bytes]]:
    """rows x partitions of a windowed partition result; frees it"""
    try:
        k, R = int(res.nsplits), int(res.nreduce)
        if k == 0:
            return []
        raw = ctypes.string_at(res.bytes, res.total) if res.total else b""
        off = np.ctypeslib.as_array(res.cell_off, shape=(k * R + 1,)).tolist()
        return [[raw[off[w * R + p]:off[w * R + p + 1]] for p in range(R)] for w in range(k)]
    finally:
        L.dgrep_batch_partitions_free(ctypes.byref(res))


class PartitionStream(Stream):
    """dgrep_stream_*_partitions: a split fed in pieces of any length, returned
    as the bytes of its map task's intermediate files. feed(piece) and finish()
    return rows x partitions: one row per window of the call that completed a
    matching line, element [w][p] = the bytes that window adds to
    mr-<task>-<p>. Joined per partition over all calls they are
    Context.map_partitions of the whole split."""

    def __init__(self, ctx: "Context", window: int, filename, nreduce: int):
        self._L = lib()
        self.ctx = ctx
        self.values = self.bounded = False
        self.nreduce = nreduce
        fname = filename.encode("utf-8", "surrogateescape") if isinstance(filename, str) else bytes(filename)
        h = ctypes.c_void_p()
        self._h = h
        ctx._check(self._L.dgrep_stream_open_partitions(ctx._h, window, fname, len(fname), nreduce, ctypes.byref(h)))

    def feed(self, piece) -> List[List[bytes]]:
        piece = piece.encode("utf-8", "surrogateescape") if isinstance(piece, str) else piece
        buf = np.frombuffer(piece, dtype=np.uint8) if len(piece) else np.zeros(1, np.uint8)
        res = _BatchPartitions()
        self.ctx._check(self._L.dgrep_stream_feed_partitions(self._h, ctypes.c_void_p(buf.ctypes.data), len(piece),
                                                             ctypes.byref(res)))
        return _take_rows(self._L, res)

    def finish(self) -> List[List[bytes]]:
        res = _BatchPartitions()
        self.ctx._check(self._L.dgrep_stream_finish_partitions(self._h, ctypes.byref(res)))
        return _take_rows(self._L, res)

    def stats(self) -> dict:
        """Stream.stats() plus dgrep_stream_partition_stats: rows returned, their
        bytes, values the long-value path took, the device buffer of encoded
        bytes now (one window's), the encoder's device ms."""
        d = Stream.stats(self)
        r, b, lv, e, ms = (ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(),
                           ctypes.c_float())
        self.ctx._check(self._L.dgrep_stream_partition_stats(self._h, ctypes.byref(r), ctypes.byref(b),
                                                             ctypes.byref(lv), ctypes.byref(e), ctypes.byref(ms)))
        d.update(rows=int(r.value), out_bytes=int(b.value), long_values=int(lv.value),
                 enc_device_bytes=int(e.value), encode_ms=float(ms.value))
        return d


class Job:
    """dgrep_job_*: the whole grep job over files of any size. add(filename,
    contents) takes a file held whole; begin(filename), feed(piece)..., end()
    one that is read piece by piece. finish() returns the content of every
    mr-out-<r>, byte for byte Context.grep_job of the same files in the same
    order, and leaves the lines read per partition in ctx.last_lines_in."""

    def __init__(self, ctx: "Context", window: int, nreduce: int):
        self._L = lib()
        self.ctx = ctx
        self.nreduce = nreduce
        h = ctypes.c_void_p()
        self._h = h
        ctx._check(self._L.dgrep_job_open(ctx._h, window, nreduce, ctypes.byref(h)))

    @staticmethod
    def _bytes(x) -> bytes:
        return x.encode("utf-8", "surrogateescape") if isinstance(x, str) else bytes(x)

    def add(self, filename, contents):
        name, raw = self._bytes(filename), self._bytes(contents)
        buf = np.frombuffer(raw, dtype=np.uint8) if len(raw) else np.zeros(1, np.uint8)
        self.ctx._check(self._L.dgrep_job_add(self._h, ctypes.c_void_p(buf.ctypes.data), len(raw), name, len(name)))

    def begin(self, filename):
        name = self._bytes(filename)
        self.ctx._check(self._L.dgrep_job_file_begin(self._h, name, len(name)))

    def feed(self, piece):
        raw = self._bytes(piece)
        buf = np.frombuffer(raw, dtype=np.uint8) if len(raw) else np.zeros(1, np.uint8)
        self.ctx._check(self._L.dgrep_job_file_feed(self._h, ctypes.c_void_p(buf.ctypes.data), len(raw)))

    def end(self):
        self.ctx._check(self._L.dgrep_job_file_end(self._h))

    def finish(self) -> List[bytes]:
        res = _ReduceBatchOut()
        self.ctx._check(self._L.dgrep_job_finish(self._h, ctypes.byref(res)))
        return self.ctx._reduce_batch_parts(res)

    def stats(self) -> dict:
        """dgrep_job_stats_get: files, packs, files by route, windows, rows,
        segments, arena bytes used and allocated, the window buffers' bytes,
        long values, arena growths, device ms of scan / encode / append /
        reduce."""
        st = _JobStats()
        self.ctx._check(self._L.dgrep_job_stats_get(self._h, ctypes.byref(st), ctypes.sizeof(st)))
        return {f: getattr(st, f) for f, _ in _JobStats._fields_}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value and self.ctx._h.value:
            self._L.dgrep_job_close(self._h)
        self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_info() -> str:
    """dgrep_build_info(): "head=<commit>[-dirty] arch=gfx950 hipflags=..."."""
    return lib().dgrep_build_info().decode()


def synth_corpus_host(n: int, seed: int, kind: int = 0) -> bytes:
    """CPU twin of dgrep_synth_corpus (same generator code, synth.h)."""
    out = ctypes.create_string_buffer(max(n, 1))
    rc = lib().dgrep_synth_corpus_host(out, n, seed, kind)
    if rc != DGREP_OK:
        raise DgrepError(rc, "synth")
    return out.raw[:n]


def synth_keywords(seed: int, count: int = 1000) -> List[bytes]:
    out = []
    buf = ctypes.create_string_buffer(16)
    for i in range(count):
        k = lib().dgrep_synth_keyword(seed, i, buf)
        out.append(buf.raw[:k])
    return out


# ---- the plugin surface (application/grep.go) --------------------------------

pattern: str = os.environ.get("DGREP_PATTERN", "")  # grep.go:11 `var pattern string = ""`

class Comm:
    """The C ABI's multi-GPU exchange (include/dgrep.h, dgrep_comm_*): an RCCL
    communicator on a Context's device and stream. Rank 0 (or any one rank)
    makes the id with :meth:`unique_id` and hands the 128 bytes to the others;
    every rank then constructs a Comm (collective)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        rc = lib().dgrep_comm_unique_id(buf)
        if rc != DGREP_OK:
            raise DgrepError(rc, "dgrep_comm_unique_id failed")
        return buf.raw

    def __init__(self, ctx: "Context", uid: bytes, nranks: int, rank: int):
        self._L = lib()
        self.ctx, self.nranks, self.rank = ctx, nranks, rank
        h = ctypes.c_void_p()
        rc = self._L.dgrep_comm_open(ctx._h, ctypes.create_string_buffer(bytes(uid), COMM_ID_BYTES), nranks, rank,
                                     ctypes.byref(h))
        self._h = h
        if rc != DGREP_OK:
            msg = self._err()
            self.close()
            raise DgrepError(rc, msg)

    def _err(self) -> str:
        m = self._L.dgrep_comm_last_error(self._h) if self._h else None
        return m.decode(errors="replace") if m else ""

    def gather_device(self, d_line: int, d_start: int, d_len: int, count: int, split: int = 0, root: int = 0):
        """dgrep_gather_records_device: (device pointer of the packed 28-B
        records, total, per-rank counts) on the root; (None, count, None) elsewhere."""
        ptr = ctypes.c_void_p()
        total = ctypes.c_uint64()
        counts = (ctypes.c_uint64 * self.nranks)()
        rc = self._L.dgrep_gather_records_device(self._h, d_line, d_start, d_len, count, split & 0xFFFFFFFF, root,
                                                 ctypes.byref(ptr), ctypes.byref(total), counts)
        if rc != DGREP_OK:
            raise DgrepError(rc, self._err())
        if self.rank != root:
            return None, total.value, None
        return ptr.value, total.value, list(counts)

    def gather(self, d_line: int, d_start: int, d_len: int, count: int, split: int = 0, root: int = 0):
        """dgrep_gather_records: (line_no, start, len, split) numpy arrays on the
        root (rank order), None elsewhere."""
        g = _Gathered()
        rc = self._L.dgrep_gather_records(self._h, d_line, d_start, d_len, count, split & 0xFFFFFFFF, root,
                                          ctypes.byref(g))
        if rc != DGREP_OK:
            raise DgrepError(rc, self._err())
        try:
            if self.rank != root:
                return None
            n = g.count
            arr = lambda p, t: np.ctypeslib.as_array(p, shape=(n,)).astype(t) if n else np.zeros(0, t)
            return (arr(g.line_no, np.uint64), arr(g.start, np.uint64), arr(g.len, np.uint64),
                    arr(g.split, np.uint32))
        finally:
            self._L.dgrep_gathered_free(ctypes.byref(g))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.dgrep_comm_close(self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ctx_local = threading.local()


def set_pattern(p: str):
    global pattern
    pattern = p


def pick_device(worker_id: int = -1) -> int:
    """dgrep_pick_device: DGREP_DEVICE, else worker_id % device count (worker_id
    < 0: DGREP_WORKER_ID, else the process id). Raises if the device is absent."""
    d = ctypes.c_int()
    rc = lib().dgrep_pick_device(worker_id, ctypes.byref(d))
    if rc != DGREP_OK:
        raise DgrepError(rc, "no such device (DGREP_DEVICE=%r, worker %d)" % (os.environ.get("DGREP_DEVICE"), worker_id))
    return d.value


def _default_device() -> int:
    """The module-level Map's device: the worker rule (pick_device) only when
    DGREP_DEVICE or DGREP_WORKER_ID says which worker this is; otherwise device
    0, as before round 3 (never a device that depends on the process id, which
    could differ from the caller's torch device)."""
    if os.environ.get("DGREP_DEVICE") or os.environ.get("DGREP_WORKER_ID"):
        return pick_device()
    return 0


def _context() -> Context:
    ctx = getattr(_ctx_local, "ctx", None)
    if ctx is None:
        ctx = Context(_default_device())
        _ctx_local.ctx = ctx
        _ctx_local.loaded = None
    if _ctx_local.loaded != pattern:
        ctx.load(pattern)
        _ctx_local.loaded = pattern
    return ctx


def format_key(filename: str, line_no: int) -> str:
    """fmt.Sprintf("%s (line number #%v)", filename, line_number+1) (grep.go:25)."""
    return "%s (line number #%d)" % (filename, line_no)


def Map(filename: str, contents) -> List[KeyValue]:
    """grep.go:13-36 on the GPU: matching lines of `contents`, in line order."""
    raw = contents.encode("utf-8", "surrogateescape") if isinstance(contents, str) else bytes(contents)
    ln, st, le = _context().scan(raw)
    kva = []
    for n, s, l in zip(ln.tolist(), st.tolist(), le.tolist()):
        v = raw[s:s + l]
        kva.append(KeyValue(format_key(filename, n), v.decode("utf-8", "surrogateescape")
                            if isinstance(contents, str) else v))
    return kva


def MapStream(filename: str, pieces, window: int = 64 << 20) -> List[KeyValue]:
    """Map(filename, b"".join(pieces)) for a worker that reads its task file
    piece by piece and never holds it whole (dgrep_stream_*): every piece is fed
    as it comes, and the Values are the line bytes the device gathered, not
    slices of host copies of the pieces. `pieces`: an iterable of bytes (Values
    are bytes) or of str (Values are str)."""
    kva = []
    text = False
    with _context().stream(window, values=True) as st:
        def take(res):
            ln, _, _, vals = res
            for n, v in zip(ln.tolist(), vals):
                kva.append((n, v))
        for piece in pieces:
            text = text or isinstance(piece, str)
            take(st.feed(piece))
        take(st.finish())
    return [KeyValue(format_key(filename, n), v.decode("utf-8", "surrogateescape") if text else v) for n, v in kva]


def MapPartitionsStream(filename, pieces, nreduce: int, window: int = 64 << 20) -> List[bytes]:
    """The map task of a worker that reads its file piece by piece, with the set
    pattern (dgrep_stream_*_partitions): element p is the byte content of
    mr-<task>-<p>, equal to Context.map_partitions(filename, b"".join(pieces),
    nreduce). Every piece is fed as it comes; the key formatting, ihash, JSON
    escaping and partitioning happen on the device, window by window."""
    parts = [[] for _ in range(nreduce)]
    with _context().partition_stream(window, filename, nreduce) as st:
        def take(rows):
            for row in rows:
                for p, cell in enumerate(row):
                    parts[p].append(cell)
        for piece in pieces:
            take(st.feed(piece))
        take(st.finish())
    return [b"".join(x) for x in parts]


def MapBatch(files: Sequence[Tuple[str, object]]) -> List[List[KeyValue]]:
    """[Map(f, c) for f, c in files] in one scan (dgrep_scan_batch): a worker
    that has read several input files (one map task each,
    map_reduce/coordinator.go:312,329-333) hands them over together. No file:
    [] without touching the GPU."""
    files = list(files)
    if not files:
        return []
    raws = [c.encode("utf-8", "surrogateescape") if isinstance(c, str) else bytes(c) for _, c in files]
    ln, st, le, _, sb = _context().scan_batch(raws)
    ln, st, le, sb = ln.tolist(), st.tolist(), le.tolist(), sb.tolist()
    out = []
    for i, (filename, contents) in enumerate(files):
        raw, text = raws[i], isinstance(contents, str)
        kva = []
        for r in range(sb[i], sb[i + 1]):
            v = raw[st[r]:st[r] + le[r]]
            kva.append(KeyValue(format_key(filename, ln[r]), v.decode("utf-8", "surrogateescape") if text else v))
        out.append(kva)
    return out


def GrepJob(files: Sequence[Tuple[str, object]], nreduce: int) -> List[bytes]:
    """The whole job for the files a worker holds, with the set pattern
    (dgrep_grep_job): element r is the content of mr-out-<r>, the "key value\n"
    lines map_reduce/worker.go:161-165 writes. No file: [] without touching the
    GPU."""
    files = list(files)
    if not files:
        return []
    return _context().grep_job(files, nreduce)


def GrepJobWindowed(files: Sequence[Tuple[str, object]], nreduce: int, window: int = 64 << 20) -> List[bytes]:
    """GrepJob for files of any size, with the set pattern (dgrep_job_*): a
    file's contents may be bytes / str, or an iterable of pieces that is fed as
    it comes and never held as a whole. Element r is the content of mr-out-<r>;
    the lines read per partition are left in the context's last_lines_in. No
    file: [] without touching the GPU."""
    files = list(files)
    if not files:
        return []
    with _context().job(window, nreduce) as job:
        for filename, contents in files:
            if isinstance(contents, (bytes, bytearray, memoryview, str)):
                job.add(filename, contents)
                continue
            job.begin(filename)
            for piece in contents:
                job.feed(piece)
            job.end()
        return job.finish()


def Reduce(key: str, values: Sequence[str]) -> str:
    """grep.go:38-40."""
    return values[0]
