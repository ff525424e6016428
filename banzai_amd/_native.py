"""ctypes binding of libbzhip.so (include/bzhip.h).  No CPU fallback: if the library or a
gfx950 device is missing, calls raise."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# $BZH_LIB selects another build of the same library (A/B timing of kernel variants, scripts/ab.sh)
LIB_PATH = os.environ.get("BZH_LIB") or os.path.join(_HERE, "libbzhip.so")

u8p = ctypes.POINTER(ctypes.c_uint8)
u16p = ctypes.POINTER(ctypes.c_uint16)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
szp = ctypes.POINTER(ctypes.c_size_t)


class BzhError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        super().__init__(f"bzhip status {status}: {detail}")


class Block(ctypes.Structure):
    _fields_ = [("in_off", ctypes.c_uint64), ("in_len", ctypes.c_uint64), ("rle_len", ctypes.c_uint32),
                ("crc", ctypes.c_uint32)]


_BLOCK_DTYPE = np.dtype([("in_off", "<u8"), ("in_len", "<u8"), ("rle_len", "<u4"), ("crc", "<u4")])
assert _BLOCK_DTYPE.itemsize == ctypes.sizeof(Block)


class Stats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in
                ("ms_plan", "ms_rle1", "ms_bwt", "ms_mtf", "ms_huff", "ms_pack", "ms_total", "ms_bwt_sort")] + \
               [(k, ctypes.c_uint64) for k in
                ("bwt_sort_launches", "bwt_sort_elems", "raw_bytes", "rle_bytes", "mtf_syms", "out_bits",
                 "bwt_rounds", "bwt_active_sum")] + \
               [("blocks", ctypes.c_uint32), ("pad", ctypes.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class DecodeStats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("ms_scan", "ms_entropy", "ms_unbwt", "ms_unrle", "ms_crc", "ms_total")] + \
               [(k, ctypes.c_uint64) for k in ("streams", "blocks", "candidates", "candidates_off_chain", "in_bytes",
                                               "out_bytes")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DecodeManyStats(ctypes.Structure):
    """bzh_decode_many_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("inputs", "inputs_failed", "streams", "blocks", "blocks_small", "batches")] + \
               [("ms_unbwt_small", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class IndexEntry(ctypes.Structure):
    """bzh_index_entry: one decoded block of an indexed input"""
    _fields_ = [("bit_pos", ctypes.c_uint64), ("end_bit", ctypes.c_uint64), ("out_off", ctypes.c_uint64),
                ("out_len", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("stream", ctypes.c_uint32), ("level", ctypes.c_uint32)]


INDEX_DTYPE = np.dtype([("bit_pos", "<u8"), ("end_bit", "<u8"), ("out_off", "<u8"), ("out_len", "<u4"), ("crc", "<u4"),
                        ("stream", "<u4"), ("level", "<u4")])
assert INDEX_DTYPE.itemsize == ctypes.sizeof(IndexEntry) == 40
idxp = ctypes.POINTER(IndexEntry)


class RecoverEntry(ctypes.Structure):
    """bzh_recover_entry: one block magic of a damaged input, kept (kind 0) or lost"""
    _fields_ = [("bit_pos", ctypes.c_uint64), ("end_bit", ctypes.c_uint64), ("out_off", ctypes.c_uint64),
                ("out_len", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("err_bit", ctypes.c_uint64)]


RECOVER_DTYPE = np.dtype([("bit_pos", "<u8"), ("end_bit", "<u8"), ("out_off", "<u8"), ("out_len", "<u4"), ("crc", "<u4"),
                          ("kind", "<u4"), ("flags", "<u4"), ("err_bit", "<u8")])
assert RECOVER_DTYPE.itemsize == ctypes.sizeof(RecoverEntry) == 48
recp = ctypes.POINTER(RecoverEntry)
LOST_TRUNC, LOST_FORMAT, LOST_BLOCK_CRC, LOST_RANDOMISED = 2, 3, 4, 6
LOST_NAMES = {LOST_TRUNC: "truncated", LOST_FORMAT: "field outside the format", LOST_BLOCK_CRC: "block CRC mismatch",
              LOST_RANDOMISED: "randomised block"}
REC_JOINED, REC_STREAM_END, REC_STREAM_OK = 1, 2, 4


class RecoverStats(ctypes.Structure):
    """bzh_recover_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("candidates", "kept", "lost", "shadowed", "footers", "streams_ok", "batches",
                                               "out_bytes")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DStreamStats(ctypes.Structure):
    """bzh_dstream_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("passes", "blocks", "streams", "blocks_redone", "tail_moves", "window_grows",
                                               "staging_grows", "in_bytes", "out_bytes", "window_peak", "staging_peak")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SyncPoint(ctypes.Structure):
    """bzh_sync_point: the entropy stage's state at a group boundary inside a block"""
    _fields_ = [("bit_pos", ctypes.c_uint64), ("entry", ctypes.c_uint32), ("group", ctypes.c_uint32), ("out_pos", ctypes.c_uint32),
                ("run", ctypes.c_uint32), ("run_weight", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("mtf", ctypes.c_uint8 * 256)]


SYNC_DTYPE = np.dtype([("bit_pos", "<u8"), ("entry", "<u4"), ("group", "<u4"), ("out_pos", "<u4"), ("run", "<u4"),
                       ("run_weight", "<u4"), ("reserved", "<u4"), ("mtf", "u1", (256,))])
assert SYNC_DTYPE.itemsize == ctypes.sizeof(SyncPoint) == 288
syncp = ctypes.POINTER(SyncPoint)


class Range(ctypes.Structure):
    """bzh_range: output bytes [off, off + len)"""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64)]


RANGE_DTYPE = np.dtype([("off", "<u8"), ("len", "<u8")])
assert RANGE_DTYPE.itemsize == ctypes.sizeof(Range) == 16
rangep = ctypes.POINTER(Range)


class DecodeRangesStats(ctypes.Structure):
    """bzh_decode_ranges_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("ranges", "pieces", "blocks_touched", "blocks_whole", "batches")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Hit(ctypes.Structure):
    """bzh_hit: a match's offset in the output and, with SEARCH_RECORDS, the delimiters in front of it"""
    _fields_ = [("off", ctypes.c_uint64), ("record", ctypes.c_uint64)]


HIT_DTYPE = np.dtype([("off", "<u8"), ("record", "<u8")])
assert HIT_DTYPE.itemsize == ctypes.sizeof(Hit) == 16
hitp = ctypes.POINTER(Hit)
SEARCH_RECORDS = 1
SEARCH_MAX_PATTERN = 256


class SearchStats(ctypes.Structure):
    """bzh_search_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("hits", "windows", "tiles", "staging_peak")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GrepEntry(ctypes.Structure):
    """bzh_grep_entry: a selected record's number, its offset and length in the decoded output, and where it lies in `out`"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("record", "off", "len", "out_off")]


GREP_ENTRY_DTYPE = np.dtype([("record", "<u8"), ("off", "<u8"), ("len", "<u8"), ("out_off", "<u8")])
assert GREP_ENTRY_DTYPE.itemsize == ctypes.sizeof(GrepEntry) == 32
grepp = ctypes.POINTER(GrepEntry)
GREP_INVERT = 1
GREP_LEN_CONTEXT = 1 << 63  # BZH_GREP_LEN_CONTEXT: bit 63 of an entry's len marks a context record (bzh_grep_set_context)
GREP_CONTEXT_ENTRY_DTYPE = np.dtype(GREP_ENTRY_DTYPE.descr + [("context", "?")])


class PatsetInfo(ctypes.Structure):
    _fields_ = [("patterns", ctypes.c_uint64), ("distinct", ctypes.c_uint64), ("min_len", ctypes.c_uint32), ("max_len", ctypes.c_uint32),
                ("states", ctypes.c_uint32), ("classes", ctypes.c_uint32), ("table_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


SET_HIT_DTYPE = np.dtype([("off", "<u8"), ("record", "<u8"), ("pattern", "<u4"), ("len", "<u4")])  # bzh_set_hit
assert SET_HIT_DTYPE.itemsize == 24
PATSET_FOLD_ASCII = 1
PATSET_MAX_PATTERNS = 65536


class RegexInfo(ctypes.Structure):
    """bzh_regex_info"""
    _fields_ = [("expressions", ctypes.c_uint64), ("min_len", ctypes.c_uint32), ("max_len", ctypes.c_uint32), ("states", ctypes.c_uint32),
                ("classes", ctypes.c_uint32), ("unbounded", ctypes.c_uint32), ("in_lds", ctypes.c_uint32), ("table_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert ctypes.sizeof(RegexInfo) == 40


class RegexLook(ctypes.Structure):
    """bzh_regex_look"""
    _fields_ = [("look_behind", ctypes.c_uint32), ("look_ahead", ctypes.c_uint32), ("contexts", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


assert ctypes.sizeof(RegexLook) == 16
REGEX_ASSERT = 1  # the syntax word of the _ex calls, apart from the flags
REGEX_WORD = 2
REGEX_LINE = 4
REGEX_FOLD_ASCII = 1
REGEX_DOTALL = 2
REGEX_NO_LDS = 4
REGEX_MAX_SPAN = 256
REGEX_MAX_EXPR = 4096


class GrepStats(ctypes.Structure):
    """bzh_grep_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("records", "selected", "out_bytes", "windows", "tiles", "carry_peak", "staging_peak")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GrepManyItem(ctypes.Structure):
    """bzh_grep_many_item: what bzh_grep says of one input of a bzh_grep_many* call"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("decoded", "records", "selected", "out_bytes")] + \
               [("status", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


GREP_MANY_ITEM_DTYPE = np.dtype([("decoded", "<u8"), ("records", "<u8"), ("selected", "<u8"), ("out_bytes", "<u8"), ("status", "<i4"),
                                 ("reserved", "<u4")])
assert GREP_MANY_ITEM_DTYPE.itemsize == ctypes.sizeof(GrepManyItem) == 40
grepmanyp = ctypes.POINTER(GrepManyItem)


class GrepManyStats(ctypes.Structure):
    """bzh_grep_many_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("inputs", "inputs_failed", "segments", "virtual_tiles", "shared_tiles", "staging_retries")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GrepContextStats(ctypes.Structure):
    """bzh_grep_context_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("matched", "context", "groups", "pending_peak")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MatchEntry(ctypes.Structure):
    """bzh_match_entry: a selected match's offset in the decoded output, its record, pattern and length, and where it lies in `out`"""
    _fields_ = [("off", ctypes.c_uint64), ("record", ctypes.c_uint64), ("pattern", ctypes.c_uint32), ("len", ctypes.c_uint32),
                ("out_off", ctypes.c_uint64)]


MATCH_DTYPE = np.dtype([("off", "<u8"), ("record", "<u8"), ("pattern", "<u4"), ("len", "<u4"), ("out_off", "<u8")])
assert MATCH_DTYPE.itemsize == ctypes.sizeof(MatchEntry) == 32
matchp = ctypes.POINTER(MatchEntry)
MATCH_RECORDS = 1


class MatchStats(ctypes.Structure):
    """bzh_match_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("matches", "out_bytes", "candidates", "entered_tiles", "open_tiles", "windows", "tiles",
                                               "carry_peak", "staging_peak")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def grep_context_rows(ent):
    """entries as the C calls fill them -> GREP_CONTEXT_ENTRY_DTYPE: `len` the real length, `context` what bit 63 of it said"""
    out = np.zeros(ent.size, dtype=GREP_CONTEXT_ENTRY_DTYPE)
    for k in ("record", "off", "out_off"):
        out[k] = ent[k]
    out["len"] = ent["len"] & np.uint64(GREP_LEN_CONTEXT - 1)
    out["context"] = (ent["len"] >> np.uint64(63)) != 0
    return out


class KStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("ms", ctypes.c_double), ("launches", ctypes.c_uint64),
                ("alg_bytes", ctypes.c_uint64)]


# name -> (restype, argtypes); also the list the symbol-export test checks against include/bzhip.h
SIGNATURES = {
    "bzh_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "bzh_destroy": (None, [ctypes.c_void_p]),
    "bzh_arch_supported": (ctypes.c_int, [ctypes.c_char_p]),
    "bzh_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "bzh_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "bzh_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "bzh_set_profiling": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "bzh_set_lanes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "bzh_set_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "bzh_get_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Stats)]),
    "bzh_debug_fault": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "bzh_get_kernel_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(KStat), ctypes.c_size_t, szp]),
    "bzh_encode": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, szp, szp]),
    "bzh_encode_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                         ctypes.c_size_t, szp, szp]),
    "bzh_encode_many_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, szp, ctypes.c_size_t, ctypes.c_void_p,
                                              ctypes.c_size_t, szp, szp]),
    "bzh_encode_many": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(u8p), szp, ctypes.c_size_t, u8p, ctypes.c_size_t,
                                       szp, szp]),
    "bzh_encode_many_bound": (ctypes.c_size_t, [ctypes.c_int, szp, ctypes.c_size_t]),
    "bzh_plan_many_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, szp, ctypes.c_size_t, szp]),
    "bzh_encode_index_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, szp,
                                               szp, ctypes.c_uint32, idxp, ctypes.c_size_t, szp, syncp, ctypes.c_size_t, szp]),
    "bzh_encode_index": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, szp, szp, ctypes.c_uint32, idxp,
                                        ctypes.c_size_t, szp, syncp, ctypes.c_size_t, szp]),
    "bzh_encode_index_bound": (ctypes.c_int, [ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32, szp, szp]),
    "bzh_decode": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, szp, szp]),
    "bzh_decode_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                         ctypes.c_size_t, szp, szp]),
    "bzh_get_decode_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(DecodeStats)]),
    "bzh_decode_many_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, szp, szp, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int), szp]),
    "bzh_decode_many": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(u8p), szp, ctypes.c_size_t, u8p, ctypes.c_size_t, szp, szp,
                                       ctypes.POINTER(ctypes.c_int), szp]),
    "bzh_decode_many_small_max": (ctypes.c_size_t, []),
    "bzh_get_decode_many_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(DecodeManyStats)]),
    "bzh_recover_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, szp, recp,
                                          ctypes.c_size_t, szp]),
    "bzh_recover": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, szp, recp, ctypes.c_size_t, szp]),
    "bzh_get_recover_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RecoverStats)]),
    "bzh_recover_stream_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, recp, ctypes.c_size_t, ctypes.c_void_p,
                                                 ctypes.c_size_t, szp]),
    "bzh_recover_stream": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, recp, ctypes.c_size_t, u8p, ctypes.c_size_t, szp]),
    "bzh_decode_index": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, idxp, ctypes.c_size_t, szp, u64p, szp]),
    "bzh_decode_index_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, idxp, ctypes.c_size_t, szp,
                                               u64p, szp]),
    "bzh_decode_index_sync": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_uint32, idxp, ctypes.c_size_t, szp, syncp,
                                             ctypes.c_size_t, szp, u64p, szp]),
    "bzh_decode_index_sync_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, idxp,
                                                    ctypes.c_size_t, szp, syncp, ctypes.c_size_t, szp, u64p, szp]),
    "bzh_decode_range_sync": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_uint64, idxp, ctypes.c_size_t, syncp,
                                             ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, u8p, ctypes.c_size_t, szp]),
    "bzh_decode_range_sync_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, idxp,
                                                    ctypes.c_size_t, syncp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64,
                                                    ctypes.c_void_p, ctypes.c_size_t, szp]),
    "bzh_index_span": (ctypes.c_int, [idxp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, szp, szp, u64p, u64p]),
    "bzh_decode_range": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_uint64, idxp, ctypes.c_size_t,
                                        ctypes.c_uint64, ctypes.c_uint64, u8p, ctypes.c_size_t, szp]),
    "bzh_decode_range_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, idxp,
                                               ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.c_size_t, szp]),
    "bzh_index_spans": (ctypes.c_int, [idxp, ctypes.c_size_t, rangep, ctypes.c_size_t, u32p, ctypes.c_size_t, szp, u64p, u64p, u64p]),
    "bzh_decode_ranges": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_uint64, idxp, ctypes.c_size_t, syncp,
                                         ctypes.c_size_t, rangep, ctypes.c_size_t, u8p, ctypes.c_size_t, szp, szp, szp]),
    "bzh_decode_ranges_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, idxp,
                                                ctypes.c_size_t, syncp, ctypes.c_size_t, rangep, ctypes.c_size_t, ctypes.c_void_p,
                                                ctypes.c_size_t, szp, szp, szp]),
    "bzh_get_decode_ranges_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(DecodeRangesStats)]),
    "bzh_decode_index_records": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint8, idxp, ctypes.c_size_t,
                                                szp, syncp, ctypes.c_size_t, szp, u64p, ctypes.c_size_t, u64p, u64p, szp]),
    "bzh_decode_index_records_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint8,
                                                       idxp, ctypes.c_size_t, szp, syncp, ctypes.c_size_t, szp, u64p, ctypes.c_size_t, u64p,
                                                       u64p, szp]),
    "bzh_count_records_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint8, idxp, ctypes.c_size_t,
                                                u64p, u64p]),
    "bzh_record_spans": (ctypes.c_int, [idxp, ctypes.c_size_t, u64p, rangep, ctypes.c_size_t, u32p, ctypes.c_size_t, szp, u64p, u64p]),
    "bzh_decode_records": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_uint64, idxp, ctypes.c_size_t, syncp,
                                          ctypes.c_size_t, u64p, ctypes.c_uint8, rangep, ctypes.c_size_t, u8p, ctypes.c_size_t, szp, szp,
                                          szp]),
    "bzh_decode_records_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, idxp, ctypes.c_size_t,
                                                 syncp, ctypes.c_size_t, u64p, ctypes.c_uint8, rangep, ctypes.c_size_t, ctypes.c_void_p,
                                                 ctypes.c_size_t, szp, szp, szp]),
    "bzh_search_raw_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, u8p, ctypes.c_size_t, ctypes.c_uint,
                                             ctypes.c_uint8, hitp, ctypes.c_size_t, szp]),
    "bzh_search_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, u8p, ctypes.c_size_t, ctypes.c_uint,
                                         ctypes.c_uint8, hitp, ctypes.c_size_t, szp, u64p, szp]),
    "bzh_search": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint8, hitp,
                                  ctypes.c_size_t, szp, u64p, szp]),
    "bzh_search_range_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, idxp, ctypes.c_size_t,
                                               syncp, ctypes.c_size_t, u64p, ctypes.c_uint64, ctypes.c_uint64, u8p, ctypes.c_size_t,
                                               ctypes.c_uint, ctypes.c_uint8, hitp, ctypes.c_size_t, szp]),
    "bzh_search_range": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_uint64, idxp, ctypes.c_size_t, syncp,
                                        ctypes.c_size_t, u64p, ctypes.c_uint64, ctypes.c_uint64, u8p, ctypes.c_size_t, ctypes.c_uint,
                                        ctypes.c_uint8, hitp, ctypes.c_size_t, szp]),
    "bzh_grep_raw_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, u8p, ctypes.c_size_t, ctypes.c_uint,
                                           ctypes.c_uint8, ctypes.c_void_p, ctypes.c_size_t, grepp, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64)]),
    "bzh_grep_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, u8p, ctypes.c_size_t, ctypes.c_uint,
                                       ctypes.c_uint8, ctypes.c_void_p, ctypes.c_size_t, grepp, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.POINTER(ctypes.c_size_t)]),
    "bzh_grep": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint8, u8p,
                                ctypes.c_size_t, grepp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64),
                                ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)]),
    "bzh_grep_index_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, idxp, ctypes.c_size_t, syncp,
                                             ctypes.c_size_t, u8p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint8, ctypes.c_void_p,
                                             ctypes.c_size_t, grepp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                             ctypes.POINTER(ctypes.c_uint64)]),
    "bzh_grep_index": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, idxp, ctypes.c_size_t, syncp, ctypes.c_size_t, u8p,
                                      ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint8, u8p, ctypes.c_size_t, grepp, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64)]),
    "bzh_get_grep_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(GrepStats)]),
    "bzh_get_match_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MatchStats)]),
    "bzh_grep_set_context": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]),
    "bzh_get_grep_context_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(GrepContextStats)]),
    "bzh_patset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.c_size_t, ctypes.c_uint,
                                         ctypes.POINTER(ctypes.c_void_p)]),
    "bzh_patset_destroy": (None, [ctypes.c_void_p]),
    "bzh_patset_get_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PatsetInfo)]),
    "bzh_regex_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint32,
                                        ctypes.POINTER(ctypes.c_void_p)]),
    "bzh_regex_get_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RegexInfo)]),
    "bzh_regex_create_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint32,
                                           ctypes.c_uint, ctypes.POINTER(ctypes.c_void_p)]),
    "bzh_regex_check_ex": (ctypes.c_int, [ctypes.POINTER(ctypes.c_char_p), szp, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint32, ctypes.c_uint,
                                          ctypes.POINTER(RegexInfo), ctypes.POINTER(RegexLook), ctypes.c_char_p, ctypes.c_size_t]),
    "bzh_regex_get_look": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RegexLook)]),
    "bzh_regex_check": (ctypes.c_int, [ctypes.POINTER(ctypes.c_char_p), szp, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint32,
                                       ctypes.POINTER(RegexInfo), ctypes.c_char_p, ctypes.c_size_t]),
    "bzh_search_set_room": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    "bzh_get_search_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SearchStats)]),
    "bzh_decode_scan": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u64p, u8p, ctypes.c_size_t, szp]),
    "bzh_stream_begin": (ctypes.c_int, [ctypes.c_void_p]),
    "bzh_stream_feed": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, u8p, ctypes.c_size_t, szp]),
    "bzh_stream_bound": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_size_t]),
    "bzh_stream_set_chunk": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    "bzh_stream_consumed": (ctypes.c_size_t, [ctypes.c_void_p]),
    "bzh_stream_begin_index": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "bzh_stream_index_pending": (ctypes.c_int, [ctypes.c_void_p, szp, szp]),
    "bzh_stream_index_take": (ctypes.c_int, [ctypes.c_void_p, idxp, ctypes.c_size_t, szp, syncp, ctypes.c_size_t, szp]),
    "bzh_index_blob_size": (ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32]),
    "bzh_index_blob_write": (ctypes.c_int, [idxp, ctypes.c_size_t, syncp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, u8p,
                                            ctypes.c_size_t, szp]),
    "bzh_index_blob_read": (ctypes.c_int, [u8p, ctypes.c_size_t, idxp, ctypes.c_size_t, szp, syncp, ctypes.c_size_t, szp, u32p, u64p]),
    "bzh_dstream_set_room": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t]),
    "bzh_dstream_begin": (ctypes.c_int, [ctypes.c_void_p]),
    "bzh_dstream_feed": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, szp, u8p, ctypes.c_size_t, szp,
                                        ctypes.POINTER(ctypes.c_int)]),
    "bzh_dstream_consumed": (ctypes.c_size_t, [ctypes.c_void_p]),
    "bzh_dstream_get_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(DStreamStats)]),
    "bzh_dstream_end": (ctypes.c_int, [ctypes.c_void_p]),
    "bzh_plan_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, szp]),
    "bzh_plan_tables_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "bzh_plan_split_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, szp]),
    "bzh_plan_blocks": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Block), ctypes.c_size_t]),
    "bzh_plan_device_nocrc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, szp]),
    "bzh_plan_crc_range": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t]),
    "bzh_plan_open": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t]),
    "bzh_encode_range_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                                               ctypes.c_size_t, u64p]),
    "bzh_assemble_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), u64p, ctypes.c_size_t,
                                           u32p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, szp]),
    "bzh_create_multi": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int]),
    "bzh_destroy_multi": (None, [ctypes.c_void_p]),
    "bzh_multi_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "bzh_multi_device_count": (ctypes.c_int, [ctypes.c_void_p]),
    "bzh_multi_encode": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, szp, szp]),
    "bzh_multi_load": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t]),
    "bzh_multi_run": (ctypes.c_int, [ctypes.c_void_p, szp]),
    "bzh_multi_fetch": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t]),
    "bzh_multi_output_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "bzh_multi_times": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_size_t]),
    "bzh_multi_debug_slab": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    "bzh_rle1_split": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.POINTER(Block), ctypes.c_size_t,
                                      szp, u8p, ctypes.c_size_t]),
    "bzh_crc32": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u32p]),
    "bzh_bwt_batch": (ctypes.c_int, [ctypes.c_void_p, u8p, u64p, u32p, ctypes.c_size_t, u8p, u32p, u8p]),
    "bzh_unbwt_batch": (ctypes.c_int, [ctypes.c_void_p, u8p, u64p, u32p, u32p, ctypes.c_size_t, u8p]),
    "bzh_bwt_roundtrip_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, u64p]),
    "bzh_bwt": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, u32p, u8p]),
    "bzh_mtf": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p, u16p, szp, u32p, u32p]),
    "bzh_mtf_batch": (ctypes.c_int, [ctypes.c_void_p, u8p, u64p, u32p, ctypes.c_size_t, u8p, u16p, u32p, u32p, u32p]),
    "bzh_huffman": (ctypes.c_int, [ctypes.c_void_p, u16p, ctypes.c_size_t, ctypes.c_uint32, u32p, u8p,
                                   ctypes.c_size_t, u64p, u8p, u32p]),
}


def build(force=False):
    """Compile libbzhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "bzhip.h"))
    newest = max(os.path.getmtime(s) for s in srcs)
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < newest:
        subprocess.check_call(["make", "-C", src_dir, "-s", "-j4"])
    return LIB_PATH


_lib = None
MISSING = []


def encode_many_bound(level, lens):
    """bzh_encode_many_bound: upper bound of the output of bzh_encode_many for these input lengths (0 for a bad level)"""
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    return int(lib().bzh_encode_many_bound(level, ptr(lens, szp) if lens.size else None, lens.size))


def decode_many_small_max():
    """bzh_decode_many_small_max (pure host): the largest block, in bytes of its last column, the LDS inverse BWT takes"""
    return int(lib().bzh_decode_many_small_max())


def encode_index_bound(level, n, interval):
    """bzh_encode_index_bound (host arithmetic, no GPU): (entries, sync points) that bzh_encode_index never exceeds"""
    me, mp = ctypes.c_size_t(0), ctypes.c_size_t(0)
    st = lib().bzh_encode_index_bound(level, n, interval, ctypes.byref(me), ctypes.byref(mp))
    if st != 0:
        raise BzhError(st, lib().bzh_strerror(st).decode())
    return int(me.value), int(mp.value)


def _entries(entries):
    """a contiguous array of the 40-byte entries (no copy when it already is one) and its ctypes pointer"""
    e = np.ascontiguousarray(entries, dtype=INDEX_DTYPE)
    return e, (e.ctypes.data_as(idxp) if e.size else None)


def _report(entries):
    """a contiguous array of the 48-byte recovery entries and its ctypes pointer"""
    e = np.ascontiguousarray(entries, dtype=RECOVER_DTYPE)
    return e, (e.ctypes.data_as(recp) if e.size else None)


def _points(points):
    """a contiguous array of the 288-byte sync points and its ctypes pointer"""
    p = np.ascontiguousarray(points, dtype=SYNC_DTYPE)
    return p, (p.ctypes.data_as(syncp) if p.size else None)


def _points_or_none(points):
    """_points; None: no points"""
    return _points(points) if points is not None else (np.empty(0, SYNC_DTYPE), None)


def _input(data):
    """the bytes of any buffer as a contiguous uint8 array without a copy (of an empty one: a byte nobody reads), and their number"""
    a = np.frombuffer(data, dtype=np.uint8)
    return (np.ascontiguousarray(a) if a.size else np.zeros(1, np.uint8)), a.size


def index_blob_write(entries, points=None, interval=0, consumed=0):
    """bzh_index_blob_write (pure host): the index file of these arrays -> bytes; interval 0: a block index blob (no points)"""
    e, ep = _entries(entries)
    q, qp = _points_or_none(points)
    need = int(lib().bzh_index_blob_size(e.size, q.size, interval))
    out = np.empty(max(need, 1), dtype=np.uint8)
    olen = ctypes.c_size_t(0)
    st = lib().bzh_index_blob_write(ep, e.size, qp, q.size, interval, consumed, ptr(out), need, ctypes.byref(olen))
    if st != 0:
        raise BzhError(st, lib().bzh_strerror(st).decode())
    return out[:olen.value].tobytes()


def index_blob_read_raw(blob, max_entries, max_pts):
    """one bzh_index_blob_read call with arrays of the given room -> (status, entries, points, count, npts, interval, consumed);
    nothing is raised, the arrays are cut to the counts only on status 0"""
    a = np.frombuffer(bytes(blob), dtype=np.uint8)
    ent = np.zeros(max(max_entries, 1), dtype=INDEX_DTYPE)
    pts = np.zeros(max(max_pts, 1), dtype=SYNC_DTYPE)
    cnt, npts, iv, cons = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    st = lib().bzh_index_blob_read(ptr(a) if a.size else ptr(np.zeros(1, np.uint8)), a.size,
                                   ent.ctypes.data_as(idxp) if max_entries else None, max_entries, ctypes.byref(cnt),
                                   pts.ctypes.data_as(syncp) if max_pts else None, max_pts, ctypes.byref(npts), ctypes.byref(iv),
                                   ctypes.byref(cons))
    if st == 0:
        ent, pts = ent[:cnt.value], pts[:npts.value]
    return st, ent, pts, int(cnt.value), int(npts.value), int(iv.value), int(cons.value)


def index_blob_read(blob):
    """bzh_index_blob_read (pure host): (entries, points, interval, consumed) of an index file of either kind (a block index:
    no points, interval 0); BzhError -6 for what is not a whole, undamaged blob"""
    st, ent, pts, cnt, npts, iv, cons = index_blob_read_raw(blob, 0, 0)  # (sizes; an empty index is read by this call)
    if st == -4:
        st, ent, pts, cnt, npts, iv, cons = index_blob_read_raw(blob, cnt, npts)
    if st != 0:
        raise BzhError(st, lib().bzh_strerror(st).decode())
    return ent.copy(), pts.copy(), iv, cons


def index_span(entries, off, length):
    """bzh_index_span (host arithmetic, no GPU): (first, last, byte_lo, byte_hi) -- the entries [first, last) that output bytes
    [off, off + length) touch, and the bytes of the indexed input that hold them"""
    if off < 0 or length < 0:
        raise ValueError("offset and length must not be negative")
    e, p = _entries(entries)
    first, last = ctypes.c_size_t(0), ctypes.c_size_t(0)
    lo, hi = ctypes.c_uint64(0), ctypes.c_uint64(0)
    st = lib().bzh_index_span(p, e.size, off, length, ctypes.byref(first), ctypes.byref(last), ctypes.byref(lo), ctypes.byref(hi))
    if st != 0:
        raise BzhError(st, lib().bzh_strerror(st).decode())
    return int(first.value), int(last.value), int(lo.value), int(hi.value)


def _ranges(ranges):
    """a contiguous array of the 16-byte ranges, from (off, len) pairs or such an array, and its ctypes pointer; len saturates
    at 2^64 - 1"""
    if isinstance(ranges, np.ndarray) and ranges.dtype == RANGE_DTYPE:
        r = np.ascontiguousarray(ranges)
    else:
        pairs = list(ranges)
        r = np.empty(len(pairs), dtype=RANGE_DTYPE)
        for k, pair in enumerate(pairs):
            off, length = pair
            for v in (off, length):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    raise TypeError(f"a range is a pair of ints, not {type(v).__name__}")
            if off < 0 or length < 0:
                raise ValueError("offset and length must not be negative")
            r[k] = (min(int(off), 2**64 - 1), min(int(length), 2**64 - 1))
    return r, (r.ctypes.data_as(rangep) if r.size else None)


def index_spans(entries, ranges):
    """bzh_index_spans (host arithmetic, no GPU): (touched, byte_lo, byte_hi, out_total) -- the entries the ranges touch,
    ascending and unique, as a uint32 array; the hull of their bytes in the indexed input; the bytes the ranges hold"""
    e, p = _entries(entries)
    r, rp = _ranges(ranges)
    cnt, lo, hi, total = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    touched = np.empty(max(int(e.size), 1), dtype=np.uint32)  # (the list is unique: never more than the entries)
    st = lib().bzh_index_spans(p, e.size, rp, r.size, ptr(touched, u32p), e.size, ctypes.byref(cnt), ctypes.byref(lo), ctypes.byref(hi),
                               ctypes.byref(total))
    if st != 0:
        raise BzhError(st, lib().bzh_strerror(st).decode())
    return touched[:cnt.value].copy(), int(lo.value), int(hi.value), int(total.value)


def _table(entries, rec_cum):
    """the record table beside `entries` as a contiguous uint64 array of entries + 1 words, and its ctypes pointer"""
    t = np.ascontiguousarray(rec_cum, dtype=np.uint64)
    if t.ndim != 1 or t.size != len(entries) + 1:
        raise ValueError(f"a record table of {t.size} words beside {len(entries)} entries (one more is needed)")
    return t, t.ctypes.data_as(u64p)


def record_spans(entries, rec_cum, ranges):
    """bzh_record_spans (host arithmetic, no GPU): (touched, byte_lo, byte_hi) -- the entries a read of these (first record,
    count) ranges must decode, ascending and unique, and the hull of their compressed bytes"""
    e, p = _entries(entries)
    t, tp = _table(e, rec_cum)
    r, rp = _ranges(ranges)
    cnt, lo, hi = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    touched = np.empty(max(int(e.size), 1), dtype=np.uint32)
    st = lib().bzh_record_spans(p, e.size, tp, rp, r.size, ptr(touched, u32p), e.size, ctypes.byref(cnt), ctypes.byref(lo), ctypes.byref(hi))
    if st != 0:
        raise BzhError(st, lib().bzh_strerror(st).decode())
    return touched[:cnt.value].copy(), int(lo.value), int(hi.value)


# bzh_match*: a grep's arguments with bzh_match_entry in place of bzh_grep_entry
for _name in ("raw_device", "device", "", "index_device", "index"):
    _res, _args = SIGNATURES["bzh_grep" + ("_" + _name if _name else "")]
    SIGNATURES["bzh_match" + ("_" + _name if _name else "")] = (_res, [matchp if a is grepp else a for a in _args])


def _patset_twin(name):
    """bzh_search* -> bzh_search_patset*, bzh_grep* -> bzh_grep_patset*, bzh_match* -> bzh_match_patset*,
    bzh_grep_many* -> bzh_grep_many_patset*"""
    for stem in ("bzh_grep_many", "bzh_search", "bzh_grep", "bzh_match"):
        if name.startswith(stem):
            return stem + "_patset" + name[len(stem):]
    return name


# bzh_grep_many*: many texts or inputs, what is looked for, the rooms, one item per input, the counts
_many_tail = [u8p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_size_t, grepp, ctypes.c_size_t, grepmanyp, szp, u64p]
SIGNATURES["bzh_grep_many_raw_device"] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, szp, szp, ctypes.c_size_t] + _many_tail)
SIGNATURES["bzh_grep_many_device"] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, szp, szp, ctypes.c_size_t] + _many_tail)
SIGNATURES["bzh_grep_many"] = (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(u8p), szp, ctypes.c_size_t] + _many_tail)
SIGNATURES["bzh_get_grep_many_stats"] = (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(GrepManyStats)])

# the calls that take a set: their twin's arguments with (pat, plen) replaced by the set, and the hits by bzh_set_hit
for _name in ("bzh_search_raw_device", "bzh_search_device", "bzh_search", "bzh_search_range_device", "bzh_search_range",
              "bzh_grep_raw_device", "bzh_grep_device", "bzh_grep", "bzh_grep_index_device", "bzh_grep_index",
              "bzh_grep_many_raw_device", "bzh_grep_many_device", "bzh_grep_many",
              "bzh_match_raw_device", "bzh_match_device", "bzh_match", "bzh_match_index_device", "bzh_match_index"):
    _res, _args = SIGNATURES[_name]
    _at = next(k for k in range(len(_args) - 1) if _args[k] is u8p and _args[k + 1] is ctypes.c_size_t and _args[k + 2] is ctypes.c_uint)
    SIGNATURES[_patset_twin(_name)] = (_res, [ctypes.c_void_p if a is hitp else a for a in _args[:_at] + [ctypes.c_void_p] + _args[_at + 2:]])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BzhError(-3, f"{LIB_PATH} is missing: build it with banzai_amd._native.build() "
                               "(there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                MISSING.append(name)  # the export test requires this list to stay empty
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def ptr(a, t=u8p):
    return a.ctypes.data_as(t)


class PatternSet:
    """A compiled set of patterns on the device of `ctx` (bzh_patset_create / bzh_patset_destroy): what the search and grep
    calls of a Context take in place of one pattern.  It outlives the context it was made with."""

    def __init__(self, ctx, patterns, ignore_case=False, flags=None, regex=False, max_span=0, syntax=0):
        """regex: `patterns` are regular expressions (bzh_regex_create; flags: BZH_REGEX_*), .info is bzh_regex_info's and
        bzh_regex_look's.  syntax: REGEX_ASSERT / REGEX_WORD / REGEX_LINE (bzh_regex_create_ex); 0 is bzh_regex_create itself, which
        refuses every assertion"""
        self._h = None
        self._destroy = lib().bzh_patset_destroy  # kept so that close() still works during interpreter shutdown
        pats = [bytes(p) for p in patterns]
        arr = (ctypes.c_char_p * max(len(pats), 1))(*pats)
        lens = np.array([len(p) for p in pats] or [0], dtype=np.uintp)
        h = ctypes.c_void_p()
        fl = ((REGEX_FOLD_ASCII if regex else PATSET_FOLD_ASCII) if ignore_case else 0) if flags is None else flags
        if regex and syntax:
            ctx.check(lib().bzh_regex_create_ex(ctx.handle, arr, ptr(lens, szp), len(pats), fl, max_span, syntax, ctypes.byref(h)))
        elif regex:
            ctx.check(lib().bzh_regex_create(ctx.handle, arr, ptr(lens, szp), len(pats), fl, max_span, ctypes.byref(h)))
        else:
            ctx.check(lib().bzh_patset_create(ctx.handle, arr, ptr(lens, szp), len(pats), fl, ctypes.byref(h)))
        self._h = h
        i = RegexInfo() if regex else PatsetInfo()
        ctx.check((lib().bzh_regex_get_info if regex else lib().bzh_patset_get_info)(h, ctypes.byref(i)))
        self.info = i.as_dict()
        if regex:
            look = RegexLook()
            ctx.check(lib().bzh_regex_get_look(h, ctypes.byref(look)))
            self.info.update(look.as_dict())

    @property
    def handle(self):
        if not self._h:
            raise ValueError("the pattern set is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Context:
    """One context per GPU (bzh_create / bzh_destroy)."""

    def __init__(self, device=0, level=9, max_batch=0):
        self._h = ctypes.c_void_p()
        self.level = level
        self._destroy = lib().bzh_destroy  # kept so that close() still works during interpreter shutdown
        st = lib().bzh_create(ctypes.byref(self._h), device, level, max_batch)
        if st != 0:
            self._h = None
            raise BzhError(st, lib().bzh_strerror(st).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, st):
        if st != 0:
            raise BzhError(st, lib().bzh_strerror(st).decode() + ": " + lib().bzh_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr):
        self.check(lib().bzh_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def set_profiling(self, on=True):
        self.check(lib().bzh_set_profiling(self._h, 1 if on else 0))

    def set_mode(self, fixed):
        """False: the reference's Huffman behaviour (default, bit-identical); True: the opt-in "fixed" mode"""
        self.check(lib().bzh_set_mode(self._h, 1 if fixed else 0))

    def set_lanes(self, lanes):
        self.check(lib().bzh_set_lanes(self._h, lanes))

    def stats(self):
        s = Stats()
        self.check(lib().bzh_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def debug_fault(self, kind):
        self.check(lib().bzh_debug_fault(self._h, kind))

    def kernel_stats(self):
        """Per-kernel-class (name, ms, launches, algorithmic bytes) of the last call made with profiling on."""
        arr = (KStat * 64)()
        cnt = ctypes.c_size_t(0)
        self.check(lib().bzh_get_kernel_stats(self._h, arr, 64, ctypes.byref(cnt)))
        return [{"name": arr[k].name.decode(), "ms": arr[k].ms, "launches": int(arr[k].launches),
                 "alg_bytes": int(arr[k].alg_bytes)} for k in range(cnt.value)]

    # ---- stage seams (host numpy in / out) ----
    def bwt(self, data):
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n = a.size
        src = np.ascontiguousarray(a) if n else np.zeros(1, np.uint8)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        p = ctypes.c_uint32(0)
        hb = np.zeros(256, dtype=np.uint8)
        self.check(lib().bzh_bwt(self._h, ptr(src), n, ptr(out), ctypes.byref(p), ptr(hb)))
        return out[:n].tobytes(), int(p.value), hb

    def bwt_batch(self, blocks):
        lens = np.array([len(b) for b in blocks], dtype=np.uint32)
        offs = np.zeros(len(blocks), dtype=np.uint64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        cat = np.frombuffer(b"".join(bytes(b) for b in blocks), dtype=np.uint8).copy()
        out = np.zeros_like(cat)
        ptrs = np.zeros(len(blocks), dtype=np.uint32)
        hb = np.zeros(len(blocks) * 256, dtype=np.uint8)
        self.check(lib().bzh_bwt_batch(self._h, ptr(cat), ptr(offs, u64p), ptr(lens, u32p), len(blocks), ptr(out),
                                       ptr(ptrs, u32p), ptr(hb)))
        res = []
        for k in range(len(blocks)):
            o = int(offs[k])
            res.append((out[o:o + int(lens[k])].tobytes(), int(ptrs[k]), hb[k * 256:(k + 1) * 256].copy()))
        return res

    def unbwt_batch(self, blocks):
        """blocks: [(bwt bytes, ptr)] -> [original bytes], computed on the GPU (bzh_unbwt_batch)"""
        lens = np.array([len(b) for b, _ in blocks], dtype=np.uint32)
        ptrs = np.array([p for _, p in blocks], dtype=np.uint32)
        offs = np.zeros(len(blocks), dtype=np.uint64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        cat = np.frombuffer(b"".join(bytes(b) for b, _ in blocks), dtype=np.uint8).copy()
        out = np.zeros_like(cat)
        self.check(lib().bzh_unbwt_batch(self._h, ptr(cat), ptr(offs, u64p), ptr(lens, u32p), ptr(ptrs, u32p),
                                         len(blocks), ptr(out)))
        return [out[int(offs[k]):int(offs[k]) + int(lens[k])].tobytes() for k in range(len(blocks))]

    def bwt_roundtrip_device(self, b0, b1):
        """forward + inverse BWT of plan blocks [b0, b1) on the device -> number of mismatching bytes"""
        bad = ctypes.c_uint64(0)
        self.check(lib().bzh_bwt_roundtrip_device(self._h, b0, b1, ctypes.byref(bad)))
        return int(bad.value)

    def mtf(self, bwt_bytes, has_byte):
        a = np.frombuffer(bytes(bwt_bytes), dtype=np.uint8).copy()
        n = a.size
        hb = np.ascontiguousarray(has_byte, dtype=np.uint8)
        syms = np.zeros(n + 2, dtype=np.uint16)
        freqs = np.zeros(258, dtype=np.uint32)
        m = ctypes.c_size_t(0)
        ns = ctypes.c_uint32(0)
        self.check(lib().bzh_mtf(self._h, ptr(a), n, ptr(hb), ptr(syms, u16p), ctypes.byref(m), ptr(freqs, u32p),
                                 ctypes.byref(ns)))
        return syms[:m.value].copy(), freqs, int(ns.value)

    def mtf_batch(self, cols):
        """cols: [(column bytes, has_byte)] -> [(syms, freqs, num_syms)], all columns in one launch (bzh_mtf_batch): their
        number decides the tile of the walk, 4,096 bytes from 64 columns on"""
        B = len(cols)
        lens = np.array([len(c) for c, _ in cols], dtype=np.uint32)
        offs = np.zeros(max(B, 1), dtype=np.uint64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        cat = np.frombuffer(b"".join(bytes(c) for c, _ in cols) or b"\0", dtype=np.uint8).copy()
        hb = np.zeros(max(B, 1) * 256, dtype=np.uint8)
        for k, (_, h) in enumerate(cols):
            hb[k * 256:(k + 1) * 256] = np.asarray(h, dtype=np.uint8)
        syms = np.zeros(int(lens.sum()) + B + 1, dtype=np.uint16)
        m = np.zeros(max(B, 1), dtype=np.uint32)
        freqs = np.zeros(max(B, 1) * 258, dtype=np.uint32)
        ns = np.zeros(max(B, 1), dtype=np.uint32)
        lens_p = lens if B else np.zeros(1, np.uint32)
        self.check(lib().bzh_mtf_batch(self._h, ptr(cat), ptr(offs, u64p), ptr(lens_p, u32p), B, ptr(hb), ptr(syms, u16p),
                                       ptr(m, u32p), ptr(freqs, u32p), ptr(ns, u32p)))
        res = []
        for k in range(B):
            o = int(offs[k]) + k
            res.append((syms[o:o + int(m[k])].copy(), freqs[k * 258:(k + 1) * 258].copy(), int(ns[k])))
        return res

    def huffman(self, syms, num_syms, freqs):
        s = np.ascontiguousarray(syms, dtype=np.uint16)
        f = np.ascontiguousarray(freqs, dtype=np.uint32)
        cap = s.size * 3 + 8192
        out = np.zeros(cap, dtype=np.uint8)
        lens = np.zeros(3 * 258, dtype=np.uint8)
        nb = ctypes.c_uint64(0)
        nt = ctypes.c_uint32(0)
        self.check(lib().bzh_huffman(self._h, ptr(s, u16p), s.size, num_syms, ptr(f, u32p), ptr(out), cap,
                                     ctypes.byref(nb), ptr(lens), ctypes.byref(nt)))
        return out[:(nb.value + 7) // 8].tobytes(), int(nb.value), lens.reshape(3, 258)[:nt.value].copy()

    def crc32(self, data):
        a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
        c = ctypes.c_uint32(0)
        self.check(lib().bzh_crc32(self._h, ptr(a), len(data), ctypes.byref(c)))
        return int(c.value)

    def rle1_split(self, data, want_bytes=True):
        """-> ([(in_off, in_len, rle_len, crc)], [rle bytes per block])"""
        n = len(data)
        a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if n else np.zeros(1, np.uint8)
        maxb = n // (4 * (100000 * self.level - 1) // 5 - 4) + 8
        blocks = (Block * maxb)()
        nb = ctypes.c_size_t(0)
        cap = n + n // 4 + 64
        out = np.zeros(cap if want_bytes else 1, dtype=np.uint8)
        self.check(lib().bzh_rle1_split(self._h, ptr(a), n, blocks, maxb, ctypes.byref(nb),
                                        ptr(out) if want_bytes else None, cap))
        self._nblocks = nb.value  # (plan_open / plan_blocks describe this plan now)
        infos = [(int(blocks[k].in_off), int(blocks[k].in_len), int(blocks[k].rle_len), int(blocks[k].crc))
                 for k in range(nb.value)]
        chunks = []
        if want_bytes:
            pos = 0
            for (_, _, rl, _) in infos:
                chunks.append(out[pos:pos + rl].tobytes())
                pos += rl
        return infos, chunks

    def encode(self, data):
        """bzh_encode: complete .bz2 stream of `data` (host buffers)."""
        n = len(data)
        a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if n else np.zeros(1, np.uint8)
        cap = n + n // 4 + 65536 + (n // 70000 + 2) * 4096
        out = np.zeros(cap, dtype=np.uint8)
        olen = ctypes.c_size_t(0)
        used = ctypes.c_size_t(0)
        self.check(lib().bzh_encode(self._h, ptr(a), n, ptr(out), cap, ctypes.byref(olen), ctypes.byref(used)))
        assert used.value == n
        return out[:olen.value].tobytes()

    def encode_index(self, data, interval):
        """bzh_encode_index: (stream, entries as an array of INDEX_DTYPE, points as an array of SYNC_DTYPE) -- the stream
        encode() writes, with the index bzh_decode_index_sync(stream, interval) would build (interval 0: no points).  The
        entries are sized by bzh_encode_index_bound, the points by the symbols the input can make (far below the bound of
        an interval of 1), and once more by the count BZH_E_CAP reports should that ever fall short."""
        n = len(data)
        a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if n else np.zeros(1, np.uint8)
        cap = n + n // 4 + 65536 + (n // 70000 + 2) * 4096
        out = np.empty(cap, dtype=np.uint8)
        olen, used, cnt, npts = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        max_ent, max_pts = encode_index_bound(self.level, n, interval)
        # (points of a block <= its symbols / 50 / interval, its symbols <= its RLE1 bytes + 1, those <= 5/4 of its input)
        room = min(max_pts, (n + n // 4 + max_ent) // 50 // max(interval, 1) + 1)
        while True:
            ent = np.empty(max(max_ent, 1), dtype=INDEX_DTYPE)
            pts = np.empty(max(room, 1), dtype=SYNC_DTYPE)
            st = lib().bzh_encode_index(self._h, ptr(a), n, ptr(out), cap, ctypes.byref(olen), ctypes.byref(used), interval,
                                        ent.ctypes.data_as(idxp), max_ent, ctypes.byref(cnt), pts.ctypes.data_as(syncp), room,
                                        ctypes.byref(npts))
            if st == -4 and npts.value > room:
                room = npts.value
                continue
            self.check(st)
            assert used.value == n
            return out[:olen.value].tobytes(), ent[:cnt.value].copy(), pts[:npts.value].copy()

    def encode_index_device(self, d_in, n, d_out, cap, interval, max_entries, max_pts):
        """bzh_encode_index_device on integer device addresses, arrays of the given room -> (stream length, entries, points)"""
        olen, used, cnt, npts = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        ent = np.empty(max(max_entries, 1), dtype=INDEX_DTYPE)
        pts = np.empty(max(max_pts, 1), dtype=SYNC_DTYPE)
        self.check(lib().bzh_encode_index_device(self._h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap, ctypes.byref(olen),
                                                 ctypes.byref(used), interval, ent.ctypes.data_as(idxp), max_entries, ctypes.byref(cnt),
                                                 pts.ctypes.data_as(syncp), max_pts, ctypes.byref(npts)))
        return int(olen.value), ent[:cnt.value], pts[:npts.value]

    def encode_many(self, items):
        """bzh_encode_many: one complete .bz2 stream per item (host buffers, one pass) -> [bytes]"""
        arrs = [np.frombuffer(x, dtype=np.uint8) for x in items]
        count = len(arrs)
        if count == 0:
            return []
        lens = np.array([a.size for a in arrs], dtype=np.uint64)
        ins = (u8p * count)(*[ptr(a) for a in arrs])
        cap = encode_many_bound(self.level, lens)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs = np.zeros(count, dtype=np.uint64)
        olens = np.zeros(count, dtype=np.uint64)
        self.check(lib().bzh_encode_many(self._h, ins, ptr(lens, szp), count, ptr(out), cap, ptr(offs, szp), ptr(olens, szp)))
        return [out[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, olens)]

    def encode_many_device(self, d_in, lens, d_out, cap):
        """bzh_encode_many_device on integer device addresses -> (offsets, lengths) of the streams"""
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        count = lens.size
        offs = np.zeros(max(count, 1), dtype=np.uint64)
        olens = np.zeros(max(count, 1), dtype=np.uint64)
        self.check(lib().bzh_encode_many_device(self._h, ctypes.c_void_p(d_in), ptr(lens, szp), count, ctypes.c_void_p(d_out),
                                                cap, ptr(offs, szp), ptr(olens, szp)))
        return offs[:count].tolist(), olens[:count].tolist()

    # ---- decode (bzh_decode*) ----
    def decode_raw(self, data, cap):
        """one bzh_decode call into a buffer of `cap` bytes -> (status, bytes or None, size reported, input bytes consumed)"""
        src, n = _input(data)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        olen = ctypes.c_size_t(0)
        used = ctypes.c_size_t(0)
        st = lib().bzh_decode(self._h, ptr(src), n, ptr(out) if cap else None, cap, ctypes.byref(olen), ctypes.byref(used))
        return st, (out[:olen.value].tobytes() if st == 0 else None), int(olen.value), int(used.value)

    def decode(self, data, size_hint=None, with_consumed=False):
        """bzh_decode: the bytes of the bzip2 stream(s) in `data` (host buffers).  The output is sized by a first guess
        from the input size, then by one retry with the size BZH_E_CAP reports."""
        n = len(data)
        cap = size_hint if size_hint is not None else 6 * n + (1 << 16)
        st, out, need, used = self.decode_raw(data, cap)
        if st == -4:
            st, out, need, used = self.decode_raw(data, need)
        self.check(st)
        return (out, used) if with_consumed else out

    def decode_device(self, d_in, n, d_out, cap):
        """bzh_decode_device on integer device addresses -> (decoded bytes, input bytes consumed)"""
        olen = ctypes.c_size_t(0)
        used = ctypes.c_size_t(0)
        self.check(lib().bzh_decode_device(self._h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap, ctypes.byref(olen),
                                           ctypes.byref(used)))
        return int(olen.value), int(used.value)

    def decode_many_raw(self, items, cap):
        """one bzh_decode_many call into a buffer of `cap` bytes -> (status of the call, buffer, out_offs, out_lens, statuses,
        consumed), the last four as lists; the buffer is None unless the call returned 0"""
        arrs = [np.frombuffer(x, dtype=np.uint8) for x in items]
        count = len(arrs)
        keep = [np.ascontiguousarray(a) if a.size else np.zeros(1, np.uint8) for a in arrs]
        lens = np.array([a.size for a in arrs], dtype=np.uint64)
        ins = (u8p * max(count, 1))(*[ptr(a) for a in keep])
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs, olens, used = (np.zeros(max(count, 1), dtype=np.uint64) for _ in range(3))
        status = np.zeros(max(count, 1), dtype=np.int32)
        st = lib().bzh_decode_many(self._h, ins, ptr(lens, szp) if count else None, count, ptr(out) if cap else None, cap, ptr(offs, szp),
                                   ptr(olens, szp), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ptr(used, szp))
        return (st, out if st == 0 else None, offs[:count].tolist(), olens[:count].tolist(), status[:count].tolist(),
                used[:count].tolist())

    def decode_many(self, items, with_status=False):
        """bzh_decode_many: every item decoded as bzh_decode would decode it alone, in one pass -> [bytes], with None where an
        input failed; with_status: (that list, [status], [input bytes consumed]).  The output is sized by a first guess, then by
        one retry with the size BZH_E_CAP reports."""
        items = list(items)
        cap = 6 * sum(len(x) for x in items) + (1 << 16)
        st, out, offs, olens, status, used = self.decode_many_raw(items, cap)
        if st == -4:
            st, out, offs, olens, status, used = self.decode_many_raw(items, offs[-1] + olens[-1])
        self.check(st)
        res = [out[o:o + n].tobytes() if s == 0 else None for o, n, s in zip(offs, olens, status)]
        return (res, status, used) if with_status else res

    def decode_many_device(self, d_in, n, offs, lens, d_out, cap):
        """bzh_decode_many_device on integer device addresses -> (status of the call, out_offs, out_lens, statuses, consumed).
        BZH_E_CAP (-4) is handed back, not raised: the arrays are set then too."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        if offs.size != lens.size:
            raise ValueError("as many offsets as lengths")
        count = offs.size
        ooffs, olens, used = (np.zeros(max(count, 1), dtype=np.uint64) for _ in range(3))
        status = np.zeros(max(count, 1), dtype=np.int32)
        st = lib().bzh_decode_many_device(self._h, ctypes.c_void_p(d_in), n, ptr(offs, szp) if count else None,
                                          ptr(lens, szp) if count else None, count, ctypes.c_void_p(d_out), cap, ptr(ooffs, szp),
                                          ptr(olens, szp), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ptr(used, szp))
        if st not in (0, -4):
            self.check(st)
        return st, ooffs[:count].tolist(), olens[:count].tolist(), status[:count].tolist(), used[:count].tolist()

    def last_error(self):
        return lib().bzh_last_error(self._h).decode()

    def decode_many_stats(self):
        s = DecodeManyStats()
        self.check(lib().bzh_get_decode_many_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    # ---- recovery (bzh_recover*) ----
    def recover_raw(self, data, cap, max_entries):
        """one bzh_recover call into a buffer of `cap` bytes and a report of `max_entries` entries -> (status, bytes or None,
        size reported, entries as a structured array of RECOVER_DTYPE or None, entries reported).  The bytes are None unless
        they fit, the entries unless they do."""
        src, n = _input(data)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        ent = np.empty(max(max_entries, 1), dtype=RECOVER_DTYPE)
        olen, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
        st = lib().bzh_recover(self._h, ptr(src), n, ptr(out) if cap else None, cap, ctypes.byref(olen),
                               ent.ctypes.data_as(recp) if max_entries else None, max_entries, ctypes.byref(cnt))
        if st not in (0, -4):
            self.check(st)
        return (st, out[:olen.value].tobytes() if olen.value <= cap else None, int(olen.value),
                ent[:cnt.value].copy() if cnt.value <= max_entries else None, int(cnt.value))

    def recover(self, data):
        """bzh_recover: (the bytes of every block of `data` that verifies, the report as a structured array of RECOVER_DTYPE).
        One call with a guessed room for the bytes and for the report; BZH_E_CAP names what either needs, and the call is
        repeated with that."""
        n = len(data)
        cap, room = 6 * n + (1 << 16), n // 1000 + 64
        for _ in range(3):
            st, out, need, ent, cnt = self.recover_raw(data, cap, room)
            if st != -4:
                break
            cap, room = max(cap, need), max(room, cnt)
        self.check(st)
        return out, ent

    def recover_device(self, d_in, n, d_out, cap, max_entries):
        """bzh_recover_device on integer device addresses -> (status, size reported, entries or None, entries reported);
        BZH_E_CAP (-4) is handed back, not raised"""
        ent = np.empty(max(max_entries, 1), dtype=RECOVER_DTYPE)
        olen, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
        st = lib().bzh_recover_device(self._h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap, ctypes.byref(olen),
                                      ent.ctypes.data_as(recp) if max_entries else None, max_entries, ctypes.byref(cnt))
        if st not in (0, -4):
            self.check(st)
        return st, int(olen.value), (ent[:cnt.value].copy() if cnt.value <= max_entries else None), int(cnt.value)

    def recover_stats(self):
        s = RecoverStats()
        self.check(lib().bzh_get_recover_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def recover_stream_raw(self, data, entries, cap):
        """one bzh_recover_stream call into a buffer of `cap` bytes -> (status, bytes or None, size reported)"""
        src, n = _input(data)
        e, p = _report(entries)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        olen = ctypes.c_size_t(0)
        st = lib().bzh_recover_stream(self._h, ptr(src), n, p, e.size, ptr(out) if cap else None, cap, ctypes.byref(olen))
        return st, (out[:olen.value].tobytes() if st == 0 else None), int(olen.value)

    def recover_stream(self, data, entries):
        """bzh_recover_stream: the kept blocks of the report, bit for bit, as one .bz2 stream of the context's level"""
        e, _ = _report(entries)
        kept = e[e["kind"] == 0]
        bits = int((kept["end_bit"].astype(object) - kept["bit_pos"].astype(object)).sum()) if kept.size else 0
        st, out, need = self.recover_stream_raw(data, e, 4 + max(0, bits + 80 + 7) // 8)
        if st == -4:
            st, out, need = self.recover_stream_raw(data, e, need)
        self.check(st)
        return out

    def recover_stream_device(self, d_in, n, entries, d_out, cap):
        """bzh_recover_stream_device on integer device addresses -> (status, size reported); nothing is raised"""
        e, p = _report(entries)
        olen = ctypes.c_size_t(0)
        st = lib().bzh_recover_stream_device(self._h, ctypes.c_void_p(d_in), n, p, e.size, ctypes.c_void_p(d_out), cap,
                                             ctypes.byref(olen))
        return st, int(olen.value)

    def decode_index(self, data):
        """bzh_decode_index: the verified block index of the stream(s) in `data` -> (entries as a structured array of
        INDEX_DTYPE, decoded bytes in total, input bytes consumed)"""
        src, n = _input(data)
        cnt, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
        # room for every block the input can hold, so that the build runs once: a block is at least 174 bits (magic, CRC,
        # origPtr, one sector of the symbol map, one selector, two tables of three lengths, one symbol and the end of block).
        # (np.empty: pages the library does not write are never touched)
        cap = n // 21 + 1
        while True:
            ent = np.empty(cap, dtype=INDEX_DTYPE)
            st = lib().bzh_decode_index(self._h, ptr(src), n, ent.ctypes.data_as(idxp), cap, ctypes.byref(cnt), ctypes.byref(total),
                                        ctypes.byref(used))
            if st == -4 and cnt.value > cap:
                cap = cnt.value
                continue
            self.check(st)
            return ent[:cnt.value].copy(), int(total.value), int(used.value)

    def decode_range(self, data, entries, off, length, in_byte_base=0):
        """bzh_decode_range: output bytes [off, off + length) of the indexed input, clipped to its total; `data` holds the
        compressed bytes from byte `in_byte_base` of that input on (all of it, or just the span of the range)"""
        if off < 0 or length < 0:
            raise ValueError("offset and length must not be negative")
        src, n = _input(data)
        e, p = _entries(entries)
        total = int(e["out_off"][-1]) + int(e["out_len"][-1]) if e.size else 0
        cap = max(0, min(length, total - off))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        got = ctypes.c_size_t(0)
        self.check(lib().bzh_decode_range(self._h, ptr(src), n, in_byte_base, p, e.size, off, length, ptr(out), cap,
                                          ctypes.byref(got)))
        return out[:got.value].tobytes()

    def decode_range_device(self, d_in, n, entries, off, length, d_out, cap, in_byte_base=0):
        """bzh_decode_range_device on integer device addresses -> bytes written at d_out"""
        e, p = _entries(entries)
        got = ctypes.c_size_t(0)
        self.check(lib().bzh_decode_range_device(self._h, ctypes.c_void_p(d_in), n, in_byte_base, p, e.size, off, length,
                                                 ctypes.c_void_p(d_out), cap, ctypes.byref(got)))
        return int(got.value)

    def decode_index_sync(self, data, interval):
        """bzh_decode_index_sync: decode_index that also records a sync point every `interval` groups of every block ->
        (entries, points as a structured array of SYNC_DTYPE, decoded bytes in total, input bytes consumed).  One call sizes
        the two arrays, a second fills them."""
        src, n = _input(data)
        cnt, npts, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
        st = lib().bzh_decode_index_sync(self._h, ptr(src), n, interval, None, 0, ctypes.byref(cnt), None, 0, ctypes.byref(npts),
                                         ctypes.byref(total), ctypes.byref(used))
        if st != -4:
            self.check(st)
        ent = np.empty(cnt.value, dtype=INDEX_DTYPE)
        pts = np.empty(npts.value, dtype=SYNC_DTYPE)
        if st == -4:
            self.check(lib().bzh_decode_index_sync(self._h, ptr(src), n, interval, ent.ctypes.data_as(idxp) if ent.size else None, ent.size,
                                                   ctypes.byref(cnt), pts.ctypes.data_as(syncp) if pts.size else None, pts.size,
                                                   ctypes.byref(npts), ctypes.byref(total), ctypes.byref(used)))
        return ent[:cnt.value], pts[:npts.value], int(total.value), int(used.value)

    def decode_range_sync(self, data, entries, points, off, length, in_byte_base=0):
        """bzh_decode_range_sync: decode_range with the blocks' entropy stage split at the sync points"""
        if off < 0 or length < 0:
            raise ValueError("offset and length must not be negative")
        src, n = _input(data)
        e, p = _entries(entries)
        q, pp = _points(points)
        total = int(e["out_off"][-1]) + int(e["out_len"][-1]) if e.size else 0
        cap = max(0, min(length, total - off))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        got = ctypes.c_size_t(0)
        self.check(lib().bzh_decode_range_sync(self._h, ptr(src), n, in_byte_base, p, e.size, pp, q.size, off, length, ptr(out), cap,
                                               ctypes.byref(got)))
        return out[:got.value].tobytes()

    def decode_range_sync_device(self, d_in, n, entries, points, off, length, d_out, cap, in_byte_base=0):
        """bzh_decode_range_sync_device on integer device addresses -> bytes written at d_out"""
        e, p = _entries(entries)
        q, pp = _points(points)
        got = ctypes.c_size_t(0)
        self.check(lib().bzh_decode_range_sync_device(self._h, ctypes.c_void_p(d_in), n, in_byte_base, p, e.size, pp, q.size, off, length,
                                                      ctypes.c_void_p(d_out), cap, ctypes.byref(got)))
        return int(got.value)

    def decode_ranges(self, comp, entries, ranges, points=None, in_byte_base=0):
        """bzh_decode_ranges: the output bytes of every (off, len) of `ranges` in one call, every touched block decoded once ->
        (bytes of all ranges back to back, their offsets in it, their lengths).  `comp` holds the compressed bytes from byte
        `in_byte_base` of the indexed input on; `points`: sync points, or None"""
        src, n = _input(comp)
        e, p = _entries(entries)
        q, pp = _points_or_none(points)
        r, rp = _ranges(ranges)
        total = int(e["out_off"][-1]) + int(e["out_len"][-1]) if e.size else 0
        off, ln = r["off"].astype(object), r["len"].astype(object)  # (Python ints: off + len does not wrap)
        cap = sum(max(0, min(int(l), total - int(o))) for o, l in zip(off, ln))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs, lens = np.zeros(max(r.size, 1), dtype=np.uintp), np.zeros(max(r.size, 1), dtype=np.uintp)
        got = ctypes.c_size_t(0)
        self.check(lib().bzh_decode_ranges(self._h, ptr(src), n, in_byte_base, p, e.size, pp, q.size, rp, r.size, ptr(out), cap,
                                           ptr(offs, szp), ptr(lens, szp), ctypes.byref(got)))
        return out[:got.value].tobytes(), [int(v) for v in offs[:r.size]], [int(v) for v in lens[:r.size]]

    def decode_ranges_device(self, d_in, n, entries, ranges, d_out, cap, points=None, in_byte_base=0):
        """bzh_decode_ranges_device on integer device addresses -> (status, out_total, offsets, lengths); the status is not
        raised, so that a caller can look at the sizes a BZH_E_CAP leaves"""
        e, p = _entries(entries)
        q, pp = _points_or_none(points)
        r, rp = _ranges(ranges)
        offs, lens = np.zeros(max(r.size, 1), dtype=np.uintp), np.zeros(max(r.size, 1), dtype=np.uintp)
        got = ctypes.c_size_t(0)
        st = lib().bzh_decode_ranges_device(self._h, ctypes.c_void_p(d_in), n, in_byte_base, p, e.size, pp, q.size, rp, r.size,
                                            ctypes.c_void_p(d_out), cap, ptr(offs, szp), ptr(lens, szp), ctypes.byref(got))
        return st, int(got.value), [int(v) for v in offs[:r.size]], [int(v) for v in lens[:r.size]]

    def decode_index_records(self, data, interval=0, delim=10):
        """bzh_decode_index_records: decode_index_sync (interval 0: entries only) that also fills the record table ->
        (entries, points, rec_cum as a uint64 array of entries + 1 words, nrecords, decoded bytes in total, input bytes
        consumed).  One call sizes the arrays, a second fills them."""
        src, n = _input(data)
        cnt, npts, used = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        total, nrec = ctypes.c_uint64(0), ctypes.c_uint64(0)
        st = lib().bzh_decode_index_records(self._h, ptr(src), n, interval, delim, None, 0, ctypes.byref(cnt), None, 0, ctypes.byref(npts),
                                            None, 0, ctypes.byref(nrec), ctypes.byref(total), ctypes.byref(used))
        if st != -4:
            self.check(st)
        ent = np.empty(cnt.value, dtype=INDEX_DTYPE)
        pts = np.empty(npts.value, dtype=SYNC_DTYPE)
        cum = np.zeros(cnt.value + 1, dtype=np.uint64)
        self.check(lib().bzh_decode_index_records(self._h, ptr(src), n, interval, delim, ent.ctypes.data_as(idxp) if ent.size else None,
                                                  ent.size, ctypes.byref(cnt), pts.ctypes.data_as(syncp) if pts.size else None, pts.size,
                                                  ctypes.byref(npts), ptr(cum, u64p), cum.size, ctypes.byref(nrec), ctypes.byref(total),
                                                  ctypes.byref(used)))
        return ent[:cnt.value], pts[:npts.value], cum[:cnt.value + 1], int(nrec.value), int(total.value), int(used.value)

    def decode_index_records_device(self, d_in, n, interval, delim, max_entries, max_pts):
        """bzh_decode_index_records_device on an integer device address, arrays of the given room -> (entries, points, rec_cum,
        nrecords, total, consumed)"""
        ent = np.empty(max(max_entries, 1), dtype=INDEX_DTYPE)
        pts = np.empty(max(max_pts, 1), dtype=SYNC_DTYPE)
        cum = np.zeros(max_entries + 1, dtype=np.uint64)
        cnt, npts, used = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        total, nrec = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.check(lib().bzh_decode_index_records_device(self._h, ctypes.c_void_p(d_in), n, interval, delim, ent.ctypes.data_as(idxp),
                                                         max_entries, ctypes.byref(cnt), pts.ctypes.data_as(syncp), max_pts,
                                                         ctypes.byref(npts), ptr(cum, u64p), cum.size, ctypes.byref(nrec),
                                                         ctypes.byref(total), ctypes.byref(used)))
        return ent[:cnt.value], pts[:npts.value], cum[:cnt.value + 1], int(nrec.value), int(total.value), int(used.value)

    def count_records_device(self, d_raw, n, entries, delim=10):
        """bzh_count_records_device: the record table of the decoded bytes at the integer device address d_raw under an index
        of them -> (rec_cum, nrecords)"""
        e, p = _entries(entries)
        cum = np.zeros(e.size + 1, dtype=np.uint64)
        nrec = ctypes.c_uint64(0)
        self.check(lib().bzh_count_records_device(self._h, ctypes.c_void_p(d_raw), n, delim, p, e.size, ptr(cum, u64p), ctypes.byref(nrec)))
        return cum, int(nrec.value)

    def decode_records_raw(self, comp, entries, rec_cum, ranges, cap, points=None, in_byte_base=0, delim=10):
        """one bzh_decode_records call with room for `cap` bytes -> (status, out_total, offsets, lengths, the buffer); nothing
        is raised, so that a caller can look at the sizes a BZH_E_CAP leaves"""
        src, n = _input(comp)
        e, p = _entries(entries)
        t, tp = _table(e, rec_cum)
        q, pp = _points_or_none(points)
        r, rp = _ranges(ranges)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs, lens = np.zeros(max(r.size, 1), dtype=np.uintp), np.zeros(max(r.size, 1), dtype=np.uintp)
        got = ctypes.c_size_t(0)
        st = lib().bzh_decode_records(self._h, ptr(src), n, in_byte_base, p, e.size, pp, q.size, tp, delim, rp, r.size, ptr(out), cap,
                                      ptr(offs, szp), ptr(lens, szp), ctypes.byref(got))
        return st, int(got.value), [int(v) for v in offs[:r.size]], [int(v) for v in lens[:r.size]], out

    def decode_records(self, comp, entries, rec_cum, ranges, points=None, in_byte_base=0, delim=10):
        """bzh_decode_records: the bytes of every (first record, count) of `ranges` -- ascending, not overlapping -- in one call
        -> (bytes of all ranges back to back, their offsets in it, their lengths).  The room is the touched blocks' decoded
        size, which disjoint ranges never exceed."""
        e, _ = _entries(entries)
        touched, _, _ = record_spans(e, rec_cum, ranges)
        cap = int(e["out_len"][touched.astype(np.int64)].sum(dtype=np.uint64)) if touched.size else 0
        st, got, offs, lens, out = self.decode_records_raw(comp, e, rec_cum, ranges, cap, points, in_byte_base, delim)
        self.check(st)
        return out[:got].tobytes(), offs, lens

    def decode_records_device(self, d_in, n, entries, rec_cum, ranges, d_out, cap, points=None, in_byte_base=0, delim=10):
        """bzh_decode_records_device on integer device addresses -> (status, out_total, offsets, lengths); not raised"""
        e, p = _entries(entries)
        t, tp = _table(e, rec_cum)
        q, pp = _points_or_none(points)
        r, rp = _ranges(ranges)
        offs, lens = np.zeros(max(r.size, 1), dtype=np.uintp), np.zeros(max(r.size, 1), dtype=np.uintp)
        got = ctypes.c_size_t(0)
        st = lib().bzh_decode_records_device(self._h, ctypes.c_void_p(d_in), n, in_byte_base, p, e.size, pp, q.size, tp, delim, rp, r.size,
                                             ctypes.c_void_p(d_out), cap, ptr(offs, szp), ptr(lens, szp), ctypes.byref(got))
        return st, int(got.value), [int(v) for v in offs[:r.size]], [int(v) for v in lens[:r.size]]

    # ---- search: every call returns (hits as a HIT_DTYPE array, nhits); `limit` is the C call's max ---------------------------
    SEARCH_GUESS = 1 << 16  # hit slots of the first try without a limit; more hits: once more, with the exact room

    def _search(self, call, limit, dtype=None):
        """call(hits pointer, max, nhits reference) -> status.  limit None: every hit (a second call when the first try's room
        was too small); else at most `limit` hits and the exact count -- BZH_E_CAP is then the answer, not an error"""
        if limit is not None and limit < 0:
            raise ValueError("search: a negative limit")
        room = self.SEARCH_GUESS if limit is None else int(limit)
        for _ in range(2):
            hits = np.zeros(max(room, 1), dtype=dtype or HIT_DTYPE)  # (dtype: SET_HIT_DTYPE, of a search for a set)
            got = ctypes.c_size_t(0)
            st = call(hits.ctypes.data_as(ctypes.c_void_p if dtype else hitp) if room else None, room, ctypes.byref(got))
            self.search_status = st  # (of the last C call: BZH_E_CAP where the limit cut the hits)
            if st == -4 and limit is None and got.value > room:
                room = int(got.value)
                continue
            if st != -4 or not 0 < room < got.value:  # (BZH_E_CAP with more hits than room: the first `room` are there)
                self.check(st)
            return hits[:min(room, int(got.value))].copy(), int(got.value)
        raise BzhError(-5, "search: the second call found more hits than the first")

    @staticmethod
    def _pattern(pattern):
        b = bytes(pattern)
        return np.frombuffer(b, dtype=np.uint8) if b else np.zeros(1, np.uint8), len(b)

    @staticmethod
    def _what(name, pattern):
        """What a search or a grep looks for -> (the C call, the arguments that name it, the hits' dtype): the call `name` with
        (pat, plen) for a byte string, its patset twin with the set for a PatternSet"""
        if isinstance(pattern, PatternSet):
            return getattr(lib(), _patset_twin(name)), (pattern.handle,), SET_HIT_DTYPE
        pat, plen = Context._pattern(pattern)
        return getattr(lib(), name), (ptr(pat), plen), None

    @staticmethod
    def _delim(delim):
        """(flags, delimiter byte) of a delimiter given as None, an int or one byte"""
        if delim is None:
            return 0, 0
        d = delim[0] if isinstance(delim, (bytes, bytearray)) and len(delim) == 1 else delim
        if not isinstance(d, int) or not 0 <= d <= 255:
            raise ValueError("search: the delimiter is one byte value")
        return SEARCH_RECORDS, d

    def search_raw_device(self, d_raw, n, pattern, delim=None, limit=None, flags=None):
        """bzh_search_raw_device on the integer device address d_raw -> (hits, nhits)"""
        fn, what, dt = self._what("bzh_search_raw_device", pattern)
        fl, d = self._delim(delim)
        fl = fl if flags is None else flags
        return self._search(lambda h, m, g: fn(self._h, ctypes.c_void_p(d_raw), n, *what, fl, d, h, m, g), limit, dt)

    def search_device(self, d_in, n, pattern, delim=None, limit=None, with_total=False):
        """bzh_search_device on the integer device address of the compressed bytes -> (hits, nhits[, out_total, consumed])"""
        fn, what, dt = self._what("bzh_search_device", pattern)
        fl, d = self._delim(delim)
        total, used = ctypes.c_uint64(0), ctypes.c_size_t(0)
        r = self._search(lambda h, m, g: fn(self._h, ctypes.c_void_p(d_in), n, *what, fl, d, h, m, g, ctypes.byref(total), ctypes.byref(used)),
                         limit, dt)
        return r + (int(total.value), int(used.value)) if with_total else r

    def search(self, data, pattern, delim=None, limit=None, with_total=False):
        """bzh_search: every occurrence of `pattern` in the decoded bytes of `data` -> (hits, nhits[, out_total, consumed])"""
        src, n = _input(data)
        fn, what, dt = self._what("bzh_search", pattern)
        fl, d = self._delim(delim)
        total, used = ctypes.c_uint64(0), ctypes.c_size_t(0)
        r = self._search(lambda h, m, g: fn(self._h, ptr(src), n, *what, fl, d, h, m, g, ctypes.byref(total), ctypes.byref(used)), limit, dt)
        return r + (int(total.value), int(used.value)) if with_total else r

    def search_range(self, comp, entries, pattern, off=0, length=None, points=None, rec_cum=None, delim=None, limit=None, in_byte_base=0,
                     d_in=None):
        """bzh_search_range (d_in: an integer device address and comp the byte count -> bzh_search_range_device): the hits wholly
        inside output [off, off + length) of the indexed input -> (hits, nhits).  Record numbers with rec_cum and delim."""
        e, p = _entries(entries)
        q, pp = _points_or_none(points)
        fl, d = self._delim(delim)
        tp = _table(e, rec_cum)[1] if rec_cum is not None else None
        length = 2**64 - 1 if length is None else length
        if d_in is not None:
            fn, what, dt = self._what("bzh_search_range_device", pattern)
            return self._search(lambda h, m, g: fn(self._h, ctypes.c_void_p(d_in), comp, in_byte_base, p, e.size, pp, q.size, tp, off, length,
                                                   *what, fl, d, h, m, g), limit, dt)
        fn, what, dt = self._what("bzh_search_range", pattern)
        src, n = _input(comp)
        return self._search(lambda h, m, g: fn(self._h, ptr(src), n, in_byte_base, p, e.size, pp, q.size, tp, off, length, *what, fl, d, h, m, g),
                            limit, dt)

    def search_set_room(self, nbytes=0):
        self.check(lib().bzh_search_set_room(self._h, nbytes))

    def search_stats(self):
        s = SearchStats()
        self.check(lib().bzh_get_search_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    # ---- grep and the matched parts alone: the selected bytes and their entries.  One body per route for both families; a family is
    # the prefix of its C calls, its entries (GREP_ENTRY_DTYPE, MATCH_DTYPE) and its flags ------------------------------------------
    GREP_GUESS = (1 << 20, 1 << 12)  # bytes and entries of the first try; more of either: once more, with the exact rooms
    _ENTRIES = {"grep": (GREP_ENTRY_DTYPE, grepp), "match": (MATCH_DTYPE, matchp)}

    def _scan(self, family, call, count_only=False):
        """call(out pointer, cap, entries pointer, max, count reference, out_total reference) -> status.  Returns (bytes,
        entries): a first try with GREP_GUESS, a second with the exact rooms when either was too small.  count_only: a counting
        call (no room is asked for) -> (count, out_total).  grep_status / match_status: the status of the last C call."""
        dtype, entp = self._ENTRIES[family]
        got, total = ctypes.c_size_t(0), ctypes.c_uint64(0)
        if count_only:
            self.check(call(None, 0, None, 0, ctypes.byref(got), ctypes.byref(total)))
            return int(got.value), int(total.value)
        cap, room = self.GREP_GUESS
        for _ in range(2):
            out = np.empty(max(cap, 1), dtype=np.uint8)
            ent = np.zeros(max(room, 1), dtype=dtype)
            st = call(ptr(out), cap, ent.ctypes.data_as(entp), room, ctypes.byref(got), ctypes.byref(total))
            setattr(self, family + "_status", st)
            if st == -4 and (total.value > cap or got.value > room):
                cap, room = int(total.value), int(got.value)
                continue
            self.check(st)
            return out[:int(total.value)].tobytes(), ent[:int(got.value)].copy()
        raise BzhError(-5, family + ": the second call selected more than the first")

    def _grep(self, call, count_only=False):
        return self._scan("grep", call, count_only)

    def _match(self, call, count_only=False):
        return self._scan("match", call, count_only)

    @staticmethod
    def _grep_args(pattern, delim, invert):
        pat, plen = Context._pattern(pattern)
        fl, d = Context._delim(delim)
        if not fl:
            raise ValueError("grep: the delimiter is one byte value")
        return pat, plen, GREP_INVERT if invert else 0, d

    @staticmethod
    def _scan_what(family, route, pattern, delim, invert=False):
        """-> (the C call bzh_<family><route> for a byte string or a PatternSet, the arguments that name what is looked for, flags,
        delimiter).  A grep needs a delimiter; a match numbers records when it is given one."""
        fl, d = Context._delim(delim)
        if family == "grep" and not fl:
            raise ValueError("grep: the delimiter is one byte value")
        fn, what, _ = Context._what("bzh_" + family + route, pattern)
        return fn, what, (GREP_INVERT if invert else 0) if family == "grep" else (MATCH_RECORDS if fl else 0), d

    def grep_set_context(self, before, after):
        """bzh_grep_set_context: sticky, read by every grep call when it begins"""
        self.check(lib().bzh_grep_set_context(self._h, before, after))

    def _grep_with_context(self, before, after, run):
        """run() between bzh_grep_set_context(before, after) and (0, 0): these wrappers leave no sticky setting behind.  With a
        context the entries come as GREP_CONTEXT_ENTRY_DTYPE."""
        if not (before or after):
            return run()
        self.grep_set_context(before, after)
        try:
            got = run()
        finally:
            self.grep_set_context(0, 0)
        return (got[0], grep_context_rows(got[1])) if isinstance(got[1], np.ndarray) else got

    def _host_call(self, family, data, pattern, delim, invert=False):
        """the `call` of _scan for bzh_<family>; the arguments are looked at here, before any C call"""
        src, n = _input(data)
        fn, what, fl, d = self._scan_what(family, "", pattern, delim, invert)
        return lambda o, c, e, m, g, t: fn(self._h, ptr(src), n, *what, fl, d, o, c, e, m, g, t, None, None)

    def _index_call(self, family, comp, entries, pattern, points, delim, invert=False):
        """... for bzh_<family>_index"""
        e, p = _entries(entries)
        q, pp = _points_or_none(points)
        src, n = _input(comp)
        fn, what, fl, d = self._scan_what(family, "_index", pattern, delim, invert)
        return lambda o, c, en, m, g, t: fn(self._h, ptr(src), n, p, e.size, pp, q.size, *what, fl, d, o, c, en, m, g, t)

    def _scan_on_device(self, family, route, head, pattern, d_out, cap, room, delim, invert=False, flags=None, tail=()):
        """the device variants, on integer device addresses: bzh_<family><route>(head..., what, flags, delim, d_out, cap, `room`
        entries, counts, tail...); the bytes stay in the caller's device buffer -> (status, count, out_total, entries)"""
        fn, what, fl, d = self._scan_what(family, route, pattern, delim, invert)
        dtype, entp = self._ENTRIES[family]
        got, total = ctypes.c_size_t(0), ctypes.c_uint64(0)
        ent = np.zeros(max(room, 1), dtype=dtype)
        st = fn(self._h, *head, *what, fl if flags is None else flags, d, ctypes.c_void_p(d_out), cap, ent.ctypes.data_as(entp) if room else None,
                room, ctypes.byref(got), ctypes.byref(total), *tail)
        return st, int(got.value), int(total.value), ent[:min(room, int(got.value))].copy()

    def _scan_index_device(self, family, d_in, n, entries, pattern, d_out, cap, room, points, delim, invert=False):
        e, p = _entries(entries)
        q, pp = _points_or_none(points)
        return self._scan_on_device(family, "_index_device", (ctypes.c_void_p(d_in), n, p, e.size, pp, q.size), pattern, d_out, cap, room, delim,
                                    invert)

    def grep(self, data, pattern, delim=b"\n", invert=False, count_only=False, before=0, after=0):
        """bzh_grep: the records of the decoded bytes of `data` that hold `pattern` -> (bytes, entries), or (nrecs, out_total)"""
        call = self._host_call("grep", data, pattern, delim, invert)
        return self._grep_with_context(before, after, lambda: self._grep(call, count_only))

    def grep_index(self, comp, entries, pattern, points=None, delim=b"\n", invert=False, count_only=False, before=0, after=0):
        """bzh_grep_index over the whole indexed input `comp` -> as grep"""
        call = self._index_call("grep", comp, entries, pattern, points, delim, invert)
        return self._grep_with_context(before, after, lambda: self._grep(call, count_only))

    def grep_raw_device(self, d_raw, n, pattern, d_out, cap, room, delim=b"\n", invert=False, flags=None):
        """bzh_grep_raw_device on integer device addresses; `room` entries -> (status, nrecs, out_total, entries)"""
        return self._scan_on_device("grep", "_raw_device", (ctypes.c_void_p(d_raw), n), pattern, d_out, cap, room, delim, invert, flags)

    def grep_device(self, d_in, n, pattern, d_out, cap, room, delim=b"\n", invert=False):
        """bzh_grep_device on integer device addresses; `room` entries -> (status, nrecs, out_total, entries)"""
        return self._scan_on_device("grep", "_device", (ctypes.c_void_p(d_in), n), pattern, d_out, cap, room, delim, invert, tail=(None, None))

    def grep_index_device(self, d_in, n, entries, pattern, d_out, cap, room, points=None, delim=b"\n", invert=False):
        """bzh_grep_index_device on integer device addresses; `room` entries -> (status, nrecs, out_total, entries)"""
        return self._scan_index_device("grep", d_in, n, entries, pattern, d_out, cap, room, points, delim, invert)

    # ---- grep over many inputs (bzh_grep_many*) ----
    def _grep_many_call(self, route, head, count, pattern, delim, invert, d_out, cap, room, flags=None):
        """bzh_grep_many<route>(head..., what, flags, delim, out, cap, `room` entries, items, counts) -> (status, nrecs, out_total,
        entries, items as a structured array of GREP_MANY_ITEM_DTYPE).  BZH_E_CAP (-4) is handed back like every status: the
        counts and the items are exact then too."""
        fn, what, fl, d = self._scan_what("grep", "_many" + route, pattern, delim, invert)
        got, total = ctypes.c_size_t(0), ctypes.c_uint64(0)
        ent = np.zeros(max(room, 1), dtype=GREP_ENTRY_DTYPE)
        items = np.zeros(max(count, 1), dtype=GREP_MANY_ITEM_DTYPE)
        st = fn(self._h, *head, *what, fl if flags is None else flags, d, d_out, cap, ent.ctypes.data_as(grepp) if room else None, room,
                items.ctypes.data_as(grepmanyp) if count else None, ctypes.byref(got), ctypes.byref(total))
        self.grep_status = st
        return st, int(got.value), int(total.value), ent[:min(room, int(got.value))].copy(), items[:count].copy()

    @staticmethod
    def _segments(offs, lens):
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        if offs.size != lens.size:
            raise ValueError("as many offsets as lengths")
        return offs, lens, (ptr(offs, szp) if offs.size else None, ptr(lens, szp) if offs.size else None, offs.size)

    def grep_many_raw_device(self, d_raw, n, offs, lens, pattern, d_out, cap, room, delim=b"\n", invert=False, flags=None):
        """bzh_grep_many_raw_device on integer device addresses: the texts d_raw[offs[k], +lens[k]) -> as _grep_many_call"""
        offs, lens, seg = self._segments(offs, lens)
        return self._grep_many_call("_raw_device", (ctypes.c_void_p(d_raw), n, *seg), offs.size, pattern, delim, invert, ctypes.c_void_p(d_out), cap,
                                    room, flags)

    def grep_many_device(self, d_in, n, offs, lens, pattern, d_out, cap, room, delim=b"\n", invert=False):
        """bzh_grep_many_device on integer device addresses: the inputs d_in[offs[k], +lens[k]) -> as _grep_many_call"""
        offs, lens, seg = self._segments(offs, lens)
        return self._grep_many_call("_device", (ctypes.c_void_p(d_in), n, *seg), offs.size, pattern, delim, invert, ctypes.c_void_p(d_out), cap, room)

    def grep_many_host_raw(self, inputs, pattern, cap, room, delim=b"\n", invert=False):
        """one bzh_grep_many call with rooms of `cap` bytes and `room` entries (0, 0: a counting call) -> (status, nrecs, out_total,
        the out buffer, entries, items)"""
        arrs = [np.frombuffer(x, dtype=np.uint8) for x in inputs]
        count = len(arrs)
        keep = [np.ascontiguousarray(a) if a.size else np.zeros(1, np.uint8) for a in arrs]
        lens = np.array([a.size for a in arrs], dtype=np.uint64)
        ins = (u8p * max(count, 1))(*[ptr(a) for a in keep])
        out = np.empty(max(cap, 1), dtype=np.uint8)
        st, got, total, ent, items = self._grep_many_call("", (ins, ptr(lens, szp) if count else None, count), count, pattern, delim, invert,
                                                          ptr(out) if cap else None, cap, room)
        return st, got, total, out, ent, items

    def grep_many(self, inputs, pattern, delim=b"\n", invert=False, count_only=False):
        """bzh_grep_many: every input grepped as bzh_grep greps it alone, in one pass -> (items, [(bytes, entries)]), a failed
        input's pair None; count_only: (items, None) from a counting call.  The rooms are a first guess, then the exact ones."""
        inputs = list(inputs)
        if count_only:
            st, _, _, _, _, items = self.grep_many_host_raw(inputs, pattern, 0, 0, delim, invert)
            self.check(st)
            return items, None
        cap, room = self.GREP_GUESS
        for _ in range(2):
            st, got, total, out, ent, items = self.grep_many_host_raw(inputs, pattern, cap, room, delim, invert)
            if st == -4 and (total > cap or got > room):
                cap, room = total, got
                continue
            self.check(st)
            res, e0 = [], 0
            for it in items:
                e = ent[e0:e0 + int(it["selected"])].copy()
                b0 = int(e["out_off"][0]) if e.size else 0
                if e.size:
                    e["out_off"] -= np.uint64(b0)  # (as bzh_grep of the input alone numbers them)
                res.append(None if it["status"] != 0 else (out[b0:b0 + int(it["out_bytes"])].tobytes(), e))
                e0 += int(it["selected"])
            return items, res
        raise BzhError(-5, "grep many: the second call selected more than the first")

    def grep_many_stats(self):
        s = GrepManyStats()
        self.check(lib().bzh_get_grep_many_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def grep_stats(self):
        s = GrepStats()
        self.check(lib().bzh_get_grep_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def grep_context_stats(self):
        s = GrepContextStats()
        self.check(lib().bzh_get_grep_context_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def matches(self, data, pattern, delim=None, count_only=False):
        """bzh_match: the non-overlapping leftmost-longest matches of `pattern` in the decoded bytes of `data` -> (bytes, entries),
        or (nmatches, out_total); delim None: no record numbers"""
        return self._match(self._host_call("match", data, pattern, delim), count_only)

    def matches_index(self, comp, entries, pattern, points=None, delim=None, count_only=False):
        """bzh_match_index over the whole indexed input `comp` -> as matches"""
        return self._match(self._index_call("match", comp, entries, pattern, points, delim), count_only)

    def match_raw_device(self, d_raw, n, pattern, d_out, cap, room, delim=None, flags=None):
        """bzh_match_raw_device on integer device addresses; `room` entries -> (status, nmatches, out_total, entries)"""
        return self._scan_on_device("match", "_raw_device", (ctypes.c_void_p(d_raw), n), pattern, d_out, cap, room, delim, flags=flags)

    def match_device(self, d_in, n, pattern, d_out, cap, room, delim=None):
        """bzh_match_device on integer device addresses; `room` entries -> (status, nmatches, out_total, entries)"""
        return self._scan_on_device("match", "_device", (ctypes.c_void_p(d_in), n), pattern, d_out, cap, room, delim, tail=(None, None))

    def match_index_device(self, d_in, n, entries, pattern, d_out, cap, room, points=None, delim=None):
        """bzh_match_index_device on integer device addresses; `room` entries -> (status, nmatches, out_total, entries)"""
        return self._scan_index_device("match", d_in, n, entries, pattern, d_out, cap, room, points, delim)

    def match_stats(self):
        s = MatchStats()
        self.check(lib().bzh_get_match_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def decode_ranges_stats(self):
        s = DecodeRangesStats()
        self.check(lib().bzh_get_decode_ranges_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def decode_stats(self):
        s = DecodeStats()
        self.check(lib().bzh_get_decode_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def decode_scan(self, data):
        """bzh_decode_scan -> [(bit position, kind)] of every block (0) and footer (1) magic in `data`, ascending"""
        src, n = _input(data)
        cnt = ctypes.c_size_t(0)
        cap = 1024
        while True:
            pos = np.zeros(cap, dtype=np.uint64)
            kind = np.zeros(cap, dtype=np.uint8)
            st = lib().bzh_decode_scan(self._h, ptr(src), n, ptr(pos, u64p), ptr(kind), cap, ctypes.byref(cnt))
            if st == -4 and cnt.value > cap:
                cap = cnt.value
                continue
            self.check(st)
            return list(zip(pos[:cnt.value].tolist(), kind[:cnt.value].tolist()))

    def plan_many_device(self, d_in, lens):
        """bzh_plan_many_device: the plan of inputs lying back to back at d_in -> [(in_off, in_len, rle_len, crc)] in input
        order, in_off relative to d_in"""
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        nb = ctypes.c_size_t(0)
        self.check(lib().bzh_plan_many_device(self._h, ctypes.c_void_p(d_in), ptr(lens, szp), lens.size, ctypes.byref(nb)))
        self._nblocks = nb.value
        return self.plan_blocks()

    def encode_host_ptr(self, in_ptr, n, out_ptr, cap):
        """bzh_encode on raw host addresses (e.g. pinned buffers): H2D + encode + D2H.  -> stream length."""
        olen = ctypes.c_size_t(0)
        used = ctypes.c_size_t(0)
        self.check(lib().bzh_encode(self._h, ctypes.cast(in_ptr, u8p), n, ctypes.cast(out_ptr, u8p), cap,
                                    ctypes.byref(olen), ctypes.byref(used)))
        return int(olen.value)

    def encode_device(self, d_in, n, d_out, cap):
        """Device-resident encode; d_in/d_out are integer device addresses.  -> stream length."""
        olen = ctypes.c_size_t(0)
        used = ctypes.c_size_t(0)
        self.check(lib().bzh_encode_device(self._h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap,
                                           ctypes.byref(olen), ctypes.byref(used)))
        return int(olen.value)

    def plan_device(self, d_in, n, crc=True):
        """-> [(in_off, in_len, rle_len, crc)]; crc=False leaves the CRCs (0 here) to encode_range_device /
        plan_crc_range (the sharded path: a rank only needs the CRCs of the blocks it encodes)"""
        nb = ctypes.c_size_t(0)
        fn = lib().bzh_plan_device if crc else lib().bzh_plan_device_nocrc
        self.check(fn(self._h, ctypes.c_void_p(d_in), n, ctypes.byref(nb)))
        self._nblocks = nb.value
        return self.plan_blocks()

    def plan_device_only(self, d_in, n, crc=True):
        """bzh_plan_device[_nocrc] without turning the block table into Python objects -> number of blocks"""
        nb = ctypes.c_size_t(0)
        fn = lib().bzh_plan_device if crc else lib().bzh_plan_device_nocrc
        self.check(fn(self._h, ctypes.c_void_p(d_in), n, ctypes.byref(nb)))
        self._nblocks = nb.value
        return int(nb.value)

    def plan_tables_device(self, d_in, n):
        """bzh_plan_tables_device: the split's run tables over d_in[0..n) (queued, no wait)"""
        self.check(lib().bzh_plan_tables_device(self._h, ctypes.c_void_p(d_in), n))

    def plan_split_device(self, start, stop=None, crc=False):
        """bzh_plan_split_device: cut blocks from offset `start` of the buffer of plan_tables_device until one starts at
        or after `stop` (None: to the end) -> number of blocks"""
        nb = ctypes.c_size_t(0)
        stop = ctypes.c_size_t(-1).value if stop is None else stop
        self.check(lib().bzh_plan_split_device(self._h, start, stop, 1 if crc else 0, ctypes.byref(nb)))
        self._nblocks = nb.value
        return int(nb.value)

    def plan_blocks_np(self):
        """the plan as one structured numpy array (fields in_off, in_len, rle_len, crc): no per-block Python objects"""
        n = getattr(self, "_nblocks", 0)
        blocks = (Block * max(1, n))()
        self.check(lib().bzh_plan_blocks(self._h, blocks, max(1, n)))
        return np.frombuffer(blocks, dtype=_BLOCK_DTYPE, count=n).copy()

    def plan_open_np(self):
        n = getattr(self, "_nblocks", 0)
        flags = np.zeros(max(1, n), dtype=np.uint8)
        self.check(lib().bzh_plan_open(self._h, ptr(flags), max(1, n)))
        return flags[:n].astype(bool)

    def plan_blocks(self):
        n = getattr(self, "_nblocks", 0)
        blocks = (Block * max(1, n))()
        self.check(lib().bzh_plan_blocks(self._h, blocks, max(1, n)))
        # one numpy view instead of 4 ctypes field reads per block (≈ 1 ms per 1000 blocks otherwise)
        arr = np.frombuffer(blocks, dtype=_BLOCK_DTYPE, count=n)
        return list(zip(arr["in_off"].tolist(), arr["in_len"].tolist(), arr["rle_len"].tolist(), arr["crc"].tolist()))

    def plan_open(self):
        """per block of the last plan: True if its cut could still move were the input longer"""
        n = getattr(self, "_nblocks", 0)
        flags = np.zeros(max(1, n), dtype=np.uint8)
        self.check(lib().bzh_plan_open(self._h, ptr(flags), max(1, n)))
        return [bool(x) for x in flags[:n]]

    def plan_crc_range(self, b0, b1):
        """CRCs of plan blocks [b0, b1) (computed now unless already known) -> [crc]"""
        self.check(lib().bzh_plan_crc_range(self._h, b0, b1))
        return [b[3] for b in self.plan_blocks()[b0:b1]]

    def encode_range_device(self, b0, b1, d_out, cap):
        nbits = ctypes.c_uint64(0)
        self.check(lib().bzh_encode_range_device(self._h, b0, b1, ctypes.c_void_p(d_out), cap, ctypes.byref(nbits)))
        return int(nbits.value)

    def assemble_device(self, segs, crcs, d_out, cap):
        """segs: [(device address, nbits)], crcs: block CRCs in block order -> stream length."""
        nseg = len(segs)
        ptrs = (ctypes.c_void_p * max(1, nseg))(*[ctypes.c_void_p(p) for p, _ in segs])
        bits = np.array([b for _, b in segs] or [0], dtype=np.uint64)
        c = np.array(list(crcs) or [0], dtype=np.uint32)
        olen = ctypes.c_size_t(0)
        self.check(lib().bzh_assemble_device(self._h, ptrs, ptr(bits, u64p), nseg, ptr(c, u32p), len(crcs),
                                             ctypes.c_void_p(d_out), cap, ctypes.byref(olen)))
        return int(olen.value)

    # ---- streaming (bzh_stream_*) ----
    def stream_begin(self, chunk_bytes=None):
        if chunk_bytes is not None:
            self.check(lib().bzh_stream_set_chunk(self._h, chunk_bytes))
        self.check(lib().bzh_stream_begin(self._h))
        # (the output buffer of the previous stream is kept: a fresh numpy array costs a page fault per 4 KiB the library
        # writes -- several milliseconds per stream for the ~30 MB a 100 MB input produces)
        if not hasattr(self, "_sbuf"):
            self._sbuf = None

    def stream_feed(self, data, eof=False):
        """-> stream bytes that became final with this feed"""
        n = len(data)
        a = np.frombuffer(data, dtype=np.uint8) if n else np.zeros(1, np.uint8)  # zero-copy view of any buffer
        need = int(lib().bzh_stream_bound(self._h, n))
        if self._sbuf is None or self._sbuf.size < need:
            self._sbuf = np.empty(need, dtype=np.uint8)
        got = ctypes.c_size_t(0)
        self.check(lib().bzh_stream_feed(self._h, ptr(np.ascontiguousarray(a)), n, 1 if eof else 0, ptr(self._sbuf),
                                         self._sbuf.size, ctypes.byref(got)))
        return self._sbuf[:got.value].tobytes()

    def stream_feed_view(self, data, eof=False):
        """as stream_feed, but returns a memoryview of the context's output buffer (valid until the next feed)"""
        n = len(data)
        a = np.frombuffer(data, dtype=np.uint8) if n else np.zeros(1, np.uint8)
        need = int(lib().bzh_stream_bound(self._h, n))
        if self._sbuf is None or self._sbuf.size < need:
            self._sbuf = np.empty(need, dtype=np.uint8)
        got = ctypes.c_size_t(0)
        self.check(lib().bzh_stream_feed(self._h, ptr(a), n, 1 if eof else 0, ptr(self._sbuf), self._sbuf.size,
                                         ctypes.byref(got)))
        return memoryview(self._sbuf)[:got.value]

    def stream_consumed(self):
        return int(lib().bzh_stream_consumed(self._h))

    def stream_begin_index(self, interval, chunk_bytes=None):
        """bzh_stream_begin_index: stream_begin for a stream that records its index (interval 0: entries only)"""
        if chunk_bytes is not None:
            self.check(lib().bzh_stream_set_chunk(self._h, chunk_bytes))
        self.check(lib().bzh_stream_begin_index(self._h, interval))
        if not hasattr(self, "_sbuf"):
            self._sbuf = None

    def stream_index_pending(self):
        """bzh_stream_index_pending -> (entries, sync points) that are final and not yet taken"""
        cnt, npts = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self.check(lib().bzh_stream_index_pending(self._h, ctypes.byref(cnt), ctypes.byref(npts)))
        return int(cnt.value), int(npts.value)

    def stream_index_take_raw(self, max_entries, max_pts):
        """one bzh_stream_index_take call with arrays of the given room -> (status, entries, points, count, npts); nothing is
        raised, the arrays are cut to the counts only on status 0"""
        ent = np.empty(max(max_entries, 1), dtype=INDEX_DTYPE)
        pts = np.empty(max(max_pts, 1), dtype=SYNC_DTYPE)
        cnt, npts = ctypes.c_size_t(0), ctypes.c_size_t(0)
        st = lib().bzh_stream_index_take(self._h, ent.ctypes.data_as(idxp) if max_entries else None, max_entries, ctypes.byref(cnt),
                                         pts.ctypes.data_as(syncp) if max_pts else None, max_pts, ctypes.byref(npts))
        if st == 0:
            ent, pts = ent[:cnt.value], pts[:npts.value]
        return st, ent, pts, int(cnt.value), int(npts.value)

    def stream_index_take(self):
        """bzh_stream_index_take, sized by bzh_stream_index_pending -> (entries as an array of INDEX_DTYPE, points as an array
        of SYNC_DTYPE): what has become final since the last take, in stream coordinates"""
        ne, npt = self.stream_index_pending()
        st, ent, pts, _, _ = self.stream_index_take_raw(ne, npt)
        self.check(st)
        return ent.copy(), pts.copy()

    # ---- streaming decode (bzh_dstream_*) ----
    def dstream_set_room(self, window=0, staging=0):
        """targets of the window and the staging buffer for the next dstream_begin (0: the library's default)"""
        self.check(lib().bzh_dstream_set_room(self._h, window, staging))

    def dstream_begin(self):
        self.check(lib().bzh_dstream_begin(self._h))

    def dstream_feed_raw(self, data, eof, out):
        """one bzh_dstream_feed call: `data` bytes-like, `out` a uint8 array whose size is the call's cap ->
        (status, input bytes used, bytes written to out, done); nothing is raised"""
        a = np.frombuffer(data, dtype=np.uint8)
        n = a.size
        used, got, done = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(0)
        st = lib().bzh_dstream_feed(self._h, ptr(np.ascontiguousarray(a)) if n else None, n, 1 if eof else 0, ctypes.byref(used),
                                    ptr(out) if out.size else None, out.size, ctypes.byref(got), ctypes.byref(done))
        return st, int(used.value), int(got.value), bool(done.value)

    def dstream_feed(self, data, eof, out):
        """bzh_dstream_feed -> (input bytes used, bytes written to out, done)"""
        st, used, got, done = self.dstream_feed_raw(data, eof, out)
        self.check(st)
        return used, got, done

    def dstream_consumed(self):
        return int(lib().bzh_dstream_consumed(self._h))

    def dstream_stats(self):
        st = DStreamStats()
        self.check(lib().bzh_dstream_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def dstream_end(self):
        self.check(lib().bzh_dstream_end(self._h))


class MultiContext:
    """Several GPUs behind one handle (bzh_create_multi): one host thread and one context per listed device inside the
    library, block ranges chained by start offset, the bit strings assembled on devices[0].  A device may be listed more
    than once (one context per entry)."""

    def __init__(self, devices, level=9):
        self.devices = [int(d) for d in devices]
        self.level = level
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        st = lib().bzh_create_multi(ctypes.byref(self._h), arr, len(self.devices), level)
        if st != 0:
            raise BzhError(st, lib().bzh_strerror(st).decode())

    def close(self):
        if self._h:
            lib().bzh_destroy_multi(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def check(self, st):
        if st != 0:
            raise BzhError(st, lib().bzh_strerror(st).decode() + ": " + lib().bzh_multi_last_error(self._h).decode())

    @staticmethod
    def _in(data):
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        return a if a.size else np.zeros(1, dtype=np.uint8), int(a.size)

    def encode(self, data):
        """bytes-like -> the whole .bz2 stream (bytes)"""
        a, n = self._in(data)
        cap = n + n // 4 + (n // 70000 + 4) * 4096 + 65536
        out = np.empty(cap, dtype=np.uint8)
        got, used = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self.check(lib().bzh_multi_encode(self._h, ptr(a), n, ptr(out), cap, ctypes.byref(got), ctypes.byref(used)))
        return out[:got.value].tobytes()

    def load(self, data):
        a, n = self._in(data)
        self.check(lib().bzh_multi_load(self._h, ptr(a), n))

    def run(self):
        got = ctypes.c_size_t(0)
        self.check(lib().bzh_multi_run(self._h, ctypes.byref(got)))
        return got.value

    def fetch(self, n):
        out = np.empty(max(1, n), dtype=np.uint8)
        self.check(lib().bzh_multi_fetch(self._h, ptr(out), out.size))
        return out[:n].tobytes()

    def debug_slab(self, nbytes):
        self.check(lib().bzh_multi_debug_slab(self._h, nbytes))

    def times(self):
        w = len(self.devices)
        buf = (ctypes.c_double * (5 * w))()
        self.check(lib().bzh_multi_times(self._h, buf, w))
        keys = ("ms_load", "ms_wait", "ms_plan", "ms_encode", "ms_copy")
        return [dict(zip(keys, (round(buf[5 * r + k], 3) for k in range(5)))) for r in range(w)]
