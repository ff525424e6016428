"""CPU: the C surface of the streaming decode -- include/bzhip.h declares the six entry points and bzh_dstream_stats, the ctypes
table matches the header, and calls that cannot be served are refused before a device is touched."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bzhip.h")
ENTRY_POINTS = ["bzh_dstream_set_room", "bzh_dstream_begin", "bzh_dstream_feed", "bzh_dstream_consumed", "bzh_dstream_get_stats",
                "bzh_dstream_end"]
STATS_FIELDS = ["passes", "blocks", "streams", "blocks_redone", "tail_moves", "window_grows", "staging_grows", "in_bytes", "out_bytes",
                "window_peak", "staging_peak"]
E_ARG = -1


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_header_declares_the_entry_points_and_the_struct():
    text = header_text()
    for name in ENTRY_POINTS:
        assert re.search(r"BZH_API\s+\w+\s+%s\s*\(" % name, text), name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*bzh_dstream_stats\s*;", text)
    assert m, "bzh_dstream_stats"
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip() for f in decl.replace("uint64_t", "").split(",")]
    assert fields == STATS_FIELDS
    feed = re.search(r"bzh_dstream_feed\s*\(([^)]*)\)", text).group(1)
    assert [a.strip() for a in feed.split(",")] == ["bzh_ctx *ctx", "const uint8_t *in", "size_t n", "int eof", "size_t *in_used",
                                                    "uint8_t *out", "size_t cap", "size_t *out_len", "int *done"]


def test_signatures_match_the_header(native):
    text = header_text()
    for name in ENTRY_POINTS:
        res, args = native.SIGNATURES[name]
        decl = re.search(r"BZH_API\s+(\w+)\s+%s\s*\(([^)]*)\)" % name, text)
        assert {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[decl.group(1)] is res, name
        assert len(args) == len(decl.group(2).split(",")), name
    assert [k for k, _ in native.DStreamStats._fields_] == STATS_FIELDS
    assert ctypes.sizeof(native.DStreamStats) == 8 * len(STATS_FIELDS)


def test_null_calls_are_argument_errors_without_a_device(native):
    lib = native.lib()
    used, got, done = ctypes.c_size_t(7), ctypes.c_size_t(7), ctypes.c_int(7)
    buf = (ctypes.c_uint8 * 16)()
    st = native.DStreamStats()
    assert lib.bzh_dstream_set_room(None, 0, 0) == E_ARG
    assert lib.bzh_dstream_begin(None) == E_ARG
    assert lib.bzh_dstream_feed(None, buf, 16, 1, ctypes.byref(used), buf, 16, ctypes.byref(got), ctypes.byref(done)) == E_ARG
    assert lib.bzh_dstream_feed(None, None, 0, 1, None, None, 0, None, None) == E_ARG
    assert lib.bzh_dstream_consumed(None) == 0
    assert lib.bzh_dstream_get_stats(None, ctypes.byref(st)) == E_ARG
    assert lib.bzh_dstream_get_stats(None, None) == E_ARG
    assert lib.bzh_dstream_end(None) == E_ARG
