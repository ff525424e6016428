"""The blocks of tests/test_decode_shapes_host.py and tests/test_gpu_decode_shapes.py: format-legal blocks no encoder writes
(tests/bz2_handbuilt.py frames them), and a short list of blocks just outside the format.  Built once a process, from seeds; the
expected bytes come from the construction (the serial inverse of bz2_handbuilt), never from a decoder."""
import functools
import random

from tests import bz2_handbuilt as hb
from tests.golden import pymodel

ALPHA19 = bytes(range(40, 59))  # 19 bytes in use: an alphabet of 21 symbols
ASCENDING = list(range(1, 20)) + [20, 20]  # a complete code: 1, 2, ..., 19, 20, 20 -- the 20-bit codes on position 18 and on EOB
EDGE_POSITIONS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255)
EDGE_RUNS = (1, 2, 3, 63, 64, 65, 127, 128, 129)
# libbz2 before 1.0.8 refuses more than 18,002 selectors; these, and only these, it may refuse
LIBBZ2_MAY_REFUSE = ("selectors_18003", "selectors_32767")
# what oracle/bz2_decode.c refuses of the accepted list (name -> why): nothing
ORACLE_REFUSES = {}


def huffman_tables(rng, num_syms, count):
    """`count` complete codes over num_syms symbols, from random frequencies (lengths up to 17)"""
    return [pymodel.build_table_from_freqs(num_syms, [rng.choice((0, 1, 3, 20, 400)) for _ in range(num_syms)]) for _ in range(count)]


def events19(rng, n):
    """about n symbols over the 19-byte alphabet: every byte once (position 18, 19 times), then positions 1..18, each of them, and
    short runs"""
    ev = list(range(1, 19)) * 2
    ev += [rng.randrange(1, 19) for _ in range(n - 19 - len(ev))]
    rng.shuffle(ev)
    out = [18] * 19
    for k, p in enumerate(ev):
        out.append(p)
        if k % 7 == 3:
            out.append(("run", 1 + k % 5))
    return out


@functools.lru_cache(maxsize=None)
def accepted():
    """{name: Built}, in a fixed order"""
    rng = random.Random(20261018)
    c = {}
    # ---- code lengths
    col19 = hb.column_of_events(ALPHA19, events19(rng, 130))
    c["lengths_1_to_20"] = hb.stream_of_column(col19, 7, 1, [ASCENDING, ASCENDING], lambda g: g & 1)
    c["lengths_20_to_1"] = hb.stream_of_column(col19, 0, 9, [ASCENDING[::-1], ASCENDING[::-1]], lambda g: 0)
    c["lengths_all_20"] = hb.stream_of_column(col19, 11, 1, [[20] * 21, [20] * 21, [20] * 21], lambda g: g % 3)
    c["lengths_5_and_6"] = hb.stream_of_column(col19, 3, 9, [[5, 6] * 10 + [5], [6, 5] * 10 + [6]], lambda g: g & 1)
    all256 = bytes(range(256))
    col256 = hb.column_of_events(all256, [255] * 256 + [rng.randrange(1, 256) for _ in range(500)])
    c["lengths_10_and_11"] = hb.stream_of_column(col256, 400, 1, [[10, 11] * 129, [11, 10] * 129], lambda g: g & 1)
    # ---- the smallest block
    c["one_byte_short_code"] = hb.stream_of_column(b"x", 0, 1, [[1, 2, 2], [20, 20, 20]], [0])
    c["one_byte_long_code"] = hb.stream_of_column(b"x", 0, 9, [[1, 2, 2], [20, 20, 20]], [1])
    c["origptr_first"] = hb.stream_of_column(b"nnbaaa", 0, 1, [[2, 2, 3, 3, 3]] * 2, [0])
    c["origptr_last"] = hb.stream_of_column(b"nnbaaa", 5, 9, [[2, 2, 3, 3, 3]] * 2, [1])
    # ---- tables and selectors
    col = hb.column_of_events(ALPHA19, events19(rng, 1950))
    six = huffman_tables(rng, 21, 6)
    c["six_tables"] = hb.stream_of_column(col, 1000, 1, six, [rng.randrange(6) for _ in range(200)].__getitem__)
    c["six_tables_one_used"] = hb.stream_of_column(col, 0, 9, six, lambda g: 0)
    c["two_tables_alternating"] = hb.stream_of_column(col, len(col) - 1, 1, six[2:4], lambda g: g & 1)
    small = hb.column_of_events(ALPHA19, events19(rng, 60))
    groups = hb.stream_of_column(small, 0, 1, six, lambda g: 0).groups
    for name, extra, level in (("selectors_1_extra", 1, 1), ("selectors_100_extra", 100, 9), ("selectors_18002", 18002 - groups, 1),
                               ("selectors_18003", 18003 - groups, 9), ("selectors_32767", 32767 - groups, 1)):
        c[name] = hb.stream_of_column(small, 5, level, six, lambda g: 5 - g % 6, extra_selectors=[rng.randrange(6) for _ in range(extra)])
    # ---- the MTF shift
    ev = [255] * 256 + [p for p in EDGE_POSITIONS for _ in range(3)] + [rng.randrange(1, 256) for _ in range(300)]
    tail = ev[256:]
    rng.shuffle(tail)
    col = hb.column_of_events(all256, ev[:256] + tail)
    c["mtf_edges"] = hb.stream_of_column(col, 123, 9, huffman_tables(rng, 258, 4), [rng.randrange(4) for _ in range(100)].__getitem__)
    c["mtf_always_255"] = hb.stream_of_column(all256 * 40, 10_000, 1, huffman_tables(rng, 258, 2) + [[9] * 258], lambda g: g % 3)
    # ---- runs
    ev = [1, 2, 3, 4] * 11 + [1, 2, 3]  # 47 symbols, then the seven digits of a run of 129: they straddle the first group's end
    for k, r in enumerate((129,) + EDGE_RUNS + EDGE_RUNS[::-1]):
        ev += [("run", r), 1 + k % 4]
    col = hb.column_of_events(b"\x00\x01\x7f\xfe\xff", ev)
    c["runs"] = hb.stream_of_column(col, 77, 1, [[3, 3, 3, 3, 3, 3, 3], [2, 2, 4, 4, 4, 4, 20]], lambda g: g & 1)
    c["run_900000"] = hb.stream_of_column(b"\x03" * 900_000, 0, 9, [[1, 2, 2], [1, 2, 2]], [0])
    # ---- columns that are no BWT of anything
    abba = b"ab" * 500 + b"ba" * 500
    for ptr, level in ((0, 1), (1, 9), (1999, 1)):
        c[f"no_bwt_abba_{ptr}"] = hb.stream_of_column(abba, ptr, level, [[2, 2, 2, 2], [1, 2, 3, 3]], lambda g: g & 1)
    ramp = all256 + all256[::-1] * 20
    c["no_bwt_ramp"] = hb.stream_of_column(ramp, 5000, 9, huffman_tables(rng, 258, 3), lambda g: 2 - g % 3)
    return c


# Table 1 is over-subscribed (21 codes of one bit) and no selector names it.  libbz2 builds its tables without checking them and so
# decodes the block; this decoder builds and checks every table up front and refuses it (include/bzhip.h), as does
# oracle/bz2_decode.c.  An over-subscribed table that IS used has no meaning worth reproducing.
@functools.lru_cache(maxsize=None)
def oversubscribed_unused_table():
    col = hb.column_of_events(ALPHA19, events19(random.Random(7), 60))
    return hb.stream_of_column(col, 0, 1, [[5, 6] * 10 + [5], [1] * 21], lambda g: 0, damage={"unchecked": 1})


@functools.lru_cache(maxsize=None)
def refused():
    """{name: stream}: each just outside the format; a status from every decoder, never a fault"""
    rng = random.Random(20261019)
    col = hb.column_of_events(ALPHA19, events19(rng, 130))
    good = [ASCENDING, ASCENDING[::-1], [5] * 21]
    ok = hb.stream_of_column(col, 3, 1, good, lambda g: g % 3)
    assert ok.groups >= 3

    def broken(tables=good, **damage):
        return hb.stream_of_column(col, 3, 1, tables, lambda g: g % 3, damage=damage).stream

    c = {}
    c["selector_slot_is_table_count"] = broken(slots=[0, 1, 3] + [0] * (ok.groups - 3))
    c["selector_slot_6"] = broken(slots=[0, 6] + [0] * (ok.groups - 2))
    c["length_runs_to_0"] = broken(tables=[[5] * 21, [2, 1, 0] + [5] * 18, [5] * 21], unchecked=1)
    c["length_runs_to_21"] = broken(tables=[[5] * 21, [19, 20, 21] + [5] * 18, [5] * 21], unchecked=1)
    c["one_table"] = hb.stream_of_column(col, 3, 1, [[5] * 21], lambda g: 0, damage={"unchecked": 1}).stream
    c["seven_tables"] = hb.stream_of_column(col, 3, 1, [[5] * 21] * 7, lambda g: g % 7, damage={"unchecked": 1}).stream
    c["nsel_0"] = broken(slots=[])
    c["nsel_one_short"] = hb.stream_of_column(col, 3, 1, good, [g % 3 for g in range(ok.groups - 1)], damage={"unchecked": 1}).stream
    c["unassigned_code"] = hb.stream_of_column(col, 3, 1, [[20] * 21] * 2, lambda g: 0, damage={"bits": {60: (21, 20)}}).stream
    c["run_900000_at_level_1"] = hb.stream_of_column(b"\x03" * 900_000, 0, 1, [[1, 2, 2]] * 2, [0], damage={"unchecked": 1}).stream
    c["origptr_is_nblock"] = broken(origptr=len(col))
    c["run_of_23_digits"] = hb.stream_of_column(b"\x03" * 5, 0, 9, [[1, 2, 2]] * 2, [0], damage={"syms": [1] * 23 + [2]}).stream
    return c
