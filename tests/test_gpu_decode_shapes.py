"""GPU: the decoder on blocks no encoder writes (tests/decode_shapes.py) -- the shapes that drive exactly the code that differs
between the one-lane CPU build of decode_core.h and the device: the lane-split look-up-table fill, the slow path behind the
10-bit table, the 64-wide slices of the MTF shift, the whole-wave run store, the segment kernel's table set, the doubling
inverse transform on columns that are no BWT of anything, and unrle_crc behind it.  The expected bytes come from the
construction; tests/test_decode_shapes_host.py holds libbz2, the strict decoder and the sanitizer build to the same bytes.
Accepted blocks first, refused ones last."""
import numpy as np
import pytest

from tests import bz2_handbuilt, decode_shapes
from tests.golden import pymodel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec(native):
    """the decoding context: level 9 (every stream's level fits), batches of 8 blocks"""
    c = native.Context(0, 9, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def concatenation():
    """every accepted stream, level 1 and level 9 mixed, as one input; and what it decodes to"""
    c = decode_shapes.accepted()
    assert [b.level for b in c.values()].count(1) >= 8 and [b.level for b in c.values()].count(9) >= 8
    return b"".join(b.stream for b in c.values()), b"".join(b.expected for b in c.values())


# ---- accepted --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(decode_shapes.accepted()))
def test_accepted_block(dec, name):
    b = decode_shapes.accepted()[name]
    got, used = dec.decode(b.stream, size_hint=len(b.expected), with_consumed=True)
    assert used == len(b.stream)
    assert got == b.expected


def test_all_in_one_call(dec, concatenation):
    s, want = concatenation
    got, used = dec.decode(s, size_hint=len(want), with_consumed=True)
    assert used == len(s) and got == want
    st = dec.decode_stats()
    n = len(decode_shapes.accepted())
    assert st["streams"] == n and st["blocks"] == n and st["out_bytes"] == len(want)


def test_index_verifies_every_crc_without_output(dec, concatenation):
    s, want = concatenation
    ent, total, used = dec.decode_index(s)
    c = list(decode_shapes.accepted().values())
    assert len(ent) == len(c) and total == len(want) and used == len(s)
    assert ent["out_len"].tolist() == [len(b.expected) for b in c]
    assert ent["crc"].tolist() == [b.crc for b in c] == [pymodel.checksum(b.expected) for b in c]
    assert ent["level"].tolist() == [b.level for b in c]
    assert ent["out_off"].tolist() == np.concatenate([[0], np.cumsum([len(b.expected) for b in c])[:-1]]).tolist()


@pytest.mark.parametrize("name", [n for n, b in decode_shapes.accepted().items() if b.nsyms > 50])
def test_segments_at_interval_one(dec, name):
    """a sync point in front of every group but the first, then every segment in a wavefront of its own with the small table set:
    six tables, 20-bit codes, selectors beyond the last group, shifts from position 255"""
    b = decode_shapes.accepted()[name]
    ent, pts, total, used = dec.decode_index_sync(b.stream, 1)
    assert len(ent) == 1 and total == len(b.expected) and used == len(b.stream)
    assert len(pts) == b.groups - 1  # the groups that hold symbols, not the selectors written (b.nsel may be far more)
    assert pts["group"].tolist() == list(range(1, b.groups)) and int(pts["out_pos"].max()) <= b.nblock
    assert dec.decode_range_sync(b.stream, ent, pts, 0, total) == b.expected
    for at in sorted(set(pts["out_pos"].tolist())):  # windows across every point's position
        lo = max(0, min(at, total - 1) - 3)
        assert dec.decode_range_sync(b.stream, ent, pts, lo, 7) == b.expected[lo:lo + 7], at


def test_inverse_transform_of_columns_that_are_no_bwt(native, dec):
    """bzh_unbwt_batch follows libbz2's walk on any column: where a cycle of the walk does not divide the block's length, the last
    byte is not the one at the origin pointer"""
    cols = [(b"ab" * 500 + b"ba" * 500, 0), (b"ab" * 500 + b"ba" * 500, 1), (b"ab" * 500 + b"ba" * 500, 1999),
            (bytes(range(256)) + bytes(range(255, -1, -1)) * 20, 5000), (b"x", 0), (b"nnbaaa", 5), (b"ab" * 2048, 4095), (b"ba" * 2048 + b"a", 7)]
    want = [bz2_handbuilt.inverse_column(col, ptr) for col, ptr in cols]
    assert sum(w[-1] != col[ptr] for w, (col, ptr) in zip(want, cols)) >= 3
    assert dec.unbwt_batch(cols) == want


# ---- refused (after everything valid) --------------------------------------------------------------------------------------
def test_refused_blocks(dec, native):
    good = decode_shapes.accepted()["six_tables"]
    for name, s in decode_shapes.refused().items():
        with pytest.raises(native.BzhError) as e:
            dec.decode(s)
        assert e.value.status == -6, (name, str(e.value))
        assert "field outside the format" in str(e.value), (name, str(e.value))
        assert dec.decode(good.stream) == good.expected  # the context decodes a valid stream right after


def test_oversubscribed_table_that_no_selector_names(dec, native):
    """The one divergence from libbz2, kept on purpose: a table with more codes than its lengths hold is refused even where no
    selector names it.  libbz2 accepts that unused-table form (it never checks a table); bzd_parse_header builds and checks every
    table up front."""
    b = decode_shapes.oversubscribed_unused_table()
    with pytest.raises(native.BzhError) as e:
        dec.decode(b.stream)
    assert e.value.status == -6 and "field outside the format" in str(e.value)
    good = decode_shapes.accepted()["lengths_5_and_6"]
    assert dec.decode(good.stream) == good.expected
