"""GPU: the record table and reads by record number (bzh_decode_index_records*, bzh_count_records_device, bzh_record_spans,
bzh_decode_records*, banzai_amd.build_record_index / decompress_records / IndexedReader.readv_records).  The truth is always
bz2.decompress(stream) cut with plain Python on the delimiter; every comparison is byte-exact.  The context takes batches of 2
blocks, so four touched blocks are two batches.  Concatenated streams of chosen sizes put block boundaries exactly where wanted."""
import bisect
import bz2
import functools
import io
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = 2**64 - 1


@functools.lru_cache(maxsize=None)
def text(n, seed, words=40):
    """n bytes of words drawn from a small seeded vocabulary (tests/test_gpu_ranges.py's generator): few symbols keep the serial
    entropy stage, which is nearly all a read costs, short"""
    rng = random.Random(seed)
    vocab = ["".join(rng.choices("etaoinshrdlucmfwypvbgkqjxz", k=rng.randrange(2, 11))) for _ in range(words)]
    return " ".join(rng.choices(vocab, k=n // 4)).encode()[:n]


@functools.lru_cache(maxsize=None)
def lines(n, seed):
    """the same text cut into lines of 0 to 200 bytes"""
    rng = random.Random(seed)
    src, out, at = text(n, seed), bytearray(), 0
    while len(out) < n:
        k = rng.randrange(201) if rng.random() < 0.9 else 0
        out += src[at:at + k] + b"\n"
        at += k
    return bytes(out[:n])


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 2)
    yield c
    c.close()


class Input:
    """a stream, its truth cut into records, and what the library says of it -- computed once, never changed"""

    def __init__(self, dec, parts, level=9, interval=4, delim=b"\n"):
        self.s = b"".join(bz2.compress(p, level) for p in parts) if parts else bz2.compress(b"", level)
        self.truth = bz2.decompress(self.s)
        assert self.truth == b"".join(parts)
        self.delim = delim
        self.pos = [i for i, b in enumerate(self.truth) if b == delim[0]]
        self.D = len(self.pos)
        cut = self.truth.split(delim)
        self.recs = [p + delim for p in cut[:-1]] + [cut[-1]]  # records 0..D by the contract, the tail maybe empty
        self.nrecords = self.D + (len(self.truth) > 0 and not self.truth.endswith(delim))
        self.ent, self.pts, self.cum, self.nrec, total, used = dec.decode_index_records(self.s, interval, delim[0])
        assert total == len(self.truth) and used == len(self.s)
        for a in (self.ent, self.pts, self.cum):
            a.setflags(write=False)

    def want(self, first, count):
        a, b = min(first, self.D + 1), min(first + count, self.D + 1)
        return b"".join(self.recs[a:b])

    def record_at(self, byte):
        """the record that holds output byte `byte`"""
        return bisect.bisect_left(self.pos, byte)

    def touched(self, ranges):
        hit = set()
        ends = np.cumsum(self.ent["out_len"].astype(np.int64))
        block = lambda p: int(np.searchsorted(ends, p, side="right"))
        for first, count in ranges:
            a, b = min(first, self.D + 1), min(first + count, self.D + 1)
            if a == b or not len(self.ent):
                continue
            lo = 0 if a == 0 else block(self.pos[a - 1])
            hi = block(self.pos[b - 1]) if b <= self.D else len(self.ent) - 1
            hit |= set(range(lo, hi + 1))
        return sorted(hit)


T10 = 10_000


@pytest.fixture(scope="module")
def placed(dec):
    """the boundary placements: three parts of about 10,000 bytes (three tiles each), one block each"""
    a, b, c = lines(T10, 1), lines(T10, 2), lines(T10, 3)
    no_nl = text(T10, 4)
    return {
        "ends in newline | begins with newline | none at all": Input(dec, [a[:-1] + b"\n", b"\n" + b[1:], no_nl]),
        "no newline at its end | 300 newlines | text": Input(dec, [a[:-1] + b"x", b"\n" * 300, c]),
        "fourteen a (count byte 10)": Input(dec, [a, b[:5000] + b"a" * 14 + b[5000:] + b"\n\n\n\n\n\n\n" + b"a" * 14, c[:-1] + b"\n"]),
        "none | none | none": Input(dec, [no_nl, text(T10, 5), text(T10, 6)]),
        "empty": Input(dec, []),
        "one byte": Input(dec, [b"x"]),
        "one newline": Input(dec, [b"\n"]),
    }


@pytest.fixture(scope="module")
def four(dec):
    """a level-1 stream of 350,000 bytes (4 blocks) with lines of 0 to 200 bytes, its sync points at interval 4"""
    inp = Input(dec, [lines(350_000, 41)], level=1)
    assert len(inp.ent) == 4 and len(inp.pts) > 8
    return inp


def check(dec, native, inp, ranges, points=None):
    """one call over ascending `ranges`: every range's bytes, the layout, the counters"""
    blob, offs, lens = dec.decode_records(inp.s, inp.ent, inp.cum, ranges, points, delim=inp.delim[0])
    run = 0
    for r, (first, count) in enumerate(ranges):
        w = inp.want(first, count)
        assert offs[r] == run and lens[r] == len(w), (r, ranges[r])
        assert blob[run:run + len(w)] == w, (r, ranges[r])
        run += len(w)
    assert len(blob) == run
    st, ds = dec.decode_ranges_stats(), dec.decode_stats()
    hit = inp.touched(ranges)
    touched, lo, hi = native.record_spans(inp.ent, inp.cum, ranges)
    assert touched.tolist() == hit
    assert st["ranges"] == len(ranges) and st["blocks_touched"] == len(hit) == ds["blocks"] and ds["out_bytes"] == run
    assert st["batches"] == (len(hit) + 1) // 2 and ds["candidates"] == 0
    return st


def boundary_ranges(inp):
    """every record adjacent to a block boundary, record 0 and the tail, ranges behind the end, a count of 2^64 - 1 -- ascending"""
    firsts = {0, inp.D, max(inp.D - 1, 0)}
    for e in inp.ent[1:]:
        b = int(e["out_off"])
        for byte in (b - 2, b - 1, b, b + 1):
            firsts.add(inp.record_at(max(byte, 0)))
    ranges = [(f, 1) for f in sorted(firsts)]
    return ranges + [(inp.D + 1, 3), (inp.D + 7, U64), (U64, U64)]


# ---- 1. the table ---------------------------------------------------------------------------------------------------------
def test_tables_equal_the_python_count(dec, native, placed, four):
    import torch
    for name, inp in list(placed.items()) + [("four blocks", four)]:
        want = [0]
        for e in inp.ent:
            o, n = int(e["out_off"]), int(e["out_len"])
            want.append(want[-1] + inp.truth[o:o + n].count(inp.delim))
        assert inp.cum.tolist() == want and inp.nrec == inp.nrecords and want[-1] == inp.D, name
        # entries and points are decode_index_sync's, byte for byte
        ent, pts, total, used = dec.decode_index_sync(inp.s, 4)
        assert ent.tobytes() == inp.ent.tobytes() and pts.tobytes() == inp.pts.tobytes(), name
        # interval 0: entries only
        ent0, pts0, cum0, nrec0, _, _ = dec.decode_index_records(inp.s, 0, inp.delim[0])
        assert ent0.tobytes() == inp.ent.tobytes() and len(pts0) == 0 and cum0.tolist() == want and nrec0 == inp.nrecords, name
        # the raw side: the same table from the decoded bytes, at every alignment of the buffer
        for shift in (0, 1, 5):
            t = torch.zeros(shift + max(len(inp.truth), 1), dtype=torch.uint8, device="cuda")
            if inp.truth:
                t[shift:] = torch.frombuffer(bytearray(inp.truth), dtype=torch.uint8)
            torch.cuda.synchronize()
            cum, nrec = dec.count_records_device(t.data_ptr() + shift, len(inp.truth), inp.ent, inp.delim[0])
            assert cum.tolist() == want and nrec == inp.nrecords, (name, shift)


def test_another_delimiter(dec, native, placed):
    inp0 = placed["fourteen a (count byte 10)"]
    for delim in (b"a", b" ", b"\x00"):
        ent, pts, cum, nrec, _, _ = dec.decode_index_records(inp0.s, 4, delim[0])
        want = [0]
        for e in ent:
            o, n = int(e["out_off"]), int(e["out_len"])
            want.append(want[-1] + inp0.truth[o:o + n].count(delim))
        assert cum.tolist() == want and nrec == want[-1] + (not inp0.truth.endswith(delim))
        cut = inp0.truth.split(delim)
        recs = [p + delim for p in cut[:-1]] + [cut[-1]]
        k = want[1] + 1  # a record of the second block
        blob, offs, lens = dec.decode_records(inp0.s, ent, cum, [(0, 1), (k, 2)], pts, delim=delim[0])
        assert blob == recs[0] + b"".join(recs[k:k + 2]) and lens == [len(recs[0]), len(b"".join(recs[k:k + 2]))]


# ---- 2. reads ---------------------------------------------------------------------------------------------------------------
def test_boundary_placements(dec, native, placed):
    for name, inp in placed.items():
        for points in (None, inp.pts):
            check(dec, native, inp, boundary_ranges(inp), points)
            check(dec, native, inp, [(0, U64)], points)                              # the whole file as one range
            check(dec, native, inp, [(r, 1) for r in range(inp.D + 2)], points)      # every record as its own range
            check(dec, native, inp, [(0, 0), (0, 1), (1, 0), (1, 0), (1, 2), (3, U64)], points)  # empty and adjacent
        check(dec, native, inp, [])
    # a block whose last byte is the boundary delimiter is touched although it gives no bytes
    inp = placed["ends in newline | begins with newline | none at all"]
    k = int(inp.cum[1])  # the record behind block 0's last newline: the lone newline that opens block 1
    st = check(dec, native, inp, [(k, 1)])
    assert inp.want(k, 1) == b"\n" and st["blocks_touched"] == 2 and native.record_spans(inp.ent, inp.cum, [(k, 1)])[0].tolist() == [0, 1]
    # fourteen a are no newline
    inp = placed["fourteen a (count byte 10)"]
    assert b"a" * 14 in b"".join(inp.recs) and inp.D == inp.truth.count(b"\n")


def test_four_blocks_two_batches(dec, native, four):
    import banzai_amd
    inp = four
    rng = random.Random(7)
    seeded = [(rng.randrange(inp.D + 20), rng.choice([0, 1, 1, 2, 5, rng.randrange(400)])) for _ in range(200)]
    rindex = banzai_amd.RecordIndex(banzai_amd.SyncIndex(banzai_amd.BlockIndex(inp.ent, len(inp.s)), inp.pts, 4), inp.delim, inp.cum, inp.nrec)
    plain = banzai_amd.RecordIndex(rindex.index.blocks, inp.delim, inp.cum, inp.nrec)
    clipped = lambda f, c: b"".join(inp.recs[:inp.nrecords][f:f + c])
    for ri in (rindex, plain):  # with and without points: any order, overlapping, through the atom cut
        assert banzai_amd.decompress_records(inp.s, ri, seeded) == [clipped(f, c) for f, c in seeded]
    for points in (None, inp.pts):
        check(dec, native, inp, boundary_ranges(inp), points)
        st = check(dec, native, inp, [(0, U64)], points)
        assert st["blocks_touched"] == 4 and st["blocks_whole"] == 4 and st["batches"] == 2
        st = check(dec, native, inp, [(r, 1) for r in range(inp.D + 1)], points)
        assert st["blocks_touched"] == 4 and st["pieces"] >= inp.D
        # one range that spans both batches, between two that do not
        m1 = inp.record_at(int(inp.ent[1]["out_off"]) + 5000)
        m2 = inp.record_at(int(inp.ent[2]["out_off"]) + 5000)
        st = check(dec, native, inp, [(3, 2), (m1, m2 - m1), (m2 + 10, 1)], points)
        assert st["blocks_touched"] == 3 and st["batches"] == 2
        st = check(dec, native, inp, [(inp.record_at(int(inp.ent[3]["out_off"]) + 5000) + 1, 2)], points)  # (both delimiters inside block 3)
        assert st["blocks_touched"] == 1 and st["batches"] == 1


# ---- 3. the room ------------------------------------------------------------------------------------------------------------
def test_cap_too_small_reports_the_room(dec, native, four):
    import torch
    inp = four
    m1 = inp.record_at(int(inp.ent[1]["out_off"]) + 5000)
    m2 = inp.record_at(int(inp.ent[2]["out_off"]) + 5000)
    ranges = [(2, 3), (m1, m2 - m1), (m2 + 4, 2)]
    want = b"".join(inp.want(f, c) for f, c in ranges)
    total = len(want)
    for cap in (total - 1, 10, 0):
        st, got, offs, lens, _ = dec.decode_records_raw(inp.s, inp.ent, inp.cum, ranges, cap, inp.pts)
        assert st == -4 and got == total and lens == [len(inp.want(f, c)) for f, c in ranges] and offs[2] == lens[0] + lens[1], cap
        assert "hold" in dec.last_error()
    st, got, offs, lens, out = dec.decode_records_raw(inp.s, inp.ent, inp.cum, ranges, total, inp.pts)
    assert st == 0 and got == total and out[:total].tobytes() == want
    # the device variant writes nothing outside d_out[0, total), at any alignment, and nothing behind a cap that is too small
    t_in = torch.frombuffer(bytearray(inp.s), dtype=torch.uint8).cuda()
    for shift in (0, 1, 3):
        t_out = torch.full((64 + shift + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st, got, offs, lens = dec.decode_records_device(t_in.data_ptr(), len(inp.s), inp.ent, inp.cum, ranges, t_out.data_ptr() + 64 + shift, total)
        assert st == 0 and got == total
        host = t_out.cpu().numpy().tobytes()
        assert host[64 + shift:64 + shift + total] == want and host[:64 + shift] == b"\xA5" * (64 + shift) and host[64 + shift + total:] == b"\xA5" * 64
    t_out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cap = lens[0] + 100
    st, got, offs, lens = dec.decode_records_device(t_in.data_ptr(), len(inp.s), inp.ent, inp.cum, ranges, t_out.data_ptr(), cap)
    assert st == -4 and got == total
    assert t_out.cpu().numpy().tobytes()[cap:] == b"\xA5" * (total + 64 - cap)


# ---- 4. what is not trusted ---------------------------------------------------------------------------------------------------
def test_untrusted_table_ranges_and_bytes(dec, native, four):
    inp = four
    good = [(5, 3), (inp.record_at(int(inp.ent[2]["out_off"]) + 9), 2)]

    def fine():
        blob, _, _ = dec.decode_records(inp.s, inp.ent, inp.cum, good, inp.pts)
        assert blob == b"".join(inp.want(f, c) for f, c in good)

    fine()
    # one count moved from a block to its neighbour: the blocks counted say otherwise
    moved = inp.cum.copy()
    moved[2] -= 1  # block 1 loses one, block 2 gains it
    cap = len(inp.truth)
    k = int(inp.cum[1]) + 3  # a record inside block 1
    st, *_ = dec.decode_records_raw(inp.s, inp.ent, moved, [(k, 2)], cap)
    assert st == -6 and "record table does not match entry 1" in dec.last_error()
    fine()
    st, *_ = dec.decode_records_raw(inp.s, inp.ent, moved, [(int(inp.cum[2]) + 3, 2)], cap, inp.pts)
    assert st == -6 and "record table does not match entry 2" in dec.last_error()
    fine()
    # a table that is none
    for at, v, what in ((0, 1, "rec_cum[0]"), (2, int(inp.cum[1]) - 1, "descend"), (1, int(inp.ent[0]["out_len"]) + 1, "more delimiters")):
        bad = inp.cum.copy()
        bad[at] = v
        if at == 1:
            bad[2:] += bad[1]
        st, *_ = dec.decode_records_raw(inp.s, inp.ent, bad, good, cap)
        assert st == -1 and what in dec.last_error(), dec.last_error()
        with pytest.raises(native.BzhError):
            native.record_spans(inp.ent, bad, good)
        fine()
    # ranges that descend or overlap
    for ranges, which in (([(9, 1), (5, 1)], "range 1"), ([(5, 3), (7, 1)], "range 1"), ([(1, 1), (2, 1), (3, 2), (4, 1)], "range 3")):
        st, *_ = dec.decode_records_raw(inp.s, inp.ent, inp.cum, ranges, cap)
        assert st == -1 and which in dec.last_error(), dec.last_error()
        fine()
    # one payload bit flipped in a touched block: as for bzh_decode_ranges
    bad = bytearray(inp.s)
    mid = (int(inp.ent[2]["bit_pos"]) + int(inp.ent[2]["end_bit"])) // 16
    bad[mid] ^= 0x10
    for points in (None, inp.pts):
        st, *_ = dec.decode_records_raw(bytes(bad), inp.ent, inp.cum, good, cap, points)
        assert st == -6 and "index entry 2" in dec.last_error(), dec.last_error()
        blob, _, _ = dec.decode_records(bytes(bad), inp.ent, inp.cum, [(5, 3)], points)  # (the damaged block is not touched)
        assert blob == inp.want(5, 3)
    fine()
    # a buffer that does not cover the hull
    touched, lo, hi = native.record_spans(inp.ent, inp.cum, good)
    blob, _, _ = dec.decode_records(inp.s[lo:hi], inp.ent, inp.cum, good, inp.pts, in_byte_base=lo)
    assert blob == b"".join(inp.want(f, c) for f, c in good)
    st, *_ = dec.decode_records_raw(inp.s[lo:hi - 1], inp.ent, inp.cum, good, cap, in_byte_base=lo)
    assert st == -1 and "the buffer holds" in dec.last_error()
    fine()


# ---- 5. Python ---------------------------------------------------------------------------------------------------------------
def test_python_layer(native, placed, four, tmp_path):
    import banzai_amd
    import torch
    for inp in (four, placed["ends in newline | begins with newline | none at all"], placed["empty"], placed["one byte"]):
        ri = banzai_amd.build_record_index(inp.s, b"\n", 4 if inp is four else 256)
        assert len(ri) == inp.nrecords and ri.rec_cum.tolist() == inp.cum.tolist() and ri.delim == 10
        recs = inp.recs[:inp.nrecords]
        rng = random.Random(3)
        ranges = [(rng.randrange(len(recs) + 3), rng.randrange(6)) for _ in range(40)] + [(0, U64), (2, 2), (1, 3), (2, 2)]
        rng.shuffle(ranges)
        want = [b"".join(recs[f:f + c]) for f, c in ranges]
        assert banzai_amd.decompress_records(inp.s, ri, ranges) == want
        # the file round trip, and a reader over a file object that is asked for the hull alone
        path = tmp_path / "records.idx"
        path.write_bytes(ri.to_bytes())
        back = banzai_amd.RecordIndex.from_bytes(path.read_bytes())
        assert back.to_bytes() == ri.to_bytes() and type(back.index) is type(ri.index)

        class Spy(io.BytesIO):
            reads = []

            def read(self, n=-1):
                Spy.reads.append((self.tell(), n))
                return super().read(n)

        Spy.reads = []
        rd = banzai_amd.IndexedReader(Spy(inp.s), back)
        assert rd.readv_records(ranges) == want
        if len(recs) > 2:
            Spy.reads = []
            assert rd.read_records(1, 1) == recs[1]
            _, lo, hi = ri.spans([(1, 1)])
            assert Spy.reads == [(lo, hi - lo)]
        # the raw side builds the same index from the decoded bytes: a device tensor, or bytes
        if inp.truth:
            t = torch.frombuffer(bytearray(inp.truth), dtype=torch.uint8).cuda()
            assert banzai_amd.record_index_of(t, ri.index).to_bytes() == ri.to_bytes()
        assert banzai_amd.record_index_of(inp.truth, ri.index, b"\n").to_bytes() == ri.to_bytes()
    # after encode_indexed the encoder's own input gives the table with no decode
    raw = lines(120_000, 9)
    out = io.BytesIO()
    index = banzai_amd.encode_indexed(io.BytesIO(raw), out, 1, 8)
    ri = banzai_amd.record_index_of(raw, index)
    assert ri.to_bytes() == banzai_amd.build_record_index(out.getvalue(), b"\n", 8).to_bytes()
    assert banzai_amd.decompress_records(out.getvalue(), ri, [(7, 2)]) == [b"".join((raw.split(b"\n")[7] + b"\n", raw.split(b"\n")[8] + b"\n"))]
