"""GPU: search inside decoded bytes that stay on the device (bzh_search_raw_device, bzh_search*, bzh_search_range*,
banzai_amd.search / search_range / IndexedReader.search / grep, bnzhip --search).  The truth is always bz2.decompress(stream)
searched with a bytes.find loop that steps by one, and truth.count(delim, 0, off) for the record of a hit.  The context takes
batches of 2 candidates, so the five blocks of the input are several batches; concatenated streams of chosen sizes put block,
batch and stream boundaries where wanted."""
import bz2
import functools
import io
import os
import random
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289)
PLENS = (1, 2, 3, 4, 5, 16, 17, 255, 256)
NEEDLE = b"QZ@needle#XJ"


@functools.lru_cache(maxsize=None)
def text(n, seed, words=40):
    """n bytes of words drawn from a small seeded vocabulary (tests/test_gpu_records.py's generator)"""
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


def find_all(truth, pat, lo=0, hi=None):
    """every occurrence that lies wholly inside truth[lo:hi], overlapping ones included"""
    hi = len(truth) if hi is None else min(hi, len(truth))
    out, at = [], truth.find(pat, lo, hi)
    while at >= 0:
        out.append(at)
        at = truth.find(pat, at + 1, hi)
    return out


def same(got, truth, pat, delim=None, lo=0, hi=None, limit=None):
    hits, nhits = got
    want = find_all(truth, pat, lo, hi)
    assert nhits == len(want), (pat[:20], lo, hi)
    kept = want if limit is None else want[:limit]
    assert hits["off"].tolist() == kept, (pat[:20], lo, hi)
    recs = [truth.count(bytes([delim]), 0, o) for o in kept] if delim is not None else [0] * len(kept)
    assert hits["record"].tolist() == recs, (pat[:20], lo, hi)
    return want


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 2)
    yield c
    c.close()


class Input:
    """three streams -- a level-1 one of three blocks, two of one block -- with NEEDLE planted across the block boundary, the batch
    boundary inside the first stream, both stream boundaries, at byte 0 and at the last byte; computed once, never changed"""

    def __init__(self, dec):
        parts = [bytearray(lines(250_000, 11)), bytearray(lines(10_000, 12)), bytearray(lines(10_000, 13))]
        pack = lambda: b"".join(bz2.compress(bytes(p), 1 if k == 0 else 9) for k, p in enumerate(parts))
        ent = dec.decode_index(pack())[0]
        assert len(ent) == 5
        bounds = [int(e["out_off"]) for e in ent[1:]]
        whole = bytearray(b"".join(parts))
        half = len(NEEDLE) // 2
        for at in [0, len(whole) - len(NEEDLE)] + [b - half for b in bounds]:
            whole[at:at + len(NEEDLE)] = NEEDLE
        cuts = [0, len(parts[0]), len(parts[0]) + len(parts[1]), len(whole)]
        parts = [whole[cuts[k]:cuts[k + 1]] for k in range(3)]
        self.s = pack()
        self.truth = bz2.decompress(self.s)
        assert self.truth == bytes(whole)
        self.ent, self.pts, self.cum, self.nrec, total, used = dec.decode_index_records(self.s, 4, 10)
        assert [int(e["out_off"]) for e in self.ent[1:]] == bounds and total == len(whole) and len(self.pts) > 8
        self.bounds = bounds
        for a in (self.ent, self.pts, self.cum):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def inp(dec):
    return Input(dec)


# ---- the raw seam: the kernel on a device buffer ----------------------------------------------------------------------------
def on_device(data):
    import torch
    t = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def test_raw_grid(dec):
    rng = random.Random(5)
    for n in NS:
        src = bytes(rng.choice(b"ab\nc") for _ in range(n))
        t = on_device(src)
        assert t.data_ptr() % 16 == 0
        for plen in PLENS:
            pat = bytes(rng.choice(b"ab") for _ in range(plen))
            if n >= plen and rng.random() < 0.8:
                at = rng.randrange(n - plen + 1)
                pat = src[at:at + plen]
            same(dec.search_raw_device(t.data_ptr(), n, pat, delim=10), src, pat, 10)  # (the delimiter is a pattern byte, often)
            same(dec.search_raw_device(t.data_ptr(), n, pat), src, pat)
        st = dec.search_stats()
        assert st["windows"] == 1 and st["tiles"] == (n + 4095) // 4096


def test_raw_fixed_places(dec):
    n = 12289
    for plen in (2, 5, 17, 256):
        pat = bytes(65 + j % 23 for j in range(plen))
        src = bytearray(b"x" * n)
        for at in (0, 16 - plen // 2 if plen <= 16 else 300, 1024 - plen // 2, 4096 - plen // 2, 8192 - 1, n - plen):
            src[at:at + plen] = pat
        src = bytes(src)
        t = on_device(src)
        want = same(dec.search_raw_device(t.data_ptr(), n, pat, delim=pat[0]), src, pat, pat[0])
        assert 0 in want and n - plen in want and len(want) >= 5
        # a pattern longer than the buffer, and a buffer of one byte value: every start is a hit, the first three are kept
        assert dec.search_raw_device(t.data_ptr(), plen - 1, pat)[1] == 0
        ones = on_device(b"z" * n)
        hits, nhits = dec.search_raw_device(ones.data_ptr(), n, b"z" * plen, delim=ord("z"), limit=3)
        assert nhits == n - plen + 1 and hits["off"].tolist() == [0, 1, 2] and hits["record"].tolist() == [0, 1, 2]
        assert dec.search_status == -4
    assert dec.search_raw_device(0, 0, b"a")[1] == 0


def test_raw_arguments(dec, native):
    t = on_device(b"abcabc" * 10)
    for bad in (b"", b"a" * 257):
        with pytest.raises(native.BzhError) as err:
            dec.search_raw_device(t.data_ptr(), 60, bad)
        assert err.value.status == -1
    with pytest.raises(native.BzhError) as err:
        dec.search_raw_device(t.data_ptr() + 1, 59, b"abc")
    assert err.value.status == -1 and "16-byte aligned" in str(err.value)
    with pytest.raises(native.BzhError) as err:
        dec.search_raw_device(t.data_ptr(), 60, b"abc", flags=2)
    assert err.value.status == -1
    pat = np.frombuffer(b"abc", dtype=np.uint8)
    got = native.ctypes.c_size_t(0)
    L = native.lib()
    assert L.bzh_search_raw_device(dec.handle, t.data_ptr(), 60, native.ptr(pat), 3, 0, 0, None, 4, native.ctypes.byref(got)) == -1
    assert L.bzh_search_raw_device(dec.handle, t.data_ptr(), 60, None, 3, 0, 0, None, 0, native.ctypes.byref(got)) == -1
    assert L.bzh_search_raw_device(dec.handle, t.data_ptr(), 60, native.ptr(pat), 3, 0, 0, None, 0, None) == -1
    assert L.bzh_search_raw_device(dec.handle, t.data_ptr(), 60, native.ptr(pat), 3, 0, 0, None, 0, native.ctypes.byref(got)) == 0
    assert got.value == 20
    with pytest.raises(native.BzhError):
        dec.search_set_room(1000)
    assert dec.search_raw_device(t.data_ptr(), 60, b"bca")[1] == 19  # (the context stays usable)


# ---- the full search ---------------------------------------------------------------------------------------------------------
def test_full_search_across_every_boundary(dec, inp):
    want = same(dec.search(inp.s, NEEDLE, delim=10), inp.truth, NEEDLE, 10)
    half = len(NEEDLE) // 2
    assert [b - half for b in inp.bounds] == want[1:-1] and want[0] == 0 and want[-1] == len(inp.truth) - len(NEEDLE)
    hits, nhits, total, used = dec.search(inp.s, NEEDLE, with_total=True)
    assert (nhits, total, used) == (6, len(inp.truth), len(inp.s)) and hits["record"].tolist() == [0] * 6
    st, ds = dec.search_stats(), dec.decode_stats()
    assert st["hits"] == 6 and st["windows"] >= 3 and ds["blocks"] == 5 and ds["streams"] == 3 and ds["out_bytes"] == len(inp.truth)
    # words with thousands of hits, one byte, and a newline in the pattern
    for pat in (inp.truth[5000:5003], b"e", b"\n", inp.truth[inp.bounds[1] - 100:inp.bounds[1] + 100]):
        same(dec.search(inp.s, pat, delim=10), inp.truth, pat, 10)


def test_full_search_limits(dec, inp, native):
    pat = inp.truth[5000:5003]
    n = len(find_all(inp.truth, pat))
    assert n > 100
    for limit in (0, n - 1, n, n + 5):
        same(dec.search(inp.s, pat, delim=10, limit=limit), inp.truth, pat, 10, limit=limit)
        assert dec.search_status == (-4 if 0 < limit < n else 0), limit


def test_full_search_runs_of_equal_bytes(dec):
    """600 equal bytes are RLE1 runs with count bytes: the search sees the expansion"""
    truth = lines(5000, 21) + b"q" * 600 + lines(5000, 22)
    s = bz2.compress(truth)
    for k in (4, 256):
        want = same(dec.search(s, b"q" * k, delim=10), truth, b"q" * k, 10)
        assert len(want) >= 600 - k + 1


def test_full_search_edges_of_the_input(dec, inp, native):
    assert dec.search(bz2.compress(b""), b"a", with_total=True)[1:] == (0, 0, 14)
    junk = inp.s + b"\0foreign bytes, QZ@needle#XJ among them"
    hits, nhits, total, used = dec.search(junk, NEEDLE, delim=10, with_total=True)
    assert (nhits, total, used) == (6, len(inp.truth), len(inp.s))
    bad = bytearray(inp.s)
    bad[len(inp.s) // 3] ^= 0x10
    with pytest.raises(native.BzhError) as e1:
        dec.decode(bytes(bad))
    with pytest.raises(native.BzhError) as e2:
        dec.search(bytes(bad), NEEDLE, delim=10)
    assert e1.value.status == e2.value.status == -6 and str(e1.value) == str(e2.value)
    same(dec.search(inp.s, NEEDLE, delim=10), inp.truth, NEEDLE, 10)


# ---- the range search --------------------------------------------------------------------------------------------------------
@pytest.fixture()
def small_room(dec):
    dec.search_set_room(1024)  # every block is a window
    yield dec
    dec.search_set_room(0)


@pytest.mark.parametrize("sync", [False, True])
def test_range_search_windows(small_room, inp, sync):
    dec = small_room
    pts = inp.pts if sync else None
    total = len(inp.truth)
    run = lambda pat, off, length, **kw: dec.search_range(inp.s, inp.ent, pat, off, length, points=pts, rec_cum=inp.cum, delim=10, **kw)
    same(run(NEEDLE, 0, None), inp.truth, NEEDLE, 10)
    assert dec.search_stats()["windows"] == 5 and dec.decode_stats()["blocks"] == 5
    # ranges that cut a match at either end, around every planted one
    for h in find_all(inp.truth, NEEDLE):
        for off, end in ((h, h + len(NEEDLE)), (h + 1, h + 40), (max(h - 40, 0), h + len(NEEDLE) - 1), (max(h - 7, 0), min(h + 30, total))):
            same(run(NEEDLE, off, end - off), inp.truth, NEEDLE, 10, off, end)
    pat = inp.truth[5000:5003]
    b1, b2 = inp.bounds[1], inp.bounds[2]
    same(run(pat, b1 - 3000, b2 - b1 + 6000), inp.truth, pat, 10, b1 - 3000, b2 + 3000)
    assert dec.search_stats()["windows"] == 3 and dec.decode_stats()["blocks"] == 3
    same(run(pat, 100, 50_000, limit=7), inp.truth, pat, 10, 100, 50_100, limit=7)
    assert dec.search_status == -4
    assert run(pat, total, 10)[1] == 0 and run(pat, total + 5, None)[1] == 0
    # without record numbers no table is needed
    same(dec.search_range(inp.s, inp.ent, pat, 70_000, 60_000, points=pts), inp.truth, pat, None, 70_000, 130_000)
    # only the span's bytes
    lo, hi = int(inp.ent[2]["bit_pos"]) // 8, (int(inp.ent[3]["end_bit"]) + 7) // 8
    off, end = int(inp.ent[2]["out_off"]) + 10, int(inp.ent[3]["out_off"]) + 10
    same(dec.search_range(inp.s[lo:hi], inp.ent, pat, off, end - off, points=pts, rec_cum=inp.cum, delim=10, in_byte_base=lo), inp.truth, pat, 10,
         off, end)


def test_range_search_checks_the_record_table(small_room, inp, native):
    dec = small_room
    pat = inp.truth[5000:5003]
    wrong = inp.cum.copy()
    wrong[4:] += 1  # one wrong difference: entry 3's
    with pytest.raises(native.BzhError) as err:
        dec.search_range(inp.s, inp.ent, pat, 0, None, rec_cum=wrong, delim=10)
    assert err.value.status == -6 and "record table does not match entry 3" in str(err.value)
    same(dec.search_range(inp.s, inp.ent, pat, 0, inp.bounds[1], rec_cum=wrong, delim=10), inp.truth, pat, 10, 0, inp.bounds[1])
    with pytest.raises(native.BzhError) as err:  # record numbers without a table
        dec.search_range(inp.s, inp.ent, pat, 0, None, delim=10)
    assert err.value.status == -1
    shape = inp.cum.copy()
    shape[0] = 1
    with pytest.raises(native.BzhError) as err:
        dec.search_range(inp.s, inp.ent, pat, 0, 10, rec_cum=shape, delim=10)
    assert err.value.status == -1


# ---- Python and the command line ---------------------------------------------------------------------------------------------
class CountingFile(io.BytesIO):
    def __init__(self, data):
        super().__init__(data)
        self.reads = []

    def read(self, n=-1):
        self.reads.append((self.tell(), n))
        return super().read(n)


def test_reader_search_and_grep(inp, native):
    import banzai_amd
    rindex = banzai_amd.RecordIndex(banzai_amd.SyncIndex(banzai_amd.BlockIndex(inp.ent.copy(), len(inp.s)), inp.pts.copy(), 4), 10, inp.cum.copy(),
                                    inp.nrec)
    assert "search" in banzai_amd.__all__ and "search_range" in banzai_amd.__all__
    same(banzai_amd.search(inp.s, NEEDLE, delim=b"\n"), inp.truth, NEEDLE, 10)
    same(banzai_amd.search_range(inp.s, rindex, NEEDLE, 5, 200_000), inp.truth, NEEDLE, 10, 5, 200_005)
    same(banzai_amd.search_range(inp.s, rindex.index, NEEDLE), inp.truth, NEEDLE)
    f = CountingFile(inp.s)
    rd = banzai_amd.IndexedReader(f, rindex)
    off, end = int(inp.ent[3]["out_off"]) - 50, int(inp.ent[3]["out_off"]) + 500
    pat = inp.truth[5000:5003]
    same(rd.search(pat, off, end), inp.truth, pat, 10, off, end)
    lo, hi = int(inp.ent[2]["bit_pos"]) // 8, (int(inp.ent[3]["end_bit"]) + 7) // 8
    assert f.reads == [(lo, hi - lo)]
    # grep: the lines of the truth that hold a hit, once each
    word = inp.truth[5000:5006]
    recs = inp.truth.split(b"\n")
    want = sorted({inp.truth.count(b"\n", 0, o) for o in find_all(inp.truth, word)})
    got = rd.grep(word)
    assert [r for r, _ in got] == want and len(want) > 3
    for r, line in got:
        assert line == recs[r] + (b"\n" if r < len(recs) - 1 else b"")
    assert rd.grep(b"no such bytes anywhere") == []
    with pytest.raises(ValueError):
        banzai_amd.IndexedReader(inp.s, rindex.index).grep(word)
    with pytest.raises(ValueError):
        banzai_amd.search(inp.s, b"")


def test_cli_search(inp, tmp_path):
    import banzai_amd
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    path, xpath = tmp_path / "t.bz2", tmp_path / "t.bzr"
    path.write_bytes(inp.s)
    rindex = banzai_amd.RecordIndex(banzai_amd.BlockIndex(inp.ent.copy(), len(inp.s)), 10, inp.cum.copy(), inp.nrec)
    xpath.write_bytes(rindex.to_bytes())
    row = lambda o: "%d\t%d\n" % (o, inp.truth.count(b"\n", 0, o))
    want = "".join(row(o) for o in find_all(inp.truth, NEEDLE))
    p = subprocess.run([exe, "--search", NEEDLE.decode(), str(path)], capture_output=True, text=True, timeout=120)
    assert (p.returncode, p.stdout) == (0, want), p.stderr
    off, end = inp.bounds[0] - 100, inp.bounds[2] + 100
    p = subprocess.run([exe, "--search", NEEDLE.hex(), "--hex", "--index", str(xpath), "--range", f"{off}:{end - off}", str(path)],
                       capture_output=True, text=True, timeout=120)
    cut = "".join(row(o) for o in find_all(inp.truth, NEEDLE, off, end))
    assert (p.returncode, p.stdout) == (0, cut) and cut.count("\n") == 3, p.stderr
    p = subprocess.run([exe, "--search", "no such bytes", "--count", str(path)], capture_output=True, text=True, timeout=120)
    assert (p.returncode, p.stdout) == (0, "0\n"), p.stderr
    assert path.exists()
