"""GPU: anchors and word boundaries of the device regex (^ $ \\A \\Z \\b \\B, the word and the line wrap: bzh_regex_create_ex,
banzai_amd.Regex(word=, line=), bnzhip -E / -w / -x) through the raw, the full, the indexed and the range routes.  Every comparison
is against Python's `re` under re.MULTILINE by the rule of tests/regex_look_truth.py: an assertion sees the real neighbours, also
outside the wanted range, so every route and every window size reports the same hits.  The context takes batches of 2 candidates,
so the blocks of the full input are several windows."""
import bz2
import os
import subprocess

import pytest

from tests import regex_look_truth as truth
from tests.test_gpu_regex import ent_rows, grep_rows, hit_rows, lines, on_device, raw_grep, raw_search, rows, text_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289)
A, W, X = truth.ASSERT, truth.WORD, truth.LINE
# (expression, span, the seed base, the hits regex_look_truth finds over the ten sizes of the word soup with these seeds: the floor;
# x+\Z has a hit only in a text that ends in x: its seed base is the one of 0..299 with the most such texts)
GRID = [(b"^[a-z]+", 256, 0, 389), (b"[0-9]+$", 256, 1, 135), (b"\\berr(or)?\\b", 256, 2, 51), (b"a\\B.", 256, 3, 3535), (b"\\A.+", 16, 4, 9), (b"x+\\Z", 256, 131, 4),
        (b"(^|\\t)time", 256, 6, 48)]


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 2)
    yield c
    c.close()


def rx(native, dec, exprs, flags=0, span=0, syntax=A):
    return native.PatternSet(dec, exprs, flags=flags, regex=True, max_span=span, syntax=syntax)


def raw_all(native, dec, src, exprs, flags=0, span=256, syntax=A):
    found = truth.hits(exprs, src, flags, span, syntax)
    with rx(native, dec, exprs, flags, span, syntax) as pset:
        raw_search(native, dec, src, pset, rows(found, src))
        raw_grep(dec, src, pset, found, False)
        raw_grep(dec, src, pset, found, True)
    return found


# ---- the raw seam ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(GRID)))
def test_raw_grid(dec, native, case):
    expr, span, base, floor = GRID[case]
    found = 0
    for n in NS:
        found += len(raw_all(native, dec, text_of(n, n + base), [expr], 0, span))
    assert found >= floor


def test_raw_planted_places_of_the_line_start(dec, native):
    """^ab at offset 0; at 16 and 1024, where the byte in front lies in another thread and another wave; at 4096 and 8192, where
    it lies in the tile before"""
    places = (0, 16, 1024, 4096, 8192)
    src = bytearray(b"." * 12289)
    for at in places:
        src[at:at + 2] = b"ab"
        if at:
            src[at - 1] = 10
    src[5000:5002] = src[9000:9003] = b"ab"  # (no line starts here)
    src[9002] = 10
    found = raw_all(native, dec, bytes(src), [b"^ab", b"\\Aab"])
    assert found == [(0, 0, 2)] + [(at, 0, 2) for at in places[1:]]
    found = raw_all(native, dec, bytes(src), [b"\\Aab", b"^ab"])
    assert found == [(0, 0, 2)] + [(at, 1, 2) for at in places[1:]]  # (the lowest expression of that length)


def test_raw_planted_places_of_the_line_end(dec, native):
    """x+$: the match ends at byte n (the text's edge); at n - 1 in front of a final 0x0A; at tile byte 4095, so that the byte
    behind it is the halo's first; 256 bytes from 4095, so that the byte behind it is the tile array's last"""
    for n in (4500, 12289):
        src = bytearray(b"." * n)
        src[n - 3:] = b"xxx"
        src[4000:4096], src[4096] = b"x" * 96, 10
        found = raw_all(native, dec, bytes(src), [b"x+$"])
        assert {(n - 3, 0, 3), (n - 1, 0, 1), (4000, 0, 96), (4095, 0, 1)} <= set(found) and len(found) == 99
        src[n - 1] = 10
        found = raw_all(native, dec, bytes(src), [b"x+$", b"x+\\Z"])
        assert {(n - 3, 0, 2), (n - 2, 0, 1)} <= set(found) and len(found) == 98
    src = bytearray(b"." * 8192)
    src[4095:4095 + 256], src[4095 + 256] = b"x" * 256, 10
    found = raw_all(native, dec, bytes(src), [b"x+$"])
    assert found == [(4095 + k, 0, 256 - k) for k in range(256)]
    src[4095 + 256], src[4096 + 256] = ord("x"), 10  # one x more: the longest match of the first start ends in front of an x
    found = raw_all(native, dec, bytes(src), [b"x+$"])
    assert found == [(4096 + k, 0, 256 - k) for k in range(256)]


def test_raw_zero_fill_is_no_neighbour(dec, native):
    """A text that ends in a word byte under \\b and \\Z, and one of exactly 4,096 bytes under $: what the tile front supplies
    behind the text -- zeros -- is not a neighbour"""
    for n in (17, 4096, 4097):
        src = b"w" * n
        assert raw_all(native, dec, src, [b"w+\\b"]) == [(s, 0, n - s) for s in range(max(0, n - 256), n)]
        assert raw_all(native, dec, src, [b"w$"]) == [(n - 1, 0, 1)]
        assert raw_all(native, dec, src, [b"w\\Z", b"\\x00"]) == [(n - 1, 0, 1)]
        assert raw_all(native, dec, src[:-1] + b"\0", [b"w\\b"]) == [(n - 2, 0, 1)]


# ---- the full path ----------------------------------------------------------------------------------------------------------------
EXPRS = [b"^[a-z]+ [a-z]+$", b"^QZ\\w+", b"\\w+XJ$", b"\\AQZ\\w+", b"\\w+XJ\\Z", b"\\bqz\\B."]


class Input:
    """two streams -- a level-1 one of two blocks and one of one block -- whose lines straddle the block edges: a line that starts
    at a block's first byte (the byte in front lies in the window before), a line whose 0x0A is the next block's first byte, and
    the stream edge in the middle of a line; the text begins and ends with a marked word, and the same words stand at the stream
    edge, where neither \\A nor \\Z holds; computed once, never changed"""

    def __init__(self, dec):
        parts = [bytearray(lines(120_000, 41)), bytearray(lines(10_000, 42))]
        pack = lambda: b"".join(bz2.compress(bytes(p), 1 if k == 0 else 9) for k, p in enumerate(parts))
        ent = dec.decode_index(pack())[0]
        assert len(ent) == 3
        b = [int(e["out_off"]) for e in ent[1:]]
        whole = bytearray(b"".join(parts))
        whole[0:8], whole[-8:] = b"QZfirst ", b" lastaXJ"
        whole[b[0] - 1:b[0] + 9] = b"\nQZblock \n"      # ^ at the first byte of a window
        whole[b[1] - 7:b[1] + 1] = b" edgeXJ\n"          # $ whose 0x0A is the next window's first byte
        whole[b[1] + 1:b[1] + 9] = b"QZafter "
        whole[60000:60010] = b"\nqz qzz q\n"
        cut = len(parts[0])
        assert cut == b[1]
        parts = [whole[:cut], whole[cut:]]
        self.s = pack()
        self.truth = bz2.decompress(self.s)
        assert self.truth == bytes(whole)
        self.ent, self.pts, self.cum, self.nrec, total, used = dec.decode_index_records(self.s, 4, 10)
        assert [int(e["out_off"]) for e in self.ent[1:]] == b and total == len(whole)
        self.bounds = b
        self.found = truth.hits(EXPRS, self.truth)
        self.want = rows(self.found, self.truth)
        for a in (self.ent, self.pts, self.cum):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def inp(dec):
    return Input(dec)


def test_full_search(dec, inp, native):
    want, b, n = inp.want, inp.bounds, len(inp.truth)
    by_start = {h[0]: (h[2], h[3]) for h in want}
    assert by_start[0] == (1, 7) and by_start[b[0]] == (1, 7) and by_start[b[1] + 1] == (1, 7)       # ^QZ\w+, and \A only at offset 0:
    assert [h[0] for h in want if h[2] == 3] == [] and (0, 3, 7) not in inp.found                       # (^ is the lower number)
    assert by_start[b[1] - 6] == (2, 6) and by_start[n - 7] == (2, 7)                                   # \w+XJ$ in front of a window's first byte, at the end
    assert sum(1 for h in want if h[2] == 0) >= 30 and by_start[60004] == (5, 3) and 60001 not in by_start and len(want) >= 50
    with rx(native, dec, EXPRS) as pset:
        hits, nhits, total, used = dec.search(inp.s, pset, 10, with_total=True)
        assert nhits == len(want) and hit_rows(hits) == want and total == n and used == len(inp.s)
        assert dec.search_stats()["windows"] >= 2 and dec.decode_stats()["streams"] == 2
        d_in = on_device(inp.s)
        hits, nhits = dec.search_device(d_in.data_ptr(), len(inp.s), pset, 10)
        assert nhits == len(want) and hit_rows(hits) == want
    # \A and \Z alone: only the true ends although the streams meet in the middle
    with rx(native, dec, [b"\\AQZ\\w+", b"\\w+XJ\\Z"]) as pset:
        hits, nhits = dec.search(inp.s, pset, 10)
        assert [h[0] for h in hit_rows(hits)] == [0] + list(range(n - 7, n - 2)) and hit_rows(hits)[0][2:] == (0, 7)


@pytest.mark.parametrize("sync", [False, True])
def test_range_search(dec, inp, native, sync):
    pts = inp.pts if sync else None
    b, n = inp.bounds, len(inp.truth)
    dec.search_set_room(1024)  # every block is a window
    try:
        with rx(native, dec, EXPRS) as pset, native.PatternSet(dec, [b"QZ\\w+", b"\\w+XJ"], regex=True) as plain:
            run = lambda off, length, p=pset: dec.search_range(inp.s, inp.ent, p, off, length, points=pts, rec_cum=inp.cum, delim=10)
            total = 0
            for off, end in ((0, n), (b[0], b[1]), (b[0], b[1] + 1), (b[0] + 1, b[1] - 1), (b[0] - 1, n), (b[1] - 6, b[1]), (b[1] + 1, n + 99), (1, b[0]),
                             (60000, 60010), (7, 7)):
                want = rows(truth.hits(EXPRS, inp.truth, 0, 256, A, off, end), inp.truth)
                hits, nhits = run(off, end - off)
                assert nhits == len(want) and hit_rows(hits) == want, (off, end)
                total += len(want)
            assert total >= 58
            # from a block's first byte to a block's last, under ^...$: the line that starts at the block's first byte and the one
            # that ends at its last are found, and one block more is decoded on each side than without assertions
            want = rows(truth.hits(EXPRS, inp.truth, 0, 256, A, b[0], b[1]), inp.truth)
            assert (b[0], 1, 7) in [(h[0], h[2], h[3]) for h in want] and (b[1] - 6, 2, 6) in [(h[0], h[2], h[3]) for h in want]
            hits, nhits = run(b[0], b[1] - b[0])
            assert hit_rows(hits) == want and dec.decode_stats()["blocks"] == 3
            run(b[0], b[1] - b[0], plain)
            assert dec.decode_stats()["blocks"] == 1
            # the device variant is handed the widened span
            off, length = b[0], b[1] - b[0]
            lo = int(inp.ent[0]["bit_pos"]) // 8
            hits, nhits = dec.search_range(inp.s[lo:], inp.ent, pset, off, length, points=pts, rec_cum=inp.cum, delim=10, in_byte_base=lo)
            assert hit_rows(hits) == want
    finally:
        dec.search_set_room(0)


def test_full_grep_and_index(dec, inp, native):
    with rx(native, dec, EXPRS) as pset:
        for invert in (False, True):
            want, ent = grep_rows(inp.found, inp.truth, invert)
            assert len(ent) >= 40
            data, got = dec.grep(inp.s, pset, b"\n", invert)
            assert data == want and ent_rows(got) == ent, invert
            dec.search_set_room(1024)
            try:
                for pts in (None, inp.pts):
                    idata, igot = dec.grep_index(inp.s, inp.ent, pset, pts, b"\n", invert)
                    assert idata == want and ent_rows(igot) == ent and dec.grep_stats()["windows"] >= 3
            finally:
                dec.search_set_room(0)
        # a delimiter that is no 0x0A: the line anchors stay about 0x0A
        want, ent = grep_rows(inp.found, inp.truth, False, b" ")
        data, got = dec.grep(inp.s, pset, b" ")
        assert data == want and ent_rows(got) == ent and len(ent) >= 40


# ---- Python and the command line -----------------------------------------------------------------------------------------------------
def test_python_wraps(inp):
    import banzai_amd
    with banzai_amd.Regex([b"qz+", b"[a-z]+"], word=True) as r:
        assert (r.info["look_behind"], r.info["look_ahead"]) == (1, 1)
        want = rows(truth.hits([b"qz+", b"[a-z]+"], inp.truth, 0, 256, W), inp.truth)
        hits, nhits = banzai_amd.search(inp.s, r, delim=b"\n")
        assert nhits == len(want) >= 1000 and hit_rows(hits) == want
        rindex = banzai_amd.build_record_index(inp.s)
        off, end = inp.bounds[0], inp.bounds[1]
        cut = rows(truth.hits([b"qz+", b"[a-z]+"], inp.truth, 0, 256, W, off, end), inp.truth)
        hits, nhits = banzai_amd.search_range(inp.s, rindex, r, off, end - off)
        assert hit_rows(hits) == cut and len(cut) >= 100
        rd = banzai_amd.IndexedReader(inp.s, rindex)
        hits, nhits = rd.search(r, off, end)
        assert hit_rows(hits) == cut
    with banzai_amd.Regex([b"[a-z]+ [a-z]+", b"QZ\\w+ "], line=True) as r:
        found = truth.hits([b"[a-z]+ [a-z]+", b"QZ\\w+ "], inp.truth, 0, 256, X)
        gwant, gent = grep_rows(found, inp.truth)
        data, ent = banzai_amd.grep(inp.s, r)
        assert data == gwant and ent_rows(ent) == gent and len(gent) >= 30
        assert banzai_amd.grep_count(inp.s, r, invert=True) == len(grep_rows(found, inp.truth, True)[1])
    with banzai_amd.Regex([b"[0-9]{4}", b"err(or)?"]) as r:  # without an assertion nothing is looked at
        assert (r.info["look_behind"], r.info["look_ahead"], r.info["contexts"]) == (0, 0, 1)
    with pytest.raises(ValueError):
        banzai_amd.Regex(b"a", word=True, line=True)
    with pytest.raises(banzai_amd._native.BzhError) as err:
        banzai_amd.Regex(b"^")
    assert "empty string" in str(err.value)


def test_cli(inp, tmp_path):
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    path = tmp_path / "t.bz2"
    path.write_bytes(inp.s)
    run = lambda *args: subprocess.run([exe, *args, str(path)], capture_output=True, timeout=120)
    word = lambda e, syntax, flags=0: truth.hits([e], inp.truth, flags, 256, syntax)
    p = run("--grep", "^[a-z]+ [a-z]+$", "-E")
    want = grep_rows(word(b"^[a-z]+ [a-z]+$", A), inp.truth)[0]
    assert (p.returncode, p.stdout) == (0, want) and len(want) > 100, p.stderr
    p = run("--grep", "qz+", "-E", "-w")
    assert (p.returncode, p.stdout) == (0, grep_rows(word(b"qz+", W), inp.truth)[0]) and p.stdout.count(b"\n") >= 1, p.stderr
    p = run("--grep", "qz", "-w", "--count")  # a literal string under -w
    lit = grep_rows(word(b"qz", W), inp.truth)[1]
    assert (p.returncode, p.stdout) == (0, b"%d\n" % len(lit)) and len(lit) >= 1, p.stderr
    p = run("--grep", "717a", "--hex", "--word-regexp", "--count")
    assert (p.returncode, p.stdout) == (0, b"%d\n" % len(lit)), p.stderr
    line = bytes(inp.truth[60001:60009])
    p = run("--grep", line.decode(), "-x", "--line-number")
    found = word(b"".join(b"\\x%02X" % c for c in line), X)
    assert len(found) == 1 and p.returncode == 0 and p.stdout.endswith(b":" + line + b"\n") and p.stdout.count(b"\n") == 1, p.stderr
    p = run("--grep", "q.", "-x", "--count")  # without -E the dot is a dot
    assert (p.returncode, p.stdout) == (0, b"0\n"), p.stderr
    p = run("--search", "\\bqz\\B.", "-E")
    want = rows(word(b"\\bqz\\B.", A), inp.truth)
    assert (p.returncode, p.stdout) == (0, b"".join(b"%d\t%d\t%d\n" % (o, r, k) for o, r, k, _ in want)) and len(want) >= 1, p.stderr
    # the argument errors
    p = run("--grep", "a", "-w", "-x")
    assert p.returncode != 0 and b"exclude each other" in p.stderr and p.stdout == b""
    p = run("--grep", "^", "-E")
    assert p.returncode != 0 and b"empty string" in p.stderr
    assert subprocess.run([exe, "-w", str(path)], capture_output=True, timeout=120).returncode != 0
