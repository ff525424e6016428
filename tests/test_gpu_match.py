"""GPU: the matched parts alone (bzh_match*: grep -o) through every route -- the raw seam, the full decode, the indexed walk, one
string, a PatternSet and a Regex, banzai_amd.matches / matches_count, IndexedReader.matches and bnzhip --grep -o / -b.  The truth
is always tests/match_truth.py over bz2.decompress(stream), the model that tests/test_match_truth.py holds to GNU grep; the
command line is held to the installed GNU grep itself where there is one."""
import bz2
import functools
import os
import random
import shutil
import subprocess

import pytest

from tests import match_truth as mt
from tests.test_gpu_grep import on_device, room_on_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
VOCAB = ["a", "ab", "abb", "aa", "b1", "1234", "77", "Ab", "AB", "needle", "Needle", "ab_", "aab"]


@functools.lru_cache(maxsize=None)
def prose(n, seed):
    """lines of filler words with a token of VOCAB now and then: every pattern of the tests matches, none densely; no byte four
    times in a row, so replacing a stretch by another such text keeps the blocks' bounds"""
    rng = random.Random(seed)
    filler = []
    for _ in range(30):
        w = rng.choice("xyzwvu")
        for _ in range(rng.randrange(1, 8)):
            w += rng.choice("xyzwvu".replace(w[-1], ""))
        filler.append(w)
    out = bytearray()
    while len(out) < n:
        words = [rng.choice(VOCAB) if rng.random() < 0.08 else rng.choice(filler) for _ in range(rng.randrange(1, 14))]
        out += " ".join(words).encode() + b"\n"
    return bytes(out[:n - 1]) + b"\n"


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dec1(native):
    """batches of one candidate: the full decode hands every block over as a window of its own"""
    c = native.Context(0, 9, 1)
    yield c
    c.close()


class Input:
    """two streams -- a level-1 one of two blocks, one of one block -- with a dense stretch of "ab" (every position of it begins
    aba or bab: no position is free, a tile inside it is open) across the block edge and across the stream edge; computed once,
    never changed"""

    def __init__(self, dec):
        parts = [bytearray(prose(150_000, 31)), bytearray(prose(12_000, 32))]
        pack = lambda: b"".join(bz2.compress(bytes(p), 1 if k == 0 else 9) for k, p in enumerate(parts))
        ent = dec.decode_index(pack())[0]
        assert len(ent) == 3
        bounds = [int(e["out_off"]) for e in ent[1:]]
        assert bounds[1] == len(parts[0])
        whole = bytearray(b"".join(parts))
        for b in bounds:
            whole[b - 8301:b + 8300] = (b"ab" * 8301)[:16601]  # (a whole tile of it on either side of the edge, wherever the tiles lie)
        parts = [whole[:bounds[1]], whole[bounds[1]:]]
        self.s = pack()
        self.truth = bz2.decompress(self.s)
        assert self.truth == bytes(whole)
        self.ent, self.pts, total, _ = dec.decode_index_sync(self.s, 4)
        self.bounds = [int(e["out_off"]) for e in self.ent[1:]]  # (a block is cut where a run ends: a bound may move by a byte or two)
        assert len(self.ent) == 3 and all(abs(a - b) < 100 for a, b in zip(self.bounds, bounds)) and total == len(whole) and len(self.pts) > 4
        for a in (self.ent, self.pts):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def inp(dec):
    return Input(dec)


WHAT = {  # name -> (the model's expressions, are they byte strings, flags, syntax, what the library is given)
    "string": ([b"needle"], True, 0, 0, lambda n, d: b"needle"),
    "dense": ([b"aba", b"bab"], True, 0, 0, lambda n, d: n.PatternSet(d, [b"aba", b"bab"])),
    "set -i": ([b"needle", b"ab", b"abb", b"b1"], True, mt.FOLD, 0, lambda n, d: n.PatternSet(d, [b"needle", b"ab", b"abb", b"b1"], ignore_case=True)),
    "[0-9]+": ([b"[0-9]+"], False, 0, 0, lambda n, d: n.PatternSet(d, [b"[0-9]+"], regex=True)),
    "a|ab": ([b"a|ab"], False, 0, 0, lambda n, d: n.PatternSet(d, [b"a|ab"], regex=True)),
    "^a+": ([b"^a+"], False, 0, 0, lambda n, d: n.PatternSet(d, [b"^a+"], regex=True, syntax=n.REGEX_ASSERT)),
    r"\bab\b": ([rb"\bab\b"], False, 0, 0, lambda n, d: n.PatternSet(d, [rb"\bab\b"], regex=True, syntax=n.REGEX_ASSERT)),
    "-w a+b?": ([b"a+b?"], False, 0, mt.WORD, lambda n, d: n.PatternSet(d, [b"a+b?"], regex=True, syntax=n.REGEX_WORD)),
}
_truths = {}


def truth_of(name, text, delim=None):
    """the model's answer, computed once for a text and shared"""
    key = (name, text, delim)
    if key not in _truths:
        exprs, literal, flags, syntax, _ = WHAT[name]
        _truths[key] = mt.matches(mt.literal(exprs) if literal else exprs, text, flags, 256, syntax | mt.ASSERT, delim)
    return _truths[key]


def given(native, dec, name):
    return WHAT[name][4](native, dec)


def close(what):
    if hasattr(what, "close"):
        what.close()


def raw(dec, src, what, want, rows, delim=None):
    """bzh_match_raw_device: the counting call, then the exact rooms; nothing behind the room is touched"""
    t = on_device(src)
    assert t.data_ptr() % 16 == 0
    assert dec.match_raw_device(t.data_ptr(), len(src), what, 0, 0, 0, delim)[:3] == (0, len(rows), len(want))
    out = room_on_device(len(want))
    st, nm, total, got = dec.match_raw_device(t.data_ptr(), len(src), what, out.data_ptr(), len(want), len(rows), delim)
    assert (st, nm, total) == (0, len(rows), len(want)), (len(src), dec.last_error())
    host = out.cpu().numpy().tobytes()
    assert host[:len(want)] == want and set(host[len(want):]) <= {0xA5}, len(src)
    assert mt.rows_of(got) == rows, len(src)
    return dec.match_stats()


# ---- the raw seam ---------------------------------------------------------------------------------------------------------------
def test_raw_sizes(dec, native):
    rng = random.Random(5)
    for n in (0, 1, 17, 4097, 12289):
        src = bytes(rng.choice(b"aab b1\n") for _ in range(n))
        for name in ("set -i", "a|ab", "-w a+b?"):
            what = given(native, dec, name)
            want, rows = truth_of(name, src, b"\n")
            raw(dec, src, what, want, rows, b"\n")
            close(what)
        want, rows = mt.matches([b"aa"], src)
        st = raw(dec, src, b"aa", want, rows)
        assert st["matches"] == len(rows) and st["out_bytes"] == len(want) and st["windows"] == 1 and st["tiles"] == (n + TILE - 1) // TILE


def test_raw_dense(dec):
    """a run of one byte over three tiles searched for two of it, from an even and from an odd offset: every tile of the run is open
    and both parities cross both edges; the same for a 256-byte pattern, with entries up to 255; a sparse text opens and enters none"""
    for begin in (4, 7):
        src = b"x" * begin + b"a" * (3 * TILE) + b"y" * 100
        want, rows = mt.matches([b"aa"], src)
        st = raw(dec, src, b"aa", want, rows)
        assert len(rows) == 3 * TILE // 2 and st["open_tiles"] >= 3 and (begin % 2 == 0 or st["entered_tiles"] >= 2), st
    for begin in (0, 1, 255):
        src = b"x" * begin + b"a" * (3 * TILE + 77)
        pat = b"a" * 256
        want, rows = mt.matches([pat], src)
        st = raw(dec, src, pat, want, rows)
        assert len(rows) == (3 * TILE + 77) // 256 and st["open_tiles"] >= 2 and (begin == 0 or st["entered_tiles"] >= 2), st
    src = bytearray(b"x" * (3 * TILE))
    src[TILE - 1:TILE + 255] = b"a" * 256  # a tile entered at 255
    want, rows = mt.matches([b"a" * 256], bytes(src))
    st = raw(dec, bytes(src), b"a" * 256, want, rows)
    assert rows == [(TILE - 1, 0, 0, 256, 0)] and st["entered_tiles"] == 1 and st["open_tiles"] == 0
    sparse = prose(12289, 3)
    want, rows = mt.matches([b"needle"], sparse, delim=b"\n")
    st = raw(dec, sparse, b"needle", want, rows, b"\n")
    assert len(rows) > 2 and st["entered_tiles"] == 0 and st["open_tiles"] == 0 and st["candidates"] == len(rows)


def test_raw_rooms(dec):
    src = prose(9000, 6)
    want, rows = mt.matches([b"ab"], src, delim=b"\n")
    assert len(rows) > 10
    t, out = on_device(src), room_on_device(len(want))
    call = lambda d_out, cap, room, **kw: dec.match_raw_device(t.data_ptr(), len(src), b"ab", d_out, cap, room, b"\n", **kw)
    assert call(0, 0, 0)[:3] == (0, len(rows), len(want))                           # not asked for: the counting call
    for cap, room in ((len(want) - 1, len(rows)), (len(want), len(rows) - 1), (0, len(rows))):  # one below, one below, asked for with no room
        st, nm, total, _ = call(out.data_ptr(), cap, room)
        assert (st, nm, total) == (-4, len(rows), len(want)) and "room for" in dec.last_error()
    st, nm, total, got = call(out.data_ptr(), len(want) + 7, len(rows) + 3)         # above the need
    assert (st, nm, total) == (0, len(rows), len(want)) and mt.rows_of(got) == rows
    st, nm, total, got = call(out.data_ptr(), len(want), len(rows))                 # the exact rooms
    assert (st, nm, total) == (0, len(rows), len(want)) and mt.rows_of(got) == rows and out.cpu().numpy().tobytes()[:len(want)] == want
    st, nm, total, got = call(0, 0, len(rows))                                      # entries alone
    assert (st, nm, total) == (0, len(rows), len(want)) and mt.rows_of(got) == rows
    assert call(0, 0, 0, flags=2)[0] == -1 and call(0, 0, 0, flags=3)[0] == -1       # an undefined flag bit
    assert dec.match_raw_device(t.data_ptr() + 4, len(src) - 4, b"ab", 0, 0, 0)[0] == -1  # the text is 16-byte aligned
    want0, rows0 = mt.matches([b"ab"], src)                                         # without the flag: record 0
    st, nm, total, got = dec.match_raw_device(t.data_ptr(), len(src), b"ab", 0, 0, len(rows))
    assert mt.rows_of(got) == rows0 and all(r[1] == 0 for r in rows0) and any(r[1] for r in rows)


# ---- the full decode and the indexed walk, every block a window ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WHAT))
def test_full_and_indexed_routes(dec, dec1, inp, native, name):
    want, rows = truth_of(name, inp.truth, b"\n")
    assert len(rows) > 20
    what = given(native, dec, name)
    data, got = dec1.matches(inp.s, what, b"\n")
    assert data == want and mt.rows_of(got) == rows, name
    st = dec1.match_stats()
    assert st["windows"] >= 3 and st["matches"] == len(rows) and 0 < st["carry_peak"] <= 257
    if name == "dense":  # the dense stretches were crossed with the cursor inside a match: tiles are open, and entered beyond their first byte
        assert st["open_tiles"] >= 2 and st["entered_tiles"] >= 1, st
    assert dec.matches(inp.s, what, b"\n", count_only=True) == (len(rows), len(want))
    dec.search_set_room(1024)  # the indexed walk in windows of one block
    try:
        for pts in (None, inp.pts):
            idata, igot = dec.matches_index(inp.s, inp.ent, what, pts, b"\n")
            assert idata == want and mt.rows_of(igot) == rows, (name, pts is not None)
            assert dec.match_stats()["windows"] >= 3
    finally:
        dec.search_set_room(0)
    close(what)


def test_record_numbers_and_rooms_on_the_full_route(dec, inp):
    want, rows = truth_of("string", inp.truth, b"\n")
    _, rows0 = truth_of("string", inp.truth)
    assert any(r[1] for r in rows) and not any(r[1] for r in rows0)
    assert mt.rows_of(dec.matches(inp.s, b"needle")[1]) == rows0
    d_in, out = on_device(inp.s), room_on_device(len(want))
    for cap, room in ((len(want) - 1, len(rows)), (len(want), len(rows) - 1)):
        st, nm, total, _ = dec.match_device(d_in.data_ptr(), len(inp.s), b"needle", out.data_ptr(), cap, room, b"\n")
        assert (st, nm, total) == (-4, len(rows), len(want)) and "room for" in dec.last_error()
    st, nm, total, got = dec.match_device(d_in.data_ptr(), len(inp.s), b"needle", out.data_ptr(), len(want), len(rows), b"\n")
    host = out.cpu().numpy().tobytes()
    assert (st, nm, total) == (0, len(rows), len(want)) and host[:len(want)] == want and set(host[len(want):]) <= {0xA5} and mt.rows_of(got) == rows
    st, nm, total, got = dec.match_index_device(d_in.data_ptr(), len(inp.s), inp.ent, b"needle", out.data_ptr(), len(want), len(rows), inp.pts, b"\n")
    assert (st, nm, total) == (0, len(rows), len(want)) and mt.rows_of(got) == rows


def test_a_damaged_block(dec, inp, native):
    bad = bytearray(inp.s)
    bad[len(inp.s) // 3] ^= 0x10
    with pytest.raises(native.BzhError) as e1:
        dec.decode(bytes(bad))
    with pytest.raises(native.BzhError) as e2:
        dec.matches(bytes(bad), b"needle")
    assert e1.value.status == e2.value.status == -6 and str(e1.value) == str(e2.value)
    want, rows = truth_of("string", inp.truth)
    data, got = dec.matches(inp.s, b"needle")  # the context is still usable
    assert data == want and mt.rows_of(got) == rows


# ---- Python and the command line --------------------------------------------------------------------------------------------------
def test_python_matches(inp, native):
    import banzai_amd
    want, rows = truth_of("string", inp.truth)
    data, got = banzai_amd.matches(inp.s, b"needle")
    assert got.dtype == native.MATCH_DTYPE and data == want and mt.rows_of(got) == rows
    assert banzai_amd.matches_count(inp.s, b"needle") == len(rows)
    data, got = banzai_amd.matches(inp.s, b"needle", limit=3)
    assert mt.rows_of(got) == rows[:3] and data == want[:rows[3][4]]
    assert banzai_amd.matches(inp.s, b"needle", limit=0)[0] == b""
    want, rows = truth_of("set -i", inp.truth, b"\n")
    with banzai_amd.PatternSet([b"needle", b"ab", b"abb", b"b1"], ignore_case=True) as pset:
        data, got = banzai_amd.matches(inp.s, pset, delim=b"\n")
        assert data == want and mt.rows_of(got) == rows
    want, rows = truth_of("-w a+b?", inp.truth, b"\n")
    index = banzai_amd.SyncIndex(banzai_amd.BlockIndex(inp.ent.copy(), len(inp.s)), inp.pts.copy(), 4)
    with banzai_amd.Regex(b"a+b?", word=True) as rx:
        data, got = banzai_amd.matches(inp.s, rx, delim=b"\n", index=index)
        assert data == want and mt.rows_of(got) == rows
        assert banzai_amd.matches_count(inp.s, rx, index=index) == len(rows)
        rd = banzai_amd.IndexedReader(inp.s, banzai_amd.build_record_index(inp.s))
        data, got = rd.matches(rx)
        assert data == want and mt.rows_of(got) == rows  # (a RecordIndex: record numbers come)
        assert mt.rows_of(rd.matches(rx, limit=5)[1]) == rows[:5]
    with pytest.raises(TypeError):
        banzai_amd.matches(inp.s, "needle")
    with pytest.raises(ValueError):
        banzai_amd.matches(inp.s, b"")


def test_cli_against_gnu_grep(tmp_path):
    """a newline-terminated text of a few hundred lines: bnzhip --grep -o / -b writes byte for byte what GNU grep writes for the
    decompressed file; where no GNU grep is installed, what the model renders for the same lines"""
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    text = prose(16_000, 21)
    assert 200 < text.count(b"\n") < 2000
    path, plain = tmp_path / "t.bz2", tmp_path / "t.txt"
    path.write_bytes(bz2.compress(text, 9))
    plain.write_bytes(text)
    gnu = shutil.which("grep")
    if gnu and "GNU grep" not in subprocess.run([gnu, "--version"], capture_output=True, text=True).stdout:
        gnu = None
    print("compared against", gnu or "the model's rendering")
    found = mt.select([b"a+b?"], text, syntax=mt.ASSERT | mt.WORD)
    assert len(found) > 30
    for mine, theirs, ln, bo in ((("-o",), ("-o",), False, False), (("-o", "-b"), ("-o", "-b"), False, True),
                                 (("-o", "--line-number"), ("-o", "-n"), True, False), (("--only-matching", "--byte-offset", "--line-number"), ("-o", "-b", "-n"), True, True)):
        p = subprocess.run([exe, "--grep", "-E", "-w", "-e", "a+b?", *mine, str(path)], capture_output=True, timeout=120)
        assert p.returncode == 0, (mine, p.stderr)
        assert p.stdout == mt.render(text, found, ln, bo), mine
        if gnu:
            q = subprocess.run([gnu, "-a", "-E", "-w", *theirs, "a+b?", str(plain)], capture_output=True, timeout=120, env=dict(os.environ, LC_ALL="C"))
            assert q.returncode == 0 and p.stdout == q.stdout, (mine, p.stdout[:300], q.stdout[:300])
    # -b alone: the offset of the line's first byte; with context lines OFF-
    lines_, offs = text.split(b"\n")[:-1], [0]
    for ln_ in lines_:
        offs.append(offs[-1] + len(ln_) + 1)
    p = subprocess.run([exe, "--grep", "needle", "-b", str(path)], capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout == b"".join(b"%d:%s\n" % (offs[k], ln_) for k, ln_ in enumerate(lines_) if b"needle" in ln_)
    if gnu:
        for mine, theirs in ((("-b",), ("-b",)), (("-b", "--line-number", "-A", "1"), ("-b", "-n", "-A", "1")), (("-o", "--count"), ("-o", "-c"))):
            p = subprocess.run([exe, "--grep", "needle", *mine, str(path)], capture_output=True, timeout=120)
            q = subprocess.run([gnu, "-a", "-F", *theirs, "needle", str(plain)], capture_output=True, timeout=120, env=dict(os.environ, LC_ALL="C"))
            assert p.returncode == 0 and q.returncode == 0 and p.stdout == q.stdout, (mine, p.stdout[:300], q.stdout[:300])
    # the indexed route writes the same
    idx = tmp_path / "t.idx"
    assert subprocess.run([exe, "--make-index", str(idx), str(path)], capture_output=True, timeout=120).returncode == 0
    p = subprocess.run([exe, "--grep", "-E", "-w", "-e", "a+b?", "-o", "-b", "--index", str(idx), str(path)], capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout == mt.render(text, found, False, True), p.stderr


def test_cli_argument_errors(tmp_path):
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    path = tmp_path / "t.bz2"
    path.write_bytes(bz2.compress(b"ab\n"))
    for extra in (("--invert",), ("-A", "1"), ("-B", "2"), ("-C", "1")):
        p = subprocess.run([exe, "--grep", "ab", "-o", *extra, str(path)], capture_output=True, timeout=60)
        assert p.returncode != 0 and b"'-o' writes the matched parts alone" in p.stderr and not p.stdout, extra
    p = subprocess.run([exe, "-d", "-o", str(path)], capture_output=True, timeout=60)
    assert p.returncode != 0 and b"go with '--grep'" in p.stderr
