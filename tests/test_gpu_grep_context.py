"""GPU: context records for the device grep (bzh_grep_set_context: grep -A -B -C) through every route -- the raw seam, the full
decode, the indexed walk, a PatternSet and a Regex, banzai_amd.grep, IndexedReader.grep and bnzhip --grep -A/-B/-C.  The truth is
always a Python split-find-dilate over bz2.decompress(stream): a record is primary when the plain grep selects it, selected when
it lies within `before` in front of a primary or `after` behind one, and the command line is held to the installed GNU grep."""
import bisect
import bz2
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_gpu_grep import NEEDLE, NS, Input, find_all, lines, on_device, room_on_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BA = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (16, 16), (17, 0), (0, 17), (5000, 5000))
CTX = 1 << 63


def records_of(truth, delim=b"\n"):
    cut = truth.split(delim)
    recs = [p + delim for p in cut[:-1]] + ([cut[-1]] if cut[-1] else [])  # (an empty tail is not a record)
    offs = [0]
    for r in recs:
        offs.append(offs[-1] + len(r))
    return recs, offs


def hit_records(truth, pat, delim=b"\n"):
    """the records inside which a match of the byte string starts"""
    _, offs = records_of(truth, delim)
    return {bisect.bisect_right(offs, s) - 1 for s in find_all(truth, pat)}


def dilate(truth, hit, before, after, invert=False, delim=b"\n"):
    """-> (bytes, [(record, off, len | context bit, out_off)], stats)"""
    recs, offs = records_of(truth, delim)
    prim = [(k in hit) != invert for k in range(len(recs))]
    edge = [0] * (len(recs) + 1)  # +1 where a primary's reach begins, -1 behind its end
    for k, p in enumerate(prim):
        if p:
            edge[max(0, k - before)] += 1
            edge[min(len(recs), k + after + 1)] -= 1
    sel, depth = [], 0
    for k in range(len(recs)):
        depth += edge[k]
        sel.append(depth > 0)
    out, ent, groups = bytearray(), [], 0
    for k, r in enumerate(recs):
        if sel[k]:
            ent.append((k, offs[k], len(r) | (0 if prim[k] else CTX), len(out)))
            out += r
            groups += k == 0 or not sel[k - 1]
    stats = {"matched": sum(prim), "context": len(ent) - sum(prim), "groups": groups, "records": len(recs)}
    return bytes(out), ent, stats


def raw_rows(entries):
    return [tuple(int(e[f]) for f in ("record", "off", "len", "out_off")) for e in entries]


def ctx_rows(entries):
    """GREP_CONTEXT_ENTRY_DTYPE -> the rows of dilate()"""
    return [(int(e["record"]), int(e["off"]), int(e["len"]) | (CTX if e["context"] else 0), int(e["out_off"])) for e in entries]


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


@pytest.fixture(scope="module")
def inp(dec):
    return Input(dec)


@pytest.fixture
def context(dec):
    """sets the context of `dec` and resets it behind the test"""
    yield dec.grep_set_context
    dec.grep_set_context(0, 0)


def raw(dec, src, pat, before, after, invert=False):
    """bzh_grep_raw_device under the context (before, after) with the exact rooms against the truth: bytes, entries, the context
    bit, the counters; nothing behind the room is touched"""
    want, ent, stats = dilate(src, hit_records(src, pat), before, after, invert)
    t = on_device(src)
    dec.grep_set_context(before, after)
    out = room_on_device(len(want))
    st, nrecs, total, got = dec.grep_raw_device(t.data_ptr(), len(src), pat, out.data_ptr(), len(want), len(ent), b"\n", invert)
    what = (len(src), pat[:20], before, after, invert)
    assert (st, nrecs, total) == (0, len(ent), len(want)), what
    host = out.cpu().numpy().tobytes()
    assert host[:len(want)] == want and set(host[len(want):]) <= {0xA5}, what
    assert raw_rows(got) == ent, what
    cs = dec.grep_context_stats()
    if before or after:
        assert (cs["matched"], cs["context"], cs["groups"], cs["pending_peak"]) == (stats["matched"], stats["context"], stats["groups"], 0), what
    else:
        assert (cs["matched"], cs["context"], cs["groups"], cs["pending_peak"]) == (len(ent), 0, 0, 0), what
    assert dec.grep_stats()["records"] == stats["records"] and dec.grep_stats()["selected"] == len(ent)
    return want, ent, stats


# ---- the raw seam ---------------------------------------------------------------------------------------------------------------
def test_raw_grid(dec, context):
    rng = random.Random(9)
    seen_context = seen_groups = 0
    for n in NS:
        for alphabet in (b"abc", b"abc" * 13 + b"\n", b"ab\nc\n", b"\n"):  # no delimiter ... delimiters only: 16 records a thread
            src = bytes(rng.choice(alphabet) for _ in range(n))
            pat = b"\n" if alphabet == b"\n" and rng.random() < 0.5 else bytes(rng.choice(b"ab") for _ in range(rng.choice((1, 2, 3))))
            for before, after in BA:
                for invert in (False, True):
                    _, ent, stats = raw(dec, src, pat, before, after, invert)
                    seen_context += stats["context"]
                    seen_groups += stats["groups"]
    assert seen_context > 1000 and seen_groups > 1000


def test_raw_planted(dec, context):
    """a primary at a tile's edge with the context reaching over one and two tile edges, a record longer than a tile as context,
    contexts that overlap, touch and leave one record between them, a primary at both ends, a primary tail, a context tail"""
    line = lambda k, hit=False: (b"HIT " if hit else b"... ") + b"x" * (k - 5) + b"\n"
    recs = [line(96)] + [line(100) for _ in range(129)]  # records end at 96 + 100 k: record 40 ends at 4096
    for at in ((40,), (41,), (81,), (0,), (129,), (41, 123)):
        src = b"".join(line(len(r), k in at) for k, r in enumerate(recs))
        for reach in (1, 30, 50, 90):
            raw(dec, src, b"HIT", 0, reach)
            raw(dec, src, b"HIT", reach, 0)
            raw(dec, src, b"HIT", reach, reach, True)
    for big in (6000, 9000):
        raw(dec, line(10, True) + line(big) + line(20) * 2, b"HIT", 0, 1)
        raw(dec, line(10) + line(big) + line(20, True) + line(20), b"HIT", 1, 0)
        raw(dec, line(10, True) + line(20) + b"y" * big, b"HIT", 0, 2)  # the tail is after-context
        raw(dec, line(10) * 30 + b"HIT " + b"y" * big, b"HIT", 3, 0)  # a primary tail with before > 0
    for gap, groups in ((2, 1), (3, 1), (4, 2)):
        src = b"".join(line(9, k in (5, 5 + gap)) for k in range(20))
        assert raw(dec, src, b"HIT", 1, 1)[2]["groups"] == groups
    raw(dec, b"", b"a", 2, 2)
    raw(dec, b"\n" * 5000, b"\n", 0xFFFFFFFF, 0xFFFFFFFF)
    assert raw(dec, line(10) * 3000 + line(10, True) + line(10) * 3000, b"HIT", 0xFFFFFFFF, 0xFFFFFFFF)[2]["context"] == 6000  # any uint32_t saturates


def test_raw_more_tiles_than_scan_threads(dec, context):
    """just over 256 tiles: a thread of the scans owns two tiles, and the contexts cross the chunk edges"""
    base = lines(200_000, 7)
    n = 256 * 4096 + 77
    src = bytearray((base * (n // len(base) + 1))[:n])
    for at in range(5000, n - len(NEEDLE), 70_001):
        src[at:at + len(NEEDLE)] = NEEDLE
    src = bytes(src)
    for before, after, invert in ((200, 200, False), (3, 0, False), (0, 3, False), (1, 1, True)):
        _, _, stats = raw(dec, src, NEEDLE, before, after, invert)
        assert stats["context"] > 10 and dec.grep_stats()["tiles"] == 257


def test_raw_rooms(dec, context):
    src = lines(9000, 6)
    word = max(src[3000:3100].split(), key=len)[:4]
    want, ent, _ = dilate(src, hit_records(src, word), 2, 1)
    assert len(ent) > 10 and any(e[2] & CTX for e in ent)
    t, out = on_device(src), room_on_device(len(want))
    context(2, 1)
    assert dec.grep_raw_device(t.data_ptr(), len(src), word, 0, 0, 0)[:3] == (0, len(ent), len(want))  # the counting call
    for cap, room in ((len(want) - 1, len(ent)), (len(want), len(ent) - 1)):
        st, nrecs, tot, _ = dec.grep_raw_device(t.data_ptr(), len(src), word, out.data_ptr(), cap, room)
        assert (st, nrecs, tot) == (-4, len(ent), len(want)) and "room for" in dec.last_error()
    st, nrecs, tot, got = dec.grep_raw_device(t.data_ptr(), len(src), word, out.data_ptr(), len(want), len(ent))
    assert (st, nrecs, tot) == (0, len(ent), len(want)) and raw_rows(got) == ent and out.cpu().numpy().tobytes()[:len(want)] == want
    st, nrecs, tot, got = dec.grep_raw_device(t.data_ptr(), len(src), word, 0, 0, len(ent))  # entries alone
    assert (st, nrecs, tot) == (0, len(ent), len(want)) and raw_rows(got) == ent
    assert dec.grep_raw_device(t.data_ptr(), len(src), word, 0, 0, 0, flags=2)[0] == -1  # no new flag bit


# ---- the full decode, every block a window ----------------------------------------------------------------------------------------
def full(dec, inp, hit, what, before, after, invert, call):
    want, ent, stats = dilate(inp.truth, hit, before, after, invert)
    data, got = call(before, after, invert)
    assert data == want and ctx_rows(got) == ent, (what, before, after, invert)
    cs, st = dec.grep_context_stats(), dec.grep_stats()
    assert (cs["matched"], cs["context"], cs["groups"]) == (stats["matched"], stats["context"], stats["groups"]), (what, before, after, invert)
    assert st["records"] == stats["records"] and st["selected"] == len(ent)
    return cs, st


@pytest.mark.parametrize("ba", [(1, 1), (3, 0), (0, 3), (200, 200)])
def test_full_grep(dec1, inp, ba):
    dec, (before, after) = dec1, ba
    dec.search_set_room(1024)  # every block is a window: of the full decode by its batches of one, of an indexed walk by the room
    try:
        peaks = []
        for pat in (NEEDLE, inp.truth[5000:5003], b"\n"):
            hit = hit_records(inp.truth, pat)
            for invert in (False, True):
                cs, st = full(dec, inp, hit, pat, before, after, invert, lambda b, a, i: dec.grep(inp.s, pat, b"\n", i, before=b, after=a))
                assert st["windows"] >= 5 and cs["pending_peak"] <= before
                peaks.append(cs["pending_peak"])
        # the edges were reached: records were carried undecided -- at most `before` of them, so none without a before-context
        assert max(peaks) > 0 if before else max(peaks) == 0
    finally:
        dec.search_set_room(0)


@pytest.mark.parametrize("sync", [False, True])
def test_index_route_equals_the_full_route(dec, inp, sync):
    pts = inp.pts if sync else None
    dec.search_set_room(1024)
    try:
        for pat, invert, (before, after) in ((NEEDLE, False, (200, 200)), (inp.truth[5000:5003], False, (1, 1)), (b"e\n", True, (3, 0)), (NEEDLE, True, (0, 3))):
            data, got = dec.grep(inp.s, pat, b"\n", invert, before=before, after=after)
            cs = dec.grep_context_stats()
            idata, igot = dec.grep_index(inp.s, inp.ent, pat, pts, b"\n", invert, before=before, after=after)
            assert idata == data and igot.tobytes() == got.tobytes() and dec.grep_context_stats() == cs
            assert data == dilate(inp.truth, hit_records(inp.truth, pat), before, after, invert)[0]
            assert dec.grep_stats()["windows"] >= 5
    finally:
        dec.search_set_room(0)


def test_patset_and_regex(dec, inp, native):
    dec.search_set_room(1024)
    try:
        recs, _ = records_of(inp.truth)
        words = [NEEDLE, inp.truth[5000:5003].upper()]
        with native.PatternSet(dec, words, ignore_case=True) as pset:
            hit = {k for k, r in enumerate(recs) if any(w.lower() in r.lower() for w in words)}
            full(dec, inp, hit, "set", 2, 3, False, lambda b, a, i: dec.grep(inp.s, pset, b"\n", i, before=b, after=a))
        with native.PatternSet(dec, [b"^[A-Z]"], regex=True, syntax=native.REGEX_ASSERT) as rx:
            hit = {k for k, r in enumerate(recs) if re.search(rb"^[A-Z]", r)}
            assert hit
            full(dec, inp, hit, "^[A-Z]", 2, 1, False, lambda b, a, i: dec.grep(inp.s, rx, b"\n", i, before=b, after=a))
        with native.PatternSet(dec, [b"q[a-z]+"], regex=True, syntax=native.REGEX_WORD) as rx:
            hit = {k for k, r in enumerate(recs) if re.search(rb"(?<![0-9A-Za-z_])q[a-z]+(?![0-9A-Za-z_])", r)}
            assert 0 < len(hit) < len(recs)
            full(dec, inp, hit, "-w", 1, 2, False, lambda b, a, i: dec.grep(inp.s, rx, b"\n", i, before=b, after=a))
            full(dec, inp, hit, "-w", 2, 0, True, lambda b, a, i: dec.grep(inp.s, rx, b"\n", i, before=b, after=a))
    finally:
        dec.search_set_room(0)


def test_full_rooms(dec, inp, context):
    pat = inp.truth[5000:5003]
    want, ent, _ = dilate(inp.truth, hit_records(inp.truth, pat), 1, 2)
    assert len(ent) > 100
    context(1, 2)
    d_in, out = on_device(inp.s), room_on_device(len(want))
    for cap, room in ((len(want) - 1, len(ent)), (len(want), len(ent) - 1)):
        st, nrecs, tot, _ = dec.grep_device(d_in.data_ptr(), len(inp.s), pat, out.data_ptr(), cap, room)
        assert (st, nrecs, tot) == (-4, len(ent), len(want)) and "room for" in dec.last_error()
    st, nrecs, tot, got = dec.grep_device(d_in.data_ptr(), len(inp.s), pat, out.data_ptr(), len(want), len(ent))
    host = out.cpu().numpy().tobytes()
    assert (st, nrecs, tot) == (0, len(ent), len(want)) and host[:len(want)] == want and set(host[len(want):]) <= {0xA5} and raw_rows(got) == ent
    assert dec.grep(inp.s, pat, count_only=True) == (len(ent), len(want))  # the setting is the context's: the counting call sees it too


# ---- the setting ------------------------------------------------------------------------------------------------------------------
def test_the_setting(dec, inp, native, context):
    pat = inp.truth[5000:5003]
    plain = dec.grep(inp.s, pat)
    assert plain[1].dtype == native.GREP_ENTRY_DTYPE and not (plain[1]["len"] >> np.uint64(63)).any()
    want, ent, _ = dilate(inp.truth, hit_records(inp.truth, pat), 1, 1)
    context(1, 1)
    for _ in range(2):  # sticky across calls
        data, got = dec.grep(inp.s, pat)
        assert data == want and raw_rows(got) == ent
    # a damaged input is still the decoder's error with the decoder's text, and the context stays usable
    bad = bytearray(inp.s)
    bad[len(inp.s) // 3] ^= 0x10
    with pytest.raises(native.BzhError) as e1:
        dec.decode(bytes(bad))
    with pytest.raises(native.BzhError) as e2:
        dec.grep(bytes(bad), pat)
    assert e1.value.status == e2.value.status == -6 and str(e1.value) == str(e2.value)
    assert dec.grep(inp.s, pat)[0] == want
    context(0, 0)  # back to 0, 0: byte for byte what a fresh context gives
    again = dec.grep(inp.s, pat)
    with native.Context(0, 9, 2) as fresh:
        first = fresh.grep(inp.s, pat)
        assert fresh.grep_context_stats() == {"matched": len(first[1]), "context": 0, "groups": 0, "pending_peak": 0}
    assert again[0] == first[0] == plain[0] and again[1].tobytes() == first[1].tobytes() == plain[1].tobytes()
    assert dec.grep_context_stats() == {"matched": len(again[1]), "context": 0, "groups": 0, "pending_peak": 0}


# ---- Python and the command line --------------------------------------------------------------------------------------------------
def test_python_grep(inp, native):
    import banzai_amd
    pat = inp.truth[5000:5006]
    hit = hit_records(inp.truth, pat)
    assert banzai_amd.grep(inp.s, pat)[1].dtype == native.GREP_ENTRY_DTYPE
    rindex = banzai_amd.build_record_index(inp.s)
    rd = banzai_amd.IndexedReader(inp.s, rindex)
    for kw, (before, after) in (({"before": 2}, (2, 0)), ({"after": 3}, (0, 3)), ({"context": 1}, (1, 1)), ({"before": 1, "after": 400}, (1, 400))):
        want, ent, stats = dilate(inp.truth, hit, before, after)
        data, got = banzai_amd.grep(inp.s, pat, **kw)
        assert got.dtype == native.GREP_CONTEXT_ENTRY_DTYPE and data == want and ctx_rows(got) == ent and got["context"].sum() == stats["context"]
        assert banzai_amd.grep_count(inp.s, pat) == stats["matched"]  # unchanged: Python leaves no setting behind
        old = rd.grep(pat, before=before, after=after)
        assert [r for r, _ in old] == [e[0] for e in ent] and b"".join(b for _, b in old) == want
    want, ent, _ = dilate(inp.truth, hit, 1, 1, True)
    index = banzai_amd.SyncIndex(banzai_amd.BlockIndex(inp.ent.copy(), len(inp.s)), inp.pts.copy(), 4)
    data, got = banzai_amd.grep(inp.s, pat, invert=True, index=index, context=1)
    assert data == want and ctx_rows(got) == ent
    with pytest.raises(ValueError):
        banzai_amd.grep(inp.s, pat, context=1, after=2)
    with pytest.raises(ValueError):
        banzai_amd.grep(inp.s, pat, before=-1)
    with pytest.raises(ValueError):
        rd.grep(pat, after=1.5)


def test_cli_against_gnu_grep(tmp_path):
    """newline-terminated text without NUL bytes: bnzhip --grep -A/-B/-C writes byte for byte what GNU grep writes for the
    decompressed file, the `--` separators and N: / N- included"""
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    text = lines(250_000, 21)
    text = text[:text.rindex(b"\n") + 1]
    path, plain = tmp_path / "t.bz2", tmp_path / "t.txt"
    path.write_bytes(bz2.compress(text, 1))
    plain.write_bytes(text)
    word = max(text[7000:7100].split(), key=len).decode()  # a long word of the text
    gnu = shutil.which("grep", path="/usr/bin:/bin")
    cases = ((("--grep", word, "-A", "2"), ("-F", "-A", "2", word)),
             (("--grep", word, "-B", "2"), ("-F", "-B", "2", word)),
             (("--grep", word, "-C", "1", "--line-number"), ("-F", "-C", "1", "-n", word)),
             (("--grep", word, "--invert", "-C", "1"), ("-F", "-v", "-C", "1", word)),
             (("--grep", word, "--count", "-C", "3"), ("-F", "-c", "-C", "3", word)),
             (("--grep", "-E", "-w", "-e", "q[a-z]+", "-C", "2"), ("-E", "-w", "-C", "2", "q[a-z]+")),
             (("--grep", word, "--before-context", "1", "--after-context", "3", "--line-number"), ("-F", "-B", "1", "-A", "3", "-n", word)),
             (("--grep", word, "--context", "0"), ("-F", "-C", "0", word)))
    hit = hit_records(text, word.encode())
    assert 2 < len(hit) < len(records_of(text)[0]) // 2
    for mine, theirs in cases:
        p = subprocess.run([exe, *mine, str(path)], capture_output=True, timeout=120)
        assert p.returncode == 0, (mine, p.stderr)
        if gnu:
            q = subprocess.run([gnu, *theirs, str(plain)], capture_output=True, timeout=120, env=dict(os.environ, LC_ALL="C"))
            assert q.returncode == 0 and p.stdout == q.stdout, (mine, p.stdout[:300], q.stdout[:300])
    # against the truth as well, so that the test says something where GNU grep is not installed
    want, ent, stats = dilate(text, hit, 2, 0)
    p = subprocess.run([exe, "--grep", word, "-B", "2", str(path)], capture_output=True, timeout=120)
    assert p.stdout.replace(b"--\n", b"") == want and p.stdout.count(b"--\n") == stats["groups"] - 1
    p = subprocess.run([exe, "--grep", word, "-B", "2", "--count", str(path)], capture_output=True, timeout=120)
    assert p.stdout == b"%d\n" % stats["matched"]
