"""bzh_recover* on the MI355X: every block of a damaged .bz2 that verifies, the report of every one that does not, and the salvage
as one valid stream.  THE YARDSTICK IS libbz2 PER BLOCK, never this library: the extents of every block are known from the
undamaged stream (a NumPy scan for the magics), extent k of the damaged bytes is cut into a stream of its own ("BZh9" + its bits
+ footer magic + its stored CRC) and bz2.decompress is asked for it.  The kept set a case expects is {k : magic k intact and
libbz2 decodes extraction k}, the flags follow from that set and from what the case did to headers and footers, and every case
first asserts that libbz2 alone gives the kept set it is named for.  Damage lies in the Huffman-coded symbols (the last third of
a block's bits), in a magic, a header or a footer -- never in the code-length tables, where an over-subscribed table no selector
names is a pinned divergence from libbz2 ("Blocks no encoder writes").  The walk itself and the gather's per-word
rule are held on the CPU (tests/test_recover_host.py); here they meet the device."""
import bz2
import os
import random
import subprocess

import numpy as np
import pytest

from banzai_amd import corpus
from tests import decode_shapes
from tests.cases import gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "banzai_amd", "bnzhip")
OK, E_ARG, E_CAP, E_DATA = 0, -1, -4, -6
BLOCK_MAGIC, FOOTER_MAGIC = 0x314159265359, 0x177245385090
JOINED, STREAM_END, STREAM_OK = 1, 2, 4
TRUNC, FORMAT, BLOCK_CRC = 2, 3, 4


# ---- the yardstick --------------------------------------------------------------------------------------------------------
def scan(buf):
    """[(bit position, is_footer)] of every magic of buf at any bit alignment, ascending: the 8 shifts of a 56-bit window a byte"""
    a = np.frombuffer(bytes(buf) + b"\0" * 7, dtype=np.uint8).astype(np.uint64)
    n = len(buf)
    w = np.zeros(n, dtype=np.uint64)
    for j in range(7):
        w |= a[j:j + n] << np.uint64(8 * (6 - j))
    hits = []
    for s in range(8):
        v = (w >> np.uint64(8 - s)) & np.uint64((1 << 48) - 1)
        for magic, footer in ((BLOCK_MAGIC, False), (FOOTER_MAGIC, True)):
            for i in np.nonzero(v == np.uint64(magic))[0]:
                if 8 * int(i) + s + 48 <= 8 * n:
                    hits.append((8 * int(i) + s, footer))
    return sorted(hits)


def bits_of(buf, a, b):
    """bits [a, b) of buf as an int (bits behind the buffer read as zero)"""
    lo, hi = a // 8, (b + 7) // 8
    chunk = bytes(buf[lo:hi]).ljust(hi - lo, b"\0")
    v = int.from_bytes(chunk, "big") if chunk else 0
    return (v >> (8 * hi - b)) & ((1 << (b - a)) - 1)


def extraction(buf, a, b):
    """extent [a, b) of buf as a stream of its own: "BZh9", the bits, the footer magic, the block's stored CRC"""
    nb = b - a
    v = (0x425A6839 << (nb + 80)) | (bits_of(buf, a, b) << 80) | (FOOTER_MAGIC << 32) | bits_of(buf, a + 48, a + 80)
    total = 32 + nb + 80
    pad = -total % 8
    return (v << pad).to_bytes((total + pad) // 8, "big")


def libbz2_block(buf, a, b):
    """what libbz2 makes of extent [a, b) of buf alone: its bytes, or None where it refuses"""
    if b > 8 * len(buf) or bits_of(buf, a, a + 48) != BLOCK_MAGIC:
        return None
    try:
        return bz2.decompress(extraction(buf, a, b))
    except (OSError, ValueError, EOFError):
        return None


class Stream:
    def __init__(self, header, blocks, footer):
        self.header, self.blocks, self.footer = header, blocks, footer  # bit of "BZh", [(start, end)], bit of the footer magic


def layout(buf):
    """the streams of an UNDAMAGED buffer, from its magics: a footer ends a stream, the next header stands at the next byte"""
    streams, header, starts = [], 0, []
    for pos, footer in scan(buf):
        if not footer:
            starts.append(pos)
            continue
        ends = starts[1:] + [pos]
        streams.append(Stream(header, list(zip(starts, ends)), pos))
        header, starts = (pos + 80 + 7) // 8 * 8, []
    assert not starts and header == 8 * len(buf), "the undamaged input is whole streams"
    return streams


def expect(buf, streams, level=9):
    """What bzh_recover must report for `buf`, whose streams lay at `streams` before the damage, from libbz2 and the rules of
    include/bzhip.h -> ([entry dict], salvage bytes, streams_ok).  An entry: bit_pos, kept, and for kept ones out_off, out_len,
    crc, end_bit, flags."""
    nbits = 8 * len(buf)
    entries, out, streams_ok, prev_footer_whole = [], b"", 0, False
    for j, s in enumerate(streams):
        head = bytes(buf[s.header // 8:s.header // 8 + 4])
        is_header = len(head) == 4 and head[:3] == b"BZh" and 49 <= head[3] <= 57
        footer_magic = s.footer + 48 <= nbits and bits_of(buf, s.footer, s.footer + 48) == FOOTER_MAGIC
        footer_whole = footer_magic and s.footer + 80 <= nbits
        header_ok = is_header and (j == 0 or prev_footer_whole)  # at byte 0, or reported by the intact footer in front of it
        prev_footer_whole = footer_whole
        reaches, fold, fits, prev_kept = header_ok, 0, True, False
        for i, (a, b) in enumerate(s.blocks):
            if a + 48 > nbits or bits_of(buf, a, a + 48) != BLOCK_MAGIC:
                reaches = prev_kept = False  # no candidate: the chain of joined blocks breaks here
                continue
            got = libbz2_block(buf, a, b)
            if got is not None and len(got) > 0 and block_bytes_behind_rle(got) > 100000 * level:
                got = None
            e = {"bit_pos": a, "kept": got is not None, "out_off": len(out), "crc": bits_of(buf, a + 48, a + 80) if a + 80 <= nbits else 0}
            if got is None:
                reaches = prev_kept = False
                entries.append(e)
                continue
            joined = (i == 0 and header_ok) or (i > 0 and prev_kept)
            if not joined:
                reaches = False
            elif i == 0:
                reaches, fold, fits = True, 0, True
            fold = (((fold << 1) | (fold >> 31)) & 0xFFFFFFFF) ^ e["crc"]
            if header_ok:
                fits = fits and block_bytes_behind_rle(got) <= 100000 * (head[3] - 48)
            flags = JOINED if joined else 0
            if i == len(s.blocks) - 1 and footer_magic:
                flags |= STREAM_END
                if footer_whole and reaches and fits and fold == bits_of(buf, s.footer + 48, s.footer + 80):
                    flags |= STREAM_OK
                    streams_ok += 1
            e.update(out_len=len(got), end_bit=b, flags=flags)
            entries.append(e)
            out += got
            prev_kept = True
        if not s.blocks and header_ok and footer_whole and bits_of(buf, s.footer + 48, s.footer + 80) == 0:
            streams_ok += 1
    return entries, out, streams_ok


def block_bytes_behind_rle(raw):
    """the bytes of a block's last column: libbz2's RLE1 of its decoded bytes (runs of 4..255 equal bytes become 4 + a count)"""
    a = np.frombuffer(raw, dtype=np.uint8)
    if a.size == 0:
        return 0
    edges = np.flatnonzero(np.diff(a)) + 1
    runs = np.diff(np.concatenate(([0], edges, [a.size])))
    full, rest = runs // 255, runs % 255
    return int((full * 5 + np.where(rest >= 4, 5, rest)).sum())


def check(ctx, buf, streams, level=9, ctx_entries=None):
    """recover(buf) entry for entry and byte for byte against libbz2 -> (salvage, report, expected entries)"""
    want, salvage, streams_ok = expect(buf, streams, level)
    out, ent = ctx.recover(buf)
    st = ctx.recover_stats()
    assert [int(e["bit_pos"]) for e in ent] == [w["bit_pos"] for w in want], "one entry per block magic outside the kept blocks"
    for e, w in zip(ent, want):
        assert (int(e["kind"]) == 0) == w["kept"], (w, e)
        assert int(e["out_off"]) == w["out_off"] and int(e["crc"]) == w["crc"], (w, e)
        if w["kept"]:
            assert (int(e["out_len"]), int(e["end_bit"]), int(e["flags"]), int(e["err_bit"])) == (w["out_len"], w["end_bit"], w["flags"], 0), (w, e)
        else:
            # (libbz2 says THAT a block is lost, not which of this decoder's checks finds it first: the cases pin the kind where
            # the damage fixes it; no case here makes a randomised block.  The failure is found at or behind the magic, inside
            # the input: a damaged symbol stream may be read on past the block's old end before a check trips.  Behind the input
            # the reader hands out zeros until the next truncation check; the longest stretch between two checks is one code
            # length table, 5 + 258 bits of zeros.)
            assert (int(e["out_len"]), int(e["end_bit"]), int(e["flags"])) == (0, 0, 0) and int(e["kind"]) in (TRUNC, FORMAT, BLOCK_CRC), (w, e)
            assert w["bit_pos"] <= int(e["err_bit"]) <= 8 * len(buf) + 263, (w, e)
    assert out == salvage
    kept = sum(w["kept"] for w in want)
    assert (st["kept"], st["lost"], st["streams_ok"], st["out_bytes"]) == (kept, len(want) - kept, streams_ok, len(salvage)), st
    ds = ctx.decode_stats()
    assert (ds["blocks"], ds["streams"], ds["candidates_off_chain"]) == (kept, streams_ok, st["shadowed"])
    return out, ent, want


def repaired(ctx, buf, ent, salvage):
    """recover_stream of the report: libbz2 reads it back to the salvage"""
    rep = ctx.recover_stream(buf, ent)
    assert rep[:4] == b"BZh" + bytes([48 + ctx.level])
    assert bz2.decompress(rep) == salvage
    return rep


def flip(buf, bit):
    b = bytearray(buf)
    b[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(b)


def payload_bit(block, frac=0.8):
    """a bit inside the Huffman-coded symbols: the last third of the block's bits"""
    a, b = block
    return a + int((b - a) * frac)


# ---- the inputs -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    rng = random.Random(20261019)
    segs = []
    for _ in range(12):  # (a) short-period text: 13 blocks of a few hundred bits, at many residues mod 32
        pat = bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 10)))
        tail = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 41)))
        segs.append((pat * (100_000 // len(pat) + 1))[:100_000 - len(tail)] + tail)
    a_raw = b"".join(segs)
    a = bz2.compress(a_raw, 1)
    # (b) one-block streams of 0-300 raw bytes, byte aligned, empty ones among them: 40 of them, and on until the blocks, laid
    # end to end from bit 32, have started at every residue mod 32 (the destination side of the gather)
    b_raws, b_streams, at, seen = [], [], 32, set()
    while len(b_raws) < 40 or len(seen) < 32:
        assert len(b_raws) < 400
        r = bytes(rng.randrange(256) for _ in range(0 if len(b_raws) % 9 == 4 else rng.randrange(0, 301)))
        z = bz2.compress(r, 9)
        for lo, hi in layout(z)[0].blocks:
            seen.add(at % 32)
            at += hi - lo
        b_raws.append(r)
        b_streams.append(z)
    b = b"".join(b_streams)
    c_raw = corpus.enwik_synthetic(260_000, seed=11).tobytes()
    c = bz2.compress(c_raw, 1)                         # (c) three blocks of 100 kB text, some 35 kB each
    built = decode_shapes.accepted()
    d_parts = [built["no_bwt_abba_0"], built["lengths_1_to_20"]]  # (d) hand-built: a column that is no BWT of anything
    d = b"".join(p.stream for p in d_parts)
    d_raw = b"".join(p.expected for p in d_parts)
    return {"a": (a, a_raw), "b": (b, b"".join(b_raws)), "c": (c, c_raw), "d": (d, d_raw)}


@pytest.fixture(scope="module")
def ctxs(native):
    made = {(lv, mb): native.Context(0, lv, mb) for lv, mb in ((1, 0), (9, 0), (9, 8))}
    yield made
    for c in made.values():
        c.close()


def to_device(buf):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(buf) + b"\0" * 16, dtype=np.uint8).copy()).to("cuda")


# ---- undamaged ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_undamaged(ctxs, inputs, name):
    """recover == decode, all blocks kept and joined, every stream STREAM_OK; the repaired stream decodes to the same bytes under
    libbz2, and for (a) and (c) on a context of the stream's level it IS the input, byte for byte"""
    buf, raw = inputs[name]
    ctx = ctxs[(9, 0)]
    streams = layout(buf)
    out, ent, want = check(ctx, buf, streams)
    assert out == raw == ctx.decode(buf)
    assert all(w["kept"] and w["flags"] & JOINED for w in want)
    assert ctx.recover_stats()["streams_ok"] == len(streams) and ctx.recover_stats()["lost"] == 0
    nblocks = sum(len(s.blocks) for s in streams)
    assert len(ent) == nblocks and {"a": 13, "c": 3}.get(name, nblocks) == nblocks
    if name == "a":  # the case is here for its bit alignments: it must not drift off that edge
        assert len({int(e["bit_pos"]) % 32 for e in ent}) >= 6
    if name == "b":  # every block byte aligned, every destination residue of the gather reached
        at, res = 32, set()
        for e in ent:
            assert int(e["bit_pos"]) % 8 == 0
            res.add(at % 32)
            at += int(e["end_bit"]) - int(e["bit_pos"])
        assert len(res) == 32
    repaired(ctx, buf, ent, raw)
    if name in ("a", "c"):
        c1 = ctxs[(1, 0)]
        out1, ent1 = c1.recover(buf)
        assert out1 == raw and c1.recover_stream(buf, ent1) == buf


def test_python_surface(inputs):
    import banzai_amd
    buf, raw = inputs["c"]
    r = banzai_amd.recover(buf)
    assert r.data == raw and r.complete and len(r.kept) == 3 and not r.lost and r.stats["streams_ok"] == 1
    dmg = flip(buf, payload_bit(layout(buf)[0].blocks[1]))
    r = banzai_amd.recover(dmg)
    assert not r.complete and len(r.kept) == 2 and len(r.lost) == 1 and r.lost[0].kind in (TRUNC, FORMAT, BLOCK_CRC)
    assert r.data == raw[:r.kept[1].out_off] + raw[len(raw) - r.kept[1].out_len:]
    for rep in (banzai_amd.recover_stream(dmg), banzai_amd.recover_stream(dmg, r), banzai_amd.recover_stream(dmg, r.blocks)):
        assert bz2.decompress(rep) == r.data
    with pytest.raises(banzai_amd.BzhError):
        banzai_amd.decompress(dmg)


# ---- damage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("how", ["flip", "hole"])
def test_payload_damage(ctxs, inputs, how, which):
    """a flipped payload bit, and 64 bytes of zeros, in the first, a middle and the last block of (c): libbz2 refuses that block
    and that block only"""
    buf, _ = inputs["c"]
    streams = layout(buf)
    blk = streams[0].blocks[which]
    at = payload_bit(blk)
    dmg = flip(buf, at) if how == "flip" else buf[:at // 8] + b"\0" * 64 + buf[at // 8 + 64:]
    assert [libbz2_block(dmg, *b) is not None for b in streams[0].blocks] == [k != which for k in range(3)]
    ctx = ctxs[(9, 0)]
    out, ent, want = check(ctx, dmg, streams)
    assert [w["kept"] for w in want] == [k != which for k in range(3)]
    e = ent[which]  # the damage lies in the symbols: whichever check trips, it is no earlier than the block's first code
    assert int(e["kind"]) in (FORMAT, BLOCK_CRC, TRUNC)
    eb = int(e["err_bit"])  # (a check of the decoded bytes -- CRC, an open run at the end -- names the magic; the entropy stage, where it gave up)
    assert eb == blk[0] or (int(e["kind"]) != BLOCK_CRC and blk[0] + 80 < eb <= 8 * len(dmg) + 263)
    repaired(ctx, dmg, ent, out)


def test_payload_damage_in_small_blocks(ctxs, inputs):
    """the same in (a), whose blocks start at many bit alignments: three blocks lost, ten kept, the repaired stream whole"""
    buf, _ = inputs["a"]
    streams = layout(buf)
    dmg = buf
    for k in (0, 6, 12):
        dmg = flip(dmg, payload_bit(streams[0].blocks[k], 0.9))
    lost = [libbz2_block(dmg, *b) is None for b in streams[0].blocks]
    assert lost == [k in (0, 6, 12) for k in range(13)]
    ctx = ctxs[(9, 0)]
    out, ent, want = check(ctx, dmg, streams)
    kept = ent[ent["kind"] == 0]
    assert len({int(e["bit_pos"]) % 32 for e in kept}) >= 6
    repaired(ctx, dmg, ent, out)


def test_flipped_bit_in_a_magic(ctxs, inputs):
    """the block behind a damaged magic is neither kept nor reported; the block in front of it is kept (a split at the next magic
    would lose it: its extent would run on to the magic after)"""
    buf, raw = inputs["c"]
    streams = layout(buf)
    dmg = flip(buf, streams[0].blocks[1][0] + 13)
    ctx = ctxs[(9, 0)]
    out, ent, want = check(ctx, dmg, streams)
    assert [int(e["bit_pos"]) for e in ent] == [streams[0].blocks[0][0], streams[0].blocks[2][0]] and all(e["kind"] == 0 for e in ent)
    assert libbz2_block(dmg, streams[0].blocks[0][0], streams[0].blocks[2][0]) is None  # bzip2recover's extent of block 0
    assert int(ent[0]["flags"]) == JOINED and int(ent[1]["flags"]) == STREAM_END
    repaired(ctx, dmg, ent, out)


def test_stream_header_zeroed(ctxs, inputs):
    buf, raw = inputs["c"]
    dmg = b"\0" * 4 + buf[4:]
    ctx = ctxs[(9, 0)]
    out, ent, want = check(ctx, dmg, layout(buf))
    assert out == raw and [int(e["flags"]) for e in ent] == [0, JOINED, JOINED | STREAM_END]
    assert ctx.recover_stats()["streams_ok"] == 0
    repaired(ctx, dmg, ent, out)


@pytest.mark.parametrize("what", ["magic", "crc"])
def test_footer_damage(ctxs, inputs, what):
    buf, raw = inputs["c"]
    streams = layout(buf)
    dmg = flip(buf, streams[0].footer + (20 if what == "magic" else 60))
    ctx = ctxs[(9, 0)]
    out, ent, want = check(ctx, dmg, streams)
    assert out == raw and int(ent[2]["flags"]) == (JOINED if what == "magic" else JOINED | STREAM_END)
    assert ctx.recover_stats()["streams_ok"] == 0


def test_truncation(ctxs, inputs):
    """inside the last block: TRUNC; directly behind a block: kept, no STREAM_END"""
    buf, raw = inputs["c"]
    streams = layout(buf)
    ctx = ctxs[(9, 0)]
    last = streams[0].blocks[2]
    cut = buf[:payload_bit(last) // 8]
    out, ent, want = check(ctx, cut, streams)
    assert [int(e["kind"]) for e in ent] == [0, 0, TRUNC] and int(ent[2]["err_bit"]) >= last[0]
    behind = buf[:(last[1] + 7) // 8]  # (the block's last bits and up to seven of the footer's)
    out, ent, want = check(ctx, behind, streams)
    assert [int(e["kind"]) for e in ent] == [0, 0, 0] and int(ent[2]["flags"]) == JOINED and out == raw
    repaired(ctx, behind, ent, raw)


def test_bytes_deleted_mid_block(ctxs, inputs):
    """30 bytes gone from block 1: it is lost, block 2 is found 240 bits earlier and kept"""
    buf, raw = inputs["c"]
    s = layout(buf)[0]
    at = payload_bit(s.blocks[1]) // 8
    dmg = buf[:at] + buf[at + 30:]
    moved = Stream(0, [s.blocks[0], (s.blocks[1][0], s.blocks[1][1] - 240), (s.blocks[2][0] - 240, s.blocks[2][1] - 240)], s.footer - 240)
    ctx = ctxs[(9, 0)]
    out, ent, want = check(ctx, dmg, [moved])
    assert [w["kept"] for w in want] == [True, False, True] and int(ent[2]["bit_pos"]) == s.blocks[2][0] - 240
    repaired(ctx, dmg, ent, out)


def test_stream_planted_in_a_lost_block(ctxs, inputs):
    """a tiny valid stream written byte-aligned into a lost block's hole is kept, between the blocks around it"""
    buf, raw = inputs["c"]
    s = layout(buf)[0]
    tiny_raw = b"planted in the hole"
    tiny = bz2.compress(tiny_raw, 9)
    at = payload_bit(s.blocks[1]) // 8
    dmg = buf[:at] + tiny + buf[at + len(tiny):]
    t = layout(tiny)[0]
    assert [libbz2_block(dmg, *b) is not None for b in s.blocks] == [True, False, True]
    ctx = ctxs[(9, 0)]
    out, ent = ctx.recover(dmg)
    assert [int(e["bit_pos"]) for e in ent] == [s.blocks[0][0], s.blocks[1][0], 8 * at + t.blocks[0][0], s.blocks[2][0]]
    assert [int(e["kind"]) == 0 for e in ent] == [True, False, True, True]
    b0, b2 = libbz2_block(dmg, *s.blocks[0]), libbz2_block(dmg, *s.blocks[2])
    assert out == b0 + tiny_raw + b2 and int(ent[2]["out_off"]) == len(b0) and int(ent[2]["out_len"]) == len(tiny_raw)
    assert int(ent[2]["flags"]) == STREAM_END and int(ent[3]["flags"]) == STREAM_END  # neither run reaches a stream header
    repaired(ctx, dmg, ent, out)


def test_block_above_the_contexts_level(ctxs):
    """a level-9 stream with a 150,000-byte block, given to a level-1 context: FORMAT, the others kept"""
    small, big = gen(40_000, "text", 5), gen(150_000, "random", 6)
    buf = bz2.compress(small, 9) + bz2.compress(big, 9) + bz2.compress(small[::-1], 9)
    streams = layout(buf)
    assert [len(s.blocks) for s in streams] == [1, 1, 1]
    ctx = ctxs[(1, 0)]
    out, ent, want = check(ctx, buf, streams, level=1)
    assert [int(e["kind"]) for e in ent] == [0, FORMAT, 0] and out == small + small[::-1]
    assert [int(e["flags"]) for e in ent] == [JOINED | STREAM_END | STREAM_OK, 0, JOINED | STREAM_END | STREAM_OK]
    repaired(ctx, buf, ent, out)


def test_nothing_to_keep(ctxs, inputs):
    """everything lost, pure noise, empty input: BZH_OK, the entries say what happened, the repaired stream is the empty one"""
    ctx = ctxs[(9, 0)]
    buf, _ = inputs["c"]
    streams = layout(buf)
    dmg = buf
    for b in streams[0].blocks:
        dmg = flip(dmg, payload_bit(b))
    out, ent, want = check(ctx, dmg, streams)
    assert out == b"" and len(ent) == 3 and all(e["kind"] != 0 for e in ent)
    empty = b"BZh9" + bytes.fromhex("177245385090") + b"\0" * 4
    assert ctx.recover_stream(dmg, ent) == empty
    noise = bytes(random.Random(3).randrange(256) for _ in range(20_000))
    for junk in (noise, b"", b"BZ", b"BZh9"):
        out, ent = ctx.recover(junk)
        assert out == b"" and len(ent) == 0 and ctx.recover_stats()["kept"] == 0
        assert ctx.recover_stream(junk, ent) == empty


# ---- sizing, batches, refusals, guard bytes -------------------------------------------------------------------------------------
def test_sizing(ctxs, inputs):
    """cap 0 with a null buffer: the full report and the exact size; one byte too few: BZH_E_CAP with the same report; max too
    small: BZH_E_CAP with the count"""
    buf, _ = inputs["c"]
    dmg = flip(buf, payload_bit(layout(buf)[0].blocks[1]))
    ctx = ctxs[(9, 0)]
    out, ent = ctx.recover(dmg)
    st, got, need, e0, cnt = ctx.recover_raw(dmg, 0, 16)
    assert (st, got, need, cnt) == (E_CAP, None, len(out), 3) and e0.tobytes() == ent.tobytes()
    st, got, need, e1, cnt = ctx.recover_raw(dmg, len(out) - 1, 16)
    assert (st, got, need, cnt) == (E_CAP, None, len(out), 3) and e1.tobytes() == ent.tobytes()
    st, got, need, e2, cnt = ctx.recover_raw(dmg, len(out), 2)
    assert (st, need, e2, cnt) == (E_CAP, len(out), None, 3) and got == out
    st, got, need, e3, cnt = ctx.recover_raw(dmg, len(out), 3)
    assert (st, got, cnt) == (OK, out, 3) and e3.tobytes() == ent.tobytes()


def test_batch_edges_on_the_device(ctxs, inputs):
    """(b) through a context of max_batch 8: a batch edge between a stream's last block and its footer, and everywhere else"""
    buf, raw = inputs["b"]
    streams = layout(buf)
    ctx = ctxs[(9, 8)]
    out, ent, want = check(ctx, buf, streams)
    assert out == raw and ctx.recover_stats()["batches"] >= 8 and ctx.recover_stats()["streams_ok"] == len(streams)
    dmg = buf
    hit = [j for j, s in enumerate(streams) if s.blocks and s.blocks[0][1] - s.blocks[0][0] > 600][::5]
    for j in hit:
        dmg = flip(dmg, payload_bit(streams[j].blocks[0], 0.9))
    out, ent, want = check(ctx, dmg, streams)
    assert sum(not w["kept"] for w in want) == len(hit) > 0
    repaired(ctx, dmg, ent, out)
    assert ent.tobytes() == ctxs[(9, 0)].recover(dmg)[1].tobytes()


def test_device_calls_keep_to_their_buffers(ctxs, inputs):
    """16 guard bytes behind every device output stay untouched: the salvage, and the repaired stream's words"""
    import torch
    buf, _ = inputs["a"]
    streams = layout(buf)
    dmg = flip(buf, payload_bit(streams[0].blocks[5], 0.9))
    ctx = ctxs[(9, 0)]
    out, ent = ctx.recover(dmg)
    d_in = to_device(dmg)
    d_out = torch.full((len(out) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    st, need, e, cnt = ctx.recover_device(d_in.data_ptr(), len(dmg), d_out.data_ptr(), len(out), 64)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().tobytes()
    assert (st, need, cnt) == (OK, len(out), 13) and got[:len(out)] == out and got[len(out):] == b"\xa5" * 16
    assert e.tobytes() == ent.tobytes()
    st, need, e, cnt = ctx.recover_device(d_in.data_ptr(), len(dmg), 0, 0, 64)  # the verification run: nothing to write to
    assert (st, need, cnt) == (E_CAP, len(out), 13) and e.tobytes() == ent.tobytes()
    rep = ctx.recover_stream(dmg, ent)
    room = (len(rep) + 3) // 4 * 4
    d_rep = torch.full((room + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    st, need = ctx.recover_stream_device(d_in.data_ptr(), len(dmg), ent, d_rep.data_ptr(), room)
    torch.cuda.synchronize()
    got = d_rep.cpu().numpy().tobytes()
    assert (st, need) == (OK, len(rep)) and got[:len(rep)] == rep and got[len(rep):room] == b"\0" * (room - len(rep))
    assert got[room:] == b"\xa5" * 16
    st, need = ctx.recover_stream_device(d_in.data_ptr(), len(dmg), ent, d_rep.data_ptr(), room - 4)
    assert (st, need) == (E_CAP, len(rep))
    torch.cuda.synchronize()
    assert bz2.decompress(rep) == out


def test_stream_refusals(ctxs, inputs):
    """overlapping entries, an end behind the input, a block of 80 bits, a lost entry with an end: BZH_E_ARG naming the entry; an
    entry that points at no magic: BZH_E_DATA; a valid call after each"""
    buf, raw = inputs["c"]
    ctx = ctxs[(9, 0)]
    out, ent = ctx.recover(buf)
    good = ctx.recover_stream(buf, ent)

    def refused(entries, status, word):
        st, got, _ = ctx.recover_stream_raw(buf, entries, len(good) + 64)
        assert st == status and got is None and word in ctx.last_error(), (st, ctx.last_error())
        assert ctx.recover_stream(buf, ent) == good

    e = ent.copy()
    e["bit_pos"][1] = e["end_bit"][0] - 1
    refused(e, E_ARG, "entry 1")
    e = ent.copy()
    e["end_bit"][2] = 8 * len(buf) + 1
    refused(e, E_ARG, "entry 2")
    e = ent.copy()
    e["end_bit"][0] = e["bit_pos"][0] + 80
    refused(e, E_ARG, "entry 0")
    e = ent.copy()
    e["kind"][1] = BLOCK_CRC
    refused(e, E_ARG, "entry 1")
    e = ent.copy()
    e["bit_pos"][1] += 1
    refused(e, E_DATA, "entry 1")
    e = ent.copy()  # lost entries are otherwise ignored
    e["kind"][1], e["end_bit"][1] = BLOCK_CRC, 0
    assert bz2.decompress(ctx.recover_stream(buf, e)) == raw[:int(ent["out_len"][0])] + raw[int(ent["out_off"][2]):]


def test_cli(native, inputs, tmp_path):
    """bnzhip --recover end to end on a damaged (c): exit code 4, the salvage, one lost line; on the undamaged file: 0"""
    buf, raw = inputs["c"]
    streams = layout(buf)
    dmg = flip(buf, payload_bit(streams[0].blocks[1]))
    want = libbz2_block(dmg, *streams[0].blocks[0]) + libbz2_block(dmg, *streams[0].blocks[2])
    z = tmp_path / "damaged.bz2"
    z.write_bytes(dmg)
    r = subprocess.run([BIN, "--recover", str(z)], capture_output=True, text=True)
    assert r.returncode == 4, r.stderr
    assert (tmp_path / "damaged").read_bytes() == want and z.exists()
    lost = [ln for ln in r.stderr.splitlines() if ln.startswith("lost:")]
    assert len(lost) == 1 and f"bit {streams[0].blocks[1][0]}:" in lost[0]
    assert "2 blocks kept, 1 lost" in r.stderr and f"{len(want)} bytes" in r.stderr
    r = subprocess.run([BIN, "--recover", "-c", "-"], input=buf, capture_output=True)
    assert r.returncode == 0 and r.stdout == raw and b"3 blocks kept, 0 lost" in r.stderr and b"1 streams whole" in r.stderr
