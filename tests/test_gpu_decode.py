"""GPU: the bzip2 decoder (bzh_decode*, banzai_amd.decompress, bnzhip -d) against libbz2 and the strict CPU decoder.
Valid streams first, damaged ones last: the wide mutation loop runs on the CPU build of the parser
(tests/test_decode_host.py), the shared GPU only sees a short, fixed list."""
import bz2
import io
import json
import os
import random
import subprocess

import numpy as np
import pytest

from tests import bz2_handbuilt, cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "banzai_amd", "bnzhip")
BLOCK_MAGIC, FOOTER_MAGIC = bytes.fromhex("314159265359"), bytes.fromhex("177245385090")


@pytest.fixture(scope="module")
def dec(native):
    """the decoding context: level 9 (every stream's level fits), batches of 8 blocks"""
    c = native.Context(0, 9, 8)
    yield c
    c.close()


def round_trip(dec, enc, data, level):
    """libbz2's stream of `data`, and the library's own in both Huffman modes, all decoded on the GPU"""
    assert dec.decode(bz2.compress(data, level)) == data
    for fixed in (False, True):
        enc.set_mode(fixed)
        try:
            s = enc.encode(data)
        finally:
            enc.set_mode(False)
        got, used = dec.decode(s, with_consumed=True)
        assert got == data and used == len(s)


# ---- valid streams ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cases.MODES)
def test_round_trips_level1(dec, ctx1, mode):
    for n in cases.SIZES_L1:
        round_trip(dec, ctx1, cases.gen(n, mode, 17), 1)


@pytest.mark.parametrize("mode", cases.MODES)
def test_round_trips_level9(dec, ctx9, mode):
    for n in cases.SIZES_L9:
        round_trip(dec, ctx9, cases.gen(n, mode, 23), 9)


def test_round_trips_boundaries_repeats_mixture(dec, ctx1, ctx9):
    bc = cases.boundary_cases()
    runlens = {}
    for k, d in enumerate(bc):  # a sample that keeps every run length: the first and the last prefix of each
        runlens.setdefault(k % 8, []).append(d)
    assert len(runlens) == 8
    for group in runlens.values():
        for d in (group[0], group[len(group) // 2], group[-1]):
            round_trip(dec, ctx1, d, 1)
    round_trip(dec, ctx1, cases.repeats(260_000, 4), 1)
    round_trip(dec, ctx9, cases.repeats(1_200_000, 5), 9)
    rng = random.Random(99)
    for _ in range(12):
        round_trip(dec, ctx1, cases.mixture(rng, 300_000), 1)
    for _ in range(4):
        round_trip(dec, ctx9, cases.mixture(rng, 2_000_000), 9)


def test_golden_streams(dec):
    v = json.load(open(os.path.join(GOLDEN, "streams.json")))["streams"]
    assert v
    for c in v:
        s = bytes.fromhex(c["stream_hex"])
        assert dec.decode(s) == bz2.decompress(s), c.get("name")


def test_hand_built_blocks(dec, native, oracle):
    """what libbz2's encoder never writes: counts above 251, a count byte equal to the run byte, a completely full block
    (nblock = 100,000 x level, one more than this library's own encoder fills), the largest expansion the format allows"""
    s = bz2_handbuilt.stream_of_rle((b"aaaa\xff" + b"bbbb\xfe") * 10000, 1)
    want = (b"a" * 259 + b"b" * 258) * 10000
    assert len(want) == 5_170_000 and bz2.decompress(s) == want == oracle.decode(s)
    assert dec.decode(s) == want
    with native.Context(0, 1, 4) as c1:  # the full block on a context of its own level: n = M + 1 through the inverse BWT
        assert c1.decode(s) == want
    s = bz2_handbuilt.stream_of_rle(b"\x05" * 5 + b"xyz", 1)
    assert dec.decode(s) == b"\x05" * 9 + b"xyz" == bz2.decompress(s)
    # ends in four equal bytes without a count: the strict decoder lets it pass, libbz2 does not -- libbz2's verdict holds
    s = bz2_handbuilt.stream_of_rle(b"qrszzzz", 1, raw=b"qrszzzz")
    with pytest.raises(Exception):
        bz2.decompress(s)
    with pytest.raises(native.BzhError) as e:
        dec.decode(s)
    assert e.value.status == -6 and "four equal bytes" in str(e.value)
    s = bz2_handbuilt.stream_of_rle(b"qrszzzz\x00", 1)
    assert dec.decode(s) == b"qrszzzz" == bz2.decompress(s)
    # level 9, 180,000 groups of four bytes and a count of 255 in one block: 46,620,000 bytes out of one block
    s = bz2_handbuilt.stream_of_rle(b"".join(bytes([65 + k % 7]) * 4 + b"\xff" for k in range(180_000)), 9)
    got = dec.decode(s)
    assert len(got) == 46_620_000 and got == bz2.decompress(s)


def test_multi_batch(dec, ctx1):
    d = cases.gen(2_400_000, "text", 2)[:1_200_000] + cases.gen(1_200_000, "shortruns", 2)
    s = bz2.compress(d, 1)
    assert dec.decode(s) == d
    st = dec.decode_stats()
    assert st["blocks"] >= 20 and st["streams"] == 1 and st["out_bytes"] == len(d) and st["in_bytes"] == len(s)
    assert dec.decode(ctx1.encode(d)) == d


def test_concatenation(dec, native, ctx1, ctx9):
    rng = np.random.default_rng(3)
    parts = [bytes(rng.integers(97, 105, int(rng.integers(1, 3000)), dtype=np.uint8)) for _ in range(1000)]
    s = b"".join(bz2.compress(p, 1 + k % 9) for k, p in enumerate(parts))  # the pbzip2 shape
    got, used = dec.decode(s, with_consumed=True)
    assert got == b"".join(parts) and used == len(s)
    assert dec.decode_stats()["streams"] == 1000
    a, b = cases.gen(1_000_000, "text", 5), cases.gen(150_000, "longruns", 6)
    mixed = ctx9.encode(a) + bz2.compress(b"", 9) + ctx1.encode(b) + bz2.compress(a[:5000], 4)
    got, used = dec.decode(mixed, with_consumed=True)
    assert got == a + b + a[:5000] == bz2.decompress(mixed) and used == len(mixed)
    assert dec.decode_stats()["streams"] == 4
    with native.Context(0, 1, 4) as c1:  # a stream above the context's level is the caller's error, not the data's
        with pytest.raises(native.BzhError) as e:
            c1.decode(ctx9.encode(a))
        assert e.value.status == -1
        assert c1.decode(ctx1.encode(b)) == b


def plant(buf, bitpos, magic):
    v = int.from_bytes(magic, "big")
    for k in range(48):
        byte, bit = (bitpos + k) // 8, 7 - (bitpos + k) % 8
        buf[byte] = (buf[byte] & ~(1 << bit)) | (((v >> (47 - k)) & 1) << bit)


def numpy_scan(data):
    """[(bit position, kind)] of both magics at every bit alignment"""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint16)
    ext = np.concatenate([a, np.zeros(1, np.uint16)])
    hits = []
    for s in range(8):
        sh = (((ext[:-1] << s) | (ext[1:] >> (8 - s))) & 0xFF).astype(np.uint8).tobytes()
        for kind, magic in ((0, BLOCK_MAGIC), (1, FOOTER_MAGIC)):
            at = sh.find(magic)
            while at >= 0:
                if at * 8 + s + 48 <= len(data) * 8:
                    hits.append((at * 8 + s, kind))
                at = sh.find(magic, at + 1)
    return sorted(hits)


def foreign_tail():
    tail = bytearray(np.random.default_rng(77).integers(0, 256, 65536, dtype=np.uint8).tobytes())
    tail[0:4] = b"\x00\x01\x02\x03"  # not a stream header
    planted = []
    for k in range(8):
        plant(tail, 8 * (1000 + 700 * k) + k, BLOCK_MAGIC)
        plant(tail, 8 * (30000 + 900 * k) + k, FOOTER_MAGIC)
        planted += [(8 * (1000 + 700 * k) + k, 0), (8 * (30000 + 900 * k) + k, 1)]
    return bytes(tail), sorted(planted)


def test_trailing_foreign_bytes_and_chain(dec):
    d = cases.gen(260_000, "text", 8)
    s = bz2.compress(d, 1)
    tail, planted = foreign_tail()
    got, used = dec.decode(s + tail, with_consumed=True)
    assert got == d and used == len(s)
    st = dec.decode_stats()
    inside = numpy_scan(s)
    assert st["candidates"] == len(numpy_scan(s + tail)) >= len(inside) + len(planted)
    assert st["blocks"] == 3 and st["streams"] == 1


def test_decode_scan(dec):
    tail, planted = foreign_tail()
    got = dec.decode_scan(tail)
    assert got == numpy_scan(tail) and set(planted) <= set(got)
    s = bz2.compress(cases.gen(700_000, "random", 4), 1) + bz2.compress(cases.gen(40_000, "text", 4), 2)
    got = dec.decode_scan(s)
    assert got == numpy_scan(s) and sum(1 for _, k in got if k == 0) >= 8 and sum(1 for _, k in got if k == 1) >= 2
    assert dec.decode_scan(b"") == [] and dec.decode_scan(BLOCK_MAGIC) == [(0, 0)]


def test_capacity(dec):
    d = cases.gen(500_000, "text", 6) + cases.gen(300_000, "longruns", 6)
    s = bz2.compress(d, 3)
    for cap in (len(d) - 1, 0):
        st, out, need, _ = dec.decode_raw(s, cap)
        assert st == -4 and out is None and need == len(d)
    st, out, need, used = dec.decode_raw(s, len(d))
    assert st == 0 and out == d and need == len(d) and used == len(s)
    assert dec.decode(s, size_hint=1) == d  # the Python layer's retry
    assert dec.decode(bz2.compress(b"", 9)) == b""


def test_device_resident(dec):
    import torch
    d = cases.gen(1_500_000, "text", 12) + cases.gen(400_000, "shortruns", 12)
    s = bz2.compress(d, 9) + bz2.compress(d[:1000], 1)
    t_in = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    t_out = torch.empty(len(d) + 1000 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n, used = dec.decode_device(t_in.data_ptr(), len(s), t_out.data_ptr(), t_out.numel())
    assert used == len(s) and n == len(d) + 1000
    assert t_out[:n].cpu().numpy().tobytes() == d + d[:1000] == dec.decode(s)


def test_python_api(native):
    import banzai_amd
    d = cases.gen(400_000, "text", 13)
    s = bz2.compress(d, 9)
    assert banzai_amd.decompress(s) == d and banzai_amd.decompress(bytearray(s)) == d and banzai_amd.decompress(memoryview(s)) == d
    out = io.BytesIO()
    assert banzai_amd.decode(io.BytesIO(s), out) == len(d) and out.getvalue() == d
    with pytest.raises(native.BzhError) as e:
        banzai_amd.decompress(s[:len(s) // 2])
    assert e.value.status == -6


def test_large(dec, ctx9, native):
    from banzai_amd import corpus
    data = corpus.workload(100_000_000)[0].tobytes()
    with native.Context(0, 9, 0) as big:
        s = big.encode(data)
        big.set_profiling(True)
        got = big.decode(s, size_hint=len(data))
        st = big.decode_stats()
    assert got == data
    print("decode of the 100 MB text:", {k: (round(v, 2) if isinstance(v, float) else v) for k, v in st.items()})


def test_cli(native, tmp_path):
    assert os.path.exists(BIN)
    d = cases.gen(300_000, "text", 1) + cases.gen(50_000, "longruns", 1)
    f = tmp_path / "a.txt"
    f.write_bytes(d)
    assert subprocess.run([BIN, str(f)]).returncode == 0 and not f.exists()
    z = tmp_path / "a.txt.bz2"
    stream = z.read_bytes()
    assert subprocess.run([BIN, "-d", str(z)], capture_output=True).returncode == 0
    assert f.read_bytes() == d and not z.exists()  # the default removes the input, as in the encode direction
    z.write_bytes(stream)
    r = subprocess.run([BIN, "-d", "-c", str(z)], capture_output=True)
    assert r.returncode == 0 and r.stdout == d and z.exists()
    r = subprocess.run([BIN, "--decompress", "-c", "-"], input=stream + bz2.compress(b"tail", 1), capture_output=True)
    assert r.returncode == 0 and r.stdout == d + b"tail"
    o = tmp_path / "o.bin"
    assert subprocess.run([BIN, "-d", "--output", str(o), str(z)], capture_output=True).returncode == 0
    assert o.read_bytes() == d and z.exists()
    assert subprocess.run([BIN, "-d", str(o)], capture_output=True).returncode == 1  # no .bz2 suffix, no explicit output
    bad = bytearray(stream)
    bad[len(bad) // 2] ^= 0x10
    zb = tmp_path / "bad.bz2"
    zb.write_bytes(bytes(bad))
    r = subprocess.run([BIN, "-d", str(zb)], capture_output=True)
    assert r.returncode == 3 and zb.exists() and not (tmp_path / "bad").exists()  # ERR_OUTPUT, input left in place


# ---- damaged streams (after everything valid) ------------------------------------------------------------------------
def first_block_fields(s):
    """bit positions inside the first block of stream `s` of: origPtr, the first selector, the first code length"""
    bits = np.unpackbits(np.frombuffer(s, dtype=np.uint8))

    def get(at, n):
        return int("".join(map(str, bits[at:at + n])), 2)
    at = 32 + 48 + 32 + 1
    orig = at
    at += 24
    groups = get(at, 16)
    at += 16 + 16 * bin(groups).count("1")
    at += 3
    nsel = get(at, 15)
    at += 15
    sel0 = at
    for _ in range(nsel):
        while bits[at]:
            at += 1
        at += 1
    return orig, sel0, at  # `at`: the 5-bit start length of the first table


def test_damaged_streams(dec, oracle, native):
    d = cases.gen(120_000, "text", 7)
    s = bytearray(oracle.encode(d, 1))
    good = bytes(s)

    def flipped(bitpos):
        bad = bytearray(s)
        bad[bitpos // 8] ^= 0x80 >> (bitpos % 8)
        return bytes(bad)

    orig, sel0, len0 = first_block_fields(good)
    damaged = [b"BZx9" + bytes(s[4:]), bytes(s[:len(s) // 2])]
    for at, bit in ((12, 0x40), (len(s) - 2, 0x01), (len(s) // 2, 0x10)):
        bad = bytearray(s)
        bad[at] ^= bit
        damaged.append(bytes(bad))
    damaged += [flipped(sel0), flipped(len0), flipped(len0 + 1), flipped(orig + 8)]
    for k, bad in enumerate(damaged):
        with pytest.raises(oracle.DecodeError):
            oracle.decode(bad)
        with pytest.raises(native.BzhError) as e:
            dec.decode(bad)
        assert e.value.status == -6, (k, str(e.value))
        assert dec.decode(good) == d  # the context decodes a valid stream right after
    # one byte behind the stream: trailing data for the strict decoder, foreign bytes under this contract
    with pytest.raises(oracle.DecodeError) as e:
        oracle.decode(good + b"\0")
    assert e.value.status == -8
    got, used = dec.decode(good + b"\0", with_consumed=True)
    assert got == d and used == len(good)
    for junk in (b"", b"BZ", b"BZh", b"BZh9", b"\0" * 64):
        with pytest.raises(native.BzhError) as e:
            dec.decode(junk)
        assert e.value.status == -6
