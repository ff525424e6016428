"""CPU: sync points on the one-lane build of decode_core.h with AddressSanitizer and UBSan (tests/decode_host/sync_host.cpp).
The GPU kernels compile the same header, so the recorder's place in the symbol loop, the segment decode with its end check and
the rule for ill-formed points are checked here, where damage can be thrown freely: for every block the model decodes every
segment on its own into a buffer of exactly its bytes, joins them against the serial last column, and damages points by the
hundred -- each must end in a status or in other bytes, never in a sanitizer report."""
import bz2
import json
import os

import numpy as np
import pytest

from tests import bz2_handbuilt, cases, sync_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def sync_host(tmp_path_factory):
    return sync_model.build(tmp_path_factory.mktemp("sync_host"))


def bits_at(s, bit, n):
    chunk = s[bit // 8:bit // 8 + 10]
    v = int.from_bytes(chunk + bytes(10 - len(chunk)), "big")
    return (v >> (80 - bit % 8 - n)) & ((1 << n) - 1)


def tables_of_first_block(s):
    """the number of Huffman tables of the first block of stream `s` (its magic is at bit 32)"""
    at = 32 + 48 + 32 + 1 + 24
    used = bits_at(s, at, 16)
    at += 16
    for g in range(16):
        if used >> (15 - g) & 1:
            at += 16
    return bits_at(s, at, 3)


def text(n, seed):
    import random
    rng = random.Random(seed)
    vocab = ["".join(rng.choices("etaoinshrdlucmfwypvbgkqjxz", k=rng.randrange(2, 11))) for _ in range(400)]
    return " ".join(rng.choices(vocab, k=n // 4 + 1)).encode()[:n]


def libbz2_streams():
    """bz2.compress output with 2 to 6 tables (libbz2 chooses by the number of symbols: 200 / 600 / 1200 / 2400), levels 1 and 9"""
    out = []
    for n in (120, 450, 1000, 2000, 260_000):
        for level in (1, 9):
            out.append(bz2.compress(text(n, n), level))
    return out


def test_segments_join_and_damage_is_caught(sync_host, tmp_path):
    streams = libbz2_streams()
    assert {tables_of_first_block(s) for s in streams} == {2, 3, 4, 5, 6}
    streams += [bytes.fromhex(c["stream_hex"]) for c in json.load(open(os.path.join(GOLDEN, "streams.json")))["streams"]]
    streams.append(bz2.compress(text(150_000, 3), 1) + bz2.compress(b"", 9) + bz2.compress(cases.gen(120_000, "shortruns", 2), 9)
                   + bz2.compress(cases.gen(90_000, "longruns", 5), 5))  # a concatenation
    full = bz2_handbuilt.stream_of_rle((b"aaaa\xff" + b"bbbb\xfe") * 10000, 1)  # nblock = 100,000
    streams.append(full)
    for interval in (7, 256):
        res, totals = sync_model.run(sync_host, tmp_path, streams, interval)
        print(f"interval {interval}: {sum(len(r[1]) for r in res)} points, {totals}")
        assert totals["damaged"] > 1000 and totals["ill_formed"] and totals["caught"]
        for (blocks, pts, _, ents), s in zip(res, streams):
            assert np.all(pts["group"] % interval == 0) and np.all(pts["group"] > 0) and np.all(pts["reserved"] == 0)
            order = list(zip(pts["entry"].tolist(), pts["group"].tolist()))
            assert order == sorted(set(order))
            assert blocks == len(ents)
            assert blocks == 0 or int(pts["entry"].max(initial=0)) < blocks
        blocks, pts, _, _ = res[-1]  # the full block: 100,000 bytes in the last column, but in runs -- fewer than 7 groups of symbols,
        assert blocks == 1 and len(pts) == 0  # so it is one segment, whose room is the whole level-1 block


def test_run_heavy_at_interval_one(sync_host, tmp_path):
    """interval 1: a point in front of every group.  Runs straddle group boundaries, so some point holds a pending run
    (run_weight > 1).  The issue also asks for a point whose out_pos equals its predecessor's -- a segment made of run digits
    only.  No valid block has one: a group is 50 symbols, and a run has at most 22 digits (the decoder refuses a run_weight
    above 2^21; 2^20 already exceeds the largest block), so every whole group holds a symbol that writes a byte.  That
    assertion is therefore left out, and the opposite is asserted: out_pos strictly ascends inside a block."""
    s = bz2.compress(sync_model.run_heavy(), 1)
    res, totals = sync_model.run(sync_host, tmp_path, [s], 1)
    blocks, pts, flips, _ = res[0]
    assert blocks == 1 and len(pts) > 20
    assert np.all(pts["group"] == np.arange(1, len(pts) + 1))
    pending = pts[pts["run_weight"] > 1]
    assert len(pending), "no run straddles a group boundary"
    assert np.all(pending["run"] + 1 >= pending["run_weight"]) and np.all(pending["run"] + 1 <= 2 * pending["run_weight"] - 1)
    assert np.all(pts["run"][pts["run_weight"] == 1] == 0)
    assert np.all(np.diff(pts["out_pos"].astype(np.int64)) > 0)
    assert totals["caught"] and flips
