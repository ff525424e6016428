"""GPU (-m gpu): the opt-in "fixed" Huffman mode (bzh_set_mode(ctx, BZH_MODE_FIXED)) bit for bit against its CPU model
(tests/fixed_model.py), at the shapes where fx_init / fx_segments / fx_build / fx_header / fx_pack_headers and the FX
forms of pack_tilebits / pack_symbols can go wrong.  tests/test_fixed_model.py checks that the inputs reach them."""
import functools
import random

import numpy as np
import pytest

from tests import cases
from tests import fixed_model as fm

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _want(data, level):
    return fm.encode(data, level)


@pytest.fixture(scope="module")
def fx9(native):
    with native.Context(0, 9, 8) as ctx:
        ctx.set_mode(True)
        yield ctx


def _edge(family, target):
    d = fm.with_m({"random": fm.random_bytes, "two": fm.two_letters}[family], target)
    assert fm.block_m(d) == target
    return d


# table count at 200 / 600 / 1200 / 2400 symbols; the last segment full (m % 50 == 0), single (1) and one short (49);
# the whole 258-symbol alphabet (random) and 4 symbols for 6 tables (two letters, no run of four)
EDGES = [("random", t) for t in (199, 200, 599, 600, 1199, 1200, 2399, 2400, 2401, 4999, 5000, 5001)] + \
    [("two", t) for t in (2449, 2450, 2451)]


@pytest.mark.parametrize("family,target", EDGES)
def test_fixed_edges(fx9, family, target):
    d = _edge(family, target)
    assert fx9.encode(d) == _want(d, 9)


@pytest.mark.parametrize("what", ["lowalpha", "shortruns", "periodic", "text", "geometric", "largest_selectors"])
def test_fixed_ties_idle_tables_deep_tables(fx9, what):
    """cost ties and tables that end an iteration with no segment (fx_build on an all-zero list), 17-bit tables, and
    a full level-9 block of incompressible bytes (18,000 selectors)"""
    d = {"lowalpha": lambda: cases.gen(50_000, "lowalpha", 1), "shortruns": lambda: cases.gen(200_000, "shortruns", 2),
         "periodic": lambda: cases.gen(30_000, "periodic", 4), "text": lambda: cases.gen(60_000, "text", 1),
         "geometric": fm.geometric, "largest_selectors": lambda: fm.random_bytes(1_000_000, 1)}[what]()
    assert fx9.encode(d) == _want(d, 9)


def _mixed(n, seed):
    """fuzz mixtures between stretches of incompressible bytes: blocks of every kind, about one per 100 kB at level 1"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += cases.mixture(rng, 300_000) + fm.random_bytes(rng.randrange(1, 200_000), rng.randrange(1 << 30))
    return bytes(out[:n])


@pytest.mark.parametrize("level", [1, 5, 9])
def test_fixed_several_blocks_and_batches(native, level):
    d = _mixed(3_000_000 if level < 9 else 4_000_000, level)
    want = _want(d, level)
    for max_batch in (2, 8, 576):
        with native.Context(0, level, max_batch) as ctx:
            ctx.set_mode(True)
            assert ctx.encode(d) == want, max_batch


def test_fixed_150_blocks_and_two_lanes(native):
    d = _mixed(23_500_000, 11)  # ~150 level-1 blocks
    want = _want(d, 1)
    with native.Context(0, 1, 576) as ctx:
        ctx.set_mode(True)
        assert ctx.encode(d) == want
    with native.Context(0, 1, 8) as ctx:
        ctx.set_mode(True)
        ctx.set_lanes(2)
        assert ctx.encode(d) == want


def test_fixed_device_entry_points(native):
    """encode_device, and plan -> encode_range_device (3 ranges) -> assemble_device"""
    import torch
    from banzai_amd import sharded
    d = _mixed(4_500_000, 7)
    n = len(d)
    want = _want(d, 9)
    dev = torch.device("cuda", 0)
    d_in = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    d_in[:n] = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(dev)
    cap = (n + (1 << 20)) & ~3
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    with native.Context(0, 9, 2) as ctx:
        ctx.set_mode(True)
        ln = ctx.encode_device(d_in.data_ptr(), n, d_out.data_ptr(), cap)
        assert d_out[:ln].cpu().numpy().tobytes() == want
        blocks = ctx.plan_device(d_in.data_ptr(), n)
        segs, keep = [], []
        for r in range(3):
            b0, b1 = sharded.block_range(len(blocks), r, 3)
            buf = torch.zeros(cap, dtype=torch.uint8, device=dev)
            segs.append((buf.data_ptr(), ctx.encode_range_device(b0, b1, buf.data_ptr(), cap)))
            keep.append(buf)
        d_out.zero_()
        ln2 = ctx.assemble_device(segs, [b[3] for b in blocks], d_out.data_ptr(), cap)
        assert d_out[:ln2].cpu().numpy().tobytes() == want


def test_fixed_streaming(native):
    d = _mixed(1_300_001, 5)
    want = _want(d, 1)
    rng = random.Random(9)
    with native.Context(0, 1, 8) as ctx:
        ctx.set_mode(True)
        for chunk_bytes in (150_000, 1 << 20):
            ctx.stream_begin(chunk_bytes)
            out, pos = [], 0
            while pos < len(d):
                c = rng.choice([1, 7, 4097, 99_999, 123_457, 333_333])
                out.append(ctx.stream_feed(d[pos:pos + c]))
                pos += c
            out.append(ctx.stream_feed(b"", eof=True))
            assert ctx.stream_consumed() == len(d) and b"".join(out) == want, chunk_bytes


def test_fixed_mode_switching(native, oracle):
    """one context, the mode flipped between inputs of 1, 2 and 5 blocks: each stream is the model's or the oracle's"""
    inputs = [_mixed(250_000, 1), _mixed(2_500_000, 2), _mixed(6_100_000, 3)]
    with native.Context(0, 9, 4) as ctx:
        for d in inputs + inputs[::-1]:
            ctx.set_mode(True)
            assert ctx.encode(d) == _want(d, 9)
            ctx.set_mode(False)
            assert ctx.encode(d) == oracle.encode(d, 9)
