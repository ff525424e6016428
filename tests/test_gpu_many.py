"""bzh_encode_many* on the MI355X: every stream bit-identical to the oracle's / to bzh_encode of its input alone, across run
edges between inputs, batch edges, empty inputs, both Huffman modes, errors and the plan seam."""
import bz2
import ctypes
import io

import numpy as np
import pytest

from tests.cases import boundary_cases, gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(native):
    made = {(lv, mb): native.Context(0, lv, mb) for lv in (1, 9) for mb in (8, 0)}
    yield made
    for c in made.values():
        c.close()


def _check_layout(ctx, items, streams):
    """offsets aligned and back to back with zero padding; every stream decodes to its input"""
    import torch
    lens = [len(x) for x in items]
    cat = b"".join(items)
    dev = torch.device("cuda", 0)
    d_in = torch.zeros(len(cat) + 16, dtype=torch.uint8, device=dev)
    if cat:
        d_in[:len(cat)] = torch.from_numpy(np.frombuffer(cat, dtype=np.uint8).copy()).to(dev)
    from banzai_amd import _native
    cap = _native.encode_many_bound(ctx.level, lens)
    d_out = torch.full((cap,), 0xAB, dtype=torch.uint8, device=dev)
    offs, olens = ctx.encode_many_device(d_in.data_ptr(), lens, d_out.data_ptr(), cap)
    host = d_out.cpu().numpy().tobytes()
    pos = 0
    for k, (o, n) in enumerate(zip(offs, olens)):
        assert o == pos and o % 4 == 0
        assert host[o:o + n] == streams[k]
        end = (o + n + 3) & ~3
        assert host[o + n:end] == b"\0" * (end - o - n)
        pos = end
        assert bz2.decompress(streams[k]) == items[k]
    return offs, olens


def _mixed(level, seed):
    rng = np.random.default_rng(seed)
    out = []
    sizes = [0, 1, 3, 4, 5, 255, 256, 4096, 65537, 250_000, 1_100_000]
    for k, mode in enumerate(["random", "lowalpha", "shortruns", "longruns", "text", "same", "periodic"]):
        for n in rng.choice(sizes, 3, replace=False):
            out.append(gen(int(n), mode, seed + k))
    out.append(gen(3_000_000, "text", seed))
    out += boundary_cases(100000 * level - 1)[:4]
    out.insert(5, b"")
    out.append(b"")
    return out


@pytest.mark.parametrize("level", [1, 9])
def test_many_matches_oracle(ctxs, oracle, level):
    items = _mixed(level, 11 * level)
    streams = ctxs[(level, 0)].encode_many(items)
    assert len(streams) == len(items)
    for x, s in zip(items, streams):
        assert s == oracle.encode(x, level)
    assert ctxs[(level, 8)].encode_many(items) == streams  # batches of 8 blocks: streams across batch edges
    _check_layout(ctxs[(level, 8)], items, streams)


@pytest.mark.parametrize("level", [1, 9])
def test_run_edges_between_inputs(ctxs, oracle, level):
    items = []
    for n in (3, 4, 5, 254, 255, 256, 257, 258, 259, 260):  # one byte repeated: every neighbour ends and begins with the same run
        items += [b"a" * n] * 6
    items += [b"xyz" + b"b" * 300, b"b" * 300 + b"q", b"b" * 4, b"b"]  # neighbours that end and begin with the same run
    M = 100000 * level - 1
    items += [b"c" * (M + 700), b"c" * 1000, b"c" * (3 * M), b"d" + b"c" * 900]  # last cuts inside a run
    got = ctxs[(level, 8)].encode_many(items)
    for x, s in zip(items, got):
        assert s == oracle.encode(x, level)


@pytest.mark.parametrize("level", [1, 9])
def test_plan_seam_equals_per_input_split(ctxs, level):
    import torch
    ctx = ctxs[(level, 8)]
    items = _mixed(level, 5)[:18] + [b"e" * 777, b"", b"e" * 3]
    lens = [len(x) for x in items]
    cat = b"".join(items)
    d_in = torch.from_numpy(np.frombuffer(cat + b"\0" * 16, dtype=np.uint8).copy()).to("cuda")
    got = ctx.plan_many_device(d_in.data_ptr(), lens)
    want, start = [], 0
    for x in items:
        infos, _ = ctx.rle1_split(x, want_bytes=False)
        want += [(o + start, n, r, c) for (o, n, r, c) in infos]
        start += len(x)
    assert got == want


@pytest.mark.parametrize("level", [1, 9])
def test_batch_edges(ctxs, level):
    M = 100000 * level - 1
    rng = np.random.default_rng(level)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731 -- one block per ~M bytes
    items = [b"", b"", rnd(10), rnd(M * 11), b"", rnd(M * 2 + 5)]  # 12 blocks then 3: spans two batches of 8, then three
    items += [rnd(M * 8 - 3000)] + [rnd(100) for _ in range(20)] + [b"", rnd(M * 5), b"", b""]
    small, big = ctxs[(level, 8)], ctxs[(level, 0)]
    want = [big.encode(x) for x in items]
    assert small.encode_many(items) == want
    assert big.encode_many(items) == want
    assert small.encode_many([b""] * 9) == [big.encode(b"")] * 9  # every input empty: no batch at all
    assert len(big.encode(b"")) == 14
    # a stream that ends exactly on a batch edge: 8 blocks of one input, then another
    eight = [x for x in items if len(x) == M * 8 - 3000]
    assert small.encode_many(eight + [b"tail"]) == [big.encode(eight[0]), big.encode(b"tail")]


def test_volume_and_periodic(ctxs, oracle):
    rng = np.random.default_rng(3)
    items = []
    for k in range(2000):
        n = int(rng.integers(1, 4097))
        kind = k % 4
        if kind == 0:
            items.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        elif kind == 1:
            items.append(gen(n, "text", k))
        elif kind == 2:
            items.append(bytes([k % 251]) * n)
        else:
            items.append(gen(n, "shortruns", k))
    items[100] = (b"abcdefg" * 150_000)[:900_000]  # near-periodic blocks among small ones
    items[1500] = (bytes(range(7, 250, 3)) * 20_000)[:1_000_001]
    got = ctxs[(9, 0)].encode_many(items)
    for k, (x, s) in enumerate(zip(items, got)):
        assert s == (ctxs[(9, 0)].encode(x) if k in (100, 1500) else oracle.encode(x, 9))


@pytest.mark.parametrize("level", [1, 9])
def test_fixed_mode(native, level):
    items = _mixed(level, 23)[:14] + [b"", b"z" * 300]
    with native.Context(0, level, 8) as many, native.Context(0, level, 0) as one:
        many.set_mode(True)
        one.set_mode(True)
        assert many.encode_many(items) == [one.encode(x) for x in items]


def test_errors_and_recovery(ctxs):
    import torch
    from banzai_amd import _native
    ctx = ctxs[(9, 8)]
    items = [gen(200_000, "text", 1), b"", gen(50_000, "random", 2), b"q" * 999]
    want = [ctxs[(9, 0)].encode(x) for x in items]
    lens = [len(x) for x in items]
    cat = b"".join(items)
    d_in = torch.from_numpy(np.frombuffer(cat + b"\0" * 32, dtype=np.uint8).copy()).to("cuda")
    cap = _native.encode_many_bound(9, lens)
    d_out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    offs, olens = ctx.encode_many_device(d_in.data_ptr(), lens, d_out.data_ptr(), cap)
    needed = (offs[-1] + olens[-1] + 3) & ~3
    with pytest.raises(_native.BzhError) as e:
        ctx.encode_many_device(d_in.data_ptr(), lens, d_out.data_ptr(), needed - 1)
    assert e.value.status == -4
    assert ctx.encode_many(items) == want  # the context is bit-exact afterwards
    offs2, olens2 = ctx.encode_many_device(d_in.data_ptr(), lens, d_out.data_ptr(), needed)
    assert (offs2, olens2) == (offs, olens)
    for bad_in, bad_out in ((d_in.data_ptr() + 1, d_out.data_ptr()), (d_in.data_ptr(), d_out.data_ptr() + 2)):
        with pytest.raises(_native.BzhError) as e:
            ctx.encode_many_device(bad_in, lens, bad_out, cap)
        assert e.value.status == -1 and "aligned" in str(e.value)
    L = _native.lib()
    lz = np.array(lens, dtype=np.uint64)
    st = L.bzh_encode_many_device(ctx.handle, None, _native.ptr(lz, _native.szp), len(lens), ctypes.c_void_p(d_out.data_ptr()),
                                  cap, None, None)
    assert st == -1 and b"null" in L.bzh_last_error(ctx.handle)
    big = np.array([0x80000000, 0x80000000, 10], dtype=np.uint64)  # past the plan's positions: refused before anything runs
    st = L.bzh_encode_many_device(ctx.handle, ctypes.c_void_p(d_in.data_ptr()), _native.ptr(big, _native.szp), 3,
                                  ctypes.c_void_p(d_out.data_ptr()), cap, _native.ptr(lz, _native.szp), _native.ptr(lz, _native.szp))
    assert st == -1 and b"position range" in L.bzh_last_error(ctx.handle)
    # host path: cap one byte short of the streams
    arrs = [np.frombuffer(x, dtype=np.uint8) for x in items]
    ins = (_native.u8p * len(arrs))(*[_native.ptr(a) for a in arrs])
    out = np.zeros(cap, dtype=np.uint8)
    o = np.zeros(len(items), dtype=np.uint64)
    n = np.zeros(len(items), dtype=np.uint64)
    st = L.bzh_encode_many(ctx.handle, ins, _native.ptr(lz, _native.szp), len(items), _native.ptr(out), offs[-1] + olens[-1] - 1,
                           _native.ptr(o, _native.szp), _native.ptr(n, _native.szp))
    assert st == -4
    assert ctx.encode_many(items) == want
    assert ctx.encode_many([]) == []


def test_stats(ctxs):
    ctx = ctxs[(1, 8)]
    items = [gen(n, "text", n) for n in (0, 10, 150_000, 400_000, 3)]
    ctx.set_profiling(True)
    try:
        ctx.encode_many(items)
        s = ctx.stats()
    finally:
        ctx.set_profiling(False)
    nblocks = sum(len(ctx.rle1_split(x, want_bytes=False)[0]) for x in items)
    assert s["blocks"] == nblocks
    assert s["raw_bytes"] == sum(len(x) for x in items)
    assert s["out_bits"] > 0 and s["ms_total"] > 0


def test_python_wrapper_groups(monkeypatch):
    import banzai_amd
    items = [gen(n, "text", n) for n in (5, 0, 30_000, 7, 120_000, 0, 64)]
    monkeypatch.setattr(banzai_amd, "MANY_GROUP_LIMIT", 40_000)
    want = []
    for x in items:
        out = io.BytesIO()
        banzai_amd.encode(io.BytesIO(x), out, 9)
        want.append(out.getvalue())
    assert banzai_amd.encode_many(items, 9) == want
    assert banzai_amd.encode_many([bytearray(items[2]), memoryview(items[4])], 9) == [want[2], want[4]]
