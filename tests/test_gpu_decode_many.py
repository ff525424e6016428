"""bzh_decode_many* on the MI355X: the output of bzh_encode_many_device read back in place, every input judged as bzh_decode judges
it alone (status, bytes, consumed), damaged inputs that fail alone, the LDS inverse BWT at its edges through hand-built columns,
batch edges, capacity and degenerate calls.  The walk itself is held on the CPU (tests/test_many_host.py), the kernel's rule too
(tests/test_unbwt_small_model.py); here they meet the device."""
import bz2
import os

import numpy as np
import pytest

from tests import bz2_handbuilt as hb
from tests import decode_shapes
from tests.cases import MODES, gen

pytestmark = pytest.mark.gpu

OK, E_ARG, E_CAP, E_DATA = 0, -1, -4, -6
ROOM = 8 << 20


@pytest.fixture(scope="module")
def ctxs(native):
    made = {(lv, mb): native.Context(0, lv, mb) for lv, mb in ((1, 0), (9, 0), (1, 8))}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture
def lds_off():
    """BZH_UNBWT_SMALL=0 for the calls made while it is set (the library reads it at every call)"""
    def switch(off):
        if off:
            os.environ["BZH_UNBWT_SMALL"] = "0"
        else:
            os.environ.pop("BZH_UNBWT_SMALL", None)
    yield switch
    os.environ.pop("BZH_UNBWT_SMALL", None)


def to_device(buf):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(buf) + b"\0" * 16, dtype=np.uint8).copy()).to("cuda")


def many(ctx, items, cap=ROOM):
    """bzh_decode_many (inputs back to back, no gaps) -> ([bytes or None], statuses, consumed, out_offs, out_lens)"""
    st, out, offs, lens, status, used = ctx.decode_many_raw(items, cap)
    assert st == OK, ctx.last_error()
    return [out[o:o + n].tobytes() if s == OK else None for o, n, s in zip(offs, lens, status)], status, used, offs, lens


def alone(ctx, item):
    """bzh_decode of one input with ample room -> (status, bytes or None, consumed)"""
    st, out, _, used = ctx.decode_raw(item, ROOM)
    return st, out, used


def check_parity(ctx, items):
    got, status, used, offs, lens = many(ctx, items)
    text = ctx.last_error()  # (before the calls below word their own)
    if any(status):
        assert text.startswith(f"decode: input {[bool(s) for s in status].index(True)}: "), text
    at = 0
    for k, item in enumerate(items):
        st, want, cons = alone(ctx, item)
        assert status[k] == st, (k, status[k], st)
        assert got[k] == want, k
        assert used[k] == cons, (k, used[k], cons)
        assert offs[k] == at and (st == OK or lens[k] == 0), k  # packed: nothing here fails behind a placed block
        at += lens[k]
    return status


def still_agrees_with_libbz2(ctx):
    data = gen(30_000, "text", 3) + gen(5_000, "random", 4)
    s = ctx.encode(data)
    assert bz2.decompress(s) == data and ctx.decode(s) == data
    assert ctx.decode(bz2.compress(data, 1)) == data


# ---- 1. round trip in place ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 9])
def test_round_trip_in_place(ctxs, native, lds_off, level):
    import torch
    ctx = ctxs[(level, 0)]
    rng = np.random.default_rng(level)
    sizes = [0, 1, 2, 5, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 4097, 6553, 6554, 8192, 10_000, 20_000, 70_000]
    items = [gen(int(rng.choice(sizes)), MODES[k % len(MODES)], k) for k in range(56)] + [b"", gen(70_000, "text", 1), b"", gen(6553, "random", 2)]
    in_lens = [len(x) for x in items]
    cat = b"".join(items)
    d_in = to_device(cat)
    cap = native.encode_many_bound(level, in_lens)
    d_comp = torch.full((cap + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    offs, lens = ctx.encode_many_device(d_in.data_ptr(), in_lens, d_comp.data_ptr(), cap)
    n = offs[-1] + lens[-1]
    assert any(o % 4 == 0 and o > p + q for o, p, q in zip(offs[1:], offs, lens)), "the layout has padding between streams"
    d_out = torch.full((len(cat) + 16,), 0xCD, dtype=torch.uint8, device="cuda")
    results = []
    for off in (False, True):
        lds_off(off)
        d_out.fill_(0xCD)
        st, ooffs, olens, status, used = ctx.decode_many_device(d_comp.data_ptr(), n, offs, lens, d_out.data_ptr(), len(cat))
        assert st == OK and status == [OK] * len(items), ctx.last_error()
        assert olens == in_lens and used == lens
        assert ooffs == np.concatenate([[0], np.cumsum(in_lens)[:-1]]).tolist()
        host = d_out.cpu().numpy().tobytes()
        assert host[:len(cat)] == cat and host[len(cat):] == b"\xcd" * 16
        ms, ds = ctx.decode_many_stats(), ctx.decode_stats()
        assert ms["inputs"] == len(items) and ms["inputs_failed"] == 0 and ms["streams"] == len(items) == ds["streams"]
        assert ms["blocks"] == ds["blocks"] >= sum(1 for x in items if x) and ds["out_bytes"] == len(cat)
        assert 1 <= ms["batches"] < len(items) // 4  # batches take the candidates of many inputs together
        results.append(ms["blocks_small"])
    assert results[0] > 0 and results[1] == 0


# ---- 2. parity with bzh_decode ------------------------------------------------------------------------------------------------
def parity_inputs():
    small = [gen(3000 + 517 * lv, MODES[lv % len(MODES)], lv) for lv in range(1, 10)]
    items = [bz2.compress(d, lv) for lv, d in zip(range(1, 10), small)]
    items.append(bz2.compress(gen(150_000, "text", 7) + gen(20_000, "random", 8), 1))      # two blocks
    items.append(items[0] + items[4])                                                     # two streams
    items.append(items[2] + bz2.compress(b"", 9) + items[8])                               # three, the middle one empty
    items.append(bz2.compress(b"", 5))                                                    # the 14-byte empty stream
    items.append(items[1] + b"\0\0\0trailing bytes that are no stream")
    items.append(items[3] + b"BZ")
    items += [b.stream for b in decode_shapes.accepted().values()]
    items += list(decode_shapes.refused().values())
    items.append(decode_shapes.oversubscribed_unused_table().stream)
    return items


@pytest.mark.parametrize("level", [9, 1])
def test_parity_with_decode(ctxs, level):
    """on the level-9 context every stream fits; on the level-1 context the streams above it are BZH_E_ARG for both"""
    ctx = ctxs[(level, 0)]
    status = check_parity(ctx, parity_inputs())
    assert status.count(OK) >= (30 if level == 9 else 10) and status.count(E_DATA) >= 10
    assert (status.count(E_ARG) > 0) == (level == 1)
    still_agrees_with_libbz2(ctx)


# ---- 3. isolation -------------------------------------------------------------------------------------------------------------
def test_isolation(ctxs):
    ctx = ctxs[(1, 0)]
    datas = [gen(2500 + 37 * k, MODES[k % len(MODES)], 100 + k) for k in range(64)]
    items = [bz2.compress(d, 1) for d in datas]
    damaged = {}
    for k in range(1, 64, 3):
        s, how = bytearray(items[k]), (k // 3) % 7
        if how == 0:
            s = s[:len(s) // 2]                      # cut mid-block; input k + 1 follows without a gap
        elif how == 1:
            s = s[:-6]                               # cut inside the footer
        elif how == 2:
            s[len(s) // 2] ^= 0x04                   # one payload bit
        elif how == 3:
            s[-3] ^= 0x10                            # the stream CRC
        elif how == 4:
            s[2] = ord("x")                          # bad magic
        elif how == 5:
            s = bytearray()                          # an empty slice
        else:
            s = bytearray(bz2.compress(datas[k], 9))  # a level-9 stream on a level-1 context
        items[k] = bytes(s)
        damaged[k] = how
    assert set(damaged.values()) == set(range(7))
    got, status, used, offs, lens = many(ctx, items)
    assert ctx.last_error().startswith(f"decode: input {min(damaged)}: ")
    ms = ctx.decode_many_stats()
    assert ms["inputs"] == 64 and ms["inputs_failed"] == len(damaged)
    for k, item in enumerate(items):
        st, want, cons = alone(ctx, item)
        assert status[k] == st, (k, damaged.get(k), status[k], st)
        if k not in damaged:
            assert st == OK and got[k] == datas[k] and used[k] == len(item), k
        else:
            assert st == (E_ARG if damaged[k] == 6 else E_DATA) and got[k] is None and lens[k] == 0, (k, damaged[k])
    for k, how in damaged.items():  # a cut input fails alone: the valid input directly behind it is whole
        if how in (0, 1):
            assert status[k + 1] == OK and got[k + 1] == datas[k + 1]
    still_agrees_with_libbz2(ctx)


# ---- 4. the kernel's edges through hand-built columns ----------------------------------------------------------------------------
def built(col, ptr, level=9):
    k = len(set(col)) + 2
    tables = [[1, 2, 2]] * 2 if k == 3 else [[9] * k, [10] * k]
    assert hb.unrle(hb.inverse_column(col, ptr))[1], "the block must not end in four equal bytes without a count"
    return hb.stream_of_column(col, ptr, level, tables, lambda g: g & 1 if k > 3 else 0)


def random_column(rng, n, alpha):
    """n random bytes over `alpha` values whose block, from any of the origin pointers used, libbz2 accepts"""
    while True:
        col = rng.integers(0, alpha, n, dtype=np.uint8).tobytes()
        if all(hb.unrle(hb.inverse_column(col, ptr))[1] for ptr in {0, n - 1, n // 3}):
            return col


def test_kernel_edges(ctxs, native, lds_off):
    ctx = ctxs[(9, 0)]
    bound = native.decode_many_small_max()
    rng = np.random.default_rng(4)
    blocks = []
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, bound - 1, bound, bound + 1):
        alpha = int(rng.choice([2, 7, 256]))
        col = random_column(rng, n, alpha)
        for ptr in sorted({0, n - 1, n // 3}):
            blocks.append(built(col, ptr))
    blocks.append(built(b"\x07" * 5000, 4999))                               # one symbol
    blocks.append(built(b"\x07" * bound, 0))
    abba = b"ab" * 500 + b"ba" * 500                                        # the walk closes a cycle that does not divide n
    blocks += [built(abba, 1), built(abba, 1999), built(b"ba" * 2048 + b"a", 7)]
    big = built(random_column(rng, 250_000, 3), 250_000 // 3)  # a mixed batch: one large block among small ones
    blocks.insert(len(blocks) // 2, big)
    small = sum(b.nblock <= bound for b in blocks)
    assert small == len(blocks) - 4  # bound + 1 three times, and the large block
    for off in (False, True):
        lds_off(off)
        got, status, used, _, _ = many(ctx, [b.stream for b in blocks])
        assert status == [OK] * len(blocks), ctx.last_error()
        for b, g in zip(blocks, got):
            assert g == b.expected, (b.nblock, off)
        ms = ctx.decode_many_stats()
        assert ms["blocks"] == len(blocks) and ms["blocks_small"] == (0 if off else small)


# ---- 5. batch edges -----------------------------------------------------------------------------------------------------------
def test_batch_edges(ctxs):
    ctx = ctxs[(1, 8)]
    datas = [gen(1500 + 211 * k, MODES[k % len(MODES)], 300 + k) for k in range(50)]
    items = [bz2.compress(d, 1) for d in datas]
    three = gen(250_000, "random", 9)  # three level-1 blocks; behind 5 one-block inputs its blocks are candidates 11..13 of batches of 8
    items.insert(5, bz2.compress(three, 1))
    datas.insert(5, three)
    check_parity(ctx, items)
    # a failure found in the second block after the first was placed: three one-block inputs and an empty stream are seven
    # candidates, so the first block of the two-block input ends the first batch and its second block opens the next
    two = bytearray(bz2.compress(gen(150_000, "random", 10), 1))
    two[len(two) - 2000] ^= 0x01
    items2 = items[:3] + [bz2.compress(b"", 1), bytes(two)] + items[3:20]
    datas2 = datas[:3] + [b"", None] + datas[3:20]
    got, status, used, offs, lens = many(ctx, items2)
    assert status[4] == E_DATA and lens[4] == 0 and alone(ctx, bytes(two))[0] == E_DATA
    gap = offs[5] - offs[4]
    assert 0 < gap <= 150_000
    for k, d in enumerate(datas2):
        if k != 4:
            assert status[k] == OK and got[k] == d and lens[k] == len(d), k
        if 0 < k and k != 5:
            assert offs[k] == offs[k - 1] + lens[k - 1], k  # packed, but for the gap behind the failed input
    still_agrees_with_libbz2(ctx)


# ---- 6. capacity --------------------------------------------------------------------------------------------------------------
def test_capacity(ctxs):
    import torch
    ctx = ctxs[(9, 0)]
    datas = [gen(4000 + 100 * k, "text", k) for k in range(20)] + [b""]
    items = [bz2.compress(d, 9) for d in datas]
    offs, at = [], 0
    for s in items:  # gaps of 0..3 bytes
        offs.append(at)
        at += len(s) + len(offs) % 4
    buf = bytearray(at)
    for o, s in zip(offs, items):
        buf[o:o + len(s)] = s
    d_in = to_device(buf)
    lens = [len(s) for s in items]
    want_offs = np.concatenate([[0], np.cumsum([len(d) for d in datas])[:-1]]).tolist()
    total = sum(len(d) for d in datas)
    st, ooffs, olens, status, used = ctx.decode_many_device(d_in.data_ptr(), at, offs, lens, None, 0)  # sizing
    assert st == E_CAP and status == [OK] * len(items) and ooffs == want_offs and olens == [len(d) for d in datas]
    assert ooffs[-1] + olens[-1] == total
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    st, ooffs, olens, status, used = ctx.decode_many_device(d_in.data_ptr(), at, offs, lens, d_out.data_ptr(), total - 1)
    assert st == E_CAP and status == [OK] * len(items) and ooffs == want_offs and ooffs[-1] + olens[-1] == total
    st, ooffs, olens, status, used = ctx.decode_many_device(d_in.data_ptr(), at, offs, lens, d_out.data_ptr(), total)
    assert st == OK and status == [OK] * len(items) and used == lens
    assert d_out.cpu().numpy().tobytes() == b"".join(datas)


# ---- 7. degenerate calls ------------------------------------------------------------------------------------------------------
def test_degenerate_calls(ctxs, native):
    import torch
    ctx = ctxs[(9, 0)]
    assert ctx.decode_many([]) == []
    s = bz2.compress(gen(3000, "text", 1), 9)
    buf = s + s
    d_in = to_device(buf)
    d_out = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    st, *_ = ctx.decode_many_device(d_in.data_ptr(), len(buf), [], [], d_out.data_ptr(), 8192)
    assert st == OK and ctx.decode_many_stats()["inputs"] == 0
    n = len(s)
    for offs, lens in (([0, n - 1], [n, n]),        # overlapping
                       ([n, 0], [n, n]),            # descending
                       ([0, n], [n, n + 1]),        # past the end
                       ([0, 2 * n + 1], [n, 0])):   # an empty slice that starts past the end
        with pytest.raises(native.BzhError) as e:
            ctx.decode_many_device(d_in.data_ptr(), len(buf), offs, lens, d_out.data_ptr(), 8192)
        assert e.value.status == E_ARG and "decode many: input 1" in str(e.value)
        still_agrees_with_libbz2(ctx)
    st, ooffs, olens, status, used = ctx.decode_many_device(d_in.data_ptr(), len(buf), [0, n], [n, n], d_out.data_ptr(), 8192)
    assert st == OK and status == [OK, OK] and olens == [3000, 3000] and ooffs == [0, 3000]


def test_public_decompress_many(native):
    import banzai_amd
    datas = [gen(5000, "text", 1), b"", gen(300_000, "lowalpha", 2)]
    items = [bz2.compress(d, 9) for d in datas]
    assert banzai_amd.decompress_many(items) == datas
    assert banzai_amd.decompress_many(banzai_amd.encode_many(datas, 9)) == datas
    bad = items[:1] + [items[2][:1000]] + items[1:]
    with pytest.raises(native.BzhError) as e:
        banzai_amd.decompress_many(bad)
    assert e.value.status == E_DATA and "input 1" in str(e.value)
    got = banzai_amd.decompress_many(bad, errors="return")
    assert got[0] == datas[0] and got[2:] == datas[1:] and isinstance(got[1], native.BzhError) and got[1].status == E_DATA
