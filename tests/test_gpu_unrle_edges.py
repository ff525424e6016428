"""Inverse RLE1 on the MI355X (banzai_amd/csrc/decode.hip, ur_load to unrle_select) at every state, thread, wave, tile, staging and
copy-out edge of tests/unrle_cases.py.  Before a case goes to the device, the path model's record of it (tests/unrle_paths_model.py)
shows that it reaches the edges it was built for.  Then, bit for bit: the full decode, the index's CRC and size (unrle_crc), the
same cases as a list through decode_many with either inverse BWT in front, a family as one multi-stream input, short blocks
behind a long one in the same slot, windows between guards (unrle_walk_win), pieces (unrle_walk_pieces) and records (unrle_count,
unrle_select, count_bytes_blocks).  Every comparison is exact, against bz2_handbuilt.unrle (which Python's bz2 confirms on the
CPU: tests/test_unrle_paths_model.py) and pymodel.checksum, never against this library's own output."""
import bz2
import os

import numpy as np
import pytest

from tests import unrle_cases as uc
from tests.golden import pymodel

pytestmark = pytest.mark.gpu

OK, E_DATA = 0, -6
PRE = b"pre"
GUARD = 0xA5


@pytest.fixture(scope="module")
def dec(native):
    """the decoding context: level 9 (every stream's level fits), batches of 8 blocks"""
    c = native.Context(0, 9, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_slot(native):
    """batches of one block: every block is decoded in the same slot, behind whatever the block before left there"""
    c = native.Context(0, 1, 1)
    yield c
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


_FRAMED = {}


def _reaches(name):
    """-> (input, truth of the input, closed, bytes in front of the block, the block's own truth, extras, record) once the model's
    record shows that the case reaches its edges; a case with `pre` has a stream of that many bytes in front of it"""
    if name not in _FRAMED:
        (_, x, level, want, extras), rec = uc.analysed(name)
        assert uc.unmet(rec, want) == [], name
        block, closed = uc.truth(name)
        front = PRE[:extras.get("pre", 0)]
        s = (bz2.compress(front, 1) if front else b"") + uc.stream(name)
        _FRAMED[name] = (s, front + block, closed, len(front), block, extras, rec)
    return _FRAMED[name]


def _still_decodes(ctx):
    s, want = _reaches("seam_s4_c255")[:2]
    assert ctx.decode(s) == want


# ---- the full decode and the index, a case a call -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(uc.FAMILIES))
def test_decode_and_index(dec, native, family):
    for name in uc.FAMILIES[family]:
        s, want, closed, front, block, _, _ = _reaches(name)
        if not closed:
            with pytest.raises(native.BzhError) as e:
                dec.decode(s)
            assert e.value.status == E_DATA and "four equal bytes" in str(e.value), name
            _still_decodes(dec)
            continue
        got, used = dec.decode(s, with_consumed=True)
        assert got == want and used == len(s), name
        ent, total, used = dec.decode_index(s)
        assert total == len(want) and used == len(s) and len(ent) == 1 + (front > 0), name
        assert int(ent[-1]["crc"]) == pymodel.checksum(block) and int(ent[-1]["out_len"]) == len(block) and int(ent[-1]["out_off"]) == front, name


@pytest.mark.parametrize("family", list(uc.FAMILIES))
def test_the_same_cases_as_a_list(dec, lds_off, family):
    """decode_many lays the output out by its own plan; with BZH_UNBWT_SMALL=0 the global-memory inverse BWT feeds the stage"""
    names = uc.FAMILIES[family]
    framed = [_reaches(n) for n in names]
    for off in (False, True) if family != "chain" else (False,):
        lds_off(off)
        res, status, used = dec.decode_many([f[0] for f in framed], with_status=True)
        assert len(res) == len(status) == len(used) == len(names) > 0
        for name, f, r, st, u in zip(names, framed, res, status, used):
            if f[2]:
                assert st == OK and r == f[1] and u == len(f[0]), (name, off)
            else:
                assert st == E_DATA and r is None, (name, off)
    lds_off(False)


@pytest.mark.parametrize("family", list(uc.FAMILIES))
def test_a_family_as_one_input(dec, family):
    """every closed case of the family end to end in one multi-stream input: other slots, other obase, another tile stride"""
    framed = [_reaches(n) for n in uc.FAMILIES[family]]
    framed = [f for f in framed if f[2]]
    s = b"".join(f[0] for f in framed)
    want = b"".join(f[1] for f in framed)
    got, used = dec.decode(s, with_consumed=True)
    assert used == len(s) and len(got) == len(want) and got == want
    ent, total, used = dec.decode_index(s)
    blocks = [b for f in framed for b in ((PRE[:f[3]], f[4]) if f[3] else (f[4],))]
    assert total == len(want) and len(ent) == len(blocks)
    assert ent["crc"].tolist() == [pymodel.checksum(b) for b in blocks]
    assert ent["out_len"].tolist() == [len(b) for b in blocks]


def test_short_blocks_behind_a_long_one_in_its_slot(one_slot, native):
    """the uint4 load of the thread that holds a block's end reads what the block before left behind n: count bytes of 255"""
    long_s, long_want = _reaches("stale_long_ff")[:2]
    for k, name in enumerate(uc.STALE_AFTER):
        s, want, closed, _, block, _, _ = _reaches(name)
        if k % 8 == 0:
            assert one_slot.decode(long_s) == long_want
        if not closed:
            with pytest.raises(native.BzhError) as e:
                one_slot.decode(s)
            assert e.value.status == E_DATA and "four equal bytes" in str(e.value), name
            continue
        assert one_slot.decode(s) == want, name
        ent, total, _ = one_slot.decode_index(s)
        assert total == len(want) and int(ent[0]["crc"]) == pymodel.checksum(block), name


# ---- windows: unrle_walk_win between guards ---------------------------------------------------------------------------------------------
def _windows_between_guards(ctx, s, truth, wins):
    """decode_range_device of every (offset, length, shift): the bytes, and not one byte outside them"""
    import torch
    ent, total, _ = ctx.decode_index(s)
    assert total == len(truth)
    t_in = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    room = 64 + 3 + max(n for _, n, _ in wins) + 64
    t_out = torch.empty((room,), dtype=torch.uint8, device="cuda")
    want_all = np.frombuffer(truth, dtype=np.uint8)
    for off, n, shift in wins:
        t_out.fill_(GUARD)
        torch.cuda.synchronize()
        got = ctx.decode_range_device(t_in.data_ptr(), len(s), ent, off, n, t_out.data_ptr() + 64 + shift, n)
        h = t_out[:64 + shift + n + 64].cpu().numpy()
        assert got == n and np.array_equal(h[64 + shift:64 + shift + n], want_all[off:off + n]), (off, n, shift)
        assert (h[:64 + shift] == GUARD).all() and (h[64 + shift + n:] == GUARD).all(), (off, n, shift)


WINDOW_GROUPS = [("seams_s%d" % s, [n for n in uc.FAMILIES["seams"] if n.startswith("seam_s%d_" % s)]) for s in range(5)] + \
                [("fat_" + c, [n for n in uc.FAMILIES["windows"] if n.endswith(c)]) for c in ("_c0", "_c255")] + [("staging", uc.FAMILIES["staging"])]


@pytest.mark.parametrize("group", [g for g, _ in WINDOW_GROUPS])
def test_windows(dec, group):
    """0, 1, 7 and 300 bytes at -2..+2 around every tile seam, inside the run a tile's first count byte stands for, up to the
    block's end and the whole block; staged tiles and tiles too large to stage; the destination at every residue mod 4"""
    names = dict(WINDOW_GROUPS)[group]
    assert names
    for name in names:
        s, truth, closed, front, _, extras, rec = _reaches(name)
        assert closed and front == 0 and rec["windows"]
        _windows_between_guards(dec, s, truth, [(w["lo"], w["hi"] - w["lo"], w["dst"]) for w in rec["windows"]])


@pytest.mark.parametrize("r", range(4))
def test_copy_out_of_a_window(dec, r):
    """the last tile's 1..8 bytes at toff = r mod 4, alone and with its neighbours, at every destination residue"""
    for name in uc.FAMILIES["copyout"]:
        if not name.startswith("copy_r%d_" % r):
            continue
        _, _, _, _, block, extras, rec = _reaches(name)
        t1, bs, sh = rec["tiles"][1], rec["bsize"], extras["pre"]
        wins = [(t1["toff"], t1["total"], sh), (t1["toff"] - 1, t1["total"] + 1, sh), (t1["toff"] - 5, 5 + t1["total"], sh)]
        if t1["total"] > 1:
            wins += [(t1["toff"] + 1, t1["total"] - 1, sh), (t1["toff"], t1["total"] - 1, sh)]
        assert all(off + n <= bs for off, n, _ in wins)
        _windows_between_guards(dec, uc.stream(name), block, wins)


# ---- pieces: unrle_walk_pieces ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", uc.FAMILIES["pieces"])
def test_pieces(dec, name):
    s, truth, closed, front, _, extras, rec = _reaches(name)
    ent, total, _ = dec.decode_index(s)
    ranges = [(lo, hi - lo) for lo, hi in extras["pieces"]]
    blob, offs, lens = dec.decode_ranges(s, ent, ranges)
    assert blob == b"".join(truth[off:off + n] for off, n in ranges), name
    assert list(lens) == [n for _, n in ranges] and list(offs) == [sum(n for _, n in ranges[:k]) for k in range(len(ranges))]
    st = dec.decode_ranges_stats()
    assert st["ranges"] == len(ranges) and st["pieces"] == len(ranges) and st["blocks_touched"] == 1


# ---- records: unrle_count, unrle_select, count_bytes_blocks -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", uc.FAMILIES["records"])
def test_records(dec, name):
    import torch
    s, truth, closed, front, _, extras, rec = _reaches(name)
    d = extras["delim"]
    pos = [i for i, v in enumerate(truth) if v == d]
    D = len(pos)
    nrecords = D + (not truth.endswith(bytes([d])))
    ent, pts, cum, nrec, total, used = dec.decode_index_records(s, 0, d)
    assert total == len(truth) and used == len(s) and len(ent) == 1 and len(pts) == 0
    assert cum.tolist() == [0, D] and nrec == nrecords, name
    t = torch.frombuffer(bytearray(truth), dtype=torch.uint8).cuda()
    cum2, nrec2 = dec.count_records_device(t.data_ptr(), len(truth), ent, d)
    assert cum2.tolist() == [0, D] and nrec2 == nrecords, name
    # reads by record number: a spread of records, and those around the first and the last delimiter of every tile
    picks = set(range(min(5, nrecords))) | set(range(max(nrecords - 5, 0), nrecords)) | set(range(0, nrecords, max(1, nrecords // 40)))
    for tl in rec["tiles"][1:]:
        j = int(np.searchsorted(pos, tl["toff"]))
        picks |= {k for k in range(j - 2, j + 3) if 0 <= k < nrecords}
    picks = sorted(picks)
    begin = lambda k: pos[k - 1] + 1 if k else 0
    end = lambda k: pos[k] + 1 if k < D else len(truth)
    blob, offs, lens = dec.decode_records(s, ent, cum, [(k, 1) for k in picks], delim=d)
    assert list(lens) == [end(k) - begin(k) for k in picks], name
    assert blob == b"".join(truth[begin(k):end(k)] for k in picks), name
    if nrecords > 3:  # one read of many records: its boundary delimiters alone are looked for
        blob, offs, lens = dec.decode_records(s, ent, cum, [(1, nrecords - 2)], delim=d)
        assert blob == truth[begin(1):end(nrecords - 2)], name
