"""MTF + RLE2 on the MI355X (banzai_amd/csrc/mtf.hip) at every list, chunk and tile edge of tests/mtf_cases.py, at both
tile sizes: symbols, m, all 258 frequencies and num_syms bit for bit the oracle's.  A case built for tiles of 2,048 bytes
goes through the stage seam on its own (bzh_mtf: one block); a case built for tiles of 4,096 goes through bzh_mtf_batch in
lists of 64 columns on a level-1 context, at slot 0, at the last slot and in the middle, and every block of every call is
compared.  Before a case goes to the device, the path model's record (tests/mtf_paths_model.py) shows that it reaches
the edge it was built for.  No tolerance anywhere."""
import numpy as np
import pytest

from tests import mtf_cases as mc

pytestmark = pytest.mark.gpu

_TRUTH = {}


def _truth(oracle, col, hb):
    key = (col, bytes(np.asarray(hb, dtype=np.uint8)))
    if key not in _TRUTH:
        _TRUTH[key] = oracle.mtf_and_rle(col, hb)
    return _TRUTH[key]


def _same(got, want, what):
    gs, gf, gn = got
    ws, wf, wn = want
    assert gn == wn, what
    assert len(gs) == len(ws), (what, len(gs), len(ws))
    assert np.array_equal(gs, ws), (what, int(np.nonzero(gs != ws)[0][0]))
    assert np.array_equal(gf, wf), what


def _reaches(name):
    (_, col, hb, TL, want), _, rec = mc.analysed(name)
    assert mc.unmet(rec, want) == [], name
    return col, hb


def _batch_equals_oracle(ctx, oracle, cols, what):
    res = ctx.mtf_batch(cols)
    assert len(res) == len(cols)
    for k, ((col, hb), got) in enumerate(zip(cols, res)):
        _same(got, _truth(oracle, col, hb), (what, k, len(col)))
    return res


@pytest.fixture(scope="module")
def ctx64(native):
    """one level-1 context for every list of this file: its tile tables keep the rows of the longer blocks before"""
    with native.Context(0, 1, 64) as c:
        yield c


def test_long_blocks_first_then_short_ones(ctx64, oracle):
    """64 blocks of the largest length, then short ones on the same context: mtf_tlast and mtf_tiles hold stale rows
    beyond the short blocks' tiles, and the bytes behind a short column are the long one's"""
    rng = np.random.default_rng(1)
    long_cols = [(mc.runny(rng, mc.LEVEL1_M, np.arange(1 + 4 * k), (1, 2, 30)[k % 3]).tobytes(), mc.hb_of(range(1 + 4 * k)))
                 for k in range(64)]
    _batch_equals_oracle(ctx64, oracle, long_cols, "long")
    short = [n for n in mc.names_at(4096) if "clen" in n or "tile_of_one" in n or "layout_" in n][:64]
    assert len(short) == 64
    _batch_equals_oracle(ctx64, oracle, [_reaches(n) for n in short], "short after long")


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_cases_of_2048_through_the_stage_seam(ctx9, oracle, family):
    names = [n for n in mc.FAMILIES[family] if mc.case(n)[3] == 2048]
    for name in names:
        col, hb = _reaches(name)
        _same(ctx9.mtf(col, hb), _truth(oracle, col, hb), name)


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_cases_of_4096_in_lists_of_64(ctx64, oracle, family):
    names = [n for n in mc.FAMILIES[family] if mc.case(n)[3] == 4096]
    assert names
    cols = [_reaches(n) for n in names]
    fill = [_reaches(n) for n in mc.names_at(4096)[::5] if n not in names]
    N = len(cols)
    for b in range(N):
        # the cases under test at slot 0, in the middle and at the last slot; other cases around them
        slots = [fill[(b + j) % len(fill)] for j in range(64)]
        slots[0], slots[31], slots[63] = cols[b], cols[(b + 2) % N], cols[(b + 1) % N]
        _batch_equals_oracle(ctx64, oracle, slots, (family, names[b]))


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_a_list_of_one_is_the_stage_seam(ctx9, oracle, family):
    """mtf_batch([c]) == [mtf(c)] for every case, those built for 4,096 included: one block is walked in tiles of 2,048"""
    for name in mc.FAMILIES[family]:
        _, col, hb, _, _ = mc.case(name)
        (one,) = ctx9.mtf_batch([(col, hb)])
        alone = ctx9.mtf(col, hb)
        _same(one, alone, name)
        _same(one, _truth(oracle, col, hb), name)


def test_lists_of_63_64_and_65(native, oracle):
    """64 and 65 columns run with tiles of 4,096, the same first 63 with tiles of 2,048: the same results block by block"""
    with native.Context(0, 1, 65) as ctx:
        r65 = _batch_equals_oracle(ctx, oracle, mc.batch_list(65), 65)
        r64 = _batch_equals_oracle(ctx, oracle, mc.batch_list(64), 64)
        r63 = _batch_equals_oracle(ctx, oracle, mc.batch_list(63), 63)
    for k in range(63):
        _same(r63[k], r64[k], k)
        _same(r63[k], r65[k], k)


def test_bad_lists_are_refused_and_the_context_goes_on(native, ctx64, oracle):
    E_ARG = -1
    good = mc.batch_list(64)
    for bad in (mc.batch_list(65), [], good[:3] + [(b"", mc.hb_of([0]))], good[:3] + [(bytes(mc.LEVEL1_M + 1), mc.hb_of([0]))]):
        with pytest.raises(native.BzhError) as e:
            ctx64.mtf_batch(bad)
        assert e.value.status == E_ARG and len(str(e.value)) > len("bzhip status -1: ")
        _batch_equals_oracle(ctx64, oracle, good, "after a refused list")
    L = native.lib()
    assert L.bzh_mtf_batch(ctx64.handle, None, None, None, 1, None, None, None, None, None) == E_ARG
    _batch_equals_oracle(ctx64, oracle, good[:7], "after a null pointer")
