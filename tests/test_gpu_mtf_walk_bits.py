"""The bit-serial parts of mtf_walk_par (banzai_amd/csrc/mtf.hip) on the MI355X, each at the edges of its own shortcuts:
the match-any that stops at `ebits`, the places comparator that skips a bit no first occurrence disagrees on, and the list
update that reads a record per 64 places from LDS.  Every column is built head by head (tests/mtf_cases.from_positions:
every byte is a run head, so the lanes of a chunk are 64 bytes in a row and the first chunk of the block sees the identity
list -- a new symbol's place is its name) and goes two ways: alone through Context.mtf (one block: tiles of 2,048) and as
member 0 of a list of 64 short columns through Context.mtf_batch (tiles of 4,096).  Symbols, m, all 258 frequencies and
num_syms are the oracle's bit for bit, as in tests/test_gpu_mtf_edges.py.  No tolerance anywhere."""
import numpy as np
import pytest

from tests import mtf_cases as mc

N_BYTES = 4133  # three tiles of 2,048, two of 4,096, a last half of 37 bytes
EDGES = mc.PLACE_EDGES  # 63, 64, 127, 128, 191, 192, 255


def _column(symbols, N):
    """the column of these run heads over names 0..N-1, through from_positions: every byte a head at a position >= 1"""
    symbols = [int(s) for s in symbols]
    lst = list(range(N))
    pos = []
    for s in symbols:
        r = lst.index(s)
        pos.append(r)
        lst.insert(0, lst.pop(r))
    col = mc.from_positions(pos, N)
    assert col.tolist() == symbols
    return col.tobytes(), mc.hb_of(range(N))


def _heads(rng, n, N, avoid):
    return mc.literal(rng, n, np.arange(N), avoid=avoid).tolist()


def _with_tail(first, N, seed):
    rng = np.random.default_rng(seed)
    return _column(first + _heads(rng, N_BYTES - len(first), N, first[-1]), N)


# ---- the ebits boundary of the match-any -------------------------------------------------------------------------------------
def _ebits_case(N):
    if N == 1:  # one name: no run head at all
        return bytes(N_BYTES), mc.hb_of([0])
    if N == 2:
        return _column(([1, 0] * N_BYTES)[:N_BYTES], 2)
    ebits = (N - 1).bit_length()
    top = 1 << (ebits - 1)
    x = N - 1 - top  # x and the highest name differ in bit ebits - 1 only
    assert 0 <= x < top and (x | top) == N - 1
    rng = np.random.default_rng(7000 + N)
    first = [N - 1, x] * 4
    return _with_tail(first + _heads(rng, 56, N, first[-1]), N, 7100 + N)


# ---- the comparator's skips, 256 names: the first chunk's new symbols sit at the places of their names ---------------------------
def _chunk_small_places():  # (a) all below 16: bits 7..4 have no first occurrence
    rng = np.random.default_rng(7201)
    return mc.literal(rng, 64, np.arange(1, 16)).tolist()


def _chunk_high_places():  # (b) all at 128 and above: every first occurrence has bit 7
    rng = np.random.default_rng(7202)
    return rng.permutation(np.arange(128, 256))[:64].tolist()


def _chunk_one_high(L):  # (d) one new symbol at place 200 in lane L, 63 new ones at places 1..63: no bit is uniform
    rng = np.random.default_rng(7300 + L)
    small = rng.permutation(np.arange(1, 64)).tolist()
    return small[:L] + [200] + small[L:]


CHUNKS = {
    "small_places": _chunk_small_places,
    "high_places": _chunk_high_places,
    "one_high_lane0": lambda: _chunk_one_high(0),
    "one_high_lane31": lambda: _chunk_one_high(31),
    "one_high_lane32": lambda: _chunk_one_high(32),
    "one_high_lane63": lambda: _chunk_one_high(63),
    "descending_top": lambda: list(range(255, 191, -1)),  # (e) cntB = lane: 0..63
    "descending_across_words": lambda: list(range(100, 36, -1)),
    "ascending": lambda: list(range(1, 65)),  # cntB = 0 in every lane
}


def _one_new_symbol(n):
    """(c) n = 64 k + 1 heads: the last chunk of the half has one head, its only new symbol"""
    rng = np.random.default_rng(7400 + n)
    return _column(_heads(rng, n, 256, 0), 256)


# ---- the list update through LDS ----------------------------------------------------------------------------------------------
def _unseen_all():
    """chunk 0: new symbols in the word of every edge place and in the word above it, none on an edge; chunk 1: the edges"""
    low = [5, 62, 65, 70, 126, 129, 130, 190, 193, 200, 254]
    c0 = [low[i % len(low)] for i in range(64)]
    c1 = [EDGES[i % len(EDGES)] for i in range(64)]
    return c0 + c1


def _unseen_one(e):
    """chunk 0: one new symbol in the word of place e and one in the word above (the top word: a second one in it);
    chunk 1: the unseen name e and its neighbour"""
    w = e >> 6
    a = 64 * w + 1
    b = 64 * (w + 1) + 7 if w < 3 else 64 * w + 33
    assert e not in (a, b)
    return [a, b] * 32 + [e, a] * 32


CASES = {}
for _N in (1, 2, 3, 64, 65, 128, 129, 255, 256):
    CASES["ebits_%d_names" % _N] = (lambda N=_N: _ebits_case(N))
for _name, _fn in CHUNKS.items():
    CASES["skip_" + _name] = (lambda fn=_fn, k=len(CASES): _with_tail(fn(), 256, 7500 + k))
for _n in (65, 1025):
    CASES["skip_one_new_symbol_%d" % _n] = (lambda n=_n: _one_new_symbol(n))
CASES["update_unseen_at_every_edge"] = lambda: _with_tail(_unseen_all(), 256, 7600)
for _e in EDGES:
    CASES["update_unseen_at_%d" % _e] = (lambda e=_e: _with_tail(_unseen_one(e), 256, 7600 + e))

_BUILT = {}
_TRUTH = {}


def _case(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def _truth(oracle, name):
    if name not in _TRUTH:
        _TRUTH[name] = oracle.mtf_and_rle(*_case(name))
    return _TRUTH[name]


def _same(got, want, what):
    gs, gf, gn = got
    ws, wf, wn = want
    assert gn == wn, what
    assert len(gs) == len(ws), (what, len(gs), len(ws))
    assert np.array_equal(gs, ws), (what, int(np.nonzero(gs != ws)[0][0]))
    assert np.array_equal(gf, wf), what


@pytest.fixture(scope="module")
def ctx64(native):
    with native.Context(0, 1, 64) as c:
        yield c


def test_the_builders_build_what_they_say():
    """(no device: the facts the cases are named for, on the columns themselves)"""
    for N in (2, 3, 64, 65, 128, 129, 255, 256):
        col = np.frombuffer(_case("ebits_%d_names" % N)[0], dtype=np.uint8)
        ebits = max(1, (N - 1).bit_length())
        assert N - 1 in col[:64] and int(col.max()) == N - 1
        assert any(int(a) ^ int(b) == 1 << (ebits - 1) for a, b in zip(col[:63], col[1:64]))
    for name, fn in CHUNKS.items():
        assert len(fn()) == 64, name
    assert max(_chunk_small_places()) < 16 and min(_chunk_high_places()) >= 128
    for L in (0, 31, 32, 63):
        c = _chunk_one_high(L)
        assert c[L] == 200 and len(set(c)) == 64
        new = np.array(c)
        for bit in range(8):  # some first occurrence has the bit, some has not: no step of the comparator is skipped
            assert 0 < int(((new >> bit) & 1).sum()) < 64, (L, bit)
    c = _unseen_all()
    assert not set(c[:64]) & set(EDGES) and set(c[64:]) == set(EDGES)
    for e in EDGES:
        assert any(s >> 6 == e >> 6 for s in c[:64]) and (e >> 6 == 3 or any(s >> 6 == (e >> 6) + 1 for s in c[:64]))
    assert len(_case("skip_one_new_symbol_65")[0]) % 64 == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_alone_in_tiles_of_2048(ctx9, oracle, name):
    col, hb = _case(name)
    _same(ctx9.mtf(col, hb), _truth(oracle, name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_member_0_of_64_in_tiles_of_4096(ctx64, oracle, name):
    names = list(CASES)
    at = names.index(name)
    others = [names[(at + 1 + j) % len(names)] for j in range(63)]  # (the cases themselves are the short columns around it)
    res = ctx64.mtf_batch([_case(n) for n in [name] + others])
    assert len(res) == 64
    _same(res[0], _truth(oracle, name), name)
    for n, got in zip(others, res[1:]):
        _same(got, _truth(oracle, n), (name, n))
