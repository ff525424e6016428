"""Symbol streams that drive the default-mode Huffman stage (banzai_amd/csrc/huffman.hip) to its table, scaling, range,
segment and pack edges, each with the facts it was built to reach -- facts of tests/huff_paths_model.py's record, so the
CPU test and the GPU test can both show that a builder still gets there before anything is compared.

A case is (name, syms, num_syms, freqs, want): `freqs` is the histogram of `syms` (uint32[258]), the last symbol is the
end-of-block symbol num_syms - 1, and `want` maps a fact to what the record must show (see unmet()).  FAMILIES groups the
case names; case(name) builds one (cached), analysed(name) adds the model's lengths and record.

The parameters of the scaling cases and of the fullest tile come from a CPU search with the model over (chain length,
multiplier); the search is not repeated here, its results are asserted.  What it did not find within 900,001 symbols:
  * two tables accepted at exponent 9: the chain of 19 reaches exponent 8 from a multiplier of 28 on (611,876 symbols; the
    case uses 32), so exponent 9 wants about 56 -- 1.2 million symbols, and still over a million if table 0 won every
    segment (frequencies 4 F instead of about 3.5 F).
"""
import functools

import numpy as np

from tests import huff_paths_model as hm

M_MAX = 900_001

ALPHABETS = (3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 194, 198, 199, 200, 201, 257, 258)
HISTOGRAMS = ("flat", "dominant", "doubling", "random")
M_EDGES = (1, 2, 49, 50, 51, 99, 100, 101, 4095, 4096, 4097, 8191, 8192, 8193, 12799, 12800, 12801)
M_ALPHABETS = (3, 50, 258)


def _close(body, ns):
    """body + end-of-block symbol -> (syms, ns, freqs)"""
    s = np.concatenate([np.asarray(body, dtype=np.uint16), np.array([ns - 1], np.uint16)])
    assert s.size <= M_MAX
    f = np.zeros(258, np.uint32)
    f[:ns] = np.bincount(s, minlength=ns)
    return s, ns, f


def shuffled(counts, seed):
    """every symbol k counts[k] times, shuffled; num_syms = len(counts) + 1"""
    counts = np.asarray(counts, dtype=np.int64)
    body = np.repeat(np.arange(counts.size, dtype=np.uint16), counts)
    np.random.default_rng(seed).shuffle(body)
    return _close(body, counts.size + 1)


def _chain(n, first, second):
    """w_i = w_(i-1) + w_(i-2) + 1: weights whose Huffman tree is one long chain, whatever way ties fall"""
    w = [first, second]
    while len(w) < n:
        w.append(w[-1] + w[-2] + 1)
    return w[:n]


# ---- alphabet edges ---------------------------------------------------------------------------------------------------
def _alphabet(ns, kind):
    n = ns - 1  # symbols of the body
    rng = np.random.default_rng(1000 * ns + HISTOGRAMS.index(kind))
    if kind == "flat":
        c = np.full(n, max(1, 3000 // n))
    elif kind == "dominant":  # (symbol 0, as the zero runs of real blocks: the range of table 0 ends at once)
        c = np.full(n, max(1, 1000 // n))
        c[0] = 3 * c.sum()
    elif kind == "doubling":
        c = np.minimum(1 << np.minimum(np.arange(n), 20), max(2, 4000 // n))
        c = c * max(1, 3000 // int(c.sum()))
    else:
        c = rng.integers(1, 40, n) * (rng.random(n) < 0.7)
        c[0] = max(c[0], 1)
        c = c * max(1, 3000 // int(c.sum()))
    want = dict(ntab=2 if ns <= 199 else 3)
    if kind == "flat" and ns >= 17:
        # (the shuffle spreads table 0's share of each symbol by a few counts; from 17 symbols on the model finds equal
        # priorities under both comparisons of an extract.  All priorities equal: the count edges m = 1, 2 and the segment
        # case in which table 1 wins nothing.)
        want.update(tie_sibling=True, tie_moved=True)
    return shuffled(c, ns) + (want,)


# ---- symbol-count edges ------------------------------------------------------------------------------------------------
def _count_edge(ns, m):
    rng = np.random.default_rng(7 * m + ns)
    body = np.minimum(rng.geometric(0.08, m - 1) - 1, ns - 2)
    want = dict(ntab=2 if ns <= 199 else 3, nseg=(m + 49) // 50, last_seg=(m - 1) % 50 + 1, ntiles=(m + 4095) // 4096)
    if ns == 258 and m <= 2:
        want.update(min_sink=8)  # tables that won nothing: 258 equal priorities, the moved element sinks to the last level
    return _close(body, ns) + (want,)


# ---- scaling: two tables -------------------------------------------------------------------------------------------------
# (chain length, multiplier in quarters) -> exponents of (table 0, table 1), as the search found them
TWO = {
    "two_exp0": (17, 4, [0, 0]),
    "two_exp1": (19, 3, [1, 0]),
    "two_exp2": (18, 4, [2, 0]),
    "two_exp3": (18, 8, [3, 0]),
    "two_exp4_upper_then_lower": (18, 12, [4, 0]),
    "two_exp5": (18, 24, [5, 0]),
    "two_exp6": (18, 48, [6, 0]),
    "two_exp7": (18, 96, [7, 0]),
    "two_both_upper": (19, 32, [6, 4]),
    "two_carry_exp8": (19, 128, [8, 5]),
}


def _two(n, k4, exps):
    c = [max(1, (w - 1) * k4 // 4 + 1) for w in _chain(n, 1, 1)]
    return shuffled(c, 1) + (dict(ntab=2, exps=exps, halves=[hm.half_of(2, e) for e in exps]),)


# ---- scaling: three tables ------------------------------------------------------------------------------------------------
# (filler count, chain length, multiplier in quarters) -> exponents: 200 fillers that form a subtree of depth 8 under a chain
THREE = {
    "three_exp0": (0, 10, 1, [0, 0, 0]),
    "three_exp1": (0, 10, 2, [1, 0, 0]),
    "three_exp2": (0, 10, 3, [2, 0, 0]),
    "three_exp3": (0, 10, 6, [3, 0, 0]),
    "three_exp4": (0, 10, 12, [4, 0, 0]),
    "three_carry_exp5": (1, 10, 32, [5, 0, 0]),
    "three_carry_exp6": (1, 10, 64, [6, 0, 0]),
    "three_table1_nonzero": (0, 11, 6, [3, 1, 0]),
    "three_different": (0, 11, 12, [4, 2, 0]),
    "three_carry_upper_lower": (0, 11, 24, [5, 3, 0]),
}


def _three(filler, n, k4, exps):
    c = [filler] * 200 + [max(1, k4 * w // 4) for w in _chain(n, 210, 211)]
    return shuffled(c, 1) + (dict(ntab=3, exps=exps, halves=[hm.half_of(3, e) for e in exps], backoff="taken"),)


# ---- ranges ------------------------------------------------------------------------------------------------------------------
def _range_backoff_single():
    """three tables; symbol 1 alone is more than half of what table 0 left: right == left, no back-off"""
    c = [1000, 1500] + [2] * 197
    return shuffled(c, 2) + (dict(ntab=3, backoff="single", ranges=[(0, 0), (1, 1), (2, 199)]),)


def _range_one_symbol():
    c = [3000, 400, 300, 200, 100]
    return shuffled(c, 3) + (dict(ntab=2, ranges=[(0, 0), (1, 5)]),)


def _range_to_last_mtf_symbol():
    """table 0 gets every symbol but the end-of-block symbol, table 1 that alone"""
    c = [10, 20, 30, 40, 50, 60, 70, 2000]
    return shuffled(c, 4) + (dict(ntab=2, ranges=[(0, 7), (8, 8)]),)


# ---- segments ----------------------------------------------------------------------------------------------------------------
def _seg_table1_wins_nothing():
    """0 1 0 1 ...: every segment holds as many symbols of table 0's range as of table 1's, and the first minimum wins;
    table 1's frequencies are all zero, its build nothing but ties.  Also a last segment of one symbol."""
    body = np.tile(np.array([0, 1], np.uint16), 1000)
    return _close(body, 3) + (dict(ntab=2, ranges=[(0, 0), (1, 2)], seg_wins_zero=1, seg_ties=[(0, 1)], last_seg=1, nseg=41),)


def _seg_tie_12():
    c = np.full(257, 12)
    return shuffled(c, 5) + (dict(ntab=3, seg_ties=[(0, 1), (1, 2)]),)


def _seg_last_49():
    c = [512, 512, 256, 256, 128, 128, 64, 64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2, 2, 2]
    s, ns, f = shuffled(c, 6)
    assert s.size == 2049
    return s, ns, f, dict(ntab=2, last_seg=49, nseg=41)


# ---- pack --------------------------------------------------------------------------------------------------------------------
def _pack_one_bit_tile():
    """tile 1 holds symbol 0 only, whose code is one bit long"""
    rng = np.random.default_rng(8)
    mixed = np.minimum(rng.geometric(0.6, 8192) - 1, 4).astype(np.uint16)
    body = np.concatenate([mixed[:4096], np.zeros(4096, np.uint16), mixed[4096:8000]])
    return _close(body, 6) + (dict(ntab=2, tile_bits={1: 4096}, ntiles=3, thread_words=[1, 2]),)


FULL_TILE = 25        # 25 * 4,096 symbols = 2,048 whole segments in front of it
FULL_TILE_BITS = 69_496  # 4,096 * 17 - 136: what the search reached (of 247 rare symbols 8 sit one level higher)


def _pack_fullest_tile():
    """A chain of ten frequent symbols over a subtree of 247 rare ones and the end-of-block symbol: the rare symbols get
    17-bit and a few 16-bit codes at scaling 1.  All 4,096 rare symbols sit in one tile, so table 0 wins their segments
    (none of its range in them) and their frequencies are exactly 4 x their counts whatever the shuffle does elsewhere."""
    ch = _chain(10, 5658, 5659)[::-1]
    rc = np.full(247, 16)
    rc[:4096 - rc.sum()] += 1
    rng = np.random.default_rng(1)
    body = np.repeat(np.arange(10, dtype=np.uint16), ch)
    rng.shuffle(body)
    rare = np.repeat(np.arange(10, 257, dtype=np.uint16), rc)
    rng.shuffle(rare)
    at = FULL_TILE * 4096
    want = dict(ntab=3, exps=[0, 0, 0], tile_bits={FULL_TILE: FULL_TILE_BITS}, unaligned_tile=FULL_TILE, longest0=17)
    return _close(np.concatenate([body[:at], rare, body[at:]]), 258) + (want,)


def _pack_three_words():
    c = np.full(16, 64)
    return shuffled(c, 9) + (dict(ntab=2, thread_words=[3]),)


# ---- registry ----------------------------------------------------------------------------------------------------------------
_BUILDERS = {}
FAMILIES = {}


def _add(family, name, fn, *args):
    _BUILDERS[name] = (fn, args)
    FAMILIES.setdefault(family, []).append(name)


for _ns in ALPHABETS:
    for _kind in HISTOGRAMS:
        _add("alphabet", "alphabet_%d_%s" % (_ns, _kind), _alphabet, _ns, _kind)
for _ns in M_ALPHABETS:
    for _m in M_EDGES:
        _add("count", "count_%d_m%d" % (_ns, _m), _count_edge, _ns, _m)
for _name, _p in TWO.items():
    _add("two_tables", _name, _two, *_p)
for _name, _p in THREE.items():
    _add("three_tables", _name, _three, *_p)
_add("ranges", "range_backoff_taken", _three, *THREE["three_exp0"])
_add("ranges", "range_backoff_single", _range_backoff_single)
_add("ranges", "range_one_symbol", _range_one_symbol)
_add("ranges", "range_to_last_mtf_symbol", _range_to_last_mtf_symbol)
_add("segments", "seg_tie_01_table1_wins_nothing_last_1", _seg_table1_wins_nothing)
_add("segments", "seg_tie_12", _seg_tie_12)
_add("segments", "seg_last_49", _seg_last_49)
_add("pack", "pack_one_bit_tile", _pack_one_bit_tile)
_add("pack", "pack_fullest_tile", _pack_fullest_tile)
_add("pack", "pack_three_words", _pack_three_words)

NAMES = [n for fam in FAMILIES.values() for n in fam]


@functools.lru_cache(maxsize=None)
def case(name):
    fn, args = _BUILDERS[name]
    s, ns, f, want = fn(*args)
    assert s[-1] == ns - 1 and np.array_equal(f[:ns], np.bincount(s, minlength=ns)) and not f[ns:].any()
    return name, s, ns, f, want


@functools.lru_cache(maxsize=None)
def analysed(name):
    """-> (case, model lengths, model record)"""
    c = case(name)
    lens, rec = hm.analyse(c[1], c[2])
    return c, lens, rec


def unmet(rec, lens, want):
    """the wanted facts that the record does not show, as a list of strings (empty: the case reaches its edge)"""
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(what)

    for k, v in want.items():
        if k in ("ntab", "exps", "halves", "backoff", "ranges", "nseg", "last_seg", "tie_sibling", "tie_moved"):
            need(rec[k] == v, "%s: %r, wanted %r" % (k, rec[k], v))
        elif k == "ntiles":
            need(len(rec["tile_bits"]) == v, "tiles: %d, wanted %d" % (len(rec["tile_bits"]), v))
        elif k == "min_sink":
            need(rec["max_sink"] >= v, "deepest sink %d, wanted %d" % (rec["max_sink"], v))
        elif k == "min_rise":
            need(rec["max_rise"] >= v, "highest rise %d, wanted %d" % (rec["max_rise"], v))
        elif k == "seg_wins_zero":
            need(rec["seg_wins"][v] == 0, "table %d won %d segments, wanted none" % (v, rec["seg_wins"][v]))
        elif k == "seg_ties":
            need(set(v) <= rec["seg_ties"], "segment ties %r, wanted %r" % (sorted(rec["seg_ties"]), v))
        elif k == "tile_bits":
            for t, b in v.items():
                need(rec["tile_bits"][t] == b, "tile %d: %d bits, wanted %d" % (t, rec["tile_bits"][t], b))
        elif k == "unaligned_tile":
            at = hm.SEAM_FRAME + rec["pack_start"] + sum(rec["tile_bits"][:v])
            need(at % 32 != 0, "tile %d starts word aligned" % v)
        elif k == "thread_words":
            need(set(v) <= rec["thread_words"], "words a thread: %r, wanted %r" % (sorted(rec["thread_words"]), v))
        elif k == "longest0":
            need(int(lens[0].max()) == v, "longest code of table 0: %d, wanted %d" % (int(lens[0].max()), v))
        else:
            raise KeyError(k)
    # what the accepted exponent means: every smaller scaling left a code longer than 17 bits, this one did not
    for lg in rec["attempt_maxlen"]:
        need(all(x > hm.MAX_LEN for x in lg[:-1]) and lg[-1] <= hm.MAX_LEN, "attempts %r" % (lg,))
    return bad
