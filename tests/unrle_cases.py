"""Blocks behind the inverse BWT built for the edges of the inverse-RLE1 back end (banzai_amd/csrc/decode.hip, ur_load to
unrle_select): which byte a thread, a wavefront or a tile begins with and in which state, constant stretches whose state map is a
rotation, the tile chain beyond 64 tiles, block ends, the staging threshold, ur_copy_out's alignments, windows, pieces, records.

A case is (name, x, level, wanted edges, extras); FAMILIES names them by family, EDGES[family] lists the edge names a family
declares.  unmet(record, wanted) holds a case's claims against tests/unrle_paths_model.py's record of it: it must be empty for
every case, and every declared edge must be wanted by a case (tests/test_unrle_paths_model.py).  The truth of every case is
bz2_handbuilt.unrle(x); stream(name) frames it with bz2_handbuilt.stream_of_rle, once a process."""
import functools
import random

import numpy as np

from tests import bz2_handbuilt
from tests import unrle_paths_model as um

TILE, WAVE, ITEMS = um.UR_TILE, um.WAVE, um.UR_ITEMS
LETTERS = bytes(b for b in range(ord("a"), ord("z") + 1) if b != ord("q"))  # literals; runs are of 0, 255 and 'q'
RUN_BYTES = (0, 255, ord("q"))
# "v": the count equals the run byte; "next": the byte behind the count equals it and starts a run of one; "again": a count of
# 255 and the run byte behind it three times more (what an encoder writes for a run of 262)
COUNT_KINDS = (0, 1, 4, 255, "v", "next", "again")
SEAMS = ((48, "thread"), (1024, "wave"), (1104, "thread"), (2048, "wave"), (3072, "wave"), (4096, "tile"), (5120, "wave"),
         (5168, "thread"), (8192, "tile"))
END_N = (1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193) + tuple(4128 + r for r in range(16))
CHAIN_TILES = (63, 64, 65, 127, 128, 129, 191, 192, 193)
MAX_TILE_TOTAL = 819 * 259


class Bld:
    """a block under construction: literals never repeat their neighbour, so only run() makes a run"""

    def __init__(self, seed):
        self.b = bytearray()
        self.rng = random.Random(seed)

    def lits(self, k, last_not=None):
        for j in range(k):
            while True:
                v = self.rng.choice(LETTERS)
                if (not self.b or v != self.b[-1]) and not (j == k - 1 and v == last_not):
                    break
            self.b.append(v)
        return self

    def upto(self, P, last_not=None):
        assert P >= len(self.b), (P, len(self.b))
        return self.lits(P - len(self.b), last_not)

    def run(self, v, c=None, eqs=4):
        assert not self.b or self.b[-1] != v
        self.b += bytes([v]) * eqs
        if c is not None:
            self.b.append(c)
        return self

    def fat(self, k):
        """k runs of 259: 5 bytes in, 259 out"""
        for j in range(k):
            v = LETTERS[j % len(LETTERS)]
            self.run(v if not self.b or self.b[-1] != v else LETTERS[(j + 1) % len(LETTERS)], 255)
        return self

    def mixed(self, k, small=False):
        """exactly k bytes of literals and whole runs with counts of every kind (small: of at most 7); ends in a literal"""
        end = len(self.b) + k
        while len(self.b) < end:
            room = end - len(self.b)
            if room >= 7 and self.rng.randrange(3) == 0:
                v = self.rng.choice(RUN_BYTES)
                self.run(v, self.rng.choice((0, 1, 4, 7) if small else (0, 1, 4, 255, v, 7)))
                self.lits(1)
            else:
                self.lits(min(room, self.rng.randrange(1, 20)))
        return self


# ---- builders: -> (x, level, wanted edges, extras) ---------------------------------------------------------------------------------
def _seam(s, ck, fat, seed):
    """every seam of SEAMS met in state s (0: the count byte is the last byte before the seam), counts of kind ck"""
    b = Bld(seed)
    want = ["seam:%s:%d" % (kind, s) for kind in ("thread", "wave", "tile")]
    fat_done = set()
    for j, (P, kind) in enumerate(SEAMS):
        v = RUN_BYTES[j % 3]
        c = v if ck == "v" else (7 if ck == "next" else (255 if ck == "again" else ck))
        start = P - (s if s else 5)
        if fat and len(b.b) // TILE not in fat_done and start - len(b.b) >= 200:
            fat_done.add(len(b.b) // TILE)
            b.lits(3).fat(33)
        b.upto(start, last_not=v).run(v, c)
        if ck in ("next", "again"):
            b.b += bytes([c]) if ck == "next" else bytes([v]) * 3
        b.lits(2)
    if fat:
        b.lits(3).fat(33)
    b.lits(20 + 3 * s + COUNT_KINDS.index(ck))
    want += ["count:%s" % ck, "run_byte:0", "run_byte:255"]
    if s == 4:
        want += ["seam_count:%s:%s" % (kind, ck) for kind in ("thread", "wave", "tile")]
    if fat:
        want += ["win:unstaged"]
    else:
        want += ["win:staged"]
    want += ["win:around_seam", "win:len0", "win:whole", "win:ends_at_block_end"] + (["win:inside_count_run"] if s == 4 and ck in (4, 255, "next", "again") else [])
    return bytes(b.b), 1, want, dict(windows=True)


def _const(v, phase, seed):
    """bytes([v]) * k from byte 700 + phase across three wave seams, a whole tile and into the next, then markers"""
    b = Bld(seed).lits(700 + phase, last_not=v)
    b.b += bytes([v]) * (2 * TILE + 500)
    b.lits(40)
    want = ["stretch:%d:tile_entry:%d" % (v, (1 - phase) % 5), "stretch:%d:fills_wave" % v, "stretch:%d:fills_tile" % v,
            "stretch:%d:markers" % v] + ["stretch:%d:crosses_wave:%d" % (v, w) for w in (1, 2, 3)]
    return bytes(b.b), 1, want, {}


_CHAIN_CUTS = (10.3, 20.6, 30.1, 40.7, 50.2, 60.4, 66.6, 80.3, 100.9, 120.2, 130.5, 150.1, 170.8, 188.3, 194.4, 210.6)


def _chain(n, vs, seed):
    """n bytes of constant stretches with seven markers between them, cut so that tiles 63..65, 127..129, 191..193 and the last
    each sit inside a stretch begun at least two tiles earlier"""
    b = Bld(seed).lits(5, last_not=vs[0])
    last = (n - 1) // TILE
    cuts = [int(c * TILE) + k for k, c in enumerate(_CHAIN_CUTS) if c + 1 < last - 2] + [n]
    for j, cut in enumerate(cuts):
        v = vs[j % len(vs)]
        b.b += bytes([v]) * (cut - len(b.b) - (7 if cut != n else 0))
        if cut != n:
            b.lits(7, last_not=vs[(j + 1) % len(vs)])
    assert len(b.b) == n
    want = ["chain:tile:%d" % t for t in CHAIN_TILES if t <= last] + ["chain:last_tile"]
    want += ["chain:tiles_over:%d" % k for k in (64, 128, 192) if last >= k]
    if vs == (0,):
        want.append("chain:output_shorter")
    return bytes(b.b), 9, want, {}


def _end(n, e, seed):
    """n bytes that leave state e behind them (4: four equal bytes and no count)"""
    tail = {0: 5, 1: 1, 2: 2, 3: 3, 4: 4}[e]
    if n < tail:
        return None
    b = Bld(seed)
    if n - tail >= 1:
        b.mixed(n - tail)
    if e == 1:
        b.lits(1)
    else:
        b.run(0 if n % 2 else 255, 3 if e == 0 else None, eqs=min(e, 4) if e else 4)
    assert len(b.b) == n
    want = ["n:%d" % n, "n_mod16:%d" % (n % 16), "end_state:%d" % e] + (["behind_n"] if n % 16 else []) + (["end:state4"] if e == 4 else [])
    return bytes(b.b), 1, want, {}


def _end_count_alone(c):
    """n = 4097 and the last tile is one count byte"""
    b = Bld(c).lits(4092).run(ord("q"), c)
    return bytes(b.b), 1, ["n:4097", "last_tile_is_count:%d" % c] + (["last_tile_total_zero"] if c == 0 else []), {}


def _stale_long():
    return (b"aaaa\xff" + b"bbbb\xff") * 2000, 1, ["behind_n:long_ff_block"], {}


def _staging_tile(c):
    return b"\x06" * 5 * 817 + b"bbbb" + bytes([c]) + b"uvwxyz"


def _staging(where, total, seed):
    """a tile that expands to exactly `total` (8,191 to 8,193, or the format's most) as first, middle or last tile"""
    if total == "max":
        S = b"".join(bytes([LETTERS[k % 5]]) * 4 + b"\xff" for k in range(819)) + b"z"
    else:
        S = _staging_tile(total - 8180)
    assert len(S) == TILE
    b = Bld(seed)
    b.lits(TILE * {"first": 0, "middle": 1, "last": 2}[where], last_not=S[0])
    b.b += S
    if where != "last":
        b.lits(TILE * (1 if where == "first" else 0) + 100)
    want = ["tile_total:%s:%s" % (where, total), "win:whole", "win:around_seam", "win:staged"] + (["win:unstaged"] if total in (8193, "max") else [])
    return bytes(b.b), 1, want, dict(windows=True)


def _copy(r, k, base):
    """tile 1 holds k literals and begins at toff = r mod 4; the block's output begins at `base` mod 4"""
    b = Bld(100 + 8 * r + k).lits(TILE - 5, last_not=ord("q")).run(ord("q"), 1 + r).lits(k)
    head = (-(base + r)) & 3
    want = ["copy:obase:%d" % base, "copy:toff:%d" % r, "copy:total:%d" % k, "copy:head:%d" % min(k, head), "copy:tail:%d" % ((k - min(k, head)) % 4)]
    if k < head:
        want.append("copy:n_lt_head")
    if (k - min(k, head)) // 4 == 0:
        want.append("copy:words0")
    return bytes(b.b), 1, want, dict(pre=base)


def _pieces_block():
    b = Bld(41).mixed(TILE, small=True)                   # tile 0: staged
    b.fat(40).upto(2 * TILE)                              # tile 1: 40 runs of 259 and literals, not staged
    b.mixed(TILE, small=True)                             # tile 2: staged, no piece meets it
    b.mixed(TILE - 96, small=True)                        # tile 3: staged and ragged
    return bytes(b.b)


def _pieces(m):
    """m pieces on a staged tile, m on one too large to stage, none on the next, the rest of m + 1 on the last"""
    x = _pieces_block()
    rec = um.analyse(x)
    toff = [t["toff"] for t in rec["tiles"]] + [rec["bsize"]]
    pieces = []
    for t in (0, 1):
        lo, hi = toff[t], toff[t + 1]
        if m == 1:
            pieces.append((lo + 5, lo + 6))                     # one byte
        else:
            pieces.append((hi - 300, hi))                       # ends on the seam
            pieces.append((lo + 10, lo + 11))                   # one byte
            pieces.append((lo + 100, lo + 400))
            if m >= 4:
                pieces.append((lo + 200, lo + 250))             # inside the one before: a shared range
            if m >= 5:
                pieces.append((lo + 1000, lo + 1007))
    pieces.append((toff[3], toff[3] + 9))
    pieces.append((toff[4] - 33, toff[4]))
    want = ["pieces:%s:%d" % (("workgroup" if m < um.PIECE_WAVES else "wave"), m), "pieces:unstaged:%d" % m, "piece:one_byte", "piece:gap_tile"]
    want += ["piece:ends_on_seam"] if m > 1 else []
    want += ["piece:shared"] if m >= 4 else []
    return x, 1, want, dict(pieces=pieces)


def _records(d, end, seed):
    """the delimiter d as a literal, as a run byte under counts of every kind, as the value of another run's count, inside runs
    that straddle a thread, a wave and a tile seam, on the first and the last byte of a tile; `end`: how the block ends"""
    other = ord("q") if d != ord("q") else 0
    b = Bld(seed).lits(20)
    b.b.append(d)
    b.lits(3).run(other, d).lits(2).run(d, 0).lits(1).run(d, 1).lits(4).run(d, d).lits(2)
    b.upto(1104 - 2, last_not=d).run(d, 9).lits(1)            # a thread seam behind the run's second byte
    b.upto(2048 - 3, last_not=d).run(d, 255).lits(1)          # a wave seam behind its third
    b.upto(TILE - 2, last_not=d).run(d, 6).lits(1)            # a tile seam behind its second
    b.upto(2 * TILE - 1, last_not=d)
    b.b += bytes([d, ord("k"), d])                            # the last byte of tile 1, a literal
    b.lits(300, last_not=d)
    if end == "literal":
        b.b.append(d)
    elif end == "run":
        b.run(d, 2)
    elif end == "run0":
        b.run(d, 0)
    want = ["rec:delim_is_run_byte", "rec:count_value_not_counted", "rec:last:%s" % end, "rec:tile_last", "rec:delim:%d" % d] + \
           ["rec:straddle:%s" % kind for kind in ("thread", "wave", "tile")]
    return bytes(b.b), 1, want, dict(delim=d)


def _records_tile_first(d):
    """the delimiter on byte 0 of tile 1 as a literal, and nowhere near"""
    b = Bld(5 + d).lits(TILE, last_not=d)
    b.b.append(d)
    b.lits(50)
    return bytes(b.b), 1, ["rec:tile_first", "rec:delim:%d" % d], dict(delim=d)


def _records_only_count(d):
    """d shows only as the value of count bytes: at a thread seam, a wave seam, a tile seam and at the block's end"""
    b = Bld(9 + d)
    for P in (48, 1024, TILE, TILE + 64):
        b.upto(P - 4, last_not=ord("q")).run(ord("q"), d).lits(1)
    b.lits(30, last_not=ord("q")).run(ord("q"), d)
    return bytes(b.b), 1, ["rec:only_count", "rec:delim:%d" % d], dict(delim=d)


# ---- registry -------------------------------------------------------------------------------------------------------------------------
_BUILDERS = {}
FAMILIES = {}


def _add(family, name, fn, *args):
    assert name not in _BUILDERS
    _BUILDERS[name] = (fn, args)
    FAMILIES.setdefault(family, []).append(name)


for _s in range(5):
    for _ck in COUNT_KINDS:
        _add("seams", "seam_s%d_c%s" % (_s, _ck), _seam, _s, _ck, False, 10 * _s + COUNT_KINDS.index(_ck))
    for _ck in (0, 255):
        _add("windows", "win_fat_s%d_c%s" % (_s, _ck), _seam, _s, _ck, True, 70 + 10 * _s + _ck % 7)
for _v in (0, 1, 2, 6, 255):
    for _p in range(5):
        _add("constant", "const_v%d_p%d" % (_v, _p), _const, _v, _p, 200 + _v + _p)
_add("chain", "chain_v0_900000", _chain, 900_000, (0,), 1)
_add("chain", "chain_mix_900000", _chain, 900_000, (6, 1, 2, 0), 2)
_add("chain", "chain_v1_790529", _chain, 790_529, (1, 2), 3)
for _n in END_N:
    for _e in range(5):
        if _end(_n, _e, 0) is not None:
            _add("ends", "end_n%d_e%d" % (_n, _e), _end, _n, _e, 1000 + 5 * _n + _e)
for _c in (0, 255):
    _add("ends", "end_n4097_count%d_alone" % _c, _end_count_alone, _c)
_add("stale", "stale_long_ff", _stale_long)
for _w in ("first", "middle", "last"):
    for _t in (8191, 8192, 8193):
        _add("staging", "staging_%s_%d" % (_w, _t), _staging, _w, _t, 300 + _t)
_add("staging", "staging_middle_max", _staging, "middle", "max", 399)
for _r in range(4):
    for _k in range(1, 9):
        for _b in range(4):
            _add("copyout", "copy_r%d_k%d_b%d" % (_r, _k, _b), _copy, _r, _k, _b)
for _m in (1, 3, 4, 5):
    _add("pieces", "pieces_%d" % _m, _pieces, _m)
for _d in (10, 0, 255):
    for _e in ("literal", "run", "run0", "other"):
        _add("records", "rec_d%d_end_%s" % (_d, _e), _records, _d, _e, 500 + _d)
    _add("records", "rec_d%d_tile_first" % _d, _records_tile_first, _d)
    _add("records", "rec_d%d_only_count" % _d, _records_only_count, _d)

NAMES = [n for fam in FAMILIES.values() for n in fam]
STALE_AFTER = [n for n in FAMILIES["ends"]]  # the short blocks decoded behind stale_long_ff in its slot

EDGES = {
    "seams": ["seam:%s:%d" % (k, s) for k in ("thread", "wave", "tile") for s in range(5)] + ["count:%s" % c for c in COUNT_KINDS] +
             ["seam_count:%s:%s" % (k, c) for k in ("thread", "wave", "tile") for c in COUNT_KINDS] + ["run_byte:0", "run_byte:255"],
    "constant": ["stretch:%d:%s" % (v, w) for v in (0, 1, 2, 6, 255) for w in
                 ["tile_entry:%d" % s for s in range(5)] + ["fills_wave", "fills_tile", "markers", "crosses_wave:1", "crosses_wave:2", "crosses_wave:3"]],
    "chain": ["chain:tile:%d" % t for t in CHAIN_TILES] + ["chain:last_tile", "chain:output_shorter"] + ["chain:tiles_over:%d" % k for k in (64, 128, 192)],
    "ends": ["n:%d" % n for n in END_N] + ["n_mod16:%d" % r for r in range(16)] + ["end_state:%d" % e for e in range(5)] +
            ["end:state4", "last_tile_total_zero", "last_tile_is_count:0", "last_tile_is_count:255", "behind_n"],
    "stale": ["behind_n:long_ff_block"],
    "staging": ["tile_total:%s:%s" % (w, t) for w in ("first", "middle", "last") for t in (8191, 8192, 8193)] + ["tile_total:middle:max"],
    "copyout": ["copy:obase:%d" % b for b in range(4)] + ["copy:toff:%d" % r for r in range(4)] + ["copy:total:%d" % k for k in range(1, 9)] +
               ["copy:head:%d" % h for h in range(4)] + ["copy:tail:%d" % t for t in range(4)] + ["copy:n_lt_head", "copy:words0"],
    "windows": ["win:staged", "win:unstaged", "win:around_seam", "win:len0", "win:whole", "win:ends_at_block_end", "win:inside_count_run"],
    "pieces": ["pieces:workgroup:1", "pieces:workgroup:3", "pieces:wave:4", "pieces:wave:5"] + ["pieces:unstaged:%d" % m for m in (1, 3, 4, 5)] +
              ["piece:one_byte", "piece:ends_on_seam", "piece:shared", "piece:gap_tile"],
    "records": ["rec:delim_is_run_byte", "rec:count_value_not_counted", "rec:only_count", "rec:last:literal", "rec:last:run", "rec:last:run0",
                "rec:last:other", "rec:straddle:thread", "rec:straddle:wave", "rec:straddle:tile", "rec:tile_first", "rec:tile_last",
                "rec:delim:0", "rec:delim:10", "rec:delim:255"],
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (name, x, level, wanted edges, extras); extras: pre (bytes of a stream in front), windows, pieces, delim"""
    fn, args = _BUILDERS[name]
    x, level, want, extras = fn(*args)
    assert 1 <= len(x) <= 100_000 * level
    return name, x, level, tuple(want), extras


@functools.lru_cache(maxsize=None)
def truth(name):
    """(what libbz2's rule makes of the case, False when it ends in four equal bytes without a count)"""
    return bz2_handbuilt.unrle(case(name)[1])


_STREAMS = {}


def stream(name):
    """the case framed as a one-block .bz2 stream, its CRCs those of the truth; framed once for equal blocks"""
    _, x, level, _, _ = case(name)
    if (x, level) not in _STREAMS:
        _STREAMS[(x, level)] = bz2_handbuilt.stream_of_rle(x, level, raw=truth(name)[0])
    return _STREAMS[(x, level)]


def windows_of(rec):
    """(lo, hi) in the block's own output: 0, 1, 7 and 300 bytes at -2..+2 around every tile seam, inside the run a tile's first
    byte stands for where it is a count, up to the block's end, and the whole block"""
    bs = rec["bsize"]
    wins = [(0, bs), (max(bs - 7, 0), bs), (max(bs - 300, 0), bs), (bs, bs)]
    for k, t in enumerate(rec["tiles"]):
        if k == 0:
            continue
        for d in (-2, -1, 0, 1, 2):
            for ln in (0, 1, 7, 300):
                lo = min(max(t["toff"] + d, 0), bs)
                wins.append((lo, min(lo + ln, bs)))
        first = t["toff"]
        i = k * TILE
        if rec["bytes"]["state"][i] == 4 and rec["x"][i] >= 3:
            c = int(rec["x"][i])
            wins += [(first + 1, first + 2), (first + 1, first + c - 1), (first + c // 2, first + c // 2 + 7)]
    return [(lo, min(hi, bs)) for lo, hi in wins]


@functools.lru_cache(maxsize=None)
def analysed(name, variant=None):
    """-> (case, record of the path model), with the case's own obase, windows, pieces and delimiter"""
    c = case(name)
    ex = c[4]
    obase = ex.get("pre", 0)
    kw = dict(obase=obase, delim=ex.get("delim"), variant=variant)
    if ex.get("windows"):
        plain = um.analyse(c[1], **kw)
        kw["windows"] = [(lo, hi, k % 4) for k, (lo, hi) in enumerate(windows_of(plain))]
    if ex.get("pieces"):
        at, pcs = 0, []
        for lo, hi in ex["pieces"]:
            pcs.append((lo, hi, at))
            at += hi - lo
        kw["pieces"] = pcs
    return c, um.analyse(c[1], **kw)


# ---- a case's claims against the model's record ---------------------------------------------------------------------------------------
def _seam_idx(kind, n):
    i = np.arange(1, n)
    if kind == "thread":
        return i[(i % ITEMS == 0) & (i % WAVE != 0)]
    if kind == "wave":
        return i[(i % WAVE == 0) & (i % TILE != 0)]
    return i[i % TILE == 0]


def _stretch_of(x, v):
    """[a, b) of the longest stretch of v in x"""
    idx = np.nonzero(np.diff(np.concatenate([[0], (x == v).astype(np.int8), [0]])))[0]
    a, b = max(zip(idx[::2], idx[1::2]), key=lambda p: p[1] - p[0])
    return int(a), int(b)


def unmet(rec, want):
    """the wanted edges that the record does not show, as a list of strings (empty: the case reaches its edges)"""
    bad = []
    x, n, st, tiles = rec["x"], rec["n"], rec["bytes"]["state"], rec["tiles"]
    counts = np.nonzero(st == 4)[0]

    def kind_ok(i, ck):
        c, v = int(x[i]), int(x[i - 1])
        if ck == "v":
            return c == v
        if ck == "again":
            return c == 255 and i + 4 < n and (x[i + 1:i + 4] == v).all() and x[i + 4] != v and st[i + 4] == 3
        if ck == "next":
            return i + 2 < n and x[i + 1] == c and x[i + 2] != c and st[i + 1] == 0 and st[i + 2] == 1
        return c == ck

    for w in want:
        p = w.split(":")
        ok = None
        if p[0] == "seam":
            ok = (st[_seam_idx(p[1], n)] == int(p[2])).any()
        elif p[0] == "count":
            ck = p[1] if p[1] in ("v", "next", "again") else int(p[1])
            ok = any(kind_ok(i, ck) for i in counts)
        elif p[0] == "seam_count":
            ck = p[2] if p[2] in ("v", "next", "again") else int(p[2])
            ok = any(st[i] == 4 and kind_ok(i, ck) for i in _seam_idx(p[1], n))
        elif p[0] == "run_byte":
            ok = any(x[i - 1] == int(p[1]) for i in counts)
        elif p[0] == "stretch":
            v = int(p[1])
            a, b = _stretch_of(x, v)
            if p[2] == "tile_entry":
                ok = a < TILE - 20 and b > 2 * TILE + 20 and tiles[1]["entry"] == int(p[3]) and tiles[2]["entry"] == (int(p[3]) + 1) % 5
            elif p[2] == "fills_wave":
                ok = any(a <= w0 and w0 + WAVE <= b for w0 in range(0, n, WAVE))
            elif p[2] == "fills_tile":
                ok = any(a <= t0 and t0 + TILE <= b for t0 in range(0, n, TILE))
            elif p[2] == "crosses_wave":
                ok = any(a < t0 + int(p[3]) * WAVE - 20 and t0 + int(p[3]) * WAVE + 20 < b for t0 in range(0, n, TILE))
            elif p[2] == "markers":
                ok = b + 6 <= n and len(set(x[b:b + 6].tolist())) >= 5 and (st[b:b + 6] != 4).all() and (np.diff(x[b:b + 7].astype(int)) != 0).all()
        elif p[0] == "chain":
            last = rec["T"] - 1
            inside = lambda t: t <= last and len(set(x[(t - 2) * TILE:min((t + 1) * TILE, n)].tolist())) == 1
            if p[1] == "tile":
                ok = inside(int(p[2]))
            elif p[1] == "last_tile":
                ok = last > 64 and inside(last)
            elif p[1] == "tiles_over":
                ok = last >= int(p[2]) and len({tl["entry"] for tl in tiles[int(p[2]) - 2:int(p[2]) + 2]}) >= 2
            elif p[1] == "output_shorter":
                ok = rec["bsize"] < n
        elif p[0] == "n":
            ok = n == int(p[1])
        elif p[0] == "n_mod16":
            ok = n % 16 == int(p[1])
        elif p[0] == "end_state":
            ok = rec["end"][2] == int(p[1]) and rec["end"][:2] == ((n - 1) // TILE, ((n - 1) % TILE) // ITEMS)
        elif p[0] == "end":
            ok = rec["end"][2] == 4
        elif p[0] == "behind_n":
            ok = (n >= 2 * END_N[13] and (x[4::5] == 255).all()) if len(p) > 1 else rec["threads"]["cnt"].reshape(-1)[(n - 1) // ITEMS] < ITEMS
        elif p[0] == "last_tile_total_zero":
            ok = rec["T"] == 2 and tiles[1]["total"] == 0 and rec["end"][0] == 1
        elif p[0] == "last_tile_is_count":
            ok = rec["T"] == 2 and n == TILE + 1 and st[TILE] == 4 and x[TILE] == int(p[1]) and tiles[1]["total"] == int(p[1])
        elif p[0] == "tile_total":
            t = {"first": 0, "middle": 1, "last": rec["T"] - 1}[p[1]]
            tot = tiles[t]["total"]
            ok = (tot >= MAX_TILE_TOTAL and not tiles[t]["staged"]) if p[2] == "max" else (tot == int(p[2]) and tiles[t]["staged"] == (tot <= um.UR_STAGE))
            ok = ok and (p[1] != "middle" or rec["T"] == 3) and (p[1] != "last" or rec["T"] == 3)
        elif p[0] == "copy":
            t1 = tiles[1] if rec["T"] > 1 else None
            if p[1] == "obase":
                ok = rec["obase"] % 4 == int(p[2])
            elif p[1] == "toff":
                ok = t1["toff"] % 4 == int(p[2])
            elif p[1] == "total":
                ok = t1["total"] == int(p[2]) and t1["staged"]
            elif p[1] == "head":
                ok = t1["head"] == int(p[2])
            elif p[1] == "tail":
                ok = t1["tail"] == int(p[2])
            elif p[1] == "n_lt_head":
                ok = t1["total"] < ((-(rec["obase"] + t1["toff"])) & 3) and t1["head"] == t1["total"]
            elif p[1] == "words0":
                ok = t1["words"] == 0
        elif p[0] == "win":
            ws = rec["windows"]
            seams = [t["toff"] for t in tiles[1:]]
            if p[1] in ("staged", "unstaged"):
                ok = any(c["staged"] == (p[1] == "staged") and 0 < c["thi"] - c["tlo"] < tiles[c["tile"]]["total"] for w_ in ws for c in w_["cuts"])
            elif p[1] == "around_seam":
                ok = all(any(w_["lo"] == s_ + d and w_["hi"] - w_["lo"] == ln for w_ in ws) for s_ in seams for d in (-2, -1, 0, 1, 2) for ln in (0, 1, 7)
                         if 0 <= s_ + d and s_ + d + ln <= rec["bsize"])
                ok = ok and any(len(w_["cuts"]) == 2 for w_ in ws)
            elif p[1] == "len0":
                ok = any(w_["lo"] == w_["hi"] and not w_["cuts"] for w_ in ws)
            elif p[1] == "whole":
                ok = any(w_["lo"] == 0 and w_["hi"] == rec["bsize"] for w_ in ws)
            elif p[1] == "ends_at_block_end":
                ok = any(w_["lo"] > 0 and w_["hi"] == rec["bsize"] and w_["hi"] > w_["lo"] for w_ in ws)
            elif p[1] == "inside_count_run":
                ok = any(st[t * TILE] == 4 and any(tiles[t]["toff"] < w_["lo"] and w_["hi"] < tiles[t]["toff"] + int(x[t * TILE]) and w_["hi"] > w_["lo"]
                                                   for w_ in ws) for t in range(1, rec["T"]))
        elif p[0] == "pieces":
            m = int(p[2])
            ok = any(r_ == p[1] and k == m for r_, k in zip(rec["piece_routes"], rec["pieces_met"]))
        elif p[0] == "piece":
            pc = rec["pieces"]
            ends = [t["toff"] + t["total"] for t in tiles[:-1]]
            if p[1] == "one_byte":
                ok = any(q["hi"] - q["lo"] == 1 for q in pc)
            elif p[1] == "ends_on_seam":
                ok = any(q["hi"] in ends for q in pc)
            elif p[1] == "shared":
                ok = any(a_ is not b_ and a_["lo"] <= b_["lo"] and b_["hi"] <= a_["hi"] for a_ in pc for b_ in pc)
            elif p[1] == "gap_tile":
                met = rec["pieces_met"]
                ok = any(met[t] == 0 and tiles[t]["total"] and any(met[:t]) and any(met[t + 1:]) for t in range(rec["T"]))
        elif p[0] == "rec":
            d = rec["delim"]
            bb, bl = rec["bytes"]["bbyte"], rec["bytes"]["blen"]
            runs = [i for i in counts if x[i - 1] == d]
            if p[1] == "delim_is_run_byte":
                ok = {0, 1, 255} <= {int(x[i]) for i in runs} | {255} and any(int(x[i]) == d for i in runs)
            elif p[1] == "count_value_not_counted":
                ok = any(x[i] == d and x[i - 1] != d for i in counts)
            elif p[1] == "only_count":
                ok = rec["count"] == 0 and sum(1 for i in counts if x[i] == d) >= 4 and (x == d).sum() == sum(1 for i in counts if x[i] == d) and \
                     all(any(st[i] == 4 and x[i] == d for i in _seam_idx(k, n)) for k in ("thread", "wave", "tile")) and st[n - 1] == 4
            elif p[1] == "last":
                lastb = st[n - 1] != 4 and x[n - 1] == d
                ok = {"literal": lastb and rec["last"], "run": st[n - 1] == 4 and x[n - 1] > 0 and rec["last"],
                      "run0": st[n - 1] == 4 and x[n - 1] == 0 and rec["last"], "other": not rec["last"]}[p[2]]
            elif p[1] == "straddle":
                ok = any(any(i - 4 < s_ <= i for s_ in _seam_idx(p[2], n)) and x[i] >= 2 for i in runs)
            elif p[1] == "tile_first":
                ok = any(x[t0] == d and st[t0] != 4 for t0 in range(TILE, n, TILE))
            elif p[1] == "tile_last":
                ok = any(x[t0 - 1] == d and st[t0 - 1] != 4 for t0 in range(TILE, n, TILE))
            elif p[1] == "delim":
                ok = d == int(p[2])
        if ok is None:
            raise KeyError(w)
        if not ok:
            bad.append(w)
    return bad
