"""Last columns that drive MTF + RLE2 (banzai_amd/csrc/mtf.hip: mtf_tile_last, mtf_prefix, mtf_walk_par) to every list,
chunk and tile edge at both tile sizes, each with the facts it was built to reach -- facts of tests/mtf_paths_model.py's
record, so the CPU test and the GPU test can both show that a builder still gets there before anything is compared.

A case is (name, col, has_byte, TL, want): `col` the column (bytes), `has_byte` uint8[256], TL the tile the case is meant
for (2,048: one block through the stage seam; 4,096: a batch of 64 blocks and more through bzh_mtf_batch) and `want` maps a
fact to what the record must show (see unmet()).  FAMILIES groups the case names; case(name) builds one (cached),
analysed(name) adds the model's outputs and record.  Every column is under 100,000 bytes, so 64 of them fit a level-1
context, except the one that needs more than 256 tiles.  The batch family is batch_list(count): lists of 63, 64 and 65
columns for one call, cases of the other families among columns of 1 byte to a whole level-1 block.

What no column reaches, and why (UNREACHED; the cases stay in the lists with what they do reach):
  * a previous occurrence at lane 33 seen from lane 34: two run heads in a row never hold the same symbol (the second one
    differs from the byte before it, which still is the first one's symbol); and lane 61 lies above lane 34.
  * position 255 beside position 1 in one word of `hist`: a word holds positions 2w and 2w + 1, so 1 shares word 0 with
    position 0, which no run head has, and 255 shares word 127 with 254.  The case brings 254 beside 255 in word 127, and
    1 and 255 into one tile.
  * the second round of mtf_prefix (more than 256 tiles) with tiles of 4,096 bytes: 1,048,577 bytes, above the largest
    block (899,999).
  * a list update with an unseen name at place 64, 128 or 192 AND a new symbol lower in the same word: those places are
    bit 0 of their word.  The update runs over them with new symbols higher in the word.
  * scattered names (holes between the present bytes) with 256 names: every byte is present.
"""
import functools

import numpy as np

from tests import mtf_paths_model as mm

ALPHABETS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
FORMS = ("literal", "runs", "scattered")
TILES = (2048, 4096)
PLACE_EDGES = (63, 64, 127, 128, 191, 192, 255)
H_EDGES = (0, 1, 63, 64, 65, 128, 1024)
PREV_PAIRS = [(63, p) for p in (0, 30, 31, 32, 33, 61)] + [(34, p) for p in (0, 30, 31, 32)]
TILE_COUNTS = (1, 7, 8, 9, 15, 16, 17)
LAYOUT_K = tuple(range(1, 14))
LEVEL1_M = 99_999

UNREACHED = {
    "chunks_prev_L34_p33": "two run heads in a row never hold the same symbol",
    "chunks_prev_L34_p61": "a previous occurrence lies below its lane",
    "positions_255_beside_1_t2048": "positions 1 and 255 are in words 0 and 127 of hist",
    "positions_255_beside_1_t4096": "positions 1 and 255 are in words 0 and 127 of hist",
    "tiles_second_round_t4096": "more than 256 tiles of 4,096 bytes are more than the largest block",
}


def hb_of(*byte_sets):
    hb = np.zeros(256, dtype=np.uint8)
    for s in byte_sets:
        hb[np.asarray(list(s), dtype=np.int64)] = 1
    return hb


def literal(rng, n, letters, avoid=None):
    """n bytes over `letters`, no two neighbours equal (one letter: a run), the first one not `avoid`"""
    letters = np.asarray(letters, dtype=np.int64)
    k = letters.size
    a = rng.integers(0, k, n)
    if k > 1:
        if n and avoid is not None and letters[a[0]] == avoid:
            a[0] = (a[0] + 1) % k
        for i in range(1, n):
            if a[i] == a[i - 1]:
                a[i] = (a[i] + 1) % k
    return letters[a].astype(np.uint8)


def runny(rng, n, letters, mean):
    letters = np.asarray(letters, dtype=np.int64)
    lens = rng.geometric(1.0 / mean, int(2 * n / mean) + 64)
    while lens.sum() < n:
        lens = np.concatenate([lens, lens])
    vals = letters[rng.integers(0, letters.size, lens.size)]
    return np.repeat(vals, lens)[:n].astype(np.uint8)


def from_positions(positions, num_names):
    """the column over bytes 0..num_names-1 (all present) whose every byte is a run head at the given list position (>= 1)"""
    lst = list(range(num_names))
    out = []
    for r in positions:
        assert 1 <= r < num_names
        c = lst.pop(r)
        lst.insert(0, c)
        out.append(c)
    return np.array(out, dtype=np.uint8)


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts])


# ---- alphabet ---------------------------------------------------------------------------------------------------------
def _present(N, form, rng):
    if form != "scattered" or N == 256:
        return np.arange(N)
    if N == 1:
        return np.array([255])
    mid = np.sort(rng.choice(np.arange(1, 255), N - 2, replace=False))
    return np.concatenate([[0], mid, [255]]).astype(np.int64)


def _alphabet(TL, N, form):
    rng = np.random.default_rng(100_000 + 10 * N + FORMS.index(form) + TL)
    present = _present(N, form, rng)
    n = 2 * TL + 37
    want = dict(num_names=N, regs=(N + 63) // 64, ebits=max(1, (N - 1).bit_length()), ntile=3)
    used = present
    if form == "scattered" and N >= 3:
        used = np.delete(present, [1] + ([N // 2] if N >= 5 else []))  # present names that never occur
        want.update(never_occurs=present.size - used.size)
    if form == "scattered" and 1 < N < 256:
        want.update(holes=True)
    col = runny(rng, n, used, 3) if form == "runs" else literal(rng, n, used)
    if form == "literal" and N > 1:
        want.update(min_heads=n - 1)
    return col, hb_of(present), want


def _last_name(TL, N, when):
    """`first`: the last name is a run head in the first chunk, and the front of the list when tile 1 begins;
    `late`: it first occurs in tile 1, the keys of tile 2 hold it"""
    rng = np.random.default_rng(200_000 + 10 * N + TL + (when == "late"))
    others, last = np.arange(N - 1), N - 1
    if when == "first":
        t0 = _cat([last], literal(rng, TL - 2, others), [last])
        rest = _cat(literal(rng, TL // 2, others), literal(rng, TL // 2 + 37, np.arange(N)))
        want = dict(num_names=N, last_name_in_first_chunk=True, ntile=3)
    else:
        t0 = literal(rng, TL, others)
        rest = _cat(literal(rng, 100, others), [last], literal(rng, TL - 101 + 37, np.arange(N), avoid=last))
        want = dict(num_names=N, last_name_first_tile=1, ntile=3)
    return _cat(t0, rest), hb_of(range(N)), want


# ---- places (256 names; the list at block entry is the identity, so places are names there) ------------------------------
def _tail(rng, n, avoid):
    return literal(rng, n, np.arange(256), avoid=avoid)


def _places_edges(TL):
    rng = np.random.default_rng(301 + TL)
    head = np.array(PLACE_EDGES)
    return _cat(head, _tail(rng, 3000, 255)), hb_of(range(256)), dict(first_places=(0, list(PLACE_EDGES)), num_names=256)


def _places_unseen(TL):
    """chunk 0 holds new symbols below the word edges and none on them; the update moves the unseen names on the edges,
    and the next chunks take them"""
    rng = np.random.default_rng(302 + TL)
    low = [1, 2, 62, 65, 70, 126, 129, 140, 190, 193, 200, 254]
    c0 = np.array([low[i % len(low)] for i in range(64)])
    edges = np.array(PLACE_EDGES)
    col = _cat(c0, edges if c0[-1] != edges[0] else edges[::-1], _tail(rng, 3000, int(edges[-1])))
    return col, hb_of(range(256)), dict(update_unseen_at=list(PLACE_EDGES), num_names=256)


def _places_word(TL, w):
    rng = np.random.default_rng(310 + w + TL)
    letters = np.arange(64 * w + (1 if w == 0 else 0), 64 * w + 64)
    c0 = literal(rng, 64, letters)
    return _cat(c0, _tail(rng, 3000, int(c0[-1]))), hb_of(range(256)), dict(all_new_in_word=w, num_names=256)


def _places_64_new(TL, kind):
    rng = np.random.default_rng(320 + TL)
    c0 = np.arange(1, 65) if kind == "low" else rng.permutation(np.arange(3, 256, 4))
    return _cat(c0, _tail(rng, 3000, int(c0[-1]))), hb_of(range(256)), dict(nfirst=64, num_names=256)


def _places_single_first(TL):
    col = _cat(np.zeros(500), np.full(700, 5), np.full(TL, 9), np.full(300, 5))
    return col, hb_of([0, 5, 9, 200]), dict(single_first_lane0=True)


# ---- chunks --------------------------------------------------------------------------------------------------------------
def _chunks_H(TL, H):
    rng = np.random.default_rng(400 + H + TL)
    letters = np.arange(1, 40)
    half = np.zeros(1024, dtype=np.uint8)
    if H:
        hs = literal(rng, H, letters)
        half[:H] = hs
        half[H:] = hs[-1]
    col = _cat(half, literal(rng, 1500, letters, avoid=int(half[-1])), np.zeros(TL))
    return col, hb_of(range(40)), dict(H=H)


def _chunks_prev(TL, L, p):
    """one chunk of 64 run heads: lane L holds the symbol of lane p; from lane 63, lanes 40 and 50 hold one symbol too (a
    predecessor in the upper half of the mask, below the lane that counts)"""
    sym = np.arange(1, 65)
    if L <= p or L == p + 1:
        sym[L] = sym[0] if L > 1 else sym[L]  # (unreachable pair: the nearest thing, lane 0)
        want = dict(unreached=UNREACHED["chunks_prev_L%d_p%d" % (L, p)], prev=(L, 0))
    else:
        sym[L] = sym[p]
        want = dict(prev=(L, p))
        if L == 63:
            sym[50] = sym[40]
            want.update(prev2=(50, 40))
    rng = np.random.default_rng(410 + TL)
    return _cat(sym, literal(rng, 200, np.arange(100, 140))), hb_of(range(256)), want


def _chunks_seen_before(TL):
    rng = np.random.default_rng(420 + TL)
    return _cat(np.arange(1, 65), [5, 9, 70, 3], literal(rng, 300, np.arange(60, 90), avoid=3)), hb_of(range(256)), dict(seen_in_chunk_before=True)


def _chunks_clen(TL, r, head):
    rng = np.random.default_rng(430 + r + TL)
    clen = 48 + r if r else 64
    n = TL + 1024 + clen
    col = literal(rng, n, np.arange(1, 30))
    if not head:
        col[-1] = col[-2]
    return col, hb_of(range(30)), dict(half=(clen, bool(head)), ntile=2)


def _chunks_tile_of_one(TL, head):
    rng = np.random.default_rng(440 + TL)
    col = literal(rng, TL + 1, np.arange(1, 30))
    if not head:
        col[-1] = col[-2]
    return col, hb_of(range(30)), dict(half=(1, bool(head)), ntile=2)


# ---- positions -----------------------------------------------------------------------------------------------------------
def _positions_all(TL, r):
    N = {1: 2, 2: 3, 255: 256}[r]
    return from_positions([r] * (2 * TL + 9), N), hb_of(range(N)), dict(pos_count={r: TL}, pos_min=r, pos_max=r)


def _positions_beside(TL):
    pos = [255] * 300 + [254, 255] * 200 + [1] * 100 + [255] * 50
    return from_positions(pos, 256), hb_of(range(256)), dict(hist_word_both=[127], pos_min=1, pos_max=255,
                                                              unreached=UNREACHED["positions_255_beside_1_t%d" % TL])


# ---- sweeps (tiles of 4,096: two sweeps of the workgroup a tile) -----------------------------------------------------------
_SL = np.arange(1, 7)  # letters of the sweep cases; byte 0 is present too


def _sweeps(TL, kind):
    assert TL == 4096
    rng = np.random.default_rng(500 + len(kind))
    lit = lambda n, avoid=None: literal(rng, n, _SL, avoid=avoid)
    if kind == "sweep0_only":  # heads in sweep 0, a run into sweep 1 and on into the next tile
        a = lit(1000)
        col = _cat(a, np.full(TL - 1000 + 300, a[-1]), lit(500, avoid=int(a[-1])))
        want = dict(tile_sweeps={0: [0]}, not_head=[TL], ntile=2)
    elif kind == "sweep1_only":
        a = lit(TL)
        col = _cat(a, np.full(2148, a[-1]), lit(TL - 2148 + 700, avoid=int(a[-1])))
        want = dict(tile_sweeps={1: [1]}, first_sweep={1: 1}, ntile=3)
    elif kind == "both_run_across_2048":
        a = lit(TL + 2000)
        col = _cat(a, np.full(100, a[-1]), lit(2500, avoid=int(a[-1])))
        want = dict(tile_sweeps={1: [0, 1]}, not_head=[TL + 2048], ntile=3)
    elif kind == "no_head":
        a = lit(TL - 10)
        col = _cat(a, np.full(10 + TL + 5, a[-1]), lit(100, avoid=int(a[-1])))
        want = dict(no_head_tiles=[1], ntile=3)
    elif kind in ("head_on_2047", "head_on_2048", "head_on_0"):
        at = TL + int(kind.split("_")[-1])
        col = _cat(np.full(at, 3), np.full(2 * TL + 50 - at, 4))
        want = dict(head_at_tile_byte=[at - TL], tile_heads={1: 1}, ntile=3)
        if at - TL == 2048:
            want.update(first_sweep={1: 1})
    elif kind == "head_amid_2047_2048":  # the same bytes as heads among heads
        col = lit(2 * TL + 50)
        want = dict(head_at_tile_byte=[0, 2047, 2048], ntile=3)
    else:
        assert kind == "wave_first_bytes"
        col = np.repeat(lit(24), 512)[:3 * TL - 100]  # a head every 512 bytes and nowhere else
        want = dict(wave_first_heads=[0, 1, 2, 3], tile_sweeps={1: [0, 1]}, ntile=3)
    return col, hb_of(range(7)), want


# ---- tiles ---------------------------------------------------------------------------------------------------------------
_TLET = np.arange(1, 21)


def _tiles_count(TL, k):
    rng = np.random.default_rng(600 + k + TL)
    return runny(rng, k * TL - 5, _TLET, 8), hb_of(range(21)), dict(ntile=k, unrolled=(k // 8 * 8, k % 8))


def _tiles_far_key(TL):
    rng = np.random.default_rng(610 + TL)
    mid = runny(rng, 8 * TL, _TLET, 8)
    col = _cat([30, 1, 30, 2], runny(rng, TL - 4, _TLET, 8), mid, [30, 1, 30, 5, 40, 2, 40, 30])
    return col, hb_of(range(21), [30, 40]), dict(ntile=10, key_age=9, first_in_last_tile=True)


def _tiles_no_head_stretch(TL):
    rng = np.random.default_rng(620 + TL)
    a = runny(rng, 2 * TL - 7, _TLET, 8)
    b = runny(rng, TL + 100, _TLET, 8)
    if b[0] == a[-1]:
        b[0] = a[-1] % 20 + 1
    col = _cat(a, np.full(7 + 3 * TL + 11, a[-1]), b)
    return col, hb_of(range(21)), dict(no_head_tiles=[2, 3, 4], tile_has_head=[1, 5], ntile=7)


def _tiles_second_round(TL):
    """more than 256 tiles of 2,048 bytes, few heads a tile, and a run from tile 255 into tile 256"""
    rng = np.random.default_rng(630)
    if TL == 4096:  # not reachable: the column stays, with what it does reach
        return runny(rng, 17 * TL + 1, _TLET, 200), hb_of(range(21)), dict(rounds=1, ntile=18, unreached=UNREACHED["tiles_second_round_t4096"])
    n = 257 * TL + 1
    col = runny(rng, n, _TLET, 700)
    col[256 * TL - 40:256 * TL + 90] = 9
    col[256 * TL - 41] = 8
    col[256 * TL + 90] = 10
    assert n >= 524_289
    return col, hb_of(range(21)), dict(rounds=2, ntile=258, not_head=[256 * TL], tile_has_head=[255, 256])


# ---- layout (tiles of 4,096: what tests/test_gpu_mtf_emit.py drives at 2,048) -------------------------------------------------
def _layout_runs(TL, k, zi, edge):
    """zero runs of z = 2^k - 2, 2^k - 1, 2^k positions (the digit count steps at 2^k - 1) whose closing head lies just
    before, on and just after byte `edge` (2,048: the sweep edge; 4,096: the tile edge) of a tile"""
    assert TL == 4096
    z = ((1 << k) - 2, (1 << k) - 1, 1 << k)[zi]
    rng = np.random.default_rng(700 + 10 * k + zi + edge)
    parts, at, closing = [], 0, []
    prev = 0
    for delta in (-1, 0, 1):
        h = (edge + delta) % TL
        while h - z - at < 2:
            h += TL
        pre = literal(rng, h - z - at, np.arange(1, 6), avoid=prev)
        parts += [pre, np.full(z, pre[-1])]
        prev = int(pre[-1])
        at = h
        if z:
            closing.append((z, h % TL))
    parts.append(literal(rng, 100, np.arange(1, 6), avoid=prev))
    want = dict(closing=closing, head_at_tile_byte=[(edge + d) % TL for d in (-1, 0, 1)])
    if z:
        want.update(digits=[mm.run_digits(z)])
    return _cat(*parts), hb_of(range(6)), want


def _layout_end(TL, kind, n):
    rng = np.random.default_rng(800 + n)
    body = literal(rng, n - 1, np.arange(1, 10))
    if kind == "head_last":
        return _cat(body, [77]), hb_of(range(10), [77]), dict(trailing_run=0, head_at_block_byte=n - 1)
    if kind == "trailing_run":
        return _cat(body[:n // 2], np.full(n - n // 2, 77)), hb_of(range(10), [77]), dict(trailing_run=n - n // 2 - 1)
    assert kind == "no_head"
    return np.full(n, 7, dtype=np.uint8), hb_of([7, 9]), dict(heads=0, trailing_run=n)


# ---- registry ------------------------------------------------------------------------------------------------------------------
_BUILDERS = {}
FAMILIES = {}


def _add(family, name, TL, fn, *args):
    _BUILDERS[name] = (fn, TL, args)
    FAMILIES.setdefault(family, []).append(name)


for _TL in TILES:
    for _N in ALPHABETS:
        for _f in FORMS:
            _add("alphabet", "alphabet_%d_%s_t%d" % (_N, _f, _TL), _TL, _alphabet, _N, _f)
        if _N > 1:
            _add("alphabet", "alphabet_%d_lastfirst_t%d" % (_N, _TL), _TL, _last_name, _N, "first")
            _add("alphabet", "alphabet_%d_lastlate_t%d" % (_N, _TL), _TL, _last_name, _N, "late")
    _add("places", "places_edges_one_chunk_t%d" % _TL, _TL, _places_edges)
    _add("places", "places_unseen_at_edges_t%d" % _TL, _TL, _places_unseen)
    for _w in range(4):
        _add("places", "places_all_in_word%d_t%d" % (_w, _TL), _TL, _places_word, _w)
    _add("places", "places_64_new_low_t%d" % _TL, _TL, _places_64_new, "low")
    _add("places", "places_64_new_spread_t%d" % _TL, _TL, _places_64_new, "spread")
    _add("places", "places_single_first_t%d" % _TL, _TL, _places_single_first)
    for _H in H_EDGES:
        _add("chunks", "chunks_H%d_t%d" % (_H, _TL), _TL, _chunks_H, _H)
    _add("chunks", "chunks_seen_in_chunk_before_t%d" % _TL, _TL, _chunks_seen_before)
    for _r in range(16):
        for _h in (1, 0):
            _add("chunks", "chunks_clen_r%d_%s_t%d" % (_r, "head" if _h else "nohead", _TL), _TL, _chunks_clen, _r, _h)
    for _h in (1, 0):
        _add("chunks", "chunks_tile_of_one_byte_%s_t%d" % ("head" if _h else "nohead", _TL), _TL, _chunks_tile_of_one, _h)
    for _r in (1, 2, 255):
        _add("positions", "positions_all_%d_t%d" % (_r, _TL), _TL, _positions_all, _r)
    _add("positions", "positions_255_beside_1_t%d" % _TL, _TL, _positions_beside)
    for _k in TILE_COUNTS:
        _add("tiles", "tiles_%d_t%d" % (_k, _TL), _TL, _tiles_count, _k)
    _add("tiles", "tiles_far_key_t%d" % _TL, _TL, _tiles_far_key)
    _add("tiles", "tiles_no_head_stretch_t%d" % _TL, _TL, _tiles_no_head_stretch)
    _add("tiles", "tiles_second_round_t%d" % _TL, _TL, _tiles_second_round)
for _L, _p in PREV_PAIRS + [(34, 33), (34, 61)]:
    _add("chunks", "chunks_prev_L%d_p%d" % (_L, _p), 2048 if (_L + _p) % 2 else 4096, _chunks_prev, _L, _p)
SWEEP_KINDS = ("sweep0_only", "sweep1_only", "both_run_across_2048", "no_head", "head_on_2047", "head_on_2048", "head_on_0",
               "head_amid_2047_2048", "wave_first_bytes")
for _kind in SWEEP_KINDS:
    _add("sweeps", "sweeps_" + _kind, 4096, _sweeps, _kind)
for _edge in (2048, 4096):
    for _k in LAYOUT_K:
        for _zi in range(3):
            _add("layout", "layout_k%d_z%d_edge%d" % (_k, _zi, _edge), 4096, _layout_runs, _k, _zi, _edge)
for _kind in ("head_last", "trailing_run", "no_head"):
    for _n in (4096, 4097, 2 * 4096 + 2049):
        _add("layout", "layout_%s_n%d" % (_kind, _n), 4096, _layout_end, _kind, _n)

NAMES = [n for fam in FAMILIES.values() for n in fam]
LONG = "tiles_second_round_t2048"  # the one column above a level-1 block


@functools.lru_cache(maxsize=None)
def case(name):
    fn, TL, args = _BUILDERS[name]
    col, hb, want = fn(TL, *args)
    col = np.ascontiguousarray(col, dtype=np.uint8)
    assert 1 <= col.size <= (LEVEL1_M if name != LONG else 899_999), (name, col.size)
    return name, col.tobytes(), hb, TL, want


@functools.lru_cache(maxsize=None)
def analysed(name):
    """-> (case, (syms, m, freqs, num_syms), record)"""
    c = case(name)
    s, m, f, ns, rec = mm.analyse(c[1], c[2], c[3])
    return c, (s, m, f, ns), rec


def names_at(TL):
    return [n for n in NAMES if _BUILDERS[n][1] == TL]


# ---- the batch family: lists of columns for one call ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_list(count):
    """`count` columns for one bzh_mtf_batch call on a level-1 context: cases of the other families in mixed order,
    lengths from 1 byte to the largest block side by side, another alphabet from neighbour to neighbour.  batch_list(63)
    and batch_list(64) are the first columns of batch_list(65)."""
    rng = np.random.default_rng(900)
    picks = [n for n in NAMES if n != LONG]
    picks = [picks[int(i)] for i in rng.permutation(len(picks))[:48]]
    cols = [(case(n)[1], case(n)[2]) for n in picks]
    for k, n in enumerate((1, 2, 3, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, LEVEL1_M, 70_001)):
        N = (2, 256, 65, 3, 129, 17, 193, 64)[k % 8]
        c = runny(rng, n, np.arange(N), (1, 3, 40)[k % 3])
        cols.insert(3 * k + 1, (c.tobytes(), hb_of(range(N))))
    assert len(cols) == 65
    out = cols[:count]
    return out


def unmet(rec, want):
    """the wanted facts that the record does not show, as a list of strings (empty: the case reaches its edge)"""
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(what)

    TL = rec["TL"]
    chunks, tiles, hp = rec["chunks"], rec["tiles"], rec["head_pos"]
    is_head = lambda p: bool(hp.size) and bool(hp[min(np.searchsorted(hp, p), hp.size - 1)] == p)
    for k, v in want.items():
        if k == "unreached":
            need(isinstance(v, str) and v, "an unreached fact needs its reason")
        elif k in ("num_names", "regs", "ebits", "ntile", "rounds", "trailing_run", "heads", "pos_min", "pos_max"):
            need(rec[k] == v, "%s: %r, wanted %r" % (k, rec[k], v))
        elif k == "never_occurs":
            need(int((rec["first_tile"] < 0).sum()) == v, "names that never occur: %d, wanted %d" % (int((rec["first_tile"] < 0).sum()), v))
        elif k == "holes":
            pass  # (a fact of has_byte, checked where the case is built: test_mtf_paths_model.py)
        elif k == "min_heads":
            need(rec["heads"] >= v, "heads: %d, wanted %d" % (rec["heads"], v))
        elif k == "last_name_in_first_chunk":
            need(bool(chunks) and chunks[0][0] == 0 and rec["num_names"] - 1 in chunks[0][5], "the last name is no head of the first chunk")
        elif k == "last_name_first_tile":
            need(rec["first_tile"][rec["num_names"] - 1] == v, "the last name first occurs in tile %d" % rec["first_tile"][rec["num_names"] - 1])
        elif k == "first_places":
            need(set(v[1]) <= set(chunks[v[0]][5].tolist()), "chunk %d: new places %r" % (v[0], chunks[v[0]][5].tolist()))
        elif k == "update_unseen_at":
            for e in v:
                ok = any(c[6] and e < rec["num_names"] and e not in c[5] and ((c[5] >> 6) == (e >> 6)).any() and
                         (e & 63 == 0 or ((c[5] >> 6 == e >> 6) & (c[5] < e)).any()) for c in chunks)
                need(ok, "no list update with place %d unseen and a new symbol in its word" % e)
        elif k == "all_new_in_word":
            need(any(c[6] and c[3] and ((c[5] >> 6) == v).all() for c in chunks), "no updating chunk with all new symbols in word %d" % v)
        elif k == "nfirst":
            need(any(c[3] == v for c in chunks), "no chunk with %d first occurrences" % v)
        elif k == "single_first_lane0":
            need(any(c[3] == 1 and c[4][0] == -1 for c in chunks), "no chunk with one first occurrence, lane 0")
        elif k == "H":
            need(any(h[3] == v for h in rec["halves"]), "no half with %d run heads" % v)
        elif k in ("prev", "prev2"):
            need(any(c[2] > v[0] and c[4][v[0]] == v[1] for c in chunks), "no lane %d with its previous occurrence at lane %d" % v)
        elif k == "seen_in_chunk_before":
            need(any(c[7] for c in chunks), "no symbol new in a chunk that the chunk before held")
        elif k == "half":
            need(any(h[2] == v[0] and h[4] == v[1] for h in rec["halves"]), "no half of %d bytes, last byte head: %r" % v)
        elif k == "pos_count":
            for pos, cnt in v.items():
                need(rec["max_in_tile"][pos] == cnt, "position %d: at most %d in a tile, wanted %d" % (pos, rec["max_in_tile"][pos], cnt))
        elif k == "hist_word_both":
            need(set(v) <= rec["hist_words_both"], "words with both counters in use: %r" % sorted(rec["hist_words_both"]))
        elif k == "tile_sweeps":
            for t, s in v.items():
                need(tiles[t]["sweeps"] == s, "tile %d: heads in sweeps %r, wanted %r" % (t, tiles[t]["sweeps"], s))
        elif k == "first_sweep":
            for t, s in v.items():
                need(tiles[t]["first_sweep"] == s, "tile %d: first head found in sweep %r" % (t, tiles[t]["first_sweep"]))
        elif k == "tile_heads":
            for t, s in v.items():
                need(tiles[t]["heads"] == s, "tile %d: %d heads" % (t, tiles[t]["heads"]))
        elif k == "not_head":
            for p in v:
                need(not is_head(p) and hp.size and hp[0] < p < hp[-1], "byte %d is a head, or no run crosses it" % p)
        elif k == "no_head_tiles":
            need(set(v) <= set(rec["no_head_tiles"]), "tiles without a head: %r" % rec["no_head_tiles"])
        elif k == "tile_has_head":
            need(all(tiles[t]["heads"] > 0 for t in v), "a tile of %r has no head" % (v,))
        elif k == "head_at_tile_byte":
            need(set(v) <= rec["head_at_tile_byte"], "no head on tile bytes %r" % sorted(set(v) - rec["head_at_tile_byte"]))
        elif k == "head_at_block_byte":
            need(is_head(v), "byte %d is no head" % v)
        elif k == "wave_first_heads":
            need(set(v) <= rec["wave_first_heads"], "wavefronts with a head on their first byte: %r" % sorted(rec["wave_first_heads"]))
        elif k == "unrolled":
            need((rec["unrolled_tiles"], rec["remainder_tiles"]) == v, "prefix: %d tiles unrolled, %d after" % (rec["unrolled_tiles"], rec["remainder_tiles"]))
        elif k == "key_age":
            need(int(rec["key_age"].max()) >= v, "oldest key: %d tiles, wanted %d" % (int(rec["key_age"].max()), v))
        elif k == "first_in_last_tile":
            need(rec["ntile"] > 1 and (rec["first_tile"] == rec["ntile"] - 1).any(), "no name first seen in the last tile")
        elif k == "closing":
            need(set(v) <= rec["closing"], "runs and closing heads missing: %r" % sorted(set(v) - rec["closing"]))
        elif k == "digits":
            need(set(v) <= rec["digit_counts"], "digit counts %r, wanted %r" % (sorted(rec["digit_counts"]), v))
        else:
            raise KeyError(k)
    return bad
