"""The layout the inverse-RLE1 kernels work from (banzai_amd/csrc/decode.hip, ur_load to unrle_select), restated in NumPy so that a
test can say which thread of which tile meets which byte in which state -- and prove that a case built for an edge reaches it.

analyse(x, ...) -> a record (dict) of a block `x` (the bytes behind the inverse BWT):
  tiles    a dict a tile: entry (state its first byte is met in), map (where each of the five states has got to behind it), total,
           toff, staged, and head / words / tail of its ur_copy_out at obase + toff
  threads  arrays of (tiles, 256): cnt, prev, state, outn, off
  bytes    arrays of n: state (the state byte i is met in), blen / bbyte (what it stands for), pos (where that begins)
  end      (tile, thread, state) of the endstate writer
  out      the block's expansion as this layout places it, image the same behind `obase` bytes of 0xA5
  tcount / last / select(k)   with a delimiter: delimiters a tile, the last-byte flag, the position of the k-th (1-based)
  windows / pieces            the cuts of every window and piece a tile, with the route the tile takes

The bytes are not taken from here: tests compare `out` with bz2_handbuilt.unrle and with Python's bz2.  The library under test is
never called.  `variant` switches one deliberate mistake on (VARIANTS): the CPU tests show that the case list tells each from the truth.
One assumption is the model's own: ur_copy_out's word store lands on the word that holds its address (the two low address bits do
not count), so a head of the wrong length moves bytes."""
import numpy as np

UR_THREADS, UR_ITEMS, UR_TILE, UR_STAGE = 256, 16, 4096, 8192
PIECE_WAVES = UR_THREADS // 64  # fewer pieces than this on a staged tile: the workgroup copies each; otherwise a wavefront a piece
WAVE = 64 * UR_ITEMS            # bytes of a tile that one wavefront loads
GUARD = 0xA5

VARIANTS = {
    "no_wave_carry": "ur_scan: the carry across wavefronts is dropped (a thread composes its own wavefront only)",
    "chain_le": "unrle_walk<false>: the tile chain composes the maps of tiles <= t instead of < t",
    "chain_one_wave": "unrle_walk<false>: the chain's total is the first wavefront's (64 tiles) alone",
    "no_prev": "ur_load: prev is not loaded at a thread's first byte",
    "stale_behind_n": "ur_load: the thread that holds the block's end takes the bytes behind n for its own (cnt = 16)",
    "count_eq_run": "the byte behind a count byte is compared with the run byte and goes on with its run when equal",
    "stage_one_more": "the staged / unstaged split: a tile of UR_STAGE + 1 bytes is staged, and its last byte finds no room",
    "head_residue": "ur_copy_out: the head is the address's residue, not what is missing to the next word",
    "count_is_delim": "bzd_ur_count: a count byte equal to the delimiter is counted",
    "end_from_full_thread": "the endstate writer is the last thread with 16 bytes, not the one that holds the last byte",
}

_ID = np.arange(5, dtype=np.int64)


def _step(s, eq, eq_run=None):
    """bzd_rl_step on arrays; eq_run: the count_eq_run variant's comparison (state 0 behind a count byte)"""
    r = np.where(s == 4, 0, np.where(eq & (s >= 1), s + 1, 1))
    if eq_run is not None:
        r = np.where((s == 0) & eq_run, 2, r)
    return r


def copy_out(g, n, variant=None):
    """ur_copy_out's split of n bytes at address g -> (head, words, tail)"""
    head = min(n, (g & 3) if variant == "head_residue" else ((-g) & 3))
    words = (n - head) // 4
    return head, words, n - head - 4 * words


def _copy_bytes(image, g, src, variant):
    head, words, tail = copy_out(g, len(src), variant)
    image[g:g + head] = src[:head]
    for i in range(words):  # (only misaligned under the variant: the store lands on the word that holds its address)
        a = (g + head + 4 * i) & ~3
        image[a:a + 4] = src[head + 4 * i:head + 4 * i + 4]
    t0 = head + 4 * words
    image[g + t0:g + t0 + tail] = src[t0:]


def analyse(x, obase=0, windows=(), pieces=(), delim=None, variant=None, behind=0xFF):
    """x: the block; obase: where its first output byte goes (an address: its residue mod 4 is what counts); windows: (lo, hi, dst)
    in the block's output, dst = the address of byte lo; pieces: (lo, hi, base) likewise; behind: the byte value that lies behind
    x in its slot (read by the stale_behind_n variant alone)"""
    assert variant is None or variant in VARIANTS
    xb = np.frombuffer(bytes(x), dtype=np.uint8)
    n = xb.size
    assert n >= 1
    T = (n + UR_TILE - 1) // UR_TILE
    N = T * UR_THREADS
    X = np.full(N * UR_ITEMS, behind, dtype=np.int64)
    X[:n] = xb
    i0 = np.arange(N, dtype=np.int64) * UR_ITEMS
    cnt = np.clip(n - i0, 0, UR_ITEMS)
    holder = (n - 1) // UR_ITEMS  # the thread (counted over the block) that holds the last byte
    taken = cnt.copy()            # bytes a thread walks
    if variant == "stale_behind_n":
        taken[holder] = UR_ITEMS
    prev = np.where((cnt > 0) & (i0 > 0), X[np.maximum(i0 - 1, 0)], 256)
    if variant == "no_prev":
        prev = np.full(N, 256, dtype=np.int64)
    B = X.reshape(N, UR_ITEMS)
    before = np.concatenate([prev[:, None], B[:, :-1]], axis=1)
    eq = B == before
    eq_run = None
    if variant == "count_eq_run":
        two = np.concatenate([[256, 256], X[:-2]]).reshape(N, UR_ITEMS)
        eq_run = B == two
    valid = np.arange(UR_ITEMS)[None, :] < taken[:, None]

    # bzd_ur_map: a thread's bytes as a map of states
    m = np.tile(_ID, (N, 1))
    for k in range(UR_ITEMS):
        new = _step(m, eq[:, k:k + 1], None if eq_run is None else eq_run[:, k:k + 1])
        m = np.where(valid[:, k:k + 1], new, m)

    # ur_scan: composition in lane order inside a wavefront, the wavefronts' totals through LDS
    def scan(maps):  # maps (G, 4, 64, 5) -> (exclusive map a thread, total a group)
        G = maps.shape[0]
        inc = np.empty_like(maps)
        inc[:, :, 0] = maps[:, :, 0]
        for l in range(1, 64):
            inc[:, :, l] = np.take_along_axis(maps[:, :, l], inc[:, :, l - 1], axis=-1)  # compose(first, then) = then[first]
        ex = np.empty_like(maps)
        ex[:, :, 0] = _ID
        ex[:, :, 1:] = inc[:, :, :-1]
        carry = np.tile(_ID, (G, 1))
        out = np.empty_like(maps)
        for w in range(UR_THREADS // 64):
            c = np.tile(_ID, (G, 1)) if variant == "no_wave_carry" else carry
            out[:, w] = np.take_along_axis(ex[:, w], np.broadcast_to(c[:, None, :], (G, 64, 5)), axis=-1)
            carry = np.take_along_axis(inc[:, w, 63], carry, axis=-1)
        return out.reshape(G, UR_THREADS, 5), carry

    ex, tmap = scan(m.reshape(T, UR_THREADS // 64, 64, 5))

    # the tile chain of unrle_walk<false>: thread j < t holds tile j's map, the same scan's total applied to state 0
    entry = np.zeros(T, dtype=np.int64)
    acc = _ID.copy()
    for t in range(T):
        upto = acc
        if variant == "chain_le":
            upto = tmap[t][acc]
        entry[t] = upto[0]
        if not (variant == "chain_one_wave" and t >= 64):
            acc = tmap[t][acc]
    state0 = ex[np.arange(T)[:, None], np.arange(UR_THREADS)[None, :], entry[:, None]].reshape(N)

    # bzd_ur_size and what bzd_ur_emit / bzd_ur_count make of the same walk
    s = state0.copy()
    bstate = np.zeros((N, UR_ITEMS), dtype=np.int64)
    blen = np.zeros((N, UR_ITEMS), dtype=np.int64)
    bbyte = np.zeros((N, UR_ITEMS), dtype=np.int64)
    for k in range(UR_ITEMS):
        v = valid[:, k]
        bstate[:, k] = s
        blen[:, k] = np.where(v, np.where(s == 4, B[:, k], 1), 0)
        bbyte[:, k] = np.where(s == 4, before[:, k], B[:, k])
        s = np.where(v, _step(s, eq[:, k], None if eq_run is None else eq_run[:, k]), s)
    s_end = s
    outn = blen.sum(axis=1)
    o2 = outn.reshape(T, UR_THREADS)
    off = np.cumsum(o2, axis=1) - o2
    total = o2.sum(axis=1)
    toff = np.cumsum(total) - total
    bsize = int(total.sum())
    staged = total <= UR_STAGE + (variant == "stage_one_more")

    writer = holder
    if variant == "end_from_full_thread":
        full = np.nonzero(cnt == UR_ITEMS)[0]
        writer = int(full[-1]) if full.size else 0
    end = (writer // UR_THREADS, writer % UR_THREADS, int(s_end[writer]))

    # where every byte's expansion begins, and the expansion as the layout places it
    flat_len = blen.reshape(-1)
    within = np.cumsum(blen, axis=1) - blen
    pos = (np.repeat(toff, UR_THREADS) + off.reshape(-1))[:, None] + within
    flat_pos = pos.reshape(-1)
    starts = np.cumsum(flat_len) - flat_len
    nout = int(flat_len.sum())
    where = np.repeat(flat_pos, flat_len) + (np.arange(nout) - np.repeat(starts, flat_len))
    vals = np.repeat(bbyte.reshape(-1), flat_len).astype(np.uint8)
    lim = np.repeat(np.repeat(toff + total, UR_TILE), flat_len)  # p.lim: no position at or behind the tile's end
    keep = where < lim
    plain = np.zeros(bsize, dtype=np.uint8)
    plain[where[keep]] = vals[keep]
    image = np.full(obase + bsize + 4, GUARD, dtype=np.uint8)
    tiles = []
    for t in range(T):
        g, tt = obase + int(toff[t]), int(total[t])
        rec = dict(entry=int(entry[t]), map=tuple(int(v) for v in tmap[t]), total=tt, toff=int(toff[t]), staged=bool(staged[t]),
                   head=None, words=None, tail=None)
        if tt and staged[t]:
            rec["head"], rec["words"], rec["tail"] = copy_out(g, tt, variant)
            src = plain[toff[t]:toff[t] + tt].copy()
            src[UR_STAGE:] = 0  # (nothing is staged behind the stage; no tile gets here but under stage_one_more)
            _copy_bytes(image, g, src, variant)
        elif tt:
            image[g:g + tt] = plain[toff[t]:toff[t] + tt]
        tiles.append(rec)
    r = dict(n=n, T=T, bsize=bsize, tiles=tiles, end=end, variant=variant, obase=obase,
             threads=dict(cnt=cnt.reshape(T, UR_THREADS), prev=prev.reshape(T, UR_THREADS), state=state0.reshape(T, UR_THREADS),
                          outn=o2, off=off),
             bytes=dict(state=bstate.reshape(-1)[:n], blen=flat_len[:n], bbyte=bbyte.reshape(-1)[:n], pos=flat_pos[:n]),
             x=xb, out=image[obase:obase + bsize].tobytes(), image=image)

    if delim is not None:
        here = np.where(bbyte == delim, blen, 0)
        if variant == "count_is_delim":
            here = here + ((bstate == 4) & (B == delim) & valid)
        r["delim"] = delim
        r["tcount"] = here.reshape(T, -1).sum(axis=1)
        r["count"] = int(here.sum())
        r["last"] = bool(bbyte.reshape(-1)[n - 1] == delim)  # (a closing count of 0 leaves the byte of its run)
        cum = np.cumsum(here.reshape(-1))

        def select(k):
            """the position of the k-th delimiter of the block (1-based), as unrle_select finds it: the tile by the tiles' counts,
            the thread by the exclusive sum, the byte by bzd_ur_select"""
            i = int(np.searchsorted(cum, k))
            return int(flat_pos[i] + k - (cum[i] - here.reshape(-1)[i]) - 1)
        r["select"] = select

    def cuts(lo, hi, dst):
        met = []
        for t in range(T):
            tt, to = int(total[t]), int(toff[t])
            a, b = max(to, lo), min(to + tt, hi)
            if tt == 0 or b <= a:
                continue
            g = dst + (a - lo)
            head, words, tail = copy_out(g, b - a, variant) if staged[t] else (None, None, None)
            met.append(dict(tile=t, tlo=a - to, thi=b - to, staged=bool(staged[t]), g=g, head=head, words=words, tail=tail))
        return met

    r["windows"] = [dict(lo=lo, hi=hi, dst=dst, cuts=cuts(lo, hi, dst)) for lo, hi, dst in windows]
    pc = [dict(lo=lo, hi=hi, base=base, cuts=cuts(lo, hi, base)) for lo, hi, base in pieces]
    r["pieces"] = pc
    met = [sum(1 for p in pc if any(c["tile"] == t for c in p["cuts"])) for t in range(T)]
    r["piece_routes"] = [None if m == 0 else ("unstaged" if not staged[t] else ("workgroup" if m < PIECE_WAVES else "wave"))
                         for t, m in enumerate(met)]
    r["pieces_met"] = met
    return r
