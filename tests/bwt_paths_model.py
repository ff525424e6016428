"""Which path the suffix sort takes for a block: a CPU statement of the decisions banzai_amd/csrc/bwt.hip and bwt_msd.h make
on the device (numpy only).  The oracle judges the output bytes; this model says which branch every block must take, so
that a test can build inputs on both sides of each threshold and a trace (BZH_TRACE_ROUNDS) can show that they got there.

Decisions restated here:
  * the batch rule (bwt.hip, SortAttempt: use_msd): level >= 2 (M >= MS_MIN_N) and a batch of at least 12 blocks, or
    BZH_INIT=msd; BZH_INIT=lsd keeps every block on the 8 passes;
  * period_detect: a near-periodic block is sorted as m of its periods plus the remainder (n' = m p + r);
  * bigram_plan: the sample test (n >= 32768: 4096 sampled 8-byte cyclic prefixes, at least half of them distinct), at most
    MS_NE_MAX non-empty cyclic 2-byte buckets, at most MS_OVER_PCT % of the suffixes in 2-byte buckets of more than MS_TILE
    (not under BZH_INIT=msd), and the greedy packing of the buckets into units (MS_TILE suffixes, 256 buckets);
  * seg_plan, levels L = 1..5: an oversized bucket of level L is an (L+1)-byte prefix of more than MS_TILE rotations, split
    by the next byte into units or level L+1 buckets; a 7-byte prefix of more than MS_TILE rotations "spans" (its tiles become
    units of one group each);
  * the depth the doubling rounds start from: 7 bytes after the bucket-first sort (bwt_msd.h), 8 after the 8 passes (bwt.hip,
    eight_passes / round_begin), and the groups at that depth: large ones (more than TAIL_G members) go to the big list, whose
    numbering runs out beyond GID_MAX groups ("on ranks"); a big list of more than 250,000 records takes five passes; a block
    with small groups only takes the depth x4 form when its small-group records times QUAD_DIV are below n.
"""
import numpy as np

MS_TILE = 8192
MS_NE_MAX = 8192
MS_SAMPLES = 4096
MS_OVER_PCT = 35
MS_MIN_N = 131072
MS_LEVELS = 5
UNIT_BUCKETS = 256      # buckets one unit of bigram_plan holds (the bucket index is one 8-bit digit)
BATCH_MIN = 12          # blocks a batch needs for the bucket-first sort (without BZH_INIT=msd)
DEPTH_MSD = 2 + MS_LEVELS  # bytes the bucket-first sort orders by
DEPTH_8PASS = 8            # bytes the 8 passes order by
TAIL_G = 64
GID_MAX = 4096
FOUR_PASS_MAX = 250000
QUAD_DIV = 10
SWEEP_DIV = 256
PD_PMAX, PD_M, PD_MINLEN = 8192, 8, 64


def _u8(x):
    return np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else x.astype(np.uint8, copy=False)


def _dense(key):
    """dense lexicographic ranks of a key array"""
    _, inv = np.unique(key, return_inverse=True)
    return inv.reshape(-1).astype(np.int64)


def prefix_ranks(x, h):
    """rank of every rotation's cyclic h-byte prefix (equal prefixes, equal ranks; lexicographic), by prefix doubling"""
    a = _u8(x)
    n = a.size
    idx = np.arange(n)
    r = _dense(a.astype(np.int64))
    k = 1
    # powers of two up to h, then one more combination for the rest
    while 2 * k <= h:
        r = _dense(r * (int(r.max()) + 1) + r[(idx + k) % n])
        k *= 2
    if k < h:
        rest = prefix_ranks(a, h - k)
        r = _dense(r * (int(rest.max()) + 1) + rest[(idx + k) % n])
    return r


def group_sizes(x, h):
    """sizes of the groups of rotations with equal cyclic h-byte prefixes (any order)"""
    if _u8(x).size == 0:
        return np.zeros(0, np.int64)
    return np.bincount(prefix_ranks(x, h))


def group_stats(x, h):
    """large groups (> TAIL_G members) and their records, records of small groups (2..TAIL_G), groups in all, at depth h"""
    c = group_sizes(x, h)
    big = c > TAIL_G
    small = (c >= 2) & ~big
    return {"groups": int(c.size), "large": int(big.sum()), "big_records": int(c[big].sum()), "small_records": int(c[small].sum())}


def period_shrink(x):
    """period_detect (bwt.hip): the length the sort sees -- m p + r for a block of k > m + 1 periods p with r != 0, else n"""
    a = _u8(x)
    n = a.size
    if n < 20 * 16:
        return n
    pmax = min(PD_PMAX, n // (PD_M + 2))
    head = a[:16].tobytes()
    lower = 1
    for _ in range(4):
        p = None
        for q in range(lower, pmax + 1):
            if a[q:q + 16].tobytes() == head:
                p = q
                break
        if p is None:
            return n
        if np.array_equal(a[:n - p], a[p:]):
            k, r = divmod(n, p)
            m = max(PD_M, -(-PD_MINLEN // p))
            if r == 0 or k < m + 2:
                return n
            return m * p + r
        lower = p + 1
    return n


def sample_distinct(x):
    """bigram_plan's sample test: distinct values among the 4096 sampled 8-byte cyclic prefixes (as its hash set counts them)"""
    a = _u8(x)
    n = a.size
    stride = n // MS_SAMPLES
    pos = np.arange(MS_SAMPLES, dtype=np.int64) * stride
    v = np.zeros(MS_SAMPLES, np.uint64)
    for q in range(8):
        v |= a[(pos + q) % n].astype(np.uint64) << np.uint64(8 * q)
    v ^= np.uint64(0xA5A5A5A5A5A5A5A5)
    v[v == 0] = 1
    return int(np.unique(v).size)


def _pack(counts, tile, unit_buckets):
    """greedy packing of bigram_plan / seg_plan over buckets in order: -> (units, sizes of the oversized buckets)"""
    units, over_sizes = 0, []
    is_open, pover, ubase, uidx, pos = False, False, 0, 0, 0
    i = 0
    for c in counts:
        c = int(c)
        if c == 0:
            continue
        over = c > tile
        if not is_open or over or pover or pos + c - ubase > tile or (unit_buckets and i - uidx >= unit_buckets):
            if over:
                over_sizes.append(c)
            else:
                units += 1
            ubase, uidx, is_open = pos, i, True
        pover = over
        pos += c
        i += 1
    return units, over_sizes


def block_plan(x, force_new=False, tile=MS_TILE, ne_max=MS_NE_MAX):
    """What bigram_plan and seg_plan decide for one block (as the sort sees it, i.e. after period_shrink).
    -> dict: n, distinct (sample test, None below 32768), ne, bigall, np (bucket-first), units, over[L] and tiles[L] for
    L = 1..5 (index 0 unused), spans, deeper (a level-2 bucket exists: levels 2-5 run), units_level[0..5]"""
    a = _u8(x)
    n = a.size
    out = {"n": n, "distinct": None, "ne": 0, "bigall": 0, "np": False, "units": 0, "over": [0] * (MS_LEVELS + 1),
           "tiles": [0] * (MS_LEVELS + 1), "spans": False, "deeper": False, "units_level": [0] * (MS_LEVELS + 1)}
    if n == 0 or (n + 15) // 16 + 16 >= 65536:
        return out
    if n >= 32768:
        out["distinct"] = sample_distinct(a)
        if out["distinct"] * 2 < MS_SAMPLES:
            return out
    bg = np.bincount(a.astype(np.int64) * 256 + np.roll(a, -1), minlength=65536)
    out["ne"] = int((bg != 0).sum())
    out["bigall"] = int(bg[bg > tile].sum())
    if out["ne"] > ne_max or (out["bigall"] * 100 > n * MS_OVER_PCT and not force_new):
        return out
    out["np"] = True
    u0, over = _pack(bg, tile, UNIT_BUCKETS)
    out["units_level"][0] = u0
    if over:
        rk = prefix_ranks(a, 2)
        for L in range(1, MS_LEVELS + 1):
            # level L: the (L+1)-byte prefixes of more than `tile` rotations, split by byte L+1
            cnt_parent = np.bincount(rk)
            big_parents = np.flatnonzero(cnt_parent > tile)
            out["over"][L] = int(big_parents.size)
            out["tiles"][L] = int(sum(-(-int(cnt_parent[p]) // tile) for p in big_parents))
            if not big_parents.size:
                break
            child = _dense(rk * 256 + a[(np.arange(n) + L + 1) % n])
            cc = np.bincount(child)
            par_of_child = np.zeros(cc.size, np.int64)
            par_of_child[child] = rk  # (non-decreasing: the children of a bucket are adjacent, in order of the next byte)
            for p in big_parents:
                kids = cc[np.searchsorted(par_of_child, p):np.searchsorted(par_of_child, p, side="right")]
                u, ov = _pack(kids, tile, 0)
                out["units_level"][L] += u
                if L == MS_LEVELS and ov:
                    out["spans"] = True
                    out["units_level"][L] += sum(-(-s // tile) for s in ov)  # one group, in tiles
            rk = child
    out["deeper"] = out["over"][2] > 0
    out["units"] = sum(out["units_level"])
    return out


def batch_plans(blocks, level, max_batch, init="default"):
    """bwt_batch over `blocks` in a context of this level and batch size: one dict per batch the sort runs --
    msd (the batch rule), per-block plans, and the totals the trace's initial-sort line prints"""
    M = 100000 * level - 1
    out = []
    for k0 in range(0, len(blocks), max_batch):
        part = blocks[k0:k0 + max_batch]
        B = len(part)
        msd = M >= MS_MIN_N and init != "lsd" and (B >= BATCH_MIN or init == "msd")
        plans = []
        for blk in part:
            a = _u8(blk)
            a = a[:period_shrink(a)]
            plans.append(block_plan(a, force_new=init == "msd") if msd else {"np": False, "n": a.size})
        tot = {"msd": msd, "plans": plans, "new": sum(p["np"] for p in plans), "old": sum(not p["np"] for p in plans)}
        if msd:
            tot["units"] = sum(p["units"] for p in plans if p["np"])
            tot["over"] = [sum(p["over"][L] for p in plans if p["np"]) for L in range(MS_LEVELS + 1)]
            tot["tiles"] = [sum(p["tiles"][L] for p in plans if p["np"]) for L in range(MS_LEVELS + 1)]
            tot["deeper"] = tot["over"][2] > 0
        out.append(tot)
    return out


def round0(x, msd):
    """what round_begin finds in round 0 for a block alone in its batch: depth, groups, big list, small list, SWEEP mode,
    whether the big list is numbered densely, and whether the small groups take the depth x4 form"""
    a = _u8(x)
    a = a[:period_shrink(a)]
    h = DEPTH_MSD if msd else DEPTH_8PASS
    g = group_stats(a, h)
    g["h"] = h
    g["sweep"] = (not msd) and g["groups"] * SWEEP_DIV < a.size
    g["on_ranks"] = g["large"] > GID_MAX
    g["quad"] = (not g["sweep"]) and g["big_records"] == 0 and g["small_records"] > 0 and g["small_records"] * QUAD_DIV < a.size
    g["passes_next"] = 4 if g["big_records"] <= FOUR_PASS_MAX else 5  # the passes round 1 launches (bounded by round 0's list)
    return g


# ---- edge families: two blocks each, one on either side ----------------------------------------------------------------

def _rng(seed):
    return np.random.default_rng(seed)


def phrase_copies(plen, copies, seed, tail=0):
    """`copies` copies of one random phrase (bytes 0..127) of `plen` bytes, each behind an 8-byte separator (bytes 128..255)
    whose first and whose last byte differ from every other separator's: every 8-byte window that reaches into a separator
    is unique, so the groups at depth 8 are exactly the plen - 7 windows of the phrase, `copies` members each (at depth 7:
    plen - 6).  `tail` random letters (16 of them: few 2-byte buckets) follow."""
    assert copies <= 128
    r = _rng(seed)
    phrase = r.integers(0, 128, plen, dtype=np.uint8)
    firsts = r.permutation(128)[:copies] + 128
    lasts = r.permutation(128)[:copies] + 128
    out = []
    for i in range(copies):
        sep = r.integers(128, 256, 8, dtype=np.uint8)
        sep[0], sep[-1] = firsts[i], lasts[i]
        out += [sep, phrase]
    out.append(_bg(r, tail))
    return np.concatenate(out).tobytes()


def _bg(r, n, lo=0x61, k=16):
    return r.integers(lo, lo + k, n, dtype=np.uint8)


def fam_sample_n(seed=1):
    """n = 32,767 / 32,768 of two 8-letter words in random order: the sample test (it only runs from 32,768 on) finds
    a handful of distinct prefixes -- bucket-first below the edge, 8 passes at it"""
    r = _rng(seed)
    w = [b"qwertyui", b"asdfghjk"]
    body = b"".join(w[int(i)] for i in r.integers(0, 2, 32768 // 8 + 1))
    return body[:32767], body[:32768]


def fam_sample_distinct(seed=2):
    """n = 65,536 (sample stride 16): the sampled positions hold D = 2,047 / 2,048 distinct 8-byte tokens, the rest is
    random letters -- 8 passes / bucket-first"""
    out = []
    for D in (2047, 2048):
        r = _rng(seed)
        a = _bg(r, 65536)
        toks = r.permutation(16 ** 4)[:D]
        for k in range(MS_SAMPLES):
            t = int(toks[k % D])
            a[k * 16:k * 16 + 8] = [0x41 + ((t >> (4 * j)) & 15) for j in (0, 1, 2, 3)] + [0x5A, 0x5A, 0x59, 0x58]
        out.append(a.tobytes())
    return tuple(out)


def _euler(edges, r):
    """a cyclic sequence whose cyclic bigrams are exactly the multiset `edges` (Hierholzer; the graph must be Eulerian)"""
    adj = {}
    for u, v in edges:
        adj.setdefault(u, []).append(v)
    for u in adj:
        r.shuffle(adj[u])
    start = edges[0][0]
    stack, path = [start], []
    while stack:
        u = stack[-1]
        if adj.get(u):
            stack.append(adj[u].pop())
        else:
            path.append(stack.pop())
    path.reverse()
    return bytes(path[:-1])


def fam_ne(seed=3):
    """NE = 8,192 / 8,193 non-empty cyclic 2-byte buckets: all 8,100 pairs of 90 letters plus 92 / 93 planted ones"""
    out = []
    for extra in (92, 93):
        r = _rng(seed)
        A = list(range(32, 122))
        edges = [(u, v) for u in A for v in A] * 2
        # planted: a -> z -> b for a new byte z adds two buckets; a -> z -> z -> b three
        k = 0
        singles = extra // 2 - (extra % 2)
        for j in range(singles):
            z = 128 + j
            edges += [(A[j], z), (z, A[j])]
            k += 2
        if extra % 2:
            z = 128 + singles
            edges += [(A[0], z), (z, z), (z, A[0])]
        seq = _euler(edges, r)
        out.append(seq)
    return tuple(out)


def fam_over_pct(seed=4):
    """n = 100,000: random letters and one run of byte 0xF0 whose 2-byte bucket holds 35,000 / 35,001 rotations:
    bigall * 100 = n * 35 / one past -- bucket-first / 8 passes (BZH_INIT=msd: bucket-first both)"""
    out = []
    for k in (35000, 35001):
        r = _rng(seed)
        bg = _bg(r, 100000 - k - 1, 0x61, 64)
        cut = bg.size // 2
        out.append(bg[:cut].tobytes() + b"\xf0" * (k + 1) + bg[cut:].tobytes())
    return tuple(out)


def fam_tile(L, seed=5):
    """an (L+2)-byte prefix W of 8,192 / 8,193 rotations (L = 0: a 2-byte bucket) inside an (L+1)-byte prefix of more than
    MS_TILE (W with another last byte, 100 times): level L+1 has one oversized bucket more (L = 5: the block spans)"""
    out = []
    for c in (8192, 8193):
        r = _rng(seed + L)
        W = bytes(range(0xC0, 0xC0 + L + 2))
        W2 = W[:-1] + b"\xfe"
        items = [W] * c + ([W2] * 100 if L else [])
        order = r.permutation(len(items))
        gaps = r.integers(8, 25, len(items))  # (random letters between: under 35 % of the suffixes in oversized 2-byte buckets)
        parts = []
        for j, i in enumerate(order):
            parts.append(items[i])
            parts.append(_bg(r, int(gaps[j]), 0x61, 64).tobytes())
        out.append(b"".join(parts))
    return tuple(out)


def fam_unit_width(seed=6):
    """256 / 257 non-empty 2-byte buckets, 5,120 / 5,140 suffixes in all: one unit / two (256 buckets a unit)"""
    out = []
    for extra in (False, True):
        r = _rng(seed)
        A = list(range(0x61, 0x71))
        edges = [(u, v) for u in A for v in A]
        if extra:  # drop a -> b, add a -> z -> b
            edges.remove((A[0], A[1]))
            edges += [(A[0], 0x7A), (0x7A, A[1])]
        seq = _euler(edges * 20, r)
        out.append(seq)
    return tuple(out)


def fam_tail_g(seed=7):
    """a 300-byte phrase 64 / 65 times: its groups are small (tail_round) / large (the big list)"""
    return phrase_copies(300, 64, seed, tail=20000), phrase_copies(300, 65, seed, tail=20000)


def fam_gid(h, seed=8):
    """65 copies of a phrase of 4,096 / 4,097 windows at depth h: 4,096 / 4,097 large groups in round 0 -- numbered densely /
    on ranks (h = 8: the 8 passes; h = 7: the bucket-first sort, with a tail that makes the sample stride, 67, prime to the
    period of the copies: the sample test then sees 4,096 distinct prefixes)"""
    tail = 8000 if h == DEPTH_MSD else 0
    return phrase_copies(4096 + h - 1, 65, seed, tail), phrase_copies(4097 + h - 1, 65, seed, tail)


def fam_five_passes(seed=9):
    """a big list of 250,000 / 250,001 records at depth 8 (80 x 3,125 / 89 x 2,809 windows): round 1 sorts it in four / five
    passes"""
    return phrase_copies(3125 + 7, 80, seed), phrase_copies(2809 + 7, 89, seed)


def fam_quad(seed=10):
    """n = 100,000 with small groups only, 9,999 / 10,000 records of them at depth 8 (33 x 303 / 50 x 200 windows): round 0
    takes the depth x4 form / the plain one (gT * QUAD_DIV < n)"""
    out = []
    for plen, copies in ((303 + 7, 33), (200 + 7, 50)):
        body = phrase_copies(plen, copies, seed)
        out.append(body + bytes(_rng(seed + 1).integers(0, 128, 100000 - len(body), dtype=np.uint8)))
    return tuple(out)


def families():
    """name -> (below, above) blocks of every edge"""
    f = {"sample_n": fam_sample_n(), "sample_distinct": fam_sample_distinct(), "ne": fam_ne(), "over_pct": fam_over_pct(),
         "unit_width": fam_unit_width(), "tail_g": fam_tail_g(), "gid8": fam_gid(8), "gid7": fam_gid(7),
         "five_passes": fam_five_passes(), "quad": fam_quad()}
    for L in range(MS_LEVELS + 1):
        f[f"tile{L}"] = fam_tile(L)
    return f


def tiny_blocks():
    return [bytes(range(65, 65 + k)) for k in (1, 2, 3)] + [b"ab" * 4, b"zzzzzzzzzzzzzzzz", b"mississippi"]


def shrunk_block():
    """near-periodic: 2,000 periods of a 7-byte word and 3 bytes more (period_detect sorts 8 periods + 3)"""
    return (b"gfedcba" * 2001)[:14003]


def mixed_batches(fam=None):
    """two orders of one level-9 batch list (families on different paths, tiny blocks, a period-shrunk block) and a
    level-2 list: (level, max_batch, blocks); every batch holds at least 12 blocks"""
    fam = fam or families()
    pick = ["sample_n", "sample_distinct", "ne", "over_pct", "unit_width", "tail_g", "quad", "tile1", "tile5"]
    blocks = [b for k in pick for b in fam[k]] + tiny_blocks() + [shrunk_block()]
    order_a = blocks
    r = _rng(11)
    order_b = [blocks[i] for i in r.permutation(len(blocks))]
    lvl2 = [fam["tile0"][0], fam["tile0"][1], fam["tile2"][1], fam["over_pct"][0], fam["over_pct"][1], fam["ne"][1], fam["unit_width"][0],
            fam["sample_distinct"][1], fam["tail_g"][1]] + tiny_blocks()[:3] + [shrunk_block()]
    return {"mixed9a": (9, 13, order_a), "mixed9b": (9, 13, order_b), "mixed2": (2, 16, lvl2)}
