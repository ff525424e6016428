"""What a symbol stream reaches in the default-mode Huffman stage: a plain Python / NumPy restatement of the reference's
huffman::encode up to the code lengths (oracle/banzai_oracle.c:803-990, lib/huffman.rs:161-460) that also records which
paths the input drives the stage through.  No HIP, no oracle.

    lens, rec = analyse(syms, num_syms)

`lens` holds the final code lengths of every table (uint8[ntab, num_syms]).  `rec` is a dict of path facts:

    ntab            2 or 3 (num_syms <= 199 or not)
    ranges          [(left, right)] of the initial tables
    backoff         middle table of three: "taken" (right--), "single" (right == left, so it is not); None with two tables
    exps            per table, the accepted exponent: scaling = 1 << exp is the first with no code longer than 17 bits
    halves          per table, who decides it in huff_build: "lower", "upper" or "carry" (the serial tail behind the last
                    attempt) -- the lower workgroup half runs exponents 0..3 of two tables, 0..2 of three; the upper 4..7, 3..4
    attempt_maxlen  per table, the longest code of every attempt 0..exp
    max_sink        levels the moved element of an extract sank at the most (heap_extract looks at four levels a pass: a
                    second pass from 4 on, a third at 8)
    max_rise        levels a new element of an insert rose at the most
    tie_sibling     an extract compared two children of equal priority
    tie_moved       an extract compared the moved element with a child of equal priority
    nseg, last_seg  number of 50-symbol segments, length of the last
    seg_wins        segments each table won in iteration 0
    seg_ties        pairs (t, u), t < u, of tables that shared the minimum cost of some segment
    table_bits      per table, bits of its delta-coded lengths
    pack_start      bit at which the symbols start in the stage's bit string (table count, selector count, selectors, tables)
    tile_bits       bits of every 4,096-symbol pack tile
    thread_words    the numbers of 32-bit output words that the 16 symbols of one pack thread touch, as a set (the stage's
                    bit string taken to start `frame` bits into a word)

The reference zeroes the LENGTH tables before iterations 1-3 (lib/huffman.rs:402-409), so table 0 wins every segment there
and the frequency lists, which are never restarted, end as f0_0 + 3 F for table 0 and f0_t for the others; every selector
is 0 and every symbol is coded with table 0.

A range that starts at num_syms (three tables, table 0 or 1 ending on the last symbol) makes the oracle and the kernel read
freqs[num_syms] and would index out of bounds in the Rust reference: analyse() asserts that the input stays clear of it.
"""
import numpy as np

MAX_LEN = 17      # lib/huffman.rs:13
SEG = 50          # lib/huffman.rs:310
TILE = 4096       # symbols a pack workgroup
ITEMS = 16        # symbols a pack thread
SEAM_FRAME = 137  # bits in front of the stage's bit string in bzh_huffman's own stream: block magic, CRC, flag, pointer, symbol map


class _Heap:
    """FrequencyQueue (lib/huffman.rs:161-267), operation for operation.  A priority (sum_frequency, max_dist) is the
    integer weight * 256 + dist: the same order as the derived lexicographic one while dist < 256."""

    def __init__(self):
        self.a = []
        self.max_sink = 0
        self.max_rise = 0
        self.tie_sibling = False
        self.tie_moved = False

    def insert(self, ident, pr):  # :196-222
        a = self.a
        a.append((pr, ident))
        init = len(a)
        if init == 1:
            return
        this = init
        while True:
            above = this >> 1
            ab = a[above - 1]
            if pr < ab[0]:
                a[this - 1] = ab
                this = above
                if this == 1:
                    break
            else:
                break
        if this != init:
            a[this - 1] = (pr, ident)
            self.max_rise = max(self.max_rise, init.bit_length() - this.bit_length())

    def extract(self):  # :225-267
        a = self.a
        last = a.pop()
        if not a:
            return last
        root = a[0]
        a[0] = last
        size, this, sunk = len(a), 1, 0
        while True:
            left = this << 1
            if left > size:
                break
            right = left + 1
            below = left
            if right <= size:
                if a[right - 1][0] < a[left - 1][0]:
                    below = right
                elif a[right - 1][0] == a[left - 1][0]:
                    self.tie_sibling = True
            bl = a[below - 1]
            if last[0] < bl[0]:
                break
            if last[0] == bl[0]:
                self.tie_moved = True
            a[this - 1] = bl
            this = below
            sunk += 1
        a[this - 1] = last
        self.max_sink = max(self.max_sink, sunk)
        return root


def build_attempt(num_syms, freqs, exp, heap=None):
    """one pass of build_table_from_freqs (:271-298) with scaling = 1 << exp -> (lengths, longest)"""
    h = heap if heap is not None else _Heap()
    h.a = []
    for s in range(num_syms):
        h.insert(s + 1, ((int(freqs[s]) >> exp) + 1) << 8)
    parent = [0] * (2 * num_syms)
    nnodes = num_syms + 1
    while True:
        pa, a = h.extract()
        pc, c = h.extract()
        if nnodes == 2 * num_syms - 1:  # Tree::tie :60-74: the last pair hangs off the root, id 0
            parent[a] = parent[c] = 0
            break
        p = nnodes
        nnodes += 1
        parent[a] = parent[c] = p
        dist = max(pa & 255, pc & 255) + 1
        assert dist < 256
        h.insert(p, (((pa >> 8) + (pc >> 8)) << 8) | dist)
    lens = []
    for s in range(num_syms):
        x, d = parent[s + 1], 1
        while x != 0:
            x = parent[x]
            d += 1
        lens.append(d)
    return lens, max(lens)


def build_lengths(num_syms, freqs, heap=None):
    """the scaling loop (:293-296) -> (lengths, accepted exponent, longest code of every attempt)"""
    longest = []
    exp = 0
    while True:
        lens, mx = build_attempt(num_syms, freqs, exp, heap)
        longest.append(mx)
        if mx <= MAX_LEN:
            return lens, exp, longest
        exp += 1


def initial_ranges(freqs, m, num_syms):
    """:333-376 -> ([(left, right)], backoff)"""
    ntab = 2 if num_syms <= 199 else 3
    remaining, left, ranges, backoff = m, 0, [], None
    for t in range(ntab):
        assert left < num_syms, "a range starts at num_syms: the reference would index freqs out of bounds"
        target = remaining // (ntab - t)
        acc, right = 0, left
        while True:
            acc += int(freqs[right])
            if acc >= target or right + 1 == num_syms:
                break
            right += 1
        if t != 0 and t != ntab - 1 and t % 2 == 1:
            if right > left:
                acc -= int(freqs[right])
                right -= 1
                backoff = "taken"
            else:
                backoff = "single"
        ranges.append((left, right))
        left = right + 1
        remaining -= acc
    return ranges, backoff


def half_of(ntab, exp):
    lo, hi = (4, 8) if ntab == 2 else (3, 5)
    return "lower" if exp < lo else "upper" if exp < hi else "carry"


def analyse(syms, num_syms, frame=SEAM_FRAME):
    s = np.asarray(syms).astype(np.int64)
    m = s.size
    assert m >= 1 and 3 <= num_syms <= 258 and int(s.max()) < num_syms
    F = np.bincount(s, minlength=num_syms).astype(np.int64)
    ranges, backoff = initial_ranges(F, m, num_syms)
    ntab = len(ranges)

    # iteration 0 (:411-454): a table's cost of a segment is 15 bits for every symbol inside its range, 0 outside
    nseg = (m + SEG - 1) // SEG
    sp = np.concatenate([s, np.full(nseg * SEG - m, -1, np.int64)]).reshape(nseg, SEG)
    cost = np.stack([((sp >= l) & (sp <= r)).sum(1) for l, r in ranges], 1)
    best = np.zeros(nseg, np.int64)
    bc = cost[:, 0].copy()
    for t in range(1, ntab):  # the first strict minimum wins
        win = cost[:, t] < bc
        best[win] = t
        bc[win] = cost[win, t]
    ties = set()
    for t in range(ntab):
        for u in range(t + 1, ntab):
            if np.any((cost[:, t] == bc) & (cost[:, u] == bc)):
                ties.add((t, u))
    tf = []
    for t in range(ntab):
        part = sp[best == t].reshape(-1)
        f0 = np.bincount(part[part >= 0], minlength=num_syms).astype(np.int64)
        tf.append(f0 + 3 * F if t == 0 else f0)  # iterations 1-3: all of it to table 0, three times

    heap = _Heap()
    lens, exps, longest = [], [], []
    for t in range(ntab):
        l, e, lg = build_lengths(num_syms, tf[t], heap)
        lens.append(l)
        exps.append(e)
        longest.append(lg)
    lens = np.array(lens, dtype=np.uint8)

    table_bits = [5 + num_syms + 2 * int(np.abs(np.diff(lens[t].astype(np.int64))).sum()) for t in range(ntab)]
    pack_start = 3 + 15 + nseg + sum(table_bits)
    sl = lens[0].astype(np.int64)[s]
    tile_bits = [int(sl[k:k + TILE].sum()) for k in range(0, m, TILE)]
    nthr = (m + ITEMS - 1) // ITEMS
    tb = np.concatenate([sl, np.zeros(nthr * ITEMS - m, np.int64)]).reshape(nthr, ITEMS).sum(1)
    start = frame + pack_start + np.concatenate([[0], np.cumsum(tb)[:-1]])
    thread_words = set(((start + tb - 1) // 32 - start // 32 + 1).tolist())

    rec = dict(ntab=ntab, ranges=ranges, backoff=backoff, exps=exps, halves=[half_of(ntab, e) for e in exps],
               attempt_maxlen=longest, max_sink=heap.max_sink, max_rise=heap.max_rise, tie_sibling=heap.tie_sibling,
               tie_moved=heap.tie_moved, nseg=nseg, last_seg=m - (nseg - 1) * SEG,
               seg_wins=[int((best == t).sum()) for t in range(ntab)], seg_ties=ties, table_bits=table_bits,
               pack_start=pack_start, tile_bits=tile_bits, thread_words=thread_words)
    return lens, rec
