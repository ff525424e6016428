"""A plain CPU model of the opt-in "fixed" Huffman mode (bzh_set_mode(ctx, BZH_MODE_FIXED)): the bytes
that mode must produce, restated from its rule (banzai_amd/csrc/huffman.hip, "Fixed" Huffman mode), which is libbz2's
sendMTFValues with the reference's heap for the code lengths.

RLE1 / block cut / CRC, BWT and MTF/RLE2 do not depend on the mode: they come from the oracle (oracle.pyoracle).  Per
block of m MTF symbols (EOB included) over an alphabet of nsyms symbols:

* ntab = 2 / 3 / 4 / 5 / 6 tables for m < 200 / < 600 / < 1200 / < 2400 / otherwise;
* initial partition: table t takes symbols from where table t-1 stopped while the frequencies it has taken stay
  below remaining / (ntab - t) (so a target of 0 takes no symbol); a middle table with t odd gives its last symbol
  back if it took more than one; lengths are 0 inside the table's range and 15 outside, a table with no symbol of its
  own has every length at 15;
* four refinement iterations: every 50-symbol segment goes to the table that codes it in the fewest bits (the first
  such table on ties), its symbols go to that table's frequency list (the lists restart every iteration, the tables
  are kept), and every table is rebuilt from its list with the reference's heap (oracle.build_table_from_freqs,
  scaling loop included; an all-zero list is a valid input);
* output: the last iteration's selectors, move-to-front over table ids, as unary; each table as a 5-bit start and
  deltas; canonical codes by increasing length, then symbol; the payload coded segment by segment with the segment's
  table.  Block header, symbol map and stream framing are those of the default mode.
"""
import numpy as np

from oracle import pyoracle

SEG = 50
ITERS = 4


def num_tables(m):
    return 2 if m < 200 else 3 if m < 600 else 4 if m < 1200 else 5 if m < 2400 else 6


def initial_partition(freqs, nsyms, m, ntab):
    """-> list of ntab half-open symbol ranges (lo, hi); lo == hi for a table with no symbol of its own"""
    ranges, left, remaining = [], 0, m
    for t in range(ntab):
        target = remaining // (ntab - t)
        right, acc = left, 0
        while acc < target and right < nsyms:
            acc += int(freqs[right])
            right += 1
        if right - left > 1 and t != 0 and t != ntab - 1 and t % 2 == 1:
            right -= 1
            acc -= int(freqs[right])
        ranges.append((left, right))
        left, remaining = right, remaining - acc
    return ranges


def initial_lengths(ranges, nsyms):
    lens = np.full((len(ranges), nsyms), 15, dtype=np.int64)
    for t, (lo, hi) in enumerate(ranges):
        lens[t, lo:hi] = 0
    return lens


def choose_tables(syms, lens):
    """-> (selector per segment, whether some segment had a cost tie)"""
    ntab, nsyms = lens.shape
    nseg = (len(syms) + SEG - 1) // SEG
    padded = np.full(nseg * SEG, nsyms, dtype=np.int64)  # a padding symbol that costs 0 in every table
    padded[:len(syms)] = syms
    cost = np.concatenate([lens, np.zeros((ntab, 1), np.int64)], axis=1)[:, padded].reshape(ntab, nseg, SEG).sum(axis=2)
    sel = np.argmin(cost, axis=0)  # the first minimum
    tie = bool(((cost == cost.min(axis=0)).sum(axis=0) > 1).any())
    return sel, tie


def table_freqs(syms, sel, ntab, nsyms):
    seg_of = np.arange(len(syms)) // SEG
    f = np.bincount(sel[seg_of] * nsyms + syms.astype(np.int64), minlength=ntab * nsyms).reshape(ntab, nsyms)
    return f


def canonical_codes(lens):
    """codes by increasing length, then by symbol"""
    codes = np.zeros(len(lens), dtype=np.int64)
    code, prev = 0, None
    for s in np.lexsort((np.arange(len(lens)), lens)):
        L = int(lens[s])
        if prev is not None:
            code = (code + 1) << (L - prev)
        codes[s] = code
        prev = L
    return codes


def _bits(values, widths):
    """MSB-first bits (np.uint8 0/1) of values[k] in widths[k] bits, concatenated"""
    values = np.asarray(values, dtype=np.int64)
    widths = np.asarray(widths, dtype=np.int64)
    if values.size == 0:
        return np.zeros(0, np.uint8)
    w = int(widths.max())
    sh = widths[:, None] - 1 - np.arange(w)[None, :]
    b = (values[:, None] >> np.maximum(sh, 0)) & 1
    return b[sh >= 0].astype(np.uint8)


def fixed_block(syms, nsyms, freqs, crc, ptr, has_byte, trace=None):
    """one block (header, symbol map, selectors, tables, payload) as MSB-first bits"""
    syms = np.asarray(syms, dtype=np.int64)
    m = len(syms)
    ntab = num_tables(m)
    ranges = initial_partition(freqs, nsyms, m, ntab)
    lens = initial_lengths(ranges, nsyms)
    segs_per_iter, tie, idle = [], False, any(lo == hi for lo, hi in ranges)
    for _ in range(ITERS):
        sel, t_tie = choose_tables(syms, lens)
        tie |= t_tie
        counts = np.bincount(sel, minlength=ntab)
        segs_per_iter.append([int(c) for c in counts])
        idle |= bool((counts == 0).any())
        tf = table_freqs(syms, sel, ntab, nsyms)
        f258 = np.zeros((ntab, 258), np.uint32)
        f258[:, :nsyms] = tf
        lens = np.stack([pyoracle.build_table_from_freqs(nsyms, f258[t]).astype(np.int64) for t in range(ntab)])
    nsel = len(sel)
    if trace is not None:
        trace.append({"m": m, "nsyms": int(nsyms), "ntab": ntab, "nsel": nsel, "ranges": ranges,
                      "segments": segs_per_iter, "tie": tie, "idle_table": idle, "max_len": int(lens.max()),
                      "table_freqs": tf})

    v, w = [0x314159, 0x265359, crc >> 16, crc & 0xFFFF, 0, ptr], [24, 24, 16, 16, 1, 24]
    sectors = np.asarray(has_byte, dtype=np.uint8)[:256].reshape(16, 16) != 0
    used = sectors.any(axis=1)
    v.append(int(sum(1 << (15 - x) for x in range(16) if used[x])))
    w.append(16)
    for x in range(16):
        if used[x]:
            v.append(int(sum(1 << (15 - y) for y in range(16) if sectors[x, y])))
            w.append(16)
    v += [ntab, nsel]
    w += [3, 15]
    order = list(range(ntab))  # selectors: move-to-front over the table ids, position j as j ones and a zero
    for s in sel:
        j = order.index(int(s))
        v.append((1 << (j + 1)) - 2)
        w.append(j + 1)
        order.insert(0, order.pop(j))
    for t in range(ntab):  # tables: a 5-bit start, then per symbol "10" (+1) / "11" (-1) steps and a "0"
        cur = int(lens[t, 0])
        v.append(cur)
        w.append(5)
        for L in lens[t]:
            L = int(L)
            while cur < L:
                v.append(2)
                w.append(2)
                cur += 1
            while cur > L:
                v.append(3)
                w.append(2)
                cur -= 1
            v.append(0)
            w.append(1)
    head = _bits(v, w)
    codes = np.stack([canonical_codes(lens[t]) for t in range(ntab)])
    tab = sel[np.arange(m) // SEG]
    payload = _bits(codes[tab, syms], lens[tab, syms])
    return np.concatenate([head, payload])


def encode(data, level=9, trace=None):
    """the fixed mode's .bz2 stream of `data`; with a list as `trace`, one dict per block is appended to it"""
    data = bytes(data)
    parts = [np.unpackbits(np.frombuffer(b"BZh" + bytes([ord("0") + level]), dtype=np.uint8))]
    off, combined = 0, 0
    while off < len(data):
        rle, crc, used = pyoracle.rle_one(data[off:], level)
        off += used
        b, ptr, hb = pyoracle.bwt(rle)
        syms, freqs, nsyms = pyoracle.mtf_and_rle(b, hb)
        parts.append(fixed_block(syms, nsyms, freqs, crc, ptr, hb, trace))
        combined = (crc ^ ((combined << 1) | (combined >> 31))) & 0xFFFFFFFF
    parts.append(_bits([0x177245, 0x385090, combined], [24, 24, 32]))
    return np.packbits(np.concatenate(parts)).tobytes()


# ---- inputs at the mode's edges (shared by tests/test_fixed_model.py, which checks that they reach them, and the GPU
# tests, which hold the kernels to the model on them) ----------------------------------------------------------------
def block_m(data, level=9):
    """MTF symbols (EOB included) of the first block of `data`"""
    rle, _, _ = pyoracle.rle_one(data, level)
    b, _, hb = pyoracle.bwt(rle)
    return len(pyoracle.mtf_and_rle(b, hb)[0])


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def two_letters(n, seed):
    """'a' and 'b' in runs of 1..3: two byte values and no run of four, so RLE1 adds no count byte (nsyms = 4)"""
    runs = np.random.default_rng(seed).integers(1, 4, n)
    return np.repeat(np.arange(n) % 2 + 97, runs)[:n].astype(np.uint8).tobytes()


def with_m(make, target, seed=0):
    """the shortest prefix of make(N, seed) (one block) whose block has exactly `target` MTF symbols"""
    for s in range(seed, seed + 8):
        src = make(4 * target + 64, s)
        n, seen = target, set()
        while n not in seen and 0 < n <= len(src):  # secant steps, then a scan around the last one
            seen.add(n)
            m = block_m(src[:n])
            if m == target:
                return src[:n]
            n = max(1, n + (target - m) * n // max(m, 1) or (1 if target > m else -1))
        for k in range(max(1, n - 400), min(len(src), n + 400) + 1):
            if block_m(src[:k]) == target:
                return src[:k]
    raise ValueError(f"no prefix with m = {target}")


def geometric(n=400_000, seed=3):
    """a geometric byte histogram (two families 128 apart): deep tables, the heap's scaling loop"""
    rng = np.random.default_rng(seed)
    return np.minimum(rng.geometric(0.35, n) - 1 + rng.integers(0, 2, n) * 128, 255).astype(np.uint8).tobytes()
