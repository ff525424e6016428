"""A serial model of the rules by which the ENCODER writes sync points (banzai_amd/csrc/sync_emit.hip): given a block's last
column it walks the run heads with a recency list and writes (group, out_pos, run, run_weight, mtf) wherever a group of 50
symbols begins whose index is a positive multiple of the interval.  The rules, as the kernel applies them per point:

  * a run head is a byte that differs from its predecessor; position 0 of the block is compared with name 0 (the smallest
    present byte).  A head g emits run_digits(z) digits for the zero run z = g - 1 - pg in front of it (pg: the head before,
    -1 at the start), then its own position symbol.  The trailing run and the end of block are a virtual head at g = n.
  * for the symbol t = 50 * group, emitted by head g after j of its digits: out_pos = pg + 1; with d = run_digits(z), j == d
    gives run = z, run_weight = 1 << d (0, 1 without a run); j < d gives run = sum over k < j of (((z + 1) >> k & 1) + 1) << k
    and run_weight = 1 << j.
  * the MTF list is the recency list behind head pg, as byte values, then zeros.

tests/test_esync_model.py holds it to the points the DECODER's recorder reports (tests/sync_model.py)."""
import functools
import random


def run_digits(z):
    return (int(z) + 1).bit_length() - 1 if z else 0


@functools.lru_cache(maxsize=None)
def text(n, seed=41, words=40):
    rng = random.Random(seed)
    vocab = ["".join(rng.choices("etaoinshrdlucmfwypvbgkqjxz", k=rng.randrange(2, 11))) for _ in range(words)]
    return " ".join(rng.choices(vocab, k=n // 4)).encode()[:n]


def points(last, interval, kinds=None):
    """last: the block's last column (bytes) -> [(group, out_pos, run, run_weight, mtf as 256 ints)]; `kinds` (a list) receives
    per point "none" (no run in front of the head), "mid" (inside a run's digits) or "head" (behind a run's last digit)"""
    n = len(last)
    present = sorted(set(last))
    lst = list(present)  # the recency list, as byte values: the initial list is the present bytes in order
    out = []
    t = 0    # symbols emitted so far
    pg = -1  # the last head
    prev = present[0] if present else 0
    heads = [p for p in range(n) if last[p] != (last[p - 1] if p else prev)] + [n]
    for g in heads:
        z = g - 1 - pg
        d = run_digits(z)
        for j in range(d + 1):  # the digits, then the head's own symbol (the end of block for g = n)
            if t > 0 and t % 50 == 0 and (t // 50) % interval == 0:
                if j == d:
                    run, weight = z, 1 << d
                else:
                    run, weight = sum(((((z + 1) >> k) & 1) + 1) << k for k in range(j)), 1 << j
                out.append((t // 50, pg + 1, run, weight, lst + [0] * (256 - len(lst))))
                if kinds is not None:
                    kinds.append("none" if d == 0 else ("head" if j == d else "mid"))
            t += 1
        if g < n:
            lst.remove(last[g])
            lst.insert(0, last[g])
            pg = g
    return out


def points_by_tiles(last, interval, TL):
    """The same points the way the kernel finds them, one point at a time from per-tile records: the tile whose output offset
    covers t (the last one with off <= t), the head inside it, the keys at the tile's entry raised by the bytes in front of
    the head, place = names with a larger key.  TL: bytes per MTF tile (the kernel's 2,048 or 4,096; tests also use tiny ones)."""
    n = len(last)
    present = sorted(set(last))
    name = {c: k for k, c in enumerate(present)}
    front = present[0] if present else 0
    is_head = [last[p] != (last[p - 1] if p else front) for p in range(n)]
    ntile = (n + TL - 1) // TL
    # mtf_tile_last + mtf_prefix: per tile the last head before it, its output offset, the keys at its entry
    tiles, carry, off = [], -1, 0
    keys = [-1 - k for k in range(len(present))]
    for tile in range(ntile):
        lo, hi = tile * TL, min(n, (tile + 1) * TL)
        tiles.append((carry, off, list(keys)))
        pg = carry
        for p in range(lo, hi):
            if is_head[p]:
                off += run_digits(p - 1 - pg) + 1
                pg = p
            keys[name[last[p]]] = p
        carry = pg
    m = off + run_digits(n - 1 - carry) + 1
    out = []
    for group in range(interval, (m + 49) // 50, interval):
        t = 50 * group
        tile = max(k for k in range(ntile) if tiles[k][1] <= t)
        pg, base, keys = tiles[tile][0], tiles[tile][1], list(tiles[tile][2])
        lo, hi = tile * TL, min(n, (tile + 1) * TL)
        g, j = n, None
        for p in range(lo, hi):
            if is_head[p]:
                cnt = run_digits(p - 1 - pg) + 1
                if base <= t < base + cnt:
                    g, j = p, t - base
                    break
                base += cnt
                pg = p
        if j is None:
            assert tile == ntile - 1  # symbols behind the last head's: the trailing run and the end of block
            j = t - base
        for p in range(lo, min(g, hi)):
            keys[name[last[p]]] = p
        z = g - 1 - pg
        d = run_digits(z)
        assert j <= d
        if j == d:
            run, weight = z, 1 << d
        else:
            run, weight = sum(((((z + 1) >> k) & 1) + 1) << k for k in range(j)), 1 << j
        mtf = [0] * 256
        for k, c in enumerate(present):
            mtf[sum(1 for other in keys if other > keys[k])] = c
        out.append((group, pg + 1, run, weight, mtf))
    return out


def points_by_lanes(last, interval, TL):
    """The kernel's steps lane for lane (numpy arrays of 64 lanes in lock step; ballots as boolean arrays, the DPP scan as a
    cumulative sum, LDS as arrays, atomicMax as maximum.at): the tile's bytes behind a 16-byte margin, run heads by comparing
    sb[16 + i] with sb[15 + i], the head before each lane from the lanes below or the carry, the owner of symbol t, keys raised
    only by the last byte of a run in front of g.  TL <= 4096.  The per-tile records come from the serial sweep above."""
    import numpy as np
    n = len(last)
    present = sorted(set(last))
    names = np.zeros(256, dtype=np.int64)
    for k, c in enumerate(present):
        names[c] = k
    col = np.frombuffer(bytes(last) + bytes(4096 + 64), dtype=np.uint8)  # (the arena's padding behind a block)
    front = present[0] if present else 0
    ntile = (n + TL - 1) // TL
    tiles, carry, off = [], -1, 0
    keys0 = [-1 - k for k in range(len(present))]
    for tile in range(ntile):  # mtf_tile_last + mtf_prefix, serially
        lo, hi = tile * TL, min(n, (tile + 1) * TL)
        tiles.append((carry, off, list(keys0)))
        for p in range(lo, hi):
            if last[p] != (last[p - 1] if p else front):
                off += run_digits(p - 1 - carry) + 1
                carry = p
            keys0[names[last[p]]] = p
    m = off + run_digits(n - 1 - carry) + 1
    offs = np.array([t[1] for t in tiles])
    lane = np.arange(64)
    digits = np.vectorize(run_digits)
    out = []
    for group in range(interval, (m + 49) // 50, interval):
        t = 50 * group
        tile = int(np.count_nonzero(offs <= t)) - 1
        me_last, me_off, kin = tiles[tile]
        rel, base_p = t - me_off, tile * TL
        tile_len = min(TL, n - base_p)
        sb = np.zeros(16 + 4096 + 16, dtype=np.uint8)
        for i in range(0, tile_len, 16):
            sb[16 + i:32 + i] = col[base_p + i:base_p + i + 16]
        sb[15] = col[base_p - 1] if base_p else 0
        keys = np.full(256, -(1 << 31), dtype=np.int64)
        keys[:len(present)] = kin
        prev, base, found, g, pg, j, r0 = me_last, 0, False, n, None, None, 0
        while r0 < tile_len and not found:
            idx = r0 + lane
            p = base_p + idx
            valid = idx < tile_len
            c, pc = sb[16 + idx], sb[15 + idx]
            head = valid & np.where(p == 0, names[c] != 0, c != pc)
            mypg, lasth = np.empty(64, dtype=np.int64), -1
            for q in range(64):
                mypg[q] = base_p + r0 + lasth if lasth >= 0 else prev
                if head[q]:
                    lasth = q
            cnt = np.where(head, digits(np.maximum(p - 1 - mypg, 0)) + 1, 0)
            incl = np.cumsum(cnt)
            owner = head & (base + incl - cnt <= rel) & (rel < base + incl)
            if owner.any():
                q = int(np.argmax(owner))
                assert owner.sum() == 1
                found, g, pg, j = True, int(p[q]), int(mypg[q]), int(rel - base - (incl[q] - cnt[q]))
            lim = g if found else base_p + tile_len
            raise_ = valid & (p < lim) & ((p + 1 >= lim) | (sb[17 + idx] != c))
            np.maximum.at(keys, names[c[raise_]], p[raise_])
            if lasth >= 0:
                prev = base_p + r0 + lasth
            base += int(incl[63])
            r0 += 64
        if not found:
            g, pg, j = n, prev, rel - base
        z = g - 1 - pg
        d = run_digits(z)
        if j < d:
            run, weight = sum(((((z + 1) >> k) & 1) + 1) << k for k in range(j)), 1 << j
        else:
            run, weight = z, 1 << d
        mtf = [0] * 256
        for k, c in enumerate(present):
            mtf[int(np.count_nonzero(keys[:len(present)] > keys[k]))] = c
        out.append((group, pg + 1, run, weight, mtf))
    return out
