"""A NumPy model of the MTF + RLE2 stage that follows the kernels' own decomposition (banzai_amd/csrc/mtf.hip), not the
oracle's loop over a recency list: dense names, per tile the last-occurrence keys and (first, last, cnt) sweep by sweep
(mtf_tile_last), the prefix over the tiles in rounds of 256 and the keys at tile entry in groups of eight tiles
(mtf_prefix), and the walk half by half and 64 run heads at a time with the chunk's formulas as the kernel states them
(mtf_walk_par).  The tile size is a parameter: 2,048 bytes (batches below 64 blocks) or 4,096 (from 64 blocks on).

analyse(col, has_byte, TL) -> (syms, m, freqs, num_syms, record).  The record says what the input reached, so a test can
prove that a column built for an edge gets there before anything is compared (tests/mtf_cases.py).

MUTANTS names one-line changes of the kind a kernel edit could make; analyse(..., mutant=name) applies one.  The CPU test
holds every one of them against the cases built for its edge (tests/test_mtf_paths_model.py)."""
import numpy as np

INT_MIN = -(1 << 31)
SWEEP = 2048  # bytes a workgroup of mtf_tile_last covers in one sweep (256 threads x 8)
HALF = 1024   # bytes mtf_walk_par compacts at a time (64 lanes x 16)

MUTANTS = (
    "regs_rounded_down",      # regs = num_names / 64
    "cnt_last_one_short",     # cnt of the last key register one short
    "ebits_one_short",        # the comparator skips the top bit of a place
    "xhi_dropped",            # predecessors at lanes 32..63 not taken out of A
    "shift_folded",           # (Ws >> (e & 63)) >> 1 written as Ws >> ((e & 63) + 1): the hardware takes six bits of it
    "ts_word2_for_word3",     # Ts of word 2 used for word 3
    "sweep_carry_dropped",    # tcarry not carried from sweep to sweep
    "first_from_sweep0_only", # s_first taken from sweep 0 only
    "carry_last_byte15",      # carry_last taken from byte 15 of the lane that holds the half's last byte
    "prefix_skips_remainder", # the unrolled key loop of mtf_prefix without its remainder
    "round2_carry_reset",     # the second round of 256 tiles starts from carry_in = -1
)


def run_digits(z):
    """symbols of a zero run of z positions (bijective base 2, common.h)"""
    return (int(z) + 1).bit_length() - 1 if z > 0 else 0


def dense_names(has_byte):
    hb = np.asarray(has_byte, dtype=np.uint8) != 0
    names = (np.cumsum(hb) - hb).astype(np.int64)  # rank among the present bytes (absent bytes: the next one's, never read)
    return names, int(hb.sum())


def _tile_last(nm, colb, names, n, TL, ntile, mutant, rec):
    """-> last[ntile][256], tiles [(first, last, cnt)]"""
    # run heads from the BYTES, as mtf_tile_last finds them (the walk compares names: asserted equal below)
    hm = np.empty(n, dtype=bool)
    hm[1:] = colb[1:] != colb[:-1]
    hm[0] = names[colb[0]] != 0
    heads = np.nonzero(hm)[0]
    last = np.full((ntile, 256), -1, dtype=np.int64)
    tiles = []
    for t in range(ntile):
        lo, hi = t * TL, min(n, (t + 1) * TL)
        np.maximum.at(last[t], nm[lo:hi], np.arange(lo, hi))
        tcarry = 0  # last run head of the sweeps before, + 1
        first, cnt = -1, 0
        sweeps_with_head, first_sweep = [], None
        for sub in range(0, TL, SWEEP):
            slo, shi = lo + sub, min(hi, lo + sub + SWEEP)
            if slo >= hi:
                break
            hs = heads[np.searchsorted(heads, slo):np.searchsorted(heads, shi)]
            carry = 0 if (mutant == "sweep_carry_dropped" and sub) else tcarry
            cur = carry - 1
            for k, p in enumerate(hs):
                p = int(p)
                if k == 0 and carry == 0 and (mutant != "first_from_sweep0_only" or sub == 0):
                    first, first_sweep = p, sub // SWEEP  # (before == 0: one thread of the tile at most)
                cnt += 1 + (run_digits(p - 1 - cur) if cur >= 0 else 0)
                cur = p
            if hs.size:
                sweeps_with_head.append(sub // SWEEP)
                for p in hs:
                    if (int(p) - slo) % 512 == 0:
                        rec["wave_first_heads"].add((int(p) - slo) // 512)
                    rec["head_at_tile_byte"].add(int(p) - lo)
            tcarry = max(carry, int(hs[-1]) + 1 if hs.size else 0)
        tiles.append([first, tcarry - 1, cnt, 0])
        rec["tiles"].append(dict(sweeps=sweeps_with_head, first_sweep=first_sweep, heads=int(np.searchsorted(heads, hi) - np.searchsorted(heads, lo))))
    return last, tiles, hm


def _prefix(last, tiles, n, ntile, num_names, out, freqs, mutant, rec):
    """-> keys[ntile][256] at tile entry; tiles get (last head before, off); writes the trailing run, EOB; -> m"""
    carry_in, off_base = -1, 0
    for t0 in range(0, ntile, 256):
        if mutant == "round2_carry_reset" and t0:
            carry_in = -1
        rnd = tiles[t0:t0 + 256]
        run_max = carry_in
        total = 0
        for me in rnd:
            carry = run_max
            run_max = max(run_max, me[1])
            tc = me[2] + (run_digits(me[0] - 1 - carry) if me[0] >= 0 else 0)
            me[1], me[3] = carry, off_base + total
            total += tc
        carry_in = run_max
        off_base += total
    rec["rounds"] = (ntile + 255) // 256
    z = n - 1 - carry_in
    d = run_digits(z)
    for k in range(d):
        bit = ((z + 1) >> k) & 1
        out[off_base + k] = bit
        freqs[bit] += 1
    eob = num_names + 1
    out[off_base + d] = eob
    freqs[eob] += 1
    rec["trailing_run"] = z
    rec["digit_counts"].add(d)
    m = off_base + d + 1
    # keys at tile entry: thread = name, eight tiles a step, then the remainder
    c = np.arange(256)
    run = np.where(c < num_names, -1 - c, INT_MIN).astype(np.int64)
    seen_in = np.full(256, -1, dtype=np.int64)  # the tile a name's key comes from
    age = np.zeros(256, dtype=np.int64)
    keys = last.copy()
    t = 0

    def step(t):
        nonlocal run, seen_in, age
        v = last[t]
        keys[t] = run
        held = seen_in >= 0
        age = np.where(held, np.maximum(age, t - seen_in), age)
        run = np.where(v >= 0, v, run)
        seen_in = np.where(v >= 0, t, seen_in)

    while t + 8 <= ntile:
        for k in range(8):
            step(t + k)
        t += 8
    rec["unrolled_tiles"], rec["remainder_tiles"] = t, ntile - t
    if mutant != "prefix_skips_remainder":
        while t < ntile:
            step(t)
            t += 1
    rec["key_age"] = age[:num_names].copy()
    occ = last[:, :num_names] >= 0
    rec["first_tile"] = np.where(occ.any(axis=0), np.argmax(occ, axis=0), -1)  # per name: the tile of its first occurrence
    for t, me in enumerate(tiles):
        rec["tiles"][t].update(first=me[0], carry=me[1], off=me[3])
    return keys, m


def _walk_tile(t, nm, n, TL, keys, me, num_names, out, freqs, mutant, rec):
    base_p = t * TL
    tile_len = min(n - base_p, TL)
    woff, prevhead = me[3], me[1]
    regs = num_names // 64 if mutant == "regs_rounded_down" else (num_names + 63) // 64
    ebits = (num_names - 1).bit_length() if num_names > 1 else 1
    if mutant == "ebits_one_short":
        ebits -= 1
    # ---- list at tile entry: E[name] = names with a larger key
    k = keys.astype(np.int64)
    counted = []
    for r in range(regs):
        cnt = min(64, num_names - 64 * r)
        if mutant == "cnt_last_one_short" and r == regs - 1:
            cnt -= 1
        counted.append(k[64 * r:64 * r + cnt])
    counted = np.concatenate(counted) if counted else np.zeros(0, np.int64)
    Etab = (counted[None, :] > k[:, None]).sum(axis=1).astype(np.int64)
    front = int(np.argmax(k))
    hist = np.zeros(128, dtype=np.int64)
    fa = fb = 0
    lanes = np.arange(64)
    lower = lanes[None, :] < lanes[:, None]  # [l, u]: u below l
    carry_last = front
    prev_syms = np.zeros(0, dtype=np.int64)  # the symbols of the chunk before, in this tile
    for cbase in range(0, tile_len, HALF):
        clen = min(tile_len - cbase, HALF)
        seg = nm[base_p + cbase:base_p + cbase + clen]
        prev = np.empty(clen, dtype=np.int64)
        prev[0] = carry_last
        prev[1:] = seg[:-1]
        chg = seg != prev
        e = clen - 1
        if mutant == "carry_last_byte15":
            at = (e >> 4) * 16 + 15  # (bytes behind the column: whatever the arena holds; the model reads name 0)
            carry_last = int(seg[at]) if at < clen else 0
        else:
            carry_last = int(seg[e])
        hoff = np.nonzero(chg)[0]
        hsym = seg[hoff]
        H = hoff.size
        last_half = cbase + HALF >= tile_len
        rec["halves"].append((t, cbase // HALF, clen, H, bool(chg[-1]), carry_last))
        for hb in range(0, H, 64):
            nact = min(64, H - hb)
            act = lanes < nact
            c = np.zeros(64, dtype=np.int64)
            c[:nact] = hsym[hb:hb + nact]
            same = act[:, None] & act[None, :] & (c[:, None] == c[None, :])
            below = same & lower
            anyb = below.any(axis=1)
            p = np.where(anyb, 63 - np.argmax(below[:, ::-1], axis=1), -1)
            islast = act & ~(same & lower.T).any(axis=1)
            Eown = Etab[c]
            # A: the lanes below me that are the last occurrence of their symbol before me
            P = act[:, None] & (p[:, None] == lanes[None, :])  # [v, u]: u is the predecessor of v
            if mutant == "xhi_dropped":
                P = P & (lanes[None, :] < 32)
            X = np.zeros((64, 64), dtype=bool)
            X[1:] = np.logical_or.accumulate(P, axis=0)[:-1]  # exclusive: the predecessors of the lanes strictly below me
            A = lower & ~X
            isfirst = act & (p < 0)
            more = hb + 64 < H or not last_half
            places = Eown[isfirst]
            MFbits = np.zeros(256, dtype=bool)
            MFbits[places] = True
            assert int(MFbits.sum()) == places.size or mutant, "places of new symbols are distinct"
            # the comparator over the bits of a place, most significant first
            gt = np.zeros((64, 64), dtype=bool)
            eq = np.broadcast_to(isfirst[None, :], (64, 64)).copy()
            for bit in range(7, -1, -1):
                if bit >= ebits:
                    continue
                mine = ((Eown >> bit) & 1).astype(bool)
                mb = isfirst & mine
                gt |= ~mine[:, None] & eq & mb[None, :]
                eq &= np.where(mine[:, None], mb[None, :], ~mb[None, :])
            cntB = (gt & lower).sum(axis=1)
            pos_seen = (A & (lanes[None, :] > p[:, None])).sum(axis=1)
            pos = np.where(p < 0, Eown + cntB, pos_seen)
            # the list when the next chunk begins
            if more:
                W = MFbits.reshape(4, 64)
                T = [int(W[1:].sum()), int(W[2:].sum()), int(W[3:].sum()), 0]
                if mutant == "ts_word2_for_word3":
                    T[3] = T[2]
                upd = np.arange(64 * regs)
                eo = Etab[upd]
                sel, sh = eo >> 6, eo & 63
                # popcount((Ws >> sh) >> 1): the bits of word sel above place sh
                suf = np.zeros((4, 65), dtype=np.int64)
                suf[:, :64] = np.cumsum(W[:, ::-1], axis=1)[:, ::-1]
                above = suf[sel, sh + 1]
                if mutant == "shift_folded":
                    above = np.where(sh == 63, suf[sel, 0], above)  # a shift by 64 is a shift by 0
                newE = eo + above + np.array(T)[sel]
            # ---- RLE2
            g = np.zeros(64, dtype=np.int64)
            g[:nact] = base_p + cbase + hoff[hb:hb + nact]
            pg = np.empty(64, dtype=np.int64)
            pg[0] = prevhead
            pg[1:] = g[:-1]
            zz = (g - pg)[:nact]  # run length + 1
            d = np.floor(np.log2(zz)).astype(np.int64)  # (exact: zz < 2^20)
            assert ((zz >> d) == 1).all()
            tot = d + 1
            sc = np.cumsum(tot)
            rel = woff + sc - tot
            pa = pos[:nact]
            for j in range(int(d.max())):
                w = d > j
                bits = (zz[w] >> j) & 1
                out[rel[w] + j] = bits
                fb += int(bits.sum())
                fa += int(w.sum()) - int(bits.sum())
            out[rel + d] = pa + 1
            woff += int(sc[-1])
            rec["digit_counts"].update(np.unique(d).tolist())
            np.add.at(hist, pa >> 1, 1 << (16 * (pa & 1)))
            prevhead = int(g[nact - 1])
            if more:
                Etab[upd] = newE
                lasts_above = (islast[None, :] & lower.T).sum(axis=1)  # last occurrences at lanes above me
                Etab[c[islast]] = lasts_above[islast]
            if mutant is None:
                assert int(pa.min()) >= 1, "position 0 never comes from a run head"
            rec["pos_min"] = min(rec["pos_min"], int(pa.min()))
            rec["pos_max"] = max(rec["pos_max"], int(pa.max()))
            # (tile, half, nact, first occurrences, p of every lane (-1: new in the chunk), places of the new symbols, list update ran,
            # new in this chunk, seen in the chunk before)
            again = int(np.isin(c[isfirst], prev_syms).sum())
            prev_syms = c[:nact].copy()
            rec["chunks"].append((t, cbase // HALF, nact, int(isfirst.sum()), p[:nact].astype(np.int8), np.sort(places), bool(more), again))
    lo, hi = hist & 0xFFFF, hist >> 16
    rec["max_one_pos_in_tile"] = max(rec["max_one_pos_in_tile"], int(lo.max()), int(hi.max()))
    rec["max_in_tile"] = np.maximum(rec["max_in_tile"], np.stack([lo, hi], axis=1).reshape(256))
    rec["hist_words_both"] |= set(np.nonzero((lo > 0) & (hi > 0))[0].tolist())
    idx = 2 * np.arange(128)
    freqs[idx + 1] += lo
    freqs[idx + 2] += hi
    freqs[0] += fa
    freqs[1] += fb


def analyse(col, has_byte, TL, mutant=None):
    """-> (syms uint16[m], m, freqs uint32[258], num_syms, record)"""
    assert TL in (2048, 4096) and (mutant is None or mutant in MUTANTS)
    colb = np.frombuffer(bytes(col), dtype=np.uint8)
    n = colb.size
    assert n >= 1
    names, num_names = dense_names(has_byte)
    assert np.asarray(has_byte, dtype=np.uint8)[colb].all(), "a byte of the column is not marked present"
    nm = names[colb]
    ntile = (n + TL - 1) // TL
    rec = dict(num_names=num_names, regs=(num_names + 63) // 64, ebits=(num_names - 1).bit_length() if num_names > 1 else 1,
               ntile=ntile, TL=TL, n=n, tiles=[], halves=[], chunks=[], pos_min=1 << 30, pos_max=-1, max_one_pos_in_tile=0,
               hist_words_both=set(), digit_counts=set(), wave_first_heads=set(), head_at_tile_byte=set(),
               max_in_tile=np.zeros(256, dtype=np.int64))
    out = np.zeros(3 * n + 64, dtype=np.int64)  # (room for a mutant's wrong offsets)
    freqs = np.zeros(259, dtype=np.int64)
    last, tiles, hm = _tile_last(nm, colb, names, n, TL, ntile, mutant, rec)
    hn = np.empty(n, dtype=bool)
    hn[1:] = nm[1:] != nm[:-1]
    hn[0] = nm[0] != 0
    assert np.array_equal(hm, hn), "run heads by byte and by name"
    keys, m = _prefix(last, tiles, n, ntile, num_names, out, freqs, mutant, rec)
    rec["no_head_tiles"] = [t for t in range(ntile) if tiles[t][0] < 0]
    for t in range(ntile):
        _walk_tile(t, nm, n, TL, keys[t], tiles[t], num_names, out, freqs, mutant, rec)
    rec["heads"] = int(hm.sum())
    hp = np.nonzero(hm)[0]
    rec["head_pos"] = hp
    zr = np.diff(hp) - 1
    # (zero run, byte in its tile of the head that closes it), runs in front of the first head left out
    rec["closing"] = set(zip(zr[zr > 0].tolist(), (hp[1:][zr > 0] % TL).tolist()))
    if rec["pos_max"] < 0:
        rec["pos_min"] = -1
    return out[:m].astype(np.uint16), m, freqs[:258].astype(np.uint32), num_names + 2, rec
