"""A model of the PATHS of banzai_amd/csrc/rle1.hip, not only of its results: the run tables, every cut as cut_block_to /
end_from_lim / cut_in_run make it, plan_split's speculative windows, rle1_emit_kernel's offsets per tile and the block CRCs
as crc_range folds them -- restated from the kernel text in plain Python and numpy, with a record of which way every
decision went.  tests/rle1_cases.py builds inputs for the edges; the CPU test holds the model's blocks, bytes and CRCs to
the oracle and the record to what every case was built to reach, so the GPU test can say what a case drives the kernels
through before it compares anything.

analyse(data, level) -> Result: .blocks [(in_off, in_len, rle_len)], .open [bool], .aux [(A, Ce)], .facts (a Counter of
the strings listed in FACTS), .windows (one dict per window of plan_split), .tiles (emit records of every tile of every
block), .crc (one dict per block); .rle(b) the RLE1 bytes of block b and .crcs the block CRCs, both by the kernels' own
arithmetic (offsets from the tables, CRC pieces shifted and folded).

Tables are computed in closed form from the run list (what the scans of plan_starts .. plan_tc add up to); everything a
single wavefront does -- gran_eval, the probe, the 64-ary search, the windows -- is restated step by step.

MUTANTS are deliberate single-decision faults of the model (never of a kernel): the CPU test shows that for each of them
some named case ends with blocks, bytes, flags or CRCs that are not the oracle's.
"""
import collections
import functools
import zlib

import numpy as np

from tests.rle_model import canon_len

RL_TILE, GRAN, GRAN_PER_TILE, WAVE_BYTES = 4096, 64, 64, 1024
PC_CHUNK = 16384
SP_W, SP_K = 15, 8
CRC_PIECE, CRC_TILE, CRC_WG_TILES = 32, 8192, 8
U32 = 0xFFFFFFFF

MUTANTS = ("probe_le_64", "fit_ignores_lim", "spec_keeps_mismatch", "no_ell_clamp", "open_zero", "emit_no_restart",
           "crc_ragged_last")

FACTS = """
tile:no_start tile:byte0_start tile:other wave:slow wave:literal chunks:1 chunks:2 seam:fwd_run seam:bwd_run
cut:first_run cut:to_end_lt cut:to_end_eq cut:end_from_lim cut:ends_M-1 cut:ends_M
probe:prefix probe:full probe:miss rounds:0 rounds:1 rounds:2 rounds:3 sel:fit sel:rsg gran:reused gran:fresh
next:gran next:nrsg next:nrsg_end cir:k<nf cir:k==nf cir:ell>=4 cir:ell<4 cir:rho0 cir:rho1 cir:rho2 cir:rho3 cir:rho4
open:0 open:1 wf:spec wf:no_origin wf:past_total wf:start_N wfcut:full wfcut:input_ended wfcut:fin wfcut:none
reject:mismatch reject:input_done reject:empty reject:stop reject:none windows:1 windows:2 windows:many
obase:start obase:first_run obase:ordinary emit:mixed_waves emit:head_outside emit:tail_outside mis:0 mis:1 mis:2 mis:3
nwords:0 nwords:>0 crc:ragged_piece crc:whole_pieces crc:ragged_tile crc:whole_tiles crc:off%16==0 crc:off%16!=0
crc:ranges1 crc:ranges>1 crc:pos<64 crc:pos>=64 crc:flat crc:grid crc:tiles>=100
""".split()


def emitted_before(d):
    """canonical bytes of the first d bytes of a run (ints or arrays)"""
    return 5 * (d // 255) + np.minimum(d % 255, 4)


# ---- the tables (plan_starts, plan_carries, plan_granules, plan_tc) ----------------------------------------------------
class Tables:
    def __init__(self, data, facts):
        a = np.frombuffer(data, dtype=np.uint8)
        n = a.size
        assert n > 0
        self.a, self.n = a, n
        self.NT = NT = (n + RL_TILE - 1) // RL_TILE
        self.NG = NG = NT * GRAN_PER_TILE
        st = np.empty(n, bool)
        st[0] = True
        np.not_equal(a[1:], a[:-1], out=st[1:])
        self.st = st
        self.RS = np.append(np.flatnonzero(st), n).astype(np.int64)  # run starts, then n
        L = np.diff(self.RS)
        self.PO = np.concatenate(([0], np.cumsum(5 * (L // 255) + np.where(L % 255 < 4, L % 255, 5)))).astype(np.int64)
        tb = np.minimum(np.arange(NT + 1, dtype=np.int64) * RL_TILE, n)
        self.tc = self.cpos(tb)  # tc[NT] = total
        gp = np.arange(NG + 1, dtype=np.int64) * GRAN
        inside = gp < n
        gq = np.minimum(gp, n)
        self.cg = np.where(inside, self.cpos(gq) - self.tc[np.minimum(np.arange(NG + 1) // GRAN_PER_TILE, NT)], 0)
        self.rsg = self.RS[np.searchsorted(self.RS, gq, side="right") - 1]
        self.nrsg = np.where(inside, self.RS[np.searchsorted(self.RS, gq, side="left")], n)  # nrsg[NG] = n
        # -- which way the table kernels went
        per_tile = np.diff(np.searchsorted(self.RS[:-1], tb, side="left"))
        byte0 = st[tb[:-1]]
        facts["tile:no_start"] += int((per_tile == 0).sum())
        facts["tile:byte0_start"] += int(byte0.sum())
        facts["tile:other"] += int(((per_tile > 0) & ~byte0).sum())
        ns = ~st
        r4 = np.zeros(n, bool)  # byte q is the 4th or a later one of equal bytes in a row (has_run_of_four)
        if n > 2:
            r4[2:] = ns[2:] & ns[1:-1] & ns[:-2]
        self.wave_slow = np.logical_or.reduceat(r4, np.arange(0, n, WAVE_BYTES))
        facts["wave:slow"] += int(self.wave_slow.sum())
        facts["wave:literal"] += int((~self.wave_slow).sum())
        chunks = (NT + PC_CHUNK - 1) // PC_CHUNK
        facts["chunks:%d" % min(chunks, 2)] += 1
        self.tile_starts = per_tile
        for c in range(1, chunks):
            # (forward: the tiles behind the seam have no run start, their covering run comes out of the carry alone;
            # backward -- chunks counted from the END -- the tile in front of the seam has none, its next start likewise)
            if per_tile[c * PC_CHUNK] == 0:
                facts["seam:fwd_run"] += 1
            if per_tile[NT - 1 - c * PC_CHUNK] == 0 and per_tile[NT - c * PC_CHUNK] == 0:
                facts["seam:bwd_run"] += 1

    def cpos(self, p):
        """canonical RLE1 bytes emitted before input position p (ints or arrays, p <= n)"""
        j = np.searchsorted(self.RS, p, side="right") - 1
        return self.PO[j] + emitted_before(p - self.RS[j])


class Gran:
    pass


class CutState:
    def __init__(self):
        self.idx, self.ev = -1, None


LANE = np.arange(64, dtype=np.int64)


class Model:
    def __init__(self, data, level, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mut = mutant
        self.facts = collections.Counter()
        self.T = Tables(data, self.facts)
        self.M = 100000 * level - 1
        self.level = level

    # ---- one granule by one wavefront ----------------------------------------------------------------------------------
    def gran_eval(self, g):
        T = self.T
        n, a = T.n, T.a
        r = Gran()
        r.pos = g * GRAN + LANE
        r.valid = r.pos < n
        byte = np.where(r.valid, a[np.minimum(r.pos, n - 1)].astype(np.int64), 0x100)
        prevb = np.empty(64, np.int64)
        prevb[1:] = byte[:-1]
        prevb[0] = a[g * GRAN - 1] if g else 0x200
        nextb = np.empty(64, np.int64)
        nextb[:-1] = byte[1:]
        nextb[63] = a[r.pos[63] + 1] if r.pos[63] + 1 < n else 0x100
        r.start = r.valid & (byte != prevb)
        is_last = nextb != byte
        ms = np.maximum.accumulate(np.where(r.start, LANE, -1))
        rs = np.where(ms >= 0, g * GRAN + ms, T.rsg[g])
        kk = (r.pos - rs) % 255
        em = np.where(r.valid, (kk < 4).astype(np.int64) + ((kk >= 3) & ((kk == 254) | is_last)), 0)
        r.cpos = int(T.tc[g // GRAN_PER_TILE]) + int(T.cg[g]) + np.cumsum(em) - em
        return r

    def _nrsg_after(self, g):
        T = self.T
        self.facts["next:nrsg_end" if g + 1 >= T.NG else "next:nrsg"] += 1
        return int(T.nrsg[min(g + 1, T.NG)])

    def next_start_in(self, gr, g, s):
        m = gr.valid & (gr.pos > s) & gr.start
        if m.any():
            self.facts["next:gran"] += 1
            return g * GRAN + int(np.argmax(m))
        return self._nrsg_after(g)

    def next_start_after(self, s):
        T = self.T
        g = s // GRAN
        pos = g * GRAN + LANE
        ok = pos < T.n
        m = ok & (pos > s) & T.st[np.minimum(pos, T.n - 1)]  # (byte != prevb, read from the input)
        if m.any():
            self.facts["next:gran"] += 1
            return g * GRAN + int(np.argmax(m))
        return self._nrsg_after(g)

    def _next(self, cs, x):
        return self.next_start_in(cs.ev, cs.idx, x) if x // GRAN == cs.idx else self.next_start_after(x)

    def _eval_into(self, cs, g):
        if g != cs.idx:
            cs.ev, cs.idx = self.gran_eval(g), g
            self.facts["gran:fresh"] += 1
        else:
            self.facts["gran:reused"] += 1

    def cut_in_run(self, Lr, R):
        nf = Lr // 255
        k = min(R // 5, nf)
        rho = R - 5 * k
        ell = 255 if k < nf else Lr - 255 * nf
        f = self.facts
        f["cir:k<nf" if k < nf else "cir:k==nf"] += 1
        f["cir:ell>=4" if ell >= 4 else "cir:ell<4"] += 1
        f["cir:rho%d" % min(rho, 5)] += 1
        if ell >= 4 and self.mut != "no_ell_clamp":
            t = min(rho, 3)  # (the 4th literal of a chunk is only taken together with its count byte)
        else:
            t = rho
        return k, t

    # ---- end_from_lim ----------------------------------------------------------------------------------------------------
    def end_from_lim(self, lim, lo_tile, cs):
        T, f = self.T, self.facts
        N, NT, tc = T.n, T.NT, T.tc
        lo, hi = lo_tile, NT - 1
        guess = lo + (lim - int(tc[lo])) // RL_TILE - 40
        w0 = min(max(guess, lo), hi)
        x = w0 + LANE
        ok = (x <= hi) & (tc[np.minimum(x, NT)] <= lim)
        if ok[0]:
            c = int(ok.sum())
            lo = w0 + c - 1
            if c < 64 or self.mut == "probe_le_64":
                hi = lo
                f["probe:prefix"] += 1
            else:
                f["probe:full"] += 1
        else:
            hi = w0 - 1
            f["probe:miss"] += 1
        rounds = 0
        while lo < hi:
            span = hi - lo
            step = (span + 63) // 64
            x = lo + (LANE + 1) * step
            ok = (x <= hi) & (tc[np.minimum(x, NT)] <= lim)
            lo += int(ok.sum()) * step
            hi = min(hi, lo + step - 1)
            rounds += 1
        f["rounds:%d" % min(rounds, 3)] += 1
        tl = lo
        gb = tl * GRAN_PER_TILE
        gidx = gb + LANE
        gok = (gidx * GRAN < N) & (int(tc[tl]) + T.cg[gidx] <= lim)
        gx = gb + int(gok.sum()) - 1
        self._eval_into(cs, gx)
        gr = cs.ev
        fit = gr.start & ((gr.cpos <= lim) | (self.mut == "fit_ignores_lim"))
        if fit.any():
            ln = 63 - int(np.argmax(fit[::-1]))
            x = gx * GRAN + ln
            Cx = int(gr.cpos[ln])
            f["sel:fit"] += 1
        else:
            x = int(T.rsg[gx])
            Cx = int(gr.cpos[0]) - int(emitted_before(gx * GRAN - x))
            f["sel:rsg"] += 1
        R = (lim - Cx) & U32
        xe = self._next(cs, x)
        Lx = xe - x
        opn = xe >= N and Lx < 255 * (R // 5 + 2)
        k, t = self.cut_in_run(Lx, R)
        return dict(end=x + 255 * k + t, R=R, kt=5 * k + t, open=opn)

    # ---- cut_block_to ------------------------------------------------------------------------------------------------------
    def cut_block_to(self, s, N, total, cs):
        """-> ((in_off, in_len, rle_len), (A, Ce), open, origin)"""
        f, M = self.facts, self.M
        e_first = self._next(cs, s)
        Lr = e_first - s
        A = canon_len(Lr)
        Ce, origin = 0, None
        if A > M:
            k, t = self.cut_in_run(Lr, M)
            consumed, out = 255 * k + t, 5 * k + t
            opn = e_first >= N and Lr < 255 * (M // 5 + 2)
            f["cut:first_run"] += 1
        else:
            if e_first >= N:
                Ce = total
            else:
                self._eval_into(cs, e_first // GRAN)
                Ce = int(cs.ev.cpos[e_first % GRAN])
            lim = M - A + Ce
            origin = lim - M
            if total <= lim:
                consumed, out, opn = N - s, A + total - Ce, True
                f["cut:to_end_eq" if total == lim else "cut:to_end_lt"] += 1
            else:
                ce = self.end_from_lim(lim, e_first // RL_TILE, cs)
                consumed = ce["end"] - s
                out = (M - ce["R"] + ce["kt"]) & U32
                opn = ce["open"]
                f["cut:end_from_lim"] += 1
        if self.mut == "open_zero":
            opn = False
        if out == M - 1:
            f["cut:ends_M-1"] += 1
        elif out == M:
            f["cut:ends_M"] += 1
        f["open:%d" % int(bool(opn))] += 1
        return (s, consumed, out), (A, Ce), bool(opn), origin

    # ---- plan_split ----------------------------------------------------------------------------------------------------------
    def split(self, start=0, stop=None):
        T, f, M = self.T, self.facts, self.M
        N, total = T.n, int(T.tc[T.NT])
        stop = U32 if stop is None else stop
        maxblocks = N // ((M - 1) * 4 // 5) + 4
        cs = [CutState() for _ in range(SP_W)]
        blocks, aux, opens, windows = [], [], [], []
        s, done = start, False
        while not done and s < N and len(blocks) < maxblocks:
            s0 = s
            recs = [[] for _ in range(SP_W)]
            w_start, w_end, w_fin, kinds, whys = [N] * SP_W, [N] * SP_W, [False] * SP_W, [""] * SP_W, [""] * SP_W
            first = self.cut_block_to(s0, N, total, cs[0])
            origin = first[3]
            for w in range(SP_W):
                if w == 0:
                    recs[0].append(first)
                    cnt, fin, sw = 1, s0 >= stop, s0 + first[0][1]
                    w_start[0], kinds[0] = s0, "known"
                else:
                    cnt, fin, sw = 0, False, N
                    lim = None if origin is None else origin + w * SP_K * M
                    if origin is None:
                        kinds[w] = "no_origin"
                    elif lim >= total:
                        kinds[w] = "past_total"
                    else:
                        sw = self.end_from_lim(lim, s0 // RL_TILE, cs[w])["end"]
                        kinds[w] = "spec"
                        if sw >= N:
                            f["wf:start_N"] += 1
                    f["wf:" + kinds[w]] += 1
                    w_start[w] = sw
                while cnt < SP_K and sw < N and not fin:
                    r = self.cut_block_to(sw, N, total, cs[w])
                    recs[w].append(r)
                    fin = sw >= stop
                    cnt += 1
                    sw += r[0][1]
                w_end[w], w_fin[w] = sw, fin
                whys[w] = "fin" if fin else ("full" if cnt == SP_K else ("none" if cnt == 0 else "input_ended"))
                f["wfcut:" + whys[w]] += 1
            kept, end_all, fin_all, why = 1, w_end[0], w_fin[0], "none"
            for w in range(1, SP_W):
                if fin_all:
                    why = "stop"
                elif end_all >= N:
                    why = "input_done"
                elif not recs[w]:
                    why = "empty"
                elif w_start[w] != end_all and self.mut != "spec_keeps_mismatch":
                    why = "mismatch"
                else:
                    end_all, fin_all = w_end[w], w_fin[w]
                    kept += 1
                    continue
                break
            for w in range(kept):
                for (d, ax, o, _) in recs[w]:
                    blocks.append(d)
                    aux.append(ax)
                    opens.append(o)
            f["reject:" + why] += 1
            f["kept:%d" % kept] += 1
            if why != "none":
                f["reject_at:%s@%d" % (why, kept)] += 1
            windows.append(dict(s0=s0, kinds=kinds, cuts=[len(r) for r in recs], whys=whys, kept=kept, reject=why,
                                reject_at=kept if why != "none" else None, nb=len(blocks)))
            s = N if fin_all else end_all
            done = fin_all or end_all >= N
        f["windows:%s" % (len(windows) if len(windows) <= 2 else "many")] += 1
        return blocks, aux, opens, windows

    # ---- rle1_emit_kernel: the offsets of every tile of a block ---------------------------------------------------------------
    def emit_tiles(self, b, d, ax):
        T, f = self.T, self.facts
        in_off, in_len, _ = d
        A, Ce = ax
        in_end = in_off + in_len
        t = np.arange(in_off // RL_TILE, (in_end - 1) // RL_TILE + 1, dtype=np.int64)
        tile0 = t * RL_TILE
        rst = T.rsg[t * GRAN_PER_TILE]
        branch = np.where(tile0 <= in_off, 0, np.where(rst <= in_off, 1, 2))
        obase = np.where(branch == 0, 0, np.where(branch == 1, emitted_before(np.maximum(tile0 - in_off, 0)), A + T.tc[t] - Ce))
        pl = np.minimum(tile0 + RL_TILE, in_end) - 1  # the tile's last byte inside the block: where its output ends
        rs = T.RS[np.searchsorted(T.RS, pl, side="right") - 1]
        is_last = (pl + 1 >= T.n) | T.st[np.minimum(pl + 1, T.n - 1)]
        dd = pl - in_off
        kk1 = dd % 255
        e1 = emitted_before(dd) + (kk1 < 4) + ((kk1 >= 3) & ((kk1 == 254) | is_last))
        kk2 = (pl - rs) % 255
        e2 = A + T.cpos(pl) - Ce + (kk2 < 4) + ((kk2 >= 3) & ((kk2 == 254) | is_last))
        oend = np.where(rs <= in_off, e1, e2)
        nout = oend - obase
        mis = obase & 3
        head = np.where(mis > 0, np.minimum(4 - mis, nout), 0)
        nwords = (nout - head) // 4
        w0 = tile0 // WAVE_BYTES
        mixed = np.zeros(t.size, bool)
        for k in range(t.size):
            ws = T.wave_slow[w0[k]:w0[k] + 4]
            mixed[k] = ws.any() and not ws.all()
        for k, name in enumerate(("start", "first_run", "ordinary")):
            f["obase:" + name] += int((branch == k).sum())
        f["emit:mixed_waves"] += int(mixed.sum())
        f["emit:head_outside"] += int((tile0 < in_off).sum())
        f["emit:tail_outside"] += int((tile0 + RL_TILE > in_end).sum())
        for m in range(4):
            f["mis:%d" % m] += int((mis == m).sum())
        f["nwords:0"] += int((nwords == 0).sum())
        f["nwords:>0"] += int((nwords > 0).sum())
        return dict(block=b, tile=t, branch=branch, obase=obase, nout=nout, mis=mis, nwords=nwords, mixed=mixed)

    def emit_bytes(self, d, ax, slab=1 << 20):
        """the block's RLE1 bytes as rle1_emit_kernel places them: every input byte's offset from the tables (or, inside
        the block's first run, from the block's start), its literal and its count byte"""
        T = self.T
        in_off, in_len, rle_len = d
        A, Ce = ax
        in_end = in_off + in_len
        out = np.zeros(rle_len, np.uint8)
        hit = np.zeros(rle_len, bool)
        for p0 in range(in_off, in_end, slab):
            p1 = min(p0 + slab, in_end)
            pos = np.arange(p0, p1, dtype=np.int64)
            st = T.st[p0:p1]
            rs = np.maximum.accumulate(np.where(st, pos, -1))
            rs = np.where(rs < 0, T.RS[np.searchsorted(T.RS, p0, side="right") - 1], rs)
            byte = T.a[p0:p1]
            is_last = np.ones(p1 - p0, bool)
            hi = min(p1, T.n - 1)
            is_last[:hi - p0] = T.st[p0 + 1:hi + 1]
            kk = (pos - rs) % 255
            lit = kk < 4
            can = lit.astype(np.int64) + ((kk >= 3) & ((kk == 254) | is_last))
            off = A + (int(T.cpos(p0)) + np.cumsum(can) - can) - Ce
            cnt = can - lit
            if self.mut != "emit_no_restart":
                first = rs <= in_off  # the block's first run: chunking restarts at in_off
                dd = pos - in_off
                kk1 = dd % 255
                kk = np.where(first, kk1, kk)
                off = np.where(first, emitted_before(dd), off)
                lit = np.where(first, kk1 < 4, lit)
                cnt = np.where(first, (kk1 >= 3) & ((kk1 == 254) | is_last), cnt).astype(np.int64)
            for o, val, m in ((off, byte, lit), (off + lit, (kk - 3).astype(np.uint8), cnt > 0)):
                m = m & (o >= 0) & (o < rle_len)  # (only a mutant writes outside)
                out[o[m]] = val[m]
                hit[o[m]] = True
        return out.tobytes() if hit.all() else None

    # ---- block CRCs: crc_range under crc_tiles_flat (the plan) or crc_tiles (plan_crc_range) ---------------------------------
    def crc_block(self, pos, d, form="flat", grid=None):
        T, f = self.T, self.facts
        in_off, in_len, _ = d
        buf = T.a[in_off:in_off + in_len]
        ntile = (in_len + CRC_TILE - 1) // CRC_TILE
        per = CRC_WG_TILES if form == "flat" else max(CRC_WG_TILES, (ntile + grid - 1) // grid)
        acc = 0
        nranges = 0
        for tA in range(0, ntile, per):
            tB = min(tA + per, ntile)
            full_end = min(tB * CRC_TILE, in_len // CRC_TILE * CRC_TILE)
            c, range_end = 0, tA * CRC_TILE
            if full_end > range_end:  # whole tiles: acc * x^65536 ^ tile, tile by tile = the CRC of their bytes
                c = raw_crc(buf[range_end:full_end])
                range_end = full_end
            if tB * CRC_TILE > in_len:  # the block's last, ragged tile: a ragged FIRST piece, then 32-byte pieces
                tile = buf[range_end:]
                r = tile.size % CRC_PIECE
                if self.mut == "crc_ragged_last":
                    tc_ = raw_crc(tile[:r]) ^ gf_mul(raw_crc(tile[r:]), pow_x(8 * r))
                else:
                    tc_ = gf_mul(raw_crc(tile[:r]), pow_x(8 * (tile.size - r))) ^ raw_crc(tile[r:])
                c = gf_mul(c, pow_x(8 * tile.size)) ^ tc_
                range_end = in_len
            acc ^= gf_mul(c, pow_x(8 * (in_len - range_end)))
            nranges += 1
        crc = acc ^ gf_mul(U32, pow_x(8 * in_len)) ^ U32
        f["crc:ragged_piece" if in_len % CRC_PIECE else "crc:whole_pieces"] += 1
        f["crc:ragged_tile" if in_len % CRC_TILE else "crc:whole_tiles"] += 1
        f["crc:off%16!=0" if in_off % 16 else "crc:off%16==0"] += 1
        f["crc:ranges>1" if nranges > 1 else "crc:ranges1"] += 1
        f["crc:pos>=64" if pos >= 64 else "crc:pos<64"] += 1
        f["crc:" + form] += 1
        if ntile >= 100:
            f["crc:tiles>=100"] += 1
        return crc, dict(len32=in_len % 32, len8192=in_len % 8192, off16=in_off % 16, ranges=nranges, pos=pos, form=form)


# ---- GF(2) arithmetic of crc_gf.h ----------------------------------------------------------------------------------------
CRC_POLY = 0x04C11DB7
_REV8 = bytes(int("{:08b}".format(i)[::-1], 2) for i in range(256))


def gf_mul(a, b):
    r = 0
    for i in range(31, -1, -1):
        r = ((r << 1) & U32) ^ (CRC_POLY if r >> 31 else 0)
        if (b >> i) & 1:
            r ^= a
    return r


@functools.lru_cache(maxsize=None)
def _pow2(k):
    return 2 if k == 0 else gf_mul(_pow2(k - 1), _pow2(k - 1))


@functools.lru_cache(maxsize=4096)
def pow_x(e):
    r, k = 1, 0
    while e:
        if e & 1:
            r = gf_mul(r, _pow2(k))
        e >>= 1
        k += 1
    return r


def crc_bzip2(buf):
    """CRC-32/BZIP2 (the reflected CRC of zlib over bit-reversed bytes, bit-reversed)"""
    c = zlib.crc32(bytes(buf).translate(_REV8))
    return int("{:032b}".format(c)[::-1], 2)


def raw_crc(buf):
    """the CRC register after `buf` from a zero start, no final XOR: what a thread of crc_range computes of its piece"""
    if len(buf) == 0:
        return 0
    return crc_bzip2(buf) ^ U32 ^ gf_mul(U32, pow_x(8 * len(buf)))


# ---- front end ------------------------------------------------------------------------------------------------------------
class Result:
    pass


def analyse(data, level, mutant=None, start=0, stop=None, tiles=True, crc="flat"):
    """the plan of `data` as plan_split cuts it from `start` (to the first block at or after `stop`), with its record;
    crc: "flat" (the plan's own CRCs), "grid" (plan_crc_range over all blocks) or None"""
    m = Model(data, level, mutant)
    r = Result()
    r.model = m
    r.blocks, r.aux, r.open, r.windows = m.split(start, stop)
    r.facts = m.facts
    r.tiles = [m.emit_tiles(b, d, ax) for b, (d, ax) in enumerate(zip(r.blocks, r.aux))] if tiles else []
    r.crc, r.crcs = [], []
    if crc:
        maxlen = max(d[1] for d in r.blocks)
        grid = min(1024, ((maxlen + CRC_TILE - 1) // CRC_TILE + CRC_WG_TILES - 1) // CRC_WG_TILES)
        for b, d in enumerate(r.blocks):
            c, rec = m.crc_block(b, d, crc, grid)
            r.crcs.append(c)
            r.crc.append(rec)
    r.rle = lambda b: m.emit_bytes(r.blocks[b], r.aux[b])
    return r


def unmet(facts, wanted):
    """the wanted facts the record does not show, as a list of strings (empty: the case reaches its edges).  A wanted entry is
    a fact, "!fact" (must not occur) or (fact, count) for an exact count."""
    bad = []
    for w in wanted:
        if isinstance(w, tuple):
            if facts[w[0]] != w[1]:
                bad.append("%s: %d times, wanted %d" % (w[0], facts[w[0]], w[1]))
        elif w.startswith("!"):
            if facts[w[1:]]:
                bad.append("%s: %d times, wanted never" % (w[1:], facts[w[1:]]))
        else:
            assert w in FACTS or w.startswith(("reject_at:", "kept:")), w
            if not facts[w]:
                bad.append("%s: never" % w)
    return bad
