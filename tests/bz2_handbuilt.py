"""Hand-built bzip2 blocks for the decoder tests: a one-block stream framed around a CHOSEN string of RLE1 bytes, the way
tests/golden/pymodel.py's encode frames a block (its stage functions do the work).  libbz2's encoder never writes a count
byte above 251 nor a completely full block, and no encoder ends a block in four equal bytes without a count; these do."""
from tests.golden import pymodel


def unrle(rle):
    """libbz2's inverse RLE1 (four equal bytes, then a count byte) -> (bytes, True) or (bytes so far, False) when the
    block ends in four equal bytes without a count"""
    out = bytearray()
    same, prev = 0, -1
    for b in rle:
        if same == 4:
            out += bytes([prev]) * b
            same, prev = 0, -1
            continue
        if b == prev:
            same += 1
        else:
            same, prev = 1, b
        out.append(b)
    return bytes(out), same != 4


def stream_of_rle(rle, level, raw=None):
    """one-block .bz2 stream whose block holds exactly the RLE1 bytes `rle`; the CRCs are those of `raw` (default: what
    libbz2's rule makes of `rle`)"""
    assert 1 <= len(rle) <= 100_000 * level
    if raw is None:
        raw, _ = unrle(rle)
    chk = pymodel.checksum(raw)
    bits = pymodel.Bits()
    bits.put_bytes(b"BZh" + bytes([48 + level]))
    col, ptr = pymodel.bwt(bytes(rle))
    present = [False] * 256
    for byte in set(col):
        present[byte] = True
    bits.put_bytes(bytes.fromhex("314159265359"))
    bits.put(chk, 32)
    bits.put(0, 1)
    bits.put(ptr, 24)
    sector_map, sectors = 0, []
    for a in range(16):
        sector = 0
        for b in range(16):
            sector = (sector << 1) | (1 if present[(a << 4) | b] else 0)
        sector_map = (sector_map << 1) | (1 if sector else 0)
        if sector:
            sectors.append(sector)
    bits.put(sector_map, 16)
    for sct in sectors:
        bits.put(sct, 16)
    syms, num_syms, freqs = pymodel.mtf_and_rle(col, present)
    pymodel.huffman_encode(bits, syms, num_syms, freqs, None)
    bits.put_bytes(bytes.fromhex("177245385090"))
    bits.put(chk, 32)  # one block: the stream CRC is the block's
    return bits.close()


# ---- a block with a CHOSEN entropy stage and a CHOSEN last column ---------------------------------------------------------
# Every encoder here writes codes of at most 17 bits, complete codes, exactly as many selectors as groups, and a last column that
# is the BWT of something.  The format allows more, and libbz2 reads it: code lengths up to 20, incomplete codes, selectors
# beyond the last group (32,767 at most), and any column with any origin pointer below its length.
class Built:
    """what stream_of_column wrote: .stream, .expected (the bytes its column stands for), .crc of them,
    .nblock, .level, and what the block really exercises --
      .nsyms            symbols written, the end-of-block symbol included
      .groups           groups of 50 those symbols need
      .nsel             selectors written
      .longest_code     the longest code of any symbol written
      .positions        the set of MTF positions written (>= 1; position 0 only ever shows as a run)
      .selector_slots   the set of unary positions the selectors were written at, in the move-to-front list of tables
      .zero_runs        the run lengths, in order
      .runs_across_groups  how many runs have their digits in two groups"""


def inverse_column(col, origptr):
    """libbz2's inverse transform, serially: tt from a stable counting sort of the column, the walk from tt[origptr].  Any column
    will do: one that is no BWT of anything walks cycles of tt that do not cover it."""
    n = len(col)
    order = sorted(range(n), key=col.__getitem__)  # stable: tt[cftab[b]++] = i
    out = bytearray(n)
    pos = order[origptr]
    for i in range(n):
        out[i] = col[pos]
        pos = order[pos]
    return bytes(out)


def column_of_events(alphabet, events):
    """the column that mtf_and_rle turns into the wanted symbols: an event is an int p >= 1 (MTF position p: the next byte is
    recency[p]) or a tuple ("run", k) (k times the byte at the front).  A run must not follow a run: the two would be one."""
    recency = sorted(set(alphabet))
    col = bytearray()
    after_run = False
    for ev in events:
        if isinstance(ev, tuple):
            assert ev[0] == "run" and ev[1] >= 1 and not after_run
            col += bytes([recency[0]]) * ev[1]
            after_run = True
        else:
            assert 1 <= ev < len(recency)
            b = recency.pop(ev)
            recency.insert(0, b)
            col.append(b)
            after_run = False
    assert set(col) == set(alphabet), "every byte of the alphabet must show in the column (the symbol map is taken from it)"
    return bytes(col)


def canonical_codes(table):
    """(length, code) a symbol, as pymodel.huffman_encode assigns them: by length, then by symbol"""
    coding = [None] * len(table)
    word = 0
    for ln in range(min(table), max(table) + 1):
        for s, l in enumerate(table):
            if l == ln:
                coding[s] = (ln, word)
                word += 1
        word <<= 1
    return coding


def stream_of_column(col, origptr, level, tables, selectors, extra_selectors=(), raw=None, damage=None):
    """one-block .bz2 stream around the last column `col` and `origptr`, coded with the code-length `tables` (lists over the
    block's alphabet: the bytes in use + 2), table selectors[g] for the g-th group of 50 symbols (a list, or a function of g), and
    `extra_selectors` written behind the last group.  The CRCs are those of `raw` (default: what libbz2's rules make of the column).  -> Built.

    damage: a dict that breaks the block on purpose (nothing is checked then) --
      "syms": the symbols to write instead of the column's;  "origptr" / "ntables" / "nsel": the value of that field;
      "slots": the unary positions to write the selectors at;  "bits": {symbol index: (value, nbits)} written in its place;
      "unchecked": nothing of its own -- the arguments themselves are outside the format"""
    damage = damage or {}
    col = bytes(col)
    present = [False] * 256
    for byte in set(col):
        present[byte] = True
    syms, num_syms, _ = pymodel.mtf_and_rle(col, present)
    syms = damage.get("syms", syms)
    groups = (len(syms) + 49) // 50
    if callable(selectors):
        selectors = [selectors(g) for g in range(groups)]
    if not damage:
        assert 1 <= len(col) <= 100_000 * level and 0 <= origptr < len(col)
        assert 2 <= len(tables) <= 6 and all(len(t) == num_syms and 1 <= min(t) and max(t) <= 20 for t in tables)
        assert len(selectors) == groups and 1 <= groups + len(extra_selectors) <= 32767
        assert all(0 <= t < len(tables) for t in list(selectors) + list(extra_selectors))
    b = Built()
    b.level, b.nblock, b.nsyms, b.groups = level, len(col), len(syms), groups
    b.expected = raw  # (a damaged block carries the CRC of its column all the same, where it has one: only the damage is wrong)
    if raw is None and 0 <= origptr < len(col) and len(col) <= 900_000:
        b.expected = unrle(inverse_column(col, origptr))[0]
    b.crc = pymodel.checksum(b.expected) if b.expected is not None else 0
    bits = pymodel.Bits()
    bits.put_bytes(b"BZh" + bytes([48 + level]))
    bits.put_bytes(bytes.fromhex("314159265359"))
    bits.put(b.crc, 32)
    bits.put(0, 1)
    bits.put(damage.get("origptr", origptr), 24)
    sector_map, sectors = 0, []
    for hi in range(16):
        sector = 0
        for lo in range(16):
            sector = (sector << 1) | (1 if present[(hi << 4) | lo] else 0)
        sector_map = (sector_map << 1) | (1 if sector else 0)
        if sector:
            sectors.append(sector)
    bits.put(sector_map, 16)
    for sct in sectors:
        bits.put(sct, 16)
    written = list(selectors) + list(extra_selectors)
    order = list(range(max(6, len(tables))))
    slots = []
    for sel in written:
        j = order.index(sel)
        slots.append(j)
        order.insert(0, order.pop(j))
    slots = damage.get("slots", slots)
    bits.put(damage.get("ntables", len(tables)), 3)
    bits.put(damage.get("nsel", len(slots)), 15)
    for j in slots:
        bits.put((1 << (j + 1)) - 2, j + 1)  # j ones and a zero
    for table in tables:
        bits.put(table[0], 5)
        acc = table[0]
        for ln in table:
            while ln != acc:
                bits.put(2 if ln > acc else 3, 2)
                acc += 1 if ln > acc else -1
            bits.put(0, 1)
    codings = [canonical_codes(t) for t in tables]
    b.longest_code = 0
    for i, s in enumerate(syms):
        if i in damage.get("bits", {}):
            bits.put(*damage["bits"][i])
            continue
        ln, word = codings[selectors[i // 50] if i // 50 < len(selectors) else 0][s]
        bits.put(word & ((1 << ln) - 1) if damage else word, ln)  # (a broken table may number more codes than its lengths hold)
        b.longest_code = max(b.longest_code, ln)
    bits.put_bytes(bytes.fromhex("177245385090"))
    bits.put(b.crc, 32)  # one block: the stream CRC is the block's
    b.stream = bits.close()
    b.nsel = len(slots)
    b.selector_slots = set(slots)
    b.positions, b.zero_runs, b.runs_across_groups = set(), [], 0
    run, weight, first = 0, 1, 0
    for i, s in enumerate(syms):
        if s <= 1:
            first = i if weight == 1 else first
            run += weight << s
            weight <<= 1
            continue
        if run:
            b.zero_runs.append(run)
            b.runs_across_groups += first // 50 != (i - 1) // 50
            run, weight = 0, 1
        if s != num_syms - 1:
            b.positions.add(s - 1)
    return b
