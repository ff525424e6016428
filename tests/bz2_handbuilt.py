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
