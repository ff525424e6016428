"""banzai_amd -- MI355X-native bzip2 block encoder with banzai's API and banzai's bits.

Mirrors the public surface of jgbyrne/banzai v0.3.1 (reference lib/lib.rs:84-153):

    encode(reader, writer, level) -> bytes consumed      (lib/lib.rs:84-132)
    encode_file(in_path, out_path) -> bytes consumed     (lib/lib.rs:141-153, level 9)
    encode_many(inputs, level) -> [bytes]               (encode() once per input, in one GPU pass)

and, beyond the reference (which "(currently)" has no decompressor, README.md:9), the way back:

    decompress(data) -> bytes                            (one or more .bz2 streams, as bz2.decompress)
    decode(reader, writer) -> bytes written

and, for a damaged archive, per block what decompress is per input (what bzip2recover is for):

    recover(data) -> Recovered                           (the bytes of every block that verifies, a report of every one that
                                                          does not; .kept, .lost, .complete)
    recover_stream(data, report=None) -> bytes           (the kept blocks, bit for bit, as one valid .bz2 stream)

and random access into a .bz2 without decoding all of it (bzip2 blocks are independent once their start bit is known):

    build_index(data) -> BlockIndex                      (every block: where it starts, what it decodes to; verified)
    decompress_range(data, index, offset, length) -> bytes
    decompress_ranges(data, index, ranges) -> [bytes]    (many (offset, length) reads in one pass: every touched block once)
    IndexedReader(source, index=None)                    (read / seek / readv over the decoded bytes of bytes or a file)
    build_sync_index(data, interval=256) -> SyncIndex    (a BlockIndex plus sync points inside the blocks: a read decodes
                                                          its blocks in parallel segments; accepted wherever a BlockIndex is)
    encode_indexed(reader, writer, level, interval=256)  (encode() that returns that index of the stream it writes: the
                                                          encoder holds it all, no decode pass) -> SyncIndex / BlockIndex

    encode_indexed_stream(reader, writer, level, interval=256)
                                                         (the same index from the streaming encoder: the input is read in
                                                          chunks and never held as a whole)

Everything is computed by hand-written HIP kernels behind the C ABI in include/bzhip.h
(libbzhip.so); there is no CPU path.  `reader` is any object with .read(), `writer` any object
with .write() (the Rust signature takes BufRead / BufWriter<W>).
"""
import collections
import io
import struct
import zlib

import numpy as np

from . import _native

__all__ = ["encode", "encode_many", "encode_file", "decompress", "decompress_many", "decode", "decode_stream", "StreamDecompressor", "build_index", "decompress_range", "decompress_ranges", "BlockIndex", "RecordIndex", "build_record_index", "record_index_of", "decompress_records", "search", "search_range", "grep", "grep_count", "grep_many", "grep_many_count", "matches", "matches_count", "PatternSet", "Regex", "regex_check",
           "IndexedReader", "build_sync_index", "SyncIndex", "encode_indexed", "encode_indexed_stream", "recover", "recover_stream", "Recovered", "RecoveredBlock", "Context", "MultiContext", "BzhError"]

Context = _native.Context
MultiContext = _native.MultiContext
BzhError = _native.BzhError

_ctx_cache = {}
_multi_cache = {}
READ_CHUNK = 16 << 20
# encode_many: bytes (+ one per input) of one bzh_encode_many call -- the plan's 32-bit position range (include/bzhip.h)
MANY_GROUP_LIMIT = 0xFFFF0000


def _ctx(level, device=0):
    key = (device, level)
    if key not in _ctx_cache:
        _ctx_cache[key] = _native.Context(device, level, 0)
    return _ctx_cache[key]


def _copying_sink(writer):
    """True for the writers that are known to copy what write() is handed before it returns (in-memory and real files):
    only they may be given a VIEW of the context's output buffer, which the next feed overwrites.  Any other writer -- a
    list's append, a queue, a transport -- may keep the object, so it gets its own bytes."""
    return isinstance(writer, (io.BytesIO, io.BufferedWriter, io.BufferedRandom, io.FileIO))


def _device_list(devices):
    """`devices=` of encode, or $BZHIP_DEVICES ("0,1,2,3"): the GPUs of one node an encode is spread over."""
    if devices is None:
        import os
        env = os.environ.get("BZHIP_DEVICES", "").strip()
        devices = [int(x) for x in env.split(",") if x.strip() != ""] if env else None
    return [int(d) for d in devices] if devices else None


def encode(reader, writer, level, device=0, devices=None):
    """bzip2-encode everything `reader` yields and write the stream to `writer`.

    Same contract as banzai::encode: `level` in 1..=9 is the block size in 100 kB units
    (anything else raises, the reference asserts at lib/lib.rs:89); returns the number of input
    bytes encoded; I/O errors of reader/writer propagate.

    `devices` (or $BZHIP_DEVICES): a list of HIP devices of this node -- the blocks are then cut and encoded on all of
    them (bzh_create_multi: one host thread and context per device inside the library, the stream assembled on the
    first) and the stream is the one a single device writes, bit for bit.  That path reads the whole input first."""
    if isinstance(level, bool) or not isinstance(level, int) or not 1 <= level <= 9:
        raise ValueError("level must be in 1..=9")
    devs = _device_list(devices)
    if devs and len(devs) > 1:
        data = reader.getvalue()[reader.tell():] if isinstance(reader, io.BytesIO) else reader.read()
        if not isinstance(data, (bytes, bytearray, memoryview)):
            raise TypeError("reader.read() must return bytes")
        key = (tuple(devs), level)
        if key not in _multi_cache:
            _multi_cache[key] = _native.MultiContext(devs, level)
        writer.write(_multi_cache[key].encode(data))
        if isinstance(reader, io.BytesIO):
            reader.seek(0, io.SEEK_END)
        if hasattr(writer, "flush"):
            writer.flush()
        return len(data)
    if devs:
        device = devs[0]
    ctx = _ctx(level, device)
    put = writer.write if _copying_sink(writer) else (lambda view: writer.write(bytes(view)))
    # incremental ingestion (the reference pulls from fill_buf as it goes, lib/rle.rs:30-92): input is
    # handed to the GPU in chunks, finished stream bytes are written as soon as they are final
    ctx.stream_begin()
    # An in-memory reader (io.BytesIO) lends its buffer, as BufRead::fill_buf lends the reference a slice of the
    # reader's own buffer (lib/rle.rs:30-92): the chunks go to the GPU from where they lie, no copy on this side.
    if isinstance(reader, io.BytesIO):
        # (getvalue() hands out the bytes object BytesIO holds -- no copy for a reader made from bytes; getbuffer()
        # would first un-share it, i.e. copy all of it)
        view = memoryview(reader.getvalue())
        pos, end = reader.tell(), len(view)
        while True:
            k = min(READ_CHUNK, max(0, end - pos))
            out = ctx.stream_feed_view(view[pos:pos + k], k == 0)
            pos += k
            if len(out):
                put(out)
            if k == 0:
                break
        reader.seek(pos)
        if hasattr(writer, "flush"):
            writer.flush()
        return ctx.stream_consumed()
    # one reusable buffer: a reader with readinto() fills it in place (no bytes object per chunk); finished stream
    # bytes go to a copying sink (BytesIO, a real file) as a view of the context's output buffer, to any other writer as bytes
    buf = bytearray(READ_CHUNK) if hasattr(reader, "readinto") else None
    while True:
        chunk = None
        if buf is not None:
            try:
                got = reader.readinto(buf)
            except (NotImplementedError, io.UnsupportedOperation):  # e.g. a RawIOBase subclass that only defines read()
                buf = None
            else:
                if got is None:
                    raise TypeError("reader.readinto() must return a byte count (blocking reader expected)")
                chunk = memoryview(buf)[:got]
        if chunk is None:
            chunk = reader.read(READ_CHUNK)
            if not isinstance(chunk, (bytes, bytearray, memoryview)):
                raise TypeError("reader.read() must return bytes")
        eof = len(chunk) == 0
        out = ctx.stream_feed_view(chunk, eof)
        if len(out):
            put(out)
        if eof:
            break
    if hasattr(writer, "flush"):
        writer.flush()
    return ctx.stream_consumed()


def encode_many(inputs, level, device=0):
    """bzip2-encode every item of `inputs` (bytes-like) into a stream of its own -> [bytes], stream k bit-identical to what
    encode() writes for item k alone.  One pass on the GPU per group of inputs (bzh_encode_many): groups stay inside the
    plan's position range, MANY_GROUP_LIMIT bytes with one more per input."""
    if isinstance(level, bool) or not isinstance(level, int) or not 1 <= level <= 9:
        raise ValueError("level must be in 1..=9")
    views = []
    for x in inputs:
        if isinstance(x, str):
            raise TypeError("encode_many takes bytes-like items, not str")
        try:
            views.append(memoryview(x).cast("B"))
        except TypeError:
            raise TypeError(f"encode_many takes bytes-like items, not {type(x).__name__}") from None
    if not views:
        return []
    ctx = _ctx(level, device)
    out, group, size = [], [], 0
    for v in views:
        if group and size + len(v) + 1 > MANY_GROUP_LIMIT:
            out.extend(ctx.encode_many(group))
            group, size = [], 0
        group.append(v)
        size += len(v) + 1
    out.extend(ctx.encode_many(group))
    return out


def encode_file(in_path, out_path, device=0, devices=None):
    """bzip2-encode a file into another file at level 9 (banzai::encode_file)."""
    with open(in_path, "rb") as inf, open(out_path, "wb") as outf:
        return encode(inf, outf, 9, device, devices)


def decompress(data, device=0):
    """Decode one or more complete bzip2 streams lying back to back in `data` (bytes-like) -> the decoded bytes, as
    bz2.decompress does: any level, any encoder.  Bytes behind the last stream that do not start another one are ignored.
    A damaged stream raises BzhError with status -6 (bzh_last_error's text says what and where).  Computed on the GPU on a
    level-9 context (bzh_decode); the output buffer is sized from the input, then once more from what the library reports."""
    if isinstance(data, str):
        raise TypeError("decompress takes a bytes-like object, not str")
    try:
        view = memoryview(data).cast("B")
    except TypeError:
        raise TypeError(f"decompress takes a bytes-like object, not {type(data).__name__}") from None
    return _ctx(9, device).decode(view)


def decompress_many(inputs, device=0, errors="raise"):
    """Decode every item of `inputs` (bytes-like; each one or more complete bzip2 streams, as decompress takes) -> [bytes], item
    k decoded exactly as decompress(item k) would, in one pass on the GPU per group of inputs (bzh_decode_many): one scan, and
    batches that take the blocks of many inputs together.  A damaged item does not touch the others.  errors="raise": the
    first failed item raises BzhError naming it; errors="return": the BzhError instance stands in that item's place.  Groups
    keep a call's inputs below MANY_GROUP_LIMIT bytes, as encode_many's do."""
    if errors not in ("raise", "return"):
        raise ValueError('errors must be "raise" or "return"')
    views = [_bytes_view(x, "decompress_many") for x in inputs]
    if not views:
        return []
    ctx = _ctx(9, device)
    out, group, size = [], [], 0

    def run(group):
        res, status, _ = ctx.decode_many(group, with_status=True)
        text, first = ctx.last_error(), True
        for k, (r, st) in enumerate(zip(res, status)):
            if st != 0:  # (the library words the first failure of a call; the others carry their status)
                err = BzhError(st, text if first else f"decode: input {k} failed")
                first = False
                if errors == "raise":
                    err.args = (f"{err.args[0]} (item {len(out) + k} of decompress_many)",)
                    raise err
                res[k] = err
        out.extend(res)

    for v in views:
        if group and size + len(v) + 1 > MANY_GROUP_LIMIT:
            run(group)
            group, size = [], 0
        group.append(v)
        size += len(v) + 1
    run(group)
    return out


RecoveredBlock = collections.namedtuple("RecoveredBlock", "bit_pos end_bit out_off out_len crc kind flags err_bit")
RecoveredBlock.__doc__ = """One entry of a recovery report (bzh_recover_entry).  kind 0: kept -- its bytes are data[out_off : out_off +
out_len]; else lost, and why (_native.LOST_*).  flags, on kept blocks: _native.REC_JOINED / REC_STREAM_END / REC_STREAM_OK."""


class Recovered(collections.namedtuple("Recovered", "data blocks stats")):
    """What recover() returns: `data`, the bytes of the kept blocks back to back; `blocks`, one RecoveredBlock per block magic
    that is not another block's payload, ascending; `stats`, bzh_recover_stats as a dict."""
    __slots__ = ()

    @property
    def kept(self):
        return [b for b in self.blocks if b.kind == 0]

    @property
    def lost(self):
        return [b for b in self.blocks if b.kind != 0]

    @property
    def complete(self):
        """Nothing is lost, and every kept block lies in a stream that checks out as a whole (STREAM_OK): every block is
        joined to a stream header or to the block before it, and every run of joined blocks ends in an intact footer."""
        bl = self.blocks
        for i, b in enumerate(bl):
            if b.kind != 0 or not b.flags & _native.REC_JOINED:
                return False
            runs_on = i + 1 < len(bl) and bl[i + 1].bit_pos == b.end_bit
            if not runs_on and not b.flags & _native.REC_STREAM_OK:
                return False
        return True


def _blocks_of(entries):
    return [RecoveredBlock(*(int(e[k]) for k in RecoveredBlock._fields)) for e in entries]


def recover(data, device=0):
    """Every block of a damaged .bz2 that still verifies (bzh_recover): `data` (bytes-like) is scanned for block magics at any
    bit alignment and every block is judged on its own -- entropy decode, size, CRC -- whatever became of its neighbours, its
    stream header or its footer.  -> Recovered(data, blocks, stats).  Nothing is raised for damage: an input without one
    block gives empty data and no blocks.  Computed on the GPU on a level-9 context."""
    view = _bytes_view(data, "recover")
    ctx = _ctx(9, device)
    out, ent = ctx.recover(view)
    return Recovered(out, _blocks_of(ent), ctx.recover_stats())


def recover_stream(data, report=None, device=0):
    """The salvage of a damaged .bz2 as one valid .bz2 stream (bzh_recover_stream): "BZh9", the kept blocks' own bits in order,
    a footer with the fold of their CRCs -- bz2.decompress of it gives recover(data).data.  report: a Recovered of the same
    data, its blocks, or a structured array of _native.RECOVER_DTYPE; None: recover(data) is run first.  A report that is not
    well formed for the data raises BzhError (-1; -6 where an entry points at no block magic)."""
    view = _bytes_view(data, "recover_stream")
    if report is not None and not isinstance(report, (Recovered, list, tuple, np.ndarray)):
        raise TypeError(f"report must be a Recovered, a list of RecoveredBlock or an array of RECOVER_DTYPE, not {type(report).__name__}")
    ctx = _ctx(9, device)
    if report is None:
        entries = ctx.recover(view)[1]
    elif isinstance(report, np.ndarray):
        entries = report
    else:
        blocks = report.blocks if isinstance(report, Recovered) else report
        entries = np.array([tuple(b) for b in blocks], dtype=_native.RECOVER_DTYPE)
    return ctx.recover_stream(view, entries)


def decode(reader, writer, device=0):
    """Decode everything `reader` yields (one or more bzip2 streams) and write the bytes to `writer` -> bytes written.
    This path reads the whole input first and writes nothing on damage; decode_stream reads and writes in chunks."""
    data = reader.getvalue()[reader.tell():] if isinstance(reader, io.BytesIO) else reader.read()
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("reader.read() must return bytes")
    out = decompress(data, device)
    if isinstance(reader, io.BytesIO):
        reader.seek(0, io.SEEK_END)
    writer.write(out)
    if hasattr(writer, "flush"):
        writer.flush()
    return len(out)


class StreamDecompressor:
    """Incremental decode of one or more bzip2 streams fed in chunks of any size (bzh_dstream_*), in the shape of
    bz2.BZ2Decompressor: bounded memory whatever the input's size.  window / staging: the targets of the compressed window and
    of the decoded staging buffer on the device, in bytes (None: the library's defaults).  It has a context of its own.

    A damaged input raises BzhError from the call whose pass finds the defect; what earlier calls returned is a prefix of the
    true output made of whole, CRC-verified blocks, and the object is then closed (any later call raises BzhError -5)."""

    OUT_CHUNK = 4 << 20

    def __init__(self, device=0, window=None, staging=None):
        self._ctx = _native.Context(device, 9, 0)
        self._ctx.dstream_set_room(window or 0, staging or 0)
        self._ctx.dstream_begin()
        self._pending = b""
        self._more_out = False
        self._buf = np.empty(self.OUT_CHUNK, dtype=np.uint8)
        self.done = False

    @property
    def needs_input(self):
        """False while decompress(b"", n) can still return bytes without new input, and once the input is finished"""
        return not (self.done or self._pending or self._more_out)

    @property
    def consumed(self):
        """input bytes up to the end of the last stream passed (bzh_decode's consumed)"""
        return self._consumed if self._ctx is None else self._ctx.dstream_consumed()

    def stats(self):
        """bzh_dstream_stats as a dict"""
        return self._ctx.dstream_stats()

    def close(self):
        """Frees the context (the window, the staging buffer, the batch workspace); idempotent"""
        if self._ctx is not None:
            self._consumed = self._ctx.dstream_consumed()
            self._ctx.close()
            self._ctx = None
            self._pending = b""
            self._more_out = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _run(self, eof, max_length):
        parts, total = [], 0
        while not self.done:
            room = self._buf.size if max_length < 0 else min(self._buf.size, max_length - total)
            if room == 0:
                break
            out = self._buf[:room]
            used, got, self.done = self._ctx.dstream_feed(self._pending, eof, out)
            self._pending = self._pending[used:]
            parts.append(out[:got].tobytes())
            total += got
            self._more_out = got == room and not self.done
            if not self._pending and got < room and not eof:
                break
        return b"".join(parts)

    def decompress(self, data, max_length=-1):
        """Feed `data` (bytes-like) -> the decoded bytes that are ready, at most max_length of them when it is >= 0; input not yet
        taken is kept for the next call (needs_input is then False).  After `done`, data is ignored."""
        view = _bytes_view(data, "StreamDecompressor.decompress")
        self._pending = self._pending + view.tobytes() if self._pending else view.tobytes()
        return self._run(False, max_length)

    def finish(self, max_length=-1):
        """The input has ended: the remaining bytes, at most max_length of them; call until `done`.  A truncated input raises."""
        return self._run(True, max_length)


def decode_stream(reader, writer, chunk=8 << 20, device=0):
    """Decode everything `reader` yields (one or more bzip2 streams), reading `chunk` bytes at a time and writing the decoded bytes
    as they arrive -> bytes written.  Memory is bounded whatever the sizes (StreamDecompressor).  Unlike decode(), which writes
    nothing on damage, the bytes in front of a defect that earlier passes verified have been written when BzhError is raised."""
    written = 0
    with StreamDecompressor(device) as d:
        while not d.done:
            data = reader.read(chunk)
            if not isinstance(data, (bytes, bytearray, memoryview)):
                raise TypeError("reader.read() must return bytes")
            if not data:
                break
            out = d.decompress(data)
            written += len(out)
            writer.write(out)
        while not d.done:
            out = d.finish()
            written += len(out)
            writer.write(out)
    if hasattr(writer, "flush"):
        writer.flush()
    return written


def _bytes_view(data, who):
    if isinstance(data, str):
        raise TypeError(f"{who} takes a bytes-like object, not str")
    try:
        return memoryview(data).cast("B")
    except TypeError:
        raise TypeError(f"{who} takes a bytes-like object, not {type(data).__name__}") from None


def _int_arg(v, name):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name} must be an int, not {type(v).__name__}")
    if v < 0:
        raise ValueError(f"{name} must not be negative")
    return v


class BlockIndex:
    """The blocks of an indexed .bz2 input (bzh_decode_index): `.entries` is a numpy structured array of the 40-byte
    bzh_index_entry layout (bit_pos, end_bit, out_off, out_len, crc, stream, level), `.size` the decoded bytes of all streams,
    `.consumed` the bytes of the input that belong to them; len() counts the blocks.  Built once per file, kept beside it with
    to_bytes() / from_bytes()."""

    MAGIC = b"BZhIDX\r\n"
    VERSION = 1
    _HEAD = struct.Struct("<8sIIQQ")  # magic, version, reserved, entries, consumed

    def __init__(self, entries, consumed=0):
        self.entries = np.ascontiguousarray(entries, dtype=_native.INDEX_DTYPE)
        what = self._ill_formed(self.entries)
        if what:
            raise ValueError(f"block index: {what}")
        self.consumed = int(consumed)
        self.size = int(self.entries["out_off"][-1]) + int(self.entries["out_len"][-1]) if self.entries.size else 0

    @staticmethod
    def _ill_formed(e):
        """what bzh_decode_range refuses an index for (None: well formed)"""
        if e.size == 0:
            return None
        if np.any(e["end_bit"] <= e["bit_pos"]):
            return "end_bit is not behind bit_pos"
        if np.any(e["bit_pos"][1:] <= e["bit_pos"][:-1]):
            return "bit_pos does not ascend"
        sums = np.concatenate([np.zeros(1, np.uint64), np.cumsum(e["out_len"][:-1], dtype=np.uint64)])  # (uint64 throughout)
        if np.any(e["out_off"] != sums):
            return "out_off is not the running sum of the sizes before it"
        if np.any((e["level"] < 1) | (e["level"] > 9)):
            return "a level outside 1..9"
        return None

    def __len__(self):
        return int(self.entries.size)

    def span(self, off, length):
        """(first, last, byte_lo, byte_hi): the entries [first, last) that decoded bytes [off, off + length) touch and the
        bytes [byte_lo, byte_hi) of the compressed input that hold them (bzh_index_span; an empty range: first == last)"""
        return _native.index_span(self.entries, _int_arg(off, "offset"), _int_arg(length, "length"))

    def to_bytes(self):
        return self._HEAD.pack(self.MAGIC, self.VERSION, 0, len(self), self.consumed) + self.entries.tobytes()

    @classmethod
    def from_bytes(cls, blob):
        view = _bytes_view(blob, "BlockIndex.from_bytes")
        if len(view) < cls._HEAD.size:
            raise ValueError("block index: truncated header")
        magic, version, _, count, consumed = cls._HEAD.unpack_from(view, 0)
        if magic != cls.MAGIC:
            raise ValueError("block index: bad magic")
        if version != cls.VERSION:
            raise ValueError(f"block index: version {version}, this library reads version {cls.VERSION}")
        if len(view) != cls._HEAD.size + count * _native.INDEX_DTYPE.itemsize:
            raise ValueError(f"block index: {len(view)} bytes do not hold a header and {count} entries")
        return cls(np.frombuffer(view, dtype=_native.INDEX_DTYPE, count=count, offset=cls._HEAD.size).copy(), consumed)


def build_index(data, device=0):
    """Index the bzip2 stream(s) in `data` (bytes-like; the same inputs decompress() takes) -> BlockIndex.  Everything a full
    decode verifies is verified while the index is built, every block and stream CRC included, but nothing is expanded: no
    output buffer is needed.  A damaged stream raises BzhError with status -6."""
    view = _bytes_view(data, "build_index")
    entries, _, consumed = _ctx(9, device).decode_index(view)
    return BlockIndex(entries, consumed)


class SyncIndex:
    """A BlockIndex (`.blocks`) with sync points inside the blocks (bzh_decode_index_sync): `.points` is a numpy structured array
    of the 288-byte bzh_sync_point layout (bit_pos, entry, group, out_pos, run, run_weight, reserved, mtf), one in front of every
    group whose number is a multiple of `.interval`.  With it a read decodes each block it touches in parallel segments.  The
    points are checked against the bytes by every read that uses them (bzh_decode_range_sync), so a blob from a file needs no
    trust; to_bytes() / from_bytes() refuse what is not a whole, well-formed blob."""

    MAGIC = b"BZhSYN\r\n"
    VERSION = 1
    _HEAD = struct.Struct("<8sIIQQII")  # magic, version, interval, bytes of the block index, points, CRC-32 of all the rest, 0

    def __init__(self, blocks, points, interval):
        if not isinstance(blocks, BlockIndex):
            raise TypeError(f"blocks must be a BlockIndex, not {type(blocks).__name__}")
        self.blocks = blocks
        self.points = np.ascontiguousarray(points, dtype=_native.SYNC_DTYPE)
        self.interval = int(interval)
        if not 1 <= self.interval <= 32767:
            raise ValueError(f"sync index: an interval of {self.interval} groups, outside 1..32767")
        what = self._ill_formed(self.blocks.entries, self.points)
        if what:
            raise ValueError(f"sync index: {what}")

    @staticmethod
    def _ill_formed(e, p):
        """what bzh_decode_range_sync refuses the points for (None: well formed)"""
        if p.size == 0:
            return None
        if np.any(p["reserved"] != 0):
            return "reserved is not 0"
        if np.any((p["group"] == 0) | (p["group"] > 32766)):
            return "group outside 1..32766"
        if np.any(p["entry"] >= e.size):
            return "entry outside the index"
        same = p["entry"][1:] == p["entry"][:-1]
        if np.any(p["entry"][1:] < p["entry"][:-1]) or np.any(same & (p["group"][1:] <= p["group"][:-1])):
            return "(entry, group) does not ascend"
        own = e[p["entry"]]
        if np.any((p["bit_pos"] <= own["bit_pos"]) | (p["bit_pos"] >= own["end_bit"])):
            return "bit_pos is not inside its entry"
        if np.any(same & (p["bit_pos"][1:] <= p["bit_pos"][:-1])):
            return "bit_pos does not ascend"
        if np.any(same & (p["out_pos"][1:] < p["out_pos"][:-1])):
            return "out_pos descends"
        if np.any(p["out_pos"].astype(np.uint64) > 100000 * own["level"].astype(np.uint64)):
            return "out_pos beyond the level's block size"
        rw, run1 = p["run_weight"].astype(np.uint64), p["run"].astype(np.uint64) + 1
        if np.any((rw == 0) | ((rw & (rw - np.uint64(1))) != 0) | (rw > (1 << 22))):
            return "run_weight is no power of two up to 2^22"
        if np.any((run1 < rw) | (run1 > 2 * rw - 1)):
            return "run and run_weight do not belong together"
        return None

    # what a BlockIndex answers, so that a SyncIndex stands wherever one does
    @property
    def entries(self):
        return self.blocks.entries

    @property
    def size(self):
        return self.blocks.size

    @property
    def consumed(self):
        return self.blocks.consumed

    def __len__(self):
        return len(self.blocks)

    def span(self, off, length):
        return self.blocks.span(off, length)

    @classmethod
    def _crc(cls, head_fields, body):
        """CRC-32 of the header (its CRC field 0) and everything behind it: no flipped bit passes"""
        return zlib.crc32(body, zlib.crc32(cls._HEAD.pack(*head_fields, 0, 0)))

    def to_bytes(self):
        inner = self.blocks.to_bytes()
        fields = (self.MAGIC, self.VERSION, self.interval, len(inner), int(self.points.size))
        body = inner + self.points.tobytes()
        return self._HEAD.pack(*fields, self._crc(fields, body), 0) + body

    @classmethod
    def from_bytes(cls, blob):
        view = _bytes_view(blob, "SyncIndex.from_bytes")
        if len(view) < cls._HEAD.size:
            raise ValueError("sync index: truncated header")
        magic, version, interval, inner, count, crc, zero = cls._HEAD.unpack_from(view, 0)
        if magic != cls.MAGIC:
            raise ValueError("sync index: bad magic")
        if version != cls.VERSION:
            raise ValueError(f"sync index: version {version}, this library reads version {cls.VERSION}")
        item = _native.SYNC_DTYPE.itemsize
        if inner > len(view) or count > len(view) // item or len(view) != cls._HEAD.size + inner + count * item:
            raise ValueError(f"sync index: {len(view)} bytes do not hold a header, a block index of {inner} bytes and {count} points")
        if zero != 0 or crc != cls._crc((magic, version, interval, inner, count), view[cls._HEAD.size:]):
            raise ValueError("sync index: the blob is damaged (its CRC differs)")
        blocks = BlockIndex.from_bytes(view[cls._HEAD.size:cls._HEAD.size + inner])
        points = np.frombuffer(view, dtype=_native.SYNC_DTYPE, count=count, offset=cls._HEAD.size + inner).copy()
        return cls(blocks, points, interval)


def build_sync_index(data, interval=256, device=0):
    """build_index that also records the sync points (bzh_decode_index_sync): one every `interval` groups of 50 symbols inside
    every block, 288 bytes each -- about 55 a level-9 block of text at the default.  Verified like build_index."""
    view = _bytes_view(data, "build_sync_index")
    if isinstance(interval, bool) or not isinstance(interval, int):
        raise TypeError(f"interval must be an int, not {type(interval).__name__}")
    if not 1 <= interval <= 32767:
        raise ValueError(f"interval must be 1..32767 groups, not {interval}")
    entries, points, _, consumed = _ctx(9, device).decode_index_sync(view, interval)
    return SyncIndex(BlockIndex(entries, consumed), points, interval)


def encode_indexed(reader, writer, level, interval=256, device=0):
    """encode() that also returns the index of the stream it writes, with no decode pass: a SyncIndex with a sync point every
    `interval` groups (what build_sync_index(stream, interval) would build, byte for byte), or a BlockIndex when interval is 0
    (build_index's).  The encoder holds everything an index records while it encodes (bzh_encode_index); the result goes
    straight into decompress_range / IndexedReader.  This path reads the whole input first."""
    if isinstance(level, bool) or not isinstance(level, int) or not 1 <= level <= 9:
        raise ValueError("level must be in 1..=9")
    if isinstance(interval, bool) or not isinstance(interval, int):
        raise TypeError(f"interval must be an int, not {type(interval).__name__}")
    if not 0 <= interval <= 32767:
        raise ValueError(f"interval must be 0 (no sync points) or 1..32767 groups, not {interval}")
    data = reader.getvalue()[reader.tell():] if isinstance(reader, io.BytesIO) else reader.read()
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("reader.read() must return bytes")
    stream, entries, points = _ctx(level, device).encode_index(data, interval)
    if isinstance(reader, io.BytesIO):
        reader.seek(0, io.SEEK_END)
    writer.write(stream)
    if hasattr(writer, "flush"):
        writer.flush()
    blocks = BlockIndex(entries, len(stream))
    return SyncIndex(blocks, points, interval) if interval else blocks


def encode_indexed_stream(reader, writer, level, interval=256, chunk=READ_CHUNK, device=0):
    """encode_indexed for inputs that are never held as a whole: encode()'s feed loop -- `chunk` bytes are read at a time, stream
    bytes are written as they become final -- on a stream that records its index (bzh_stream_begin_index), which is taken after
    every feed (bzh_stream_index_take), so the library holds no more of it than one pass found.  Returns what encode_indexed
    returns for the same input, byte for byte: a SyncIndex, or a BlockIndex when interval is 0, `consumed` the stream's length."""
    if isinstance(level, bool) or not isinstance(level, int) or not 1 <= level <= 9:
        raise ValueError("level must be in 1..=9")
    if isinstance(interval, bool) or not isinstance(interval, int):
        raise TypeError(f"interval must be an int, not {type(interval).__name__}")
    if not 0 <= interval <= 32767:
        raise ValueError(f"interval must be 0 (no sync points) or 1..32767 groups, not {interval}")
    if isinstance(chunk, bool) or not isinstance(chunk, int):
        raise TypeError(f"chunk must be an int, not {type(chunk).__name__}")
    if chunk < 1:
        raise ValueError(f"chunk must be at least 1 byte, not {chunk}")
    ctx = _ctx(level, device)
    put = writer.write if _copying_sink(writer) else (lambda view: writer.write(bytes(view)))
    ents, pts, written = [], [], 0
    ctx.stream_begin_index(interval)
    view = pos = None
    if isinstance(reader, io.BytesIO):  # (lends its buffer, as in encode)
        view, pos = memoryview(reader.getvalue()), reader.tell()
    while True:
        if view is not None:
            data = view[pos:pos + chunk]
            pos += len(data)
        else:
            data = reader.read(chunk)
            if not isinstance(data, (bytes, bytearray, memoryview)):
                raise TypeError("reader.read() must return bytes")
        eof = len(data) == 0
        out = ctx.stream_feed_view(data, eof)
        if len(out):
            written += len(out)
            put(out)
        e, p = ctx.stream_index_take()
        if e.size:
            ents.append(e)
        if p.size:
            pts.append(p)
        if eof:
            break
    if view is not None:
        reader.seek(pos)
    if hasattr(writer, "flush"):
        writer.flush()
    blocks = BlockIndex(np.concatenate(ents) if ents else np.zeros(0, dtype=_native.INDEX_DTYPE), written)
    if not interval:
        return blocks
    return SyncIndex(blocks, np.concatenate(pts) if pts else np.zeros(0, dtype=_native.SYNC_DTYPE), interval)


def _index_arg(index):
    if not isinstance(index, (BlockIndex, SyncIndex)):
        raise TypeError(f"index must be a BlockIndex or a SyncIndex, not {type(index).__name__}")
    return index


def _decode_range(ctx, comp, index, offset, length, lo):
    """bzh_decode_range, or bzh_decode_range_sync when the index has sync points to offer"""
    if isinstance(index, SyncIndex):
        return ctx.decode_range_sync(comp, index.entries, index.points, offset, length, in_byte_base=lo)
    return ctx.decode_range(comp, index.entries, offset, length, in_byte_base=lo)


def decompress_range(data, index, offset, length, device=0):
    """Decoded bytes [offset, offset + length) of the indexed `data` (bytes-like), clipped to the decoded size -> bytes.  Only
    the blocks the range touches are decoded, from only their compressed bytes; each one's CRC is verified, stream CRCs are not
    (build_index has), and damage in other blocks goes unseen.  A block that does not match its entry raises BzhError -6."""
    view = _bytes_view(data, "decompress_range")
    index = _index_arg(index)
    offset, length = _int_arg(offset, "offset"), _int_arg(length, "length")
    _, _, lo, hi = index.span(offset, length)
    return _decode_range(_ctx(9, device), view[lo:hi], index, offset, length, lo)


def _points_arg(index):
    return index.points if isinstance(index, SyncIndex) else None


def _split(blob, offs, lens):
    return [blob[o:o + n] for o, n in zip(offs, lens)]


def decompress_ranges(data, index, ranges, device=0):
    """decompress_range for many (offset, length) pairs in ONE call -> a list of bytes, one per range in the order given, each
    clipped to the decoded size.  The ranges may overlap, repeat, be empty and come in any order; every block they touch is
    decoded and verified once, all of them in shared batches, so many short reads cost about what one costs
    (bzh_decode_ranges).  Of `data` the bytes from the first touched block to the last go to the device: for sparse reads over a
    large archive use IndexedReader.readv, which hands over the touched blocks alone."""
    view = _bytes_view(data, "decompress_ranges")
    index = _index_arg(index)
    r, _ = _native._ranges(ranges)
    _, lo, hi, _ = _native.index_spans(index.entries, r)
    blob, offs, lens = _ctx(9, device).decode_ranges(view[lo:hi], index.entries, r, _points_arg(index), in_byte_base=lo)
    return _split(blob, offs, lens)


_SubIndex = collections.namedtuple("_SubIndex", "touched entries points ranges runs")


def _subindex(index, ranges):
    """The index of the touched blocks alone, for compressed bytes that hold nothing else (host arithmetic over the arrays, no
    device).  -> touched: the entries the ranges touch, ascending; runs: an (n, 2) array of the byte spans [lo, hi) of the
    source to lay back to back, one per run of adjacent touched entries; entries: those of `touched`, bit positions rebased to
    that buffer and out_off the running sum from 0; points: the sync points of those entries, renumbered and rebased the same
    way (None for a BlockIndex); ranges: the ranges, clipped, in the sub-index's output coordinates -- the same bytes."""
    e = index.entries
    r, _ = _native._ranges(ranges)
    touched, _, _, _ = _native.index_spans(e, r)
    t = touched.astype(np.int64)
    se = e[t].copy()
    byte_lo, byte_hi = se["bit_pos"] // np.uint64(8), (se["end_bit"] + np.uint64(7)) // np.uint64(8)
    first = np.ones(t.size, dtype=bool)  # of a run of adjacent entries
    first[1:] = t[1:] != t[:-1] + 1
    last = np.ones(t.size, dtype=bool)
    last[:-1] = first[1:]
    runs = np.stack([byte_lo[first], byte_hi[last]], axis=1) if t.size else np.zeros((0, 2), np.uint64)
    run_base = np.concatenate([np.zeros(1, np.uint64), np.cumsum(runs[:, 1] - runs[:, 0], dtype=np.uint64)[:-1]])
    # what an entry's bit positions lose: its run starts at run_base of the buffer, not at runs[., 0] of the source
    shift = (np.uint64(8) * (runs[:, 0] - run_base))[np.cumsum(first) - 1] if t.size else np.zeros(0, np.uint64)
    se["bit_pos"] -= shift
    se["end_bit"] -= shift
    old_off = se["out_off"].copy()
    se["out_off"] = np.concatenate([np.zeros(1, np.uint64), np.cumsum(se["out_len"][:-1], dtype=np.uint64)])
    # a range's entries are adjacent in both indexes, so it moves as its first entry moves
    total = np.uint64(index.size)
    off = np.minimum(r["off"], total)
    length = np.minimum(r["len"], total - off)
    sub = np.zeros(r.size, dtype=_native.RANGE_DTYPE)
    live = length > 0
    if t.size:
        ends = e["out_off"] + e["out_len"].astype(np.uint64)
        j = np.searchsorted(t, np.searchsorted(ends, off[live], side="right"))  # the touched number of the range's first entry
        sub["off"][live] = off[live] - old_off[j] + se["out_off"][j]
        sub["len"][live] = length[live]
    points = None
    if isinstance(index, SyncIndex):
        p = index.points
        points = p[np.isin(p["entry"], touched)].copy()
        j = np.searchsorted(t, points["entry"])
        points["entry"] = j
        points["bit_pos"] -= shift[j]
    return _SubIndex(touched, se, points, sub, runs)


class RecordIndex:
    """A BlockIndex or SyncIndex (`.index`) with a record table beside it (bzh_decode_index_records): `.rec_cum` is a uint64 array
    of len(index) + 1 words, rec_cum[e] = the `.delim` bytes of the decoded output in front of block e, rec_cum[-1] all of them.
    Record r is the bytes behind delimiter r up to and with delimiter r + 1 (the delimiter belongs to the record it ends); a
    last record without a delimiter counts when it is not empty: len() is `.nrecords`.  The table is checked against the bytes by
    every read that uses it; to_bytes() / from_bytes() refuse what is not a whole, well-formed blob."""

    MAGIC = b"BZhREC\r\n"
    VERSION = 1
    _HEAD = struct.Struct("<8sIIQQII")  # magic, version, delim, entries, nrecords, CRC-32 of all the rest, 0

    def __init__(self, index, delim, rec_cum, nrecords):
        self.index = _index_arg(index)
        self.delim = _delim_arg(delim)
        self.rec_cum = np.ascontiguousarray(rec_cum, dtype=np.uint64)
        self.nrecords = int(nrecords)
        what = self._ill_formed(self.index.entries, self.rec_cum, self.nrecords, self.index.size)
        if what:
            raise ValueError(f"record index: {what}")

    @staticmethod
    def _ill_formed(e, t, nrecords, total):
        """what bzh_decode_records refuses a table for, and a record count that cannot belong to it (None: well formed)"""
        if t.ndim != 1 or t.size != e.size + 1:
            return f"a table of {t.size} words beside {e.size} entries"
        if t[0] != 0:
            return "rec_cum[0] is not 0"
        if np.any(t[1:] < t[:-1]):
            return "the counts descend"
        if np.any(t[1:] - t[:-1] > e["out_len"]):
            return "more delimiters than an entry has bytes"
        d = int(t[-1])
        if nrecords not in ((d,) if total == 0 or d == total else (d, d + 1)):
            return f"{nrecords} records over {d} delimiters"
        return None

    # what the wrapped index answers, so that a RecordIndex stands wherever one does
    @property
    def entries(self):
        return self.index.entries

    @property
    def size(self):
        return self.index.size

    @property
    def consumed(self):
        return self.index.consumed

    def __len__(self):
        return self.nrecords

    def spans(self, ranges):
        """(touched, byte_lo, byte_hi): the blocks a read of these (first record, count) ranges decodes, and the hull of their
        compressed bytes (bzh_record_spans)"""
        return _native.record_spans(self.entries, self.rec_cum, ranges)

    @classmethod
    def _crc(cls, head_fields, body):
        return zlib.crc32(body, zlib.crc32(cls._HEAD.pack(*head_fields, 0, 0)))

    def to_bytes(self):
        fields = (self.MAGIC, self.VERSION, self.delim, len(self.index), self.nrecords)
        body = self.index.to_bytes() + self.rec_cum.tobytes()
        return self._HEAD.pack(*fields, self._crc(fields, body), 0) + body

    @classmethod
    def from_bytes(cls, blob):
        view = _bytes_view(blob, "RecordIndex.from_bytes")
        if len(view) < cls._HEAD.size:
            raise ValueError("record index: truncated header")
        magic, version, delim, count, nrecords, crc, zero = cls._HEAD.unpack_from(view, 0)
        if magic != cls.MAGIC:
            raise ValueError("record index: bad magic")
        if version != cls.VERSION:
            raise ValueError(f"record index: version {version}, this library reads version {cls.VERSION}")
        if delim > 255:
            raise ValueError(f"record index: a delimiter of {delim}, no byte value")
        table = 8 * (count + 1)
        if count >= len(view) // 8 or len(view) < cls._HEAD.size + table:
            raise ValueError(f"record index: {len(view)} bytes do not hold a header, an index and a table of {count} entries")
        if zero != 0 or crc != cls._crc((magic, version, delim, count, nrecords), view[cls._HEAD.size:]):
            raise ValueError("record index: the blob is damaged (its CRC differs)")
        inner = view[cls._HEAD.size:len(view) - table]
        index = (SyncIndex if bytes(inner[:8]) == SyncIndex.MAGIC else BlockIndex).from_bytes(inner)
        if len(index) != count:
            raise ValueError(f"record index: a table of {count} entries beside an index of {len(index)}")
        rec_cum = np.frombuffer(view, dtype=np.uint64, count=count + 1, offset=len(view) - table).copy()
        return cls(index, delim, rec_cum, nrecords)


def _delim_arg(delim):
    if isinstance(delim, (bytes, bytearray)) and len(delim) == 1:
        return delim[0]
    if isinstance(delim, int) and not isinstance(delim, bool) and 0 <= delim <= 255:
        return delim
    raise ValueError("delim must be one byte (bytes of length 1, or an int 0..255)")


def _record_index_arg(rindex):
    if not isinstance(rindex, RecordIndex):
        raise TypeError(f"rindex must be a RecordIndex, not {type(rindex).__name__}")
    return rindex


def build_record_index(data, delim=b"\n", interval=256, device=0):
    """build_sync_index (interval 0: build_index) that also counts the `delim` bytes of every block (bzh_decode_index_records)
    -> RecordIndex.  The count is folded from the bytes behind each block's inverse BWT where its CRC is: nothing is expanded."""
    view = _bytes_view(data, "build_record_index")
    d = _delim_arg(delim)
    if isinstance(interval, bool) or not isinstance(interval, int):
        raise TypeError(f"interval must be an int, not {type(interval).__name__}")
    if not 0 <= interval <= 32767:
        raise ValueError(f"interval must be 0 (no sync points) or 1..32767 groups, not {interval}")
    entries, points, rec_cum, nrecords, _, consumed = _ctx(9, device).decode_index_records(view, interval, d)
    blocks = BlockIndex(entries, consumed)
    return RecordIndex(SyncIndex(blocks, points, interval) if interval else blocks, d, rec_cum, nrecords)


def record_index_of(raw, index, delim=b"\n", device=0):
    """The RecordIndex of `index` from the DECODED bytes it indexes -- after encode_indexed the encoder's own input --, as one
    pass over them at memory bandwidth instead of a decode (bzh_count_records_device).  `raw` is a device tensor of bytes
    (anything with data_ptr() and numel(), as a torch uint8 tensor on the GPU), or bytes-like, which is uploaded with torch."""
    index = _index_arg(index)
    d = _delim_arg(delim)
    if hasattr(raw, "data_ptr") and hasattr(raw, "numel"):
        keep, addr, n = raw, int(raw.data_ptr()), int(raw.numel()) * int(raw.element_size())
    else:
        import torch
        view = _bytes_view(raw, "record_index_of")
        keep = torch.frombuffer(bytearray(view) or bytearray(1), dtype=torch.uint8).to(f"cuda:{device}")
        addr, n = int(keep.data_ptr()), len(view)
        torch.cuda.synchronize(device)
    rec_cum, nrecords = _ctx(9, device).count_records_device(addr, n, index.entries, d)
    del keep
    return RecordIndex(index, d, rec_cum, nrecords)


def _record_atoms(ranges, nrecords):
    """Cuts (first, count) ranges of records -- in any order, overlapping, repeated, empty, behind the end -- at every boundary
    into ascending disjoint atoms, what bzh_decode_records takes.  -> (atoms, spans): atoms is a list of (first, count), spans[r]
    = (i0, i1) says that range r is atoms[i0:i1] joined.  Everything is clipped at nrecords: the empty tail is no record."""
    clipped = []
    for pair in ranges:
        first, count = pair
        first, count = _int_arg(first, "first"), _int_arg(count, "count")
        a = min(first, nrecords)
        clipped.append((a, min(a + count, nrecords)))
    cuts = sorted({c for a, b in clipped if a < b for c in (a, b)})
    at = {c: i for i, c in enumerate(cuts)}
    covered = [0] * (len(cuts) + 1)  # a difference array over the intervals between the cuts
    for a, b in clipped:
        if a < b:
            covered[at[a]] += 1
            covered[at[b]] -= 1
    atoms, atom_of, depth = [], [0] * (len(cuts) + 1), 0
    for i in range(len(cuts) - 1):
        depth += covered[i]
        atom_of[i] = len(atoms)
        if depth > 0:
            atoms.append((cuts[i], cuts[i + 1] - cuts[i]))
    if cuts:
        atom_of[len(cuts) - 1] = len(atoms)
    spans = [(atom_of[at[a]], atom_of[at[b]]) if a < b else (0, 0) for a, b in clipped]
    return atoms, spans


def _read_records(rindex, ranges, fetch, device):
    """decompress_records over `fetch(lo, hi)`, which hands over bytes [lo, hi) of the compressed source"""
    atoms, spans = _record_atoms(ranges, rindex.nrecords)
    if not atoms:
        return [b"" for _ in spans]
    _, lo, hi = rindex.spans(atoms)
    blob, offs, lens = _ctx(9, device).decode_records(fetch(lo, hi), rindex.entries, rindex.rec_cum, atoms, _points_arg(rindex.index),
                                                      in_byte_base=lo, delim=rindex.delim)
    parts = _split(blob, offs, lens)
    return [b"".join(parts[i0:i1]) for i0, i1 in spans]


def decompress_records(data, rindex, ranges, device=0):
    """The records of many (first, count) pairs of the indexed `data` in ONE call -> a list of bytes, one per pair in the order
    given: records first .. first + count - 1, delimiters included, clipped at len(rindex).  The pairs may come in any order,
    overlap, repeat, be empty or lie behind the end.  Only the blocks that hold them are decoded, each once and verified
    (bzh_decode_records); the record boundaries are found on the device."""
    view = _bytes_view(data, "decompress_records")
    return _read_records(_record_index_arg(rindex), ranges, lambda lo, hi: view[lo:hi], device)


class PatternSet(_native.PatternSet):
    """A set of byte strings (1..65536 of 1..256 bytes each) compiled for one pass: grep -F -f FILE, -e A -e B, and with
    `ignore_case` -i over ASCII letters (nothing else folds).  search, search_range, grep, grep_count, IndexedReader.search and
    IndexedReader.grep take it wherever they take `pattern`; the hits of a search then carry two more fields, `pattern` (the
    pattern's index in `patterns`; of patterns that are equal after folding, the lowest) and `len`, and ascend by `off`, then
    `len`.  The set lies on `device`; `.info` says what the compile made of it.  close() frees it (so does the collector)."""

    def __init__(self, patterns, ignore_case=False, device=0):
        pats = [_pattern_arg(p) for p in patterns]
        if not 1 <= len(pats) <= _native.PATSET_MAX_PATTERNS:
            raise ValueError(f"a pattern set holds 1..{_native.PATSET_MAX_PATTERNS} patterns, not {len(pats)}")
        self.device = device
        super().__init__(_ctx(9, device), pats, bool(ignore_case))


def _regex_args(patterns, ignore_case, dotall, max_span, word=False, line=False):
    """what Regex and regex_check are given -> (the expressions, the flags, the span, the syntax word), refused before a device is
    touched.  Assertions are always admitted."""
    if word and line:
        raise ValueError("word=True and line=True exclude each other")
    if isinstance(patterns, str):
        raise TypeError("a regular expression must be bytes-like, not str")
    if isinstance(patterns, (bytes, bytearray, memoryview)):
        patterns = [patterns]
    exprs = []
    for p in patterns:
        if not isinstance(p, (bytes, bytearray, memoryview)):
            raise TypeError(f"a regular expression must be bytes-like, not {type(p).__name__}")
        p = bytes(p)
        if not 1 <= len(p) <= _native.REGEX_MAX_EXPR:
            raise ValueError(f"a regular expression must hold 1..{_native.REGEX_MAX_EXPR} bytes, not {len(p)}")
        exprs.append(p)
    if not 1 <= len(exprs) <= _native.PATSET_MAX_PATTERNS:
        raise ValueError(f"1..{_native.PATSET_MAX_PATTERNS} regular expressions are compiled together, not {len(exprs)}")
    span = _int_arg(max_span, "max_span")
    if not 1 <= span <= _native.REGEX_MAX_SPAN:
        raise ValueError(f"max_span must lie in 1..{_native.REGEX_MAX_SPAN}, not {span}")
    flags = (_native.REGEX_FOLD_ASCII if ignore_case else 0) | (_native.REGEX_DOTALL if dotall else 0)
    return exprs, flags, span, _native.REGEX_ASSERT | (_native.REGEX_WORD if word else 0) | (_native.REGEX_LINE if line else 0)


class Regex(_native.PatternSet):
    """Regular expressions (bytes, or a list of 1..65536 of them, 1..4096 bytes each) compiled into one DFA that every start
    position of the decoded text walks on the device: grep -E.  The syntax is a subset of Python's `re` on bytes -- literals,
    the usual escapes, \\d \\w \\s and their complements, `.`, classes, groups, `|`, `? * + {m} {m,} {m,n}`, and the assertions
    ^ $ \\A \\Z \\b \\B anywhere in an expression, as `re` has them under re.MULTILINE: ^ at offset 0 of the whole decoded text
    and behind every 0x0A, $ at its end and in front of every 0x0A (whatever `delim` a call is given), \\A and \\Z only at the two
    ends, \\b between a byte of [0-9A-Za-z_] and one that is none (the text's ends count as none; folding changes nothing).  An
    assertion sees the real neighbours, also outside the range of a search_range, so every route reports the same hits; it consumes
    nothing, and an expression that can match the empty string (^, ^$, \\b) is refused.  Backreferences, lookaround and lazy
    quantifiers are refused with the expression's number and the byte.  `word=True` matches every expression as grep -w does --
    not preceded and not followed by a word byte, every length tried --, `line=True` as grep -x: ^(?:e)$.  It goes wherever
    `pattern` goes: search, search_range, grep, grep_count, IndexedReader.search and IndexedReader.grep.  A search reports ONE hit
    per start at which some expression matches: `len` is the longest match of at most `max_span` (1..256) bytes, `pattern` the
    lowest-numbered expression that matches exactly that length; overlapping starts are all hits.  A match longer than
    `max_span` is not found; `.info["unbounded"]` says that the expressions have such matches.  `ignore_case` folds ASCII
    letters (re.IGNORECASE on bytes), `dotall` lets `.` take 0x0A.  `.info` carries the fields of bzh_regex_info and of
    bzh_regex_look: `look_behind`, `look_ahead` (1: some assertion sees the byte in front of a start, behind a match; both 0
    without assertions, and the automaton is what it was) and `contexts`."""

    def __init__(self, patterns, ignore_case=False, dotall=False, max_span=256, word=False, line=False, device=0, _no_lds=False):
        exprs, flags, span, syntax = _regex_args(patterns, ignore_case, dotall, max_span, word, line)
        self.device = device
        super().__init__(_ctx(9, device), exprs, flags=flags | (_native.REGEX_NO_LDS if _no_lds else 0), regex=True, max_span=span, syntax=syntax)


def regex_check(patterns, ignore_case=False, dotall=False, max_span=256, word=False, line=False):
    """The compile of Regex alone, on the host, without a device -> the dictionary Regex(...).info would hold; ValueError with the
    compiler's message (the expression's number and the byte) for what it refuses (bzh_regex_check_ex)."""
    import ctypes
    exprs, flags, span, syntax = _regex_args(patterns, ignore_case, dotall, max_span, word, line)
    arr = (ctypes.c_char_p * len(exprs))(*exprs)
    lens = (ctypes.c_size_t * len(exprs))(*[len(e) for e in exprs])
    info, look, err = _native.RegexInfo(), _native.RegexLook(), ctypes.create_string_buffer(256)
    st = _native.lib().bzh_regex_check_ex(arr, lens, len(exprs), flags, span, syntax, ctypes.byref(info), ctypes.byref(look), err, len(err))
    if st != 0:
        raise ValueError(err.value.decode("latin-1"))
    return dict(info.as_dict(), **look.as_dict())


def _pattern_arg(pattern):
    if isinstance(pattern, _native.PatternSet):
        return pattern
    if not isinstance(pattern, (bytes, bytearray, memoryview)):
        raise TypeError(f"pattern must be bytes-like, not {type(pattern).__name__}")
    pattern = bytes(pattern)
    if not 1 <= len(pattern) <= _native.SEARCH_MAX_PATTERN:
        raise ValueError(f"pattern must hold 1..{_native.SEARCH_MAX_PATTERN} bytes, not {len(pattern)}")
    return pattern


def _limit_arg(limit):
    return None if limit is None else _int_arg(limit, "limit")


def search(data, pattern, delim=None, limit=None, device=0):
    """Every occurrence of the byte string `pattern` (1..256 bytes) in the DECODED bytes of `data` (bytes-like .bz2 stream(s)),
    overlapping ones included -> (hits, nhits): hits is a structured array with fields `off` (the offset in the decoded output)
    and `record`, ascending; nhits the exact count.  With `delim` (one byte) `record` is the number of delimiters in front of the
    hit -- the record number read_records takes --, else 0.  `limit` caps the hits returned, not the count.  The decoded bytes
    stay on the device, and everything decompress verifies is verified (bzh_search).  `pattern` may be a PatternSet: every
    (offset, pattern) pair in one pass, with the fields `pattern` and `len` beside the two, by offset, then length."""
    view = _bytes_view(data, "search")
    d = None if delim is None else _delim_arg(delim)
    return _ctx(9, device).search(view, _pattern_arg(pattern), d, _limit_arg(limit))


def _search_range(index, fetch, pattern, offset, length, limit, device):
    """search_range over `fetch(lo, hi)`, which hands over bytes [lo, hi) of the compressed source"""
    rindex = index if isinstance(index, RecordIndex) else None
    index = _index_arg(rindex.index if rindex is not None else index)
    pattern, limit = _pattern_arg(pattern), _limit_arg(limit)
    offset = _int_arg(offset, "offset")
    length = max(0, index.size - offset) if length is None else _int_arg(length, "length")
    # an automaton with assertions looks at the byte in front of the range and at the byte behind it: the blocks of the widened
    # range are decoded, so the compressed bytes of the widened span go up (the hits stay inside the wanted range)
    look = getattr(pattern, "info", {})
    back = min(offset, look.get("look_behind", 0)) if offset > 0 else 0
    _, _, lo, hi = index.span(offset - back, length + back + look.get("look_ahead", 0))
    return _ctx(9, device).search_range(fetch(lo, hi), index.entries, pattern, offset, length, _points_arg(index),
                                        rindex.rec_cum if rindex is not None else None, rindex.delim if rindex is not None else None,
                                        limit, in_byte_base=lo)


def search_range(data, index, pattern, offset=0, length=None, limit=None, device=0):
    """search() inside decoded bytes [offset, offset + length) of the indexed `data`: the hits that lie wholly inside the range,
    from only the blocks it touches, each decoded once and verified against its entry (bzh_search_range).  `index` is a
    BlockIndex, a SyncIndex or a RecordIndex; record numbers come when it is a RecordIndex."""
    view = _bytes_view(data, "search_range")
    return _search_range(index, lambda lo, hi: view[lo:hi], pattern, offset, length, limit, device)


def _context_arg(before, after, context, who="grep"):
    """before / after / context as grep's -B -A -C -> (before, after), each a uint32"""
    if context is not None:
        if before or after:
            raise ValueError(f"{who}: context= stands for before= and after=; give it alone")
        before = after = context
    for name, v in (("before", before), ("after", after)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{who}: {name} must be an integer in [0, 2^32)")
    return int(before), int(after)


def _grep(data, pattern, delim, invert, index, device, count_only, before=0, after=0):
    view = _bytes_view(data, "grep")
    pattern, d = _pattern_arg(pattern), _delim_arg(delim)
    ctx = _ctx(9, device)
    kw = {"before": before, "after": after} if before or after else {}
    if index is None:
        return ctx.grep(view, pattern, d, bool(invert), count_only, **kw)
    index = _index_arg(index)
    return ctx.grep_index(view, index.entries, pattern, _points_arg(index), d, bool(invert), count_only, **kw)


def grep(data, pattern, delim=b"\n", invert=False, index=None, device=0, before=0, after=0, context=None):
    """The records (lines) of the DECODED bytes of `data` (bytes-like .bz2 stream(s)) in which a match of the byte string
    `pattern` (1..256 bytes) starts, or with `invert` those in which none does -> (bytes, entries): the selected records back to
    back, each with its delimiter, and a structured array with fields `record` (the number read_records takes), `off` and `len`
    (in the decoded output) and `out_off` (in the bytes returned).  The records are selected and compacted on the device: only
    they cross to the host, and every block is decoded once.  Everything decompress verifies is verified (bzh_grep).  With
    `index` (a BlockIndex or SyncIndex of `data`) the blocks go through the indexed front, in parallel segments where the index
    has sync points, and are checked against their entries (bzh_grep_index).  `pattern` may be a PatternSet: the records in
    which a match of any of its patterns starts, in one pass (grep -F -f FILE, -e A -e B, -i).
    CONTEXT (grep -B -A -C): with `before` / `after` records of context, or `context` for both, every record within `before` in
    front of a selected record or `after` behind one comes too, once and in order, chosen on the device in the same pass
    (bzh_grep_set_context).  The entries then carry a bool field `context`: True for a record that is there only as context."""
    before, after = _context_arg(before, after, context)
    return _grep(data, pattern, delim, invert, index, device, False, before, after)


def grep_count(data, pattern, delim=b"\n", invert=False, index=None, device=0):
    """The number of records grep() would return; nothing but two words crosses to the host."""
    return _grep(data, pattern, delim, invert, index, device, True)[0]


def _grep_many(inputs, pattern, delim, invert, device, errors, count_only):
    if errors not in ("raise", "return"):
        raise ValueError('errors must be "raise" or "return"')
    views = [_bytes_view(x, "grep_many") for x in inputs]
    pattern, d = _pattern_arg(pattern), _delim_arg(delim)
    if not views:
        return []
    ctx = _ctx(9, device)
    out, group, size = [], [], 0

    def run(group):
        items, res = ctx.grep_many(group, pattern, d, bool(invert), count_only)
        text, first, base = ctx.last_error(), True, len(out)
        for k, it in enumerate(items):
            st = int(it["status"])
            if st != 0:  # (the library words the first failure of a call; the others carry their status)
                err = BzhError(st, text if first else f"decode: input {k} failed")
                first = False
                if errors == "raise":
                    err.args = (f"{err.args[0]} (item {base + k} of grep_many)",)
                    raise err
                out.append(err)
            else:
                out.append(int(it["selected"]) if count_only else res[k])

    for v in views:
        if group and size + len(v) + 1 > MANY_GROUP_LIMIT:
            run(group)
            group, size = [], 0
        group.append(v)
        size += len(v) + 1
    run(group)
    return out


def grep_many(inputs, pattern, delim=b"\n", invert=False, device=0, errors="raise"):
    """grep() over every item of `inputs` (bytes-like; each one or more complete bzip2 streams) in one pass on the GPU per group
    of inputs (bzh_grep_many) -> [(bytes, entries)], item k equal to grep(inputs[k], pattern, delim, invert): the inputs are
    decoded into one device buffer as many texts with walls between them -- no match crosses from one input into the next, record
    numbers and offsets restart with every input, and an assertion of a Regex sees an input's two ends as the text's edges.
    `pattern` is bytes, a PatternSet or a Regex.  A damaged item does not touch the others.  errors="raise": the first failed item
    raises BzhError naming it; errors="return": the BzhError instance stands in that item's place.  Groups keep a call's inputs
    below MANY_GROUP_LIMIT bytes, as decompress_many's do."""
    return _grep_many(inputs, pattern, delim, invert, device, errors, False)


def grep_many_count(inputs, pattern, delim=b"\n", invert=False, device=0, errors="raise"):
    """The number of records grep_many() would return for every item -> [int]; only the counts cross to the host."""
    return _grep_many(inputs, pattern, delim, invert, device, errors, True)


def _matches(data, pattern, delim, index, device, count_only):
    view = _bytes_view(data, "matches")
    pattern = _pattern_arg(pattern)
    d = None if delim is None else _delim_arg(delim)
    ctx = _ctx(9, device)
    if index is None:
        return ctx.matches(view, pattern, d, count_only)
    index = _index_arg(index)
    return ctx.matches_index(view, index.entries, pattern, _points_arg(index), d, count_only)


def _limit_matches(got, limit):
    """the first `limit` matches of (bytes, entries) and their bytes"""
    out, ent = got
    if limit is None or len(ent) <= limit:
        return got
    ent = ent[:limit]
    return out[:int(ent["out_off"][-1] + ent["len"][-1]) if limit else 0], ent


def matches(data, pattern, delim=None, index=None, limit=None, device=0):
    """What grep -o prints: the NON-OVERLAPPING, LEFTMOST-LONGEST matches of `pattern` in the DECODED bytes of `data` (bytes-like
    .bz2 stream(s)) -> (bytes, entries): the matched parts back to back, with no separator, and a structured array with fields
    `off` (in the decoded output), `record`, `pattern`, `len` and `out_off` (in the bytes returned), ascending by `off`.  The
    selection walks a cursor over the whole decoded text: the next match is at the lowest offset at or behind the cursor that holds
    one, it is the longest match there, and the cursor moves behind it -- b"aa" in b"aaaa" has three hits under search() and two
    matches here.  With `delim` (one byte) `record` is the number of delimiters in front of the match, else 0; `pattern` is 0 for
    a byte string.  `pattern` may be a PatternSet or a Regex.  `limit` caps what is returned, not the count (matches_count).  The
    matches are selected and compacted on the device: only they cross to the host (bzh_match; with `index`, a BlockIndex or
    SyncIndex of `data`, bzh_match_index)."""
    return _limit_matches(_matches(data, pattern, delim, index, device, False), _limit_arg(limit))


def matches_count(data, pattern, delim=None, index=None, device=0):
    """The number of matches matches() would return; nothing but two words crosses to the host."""
    return _matches(data, pattern, delim, index, device, True)[0]


class IndexedReader(io.RawIOBase):
    """A seekable, read-only file of the DECODED bytes of `source`: bytes-like, or a seekable binary file holding .bz2
    stream(s).  Every read decodes just the blocks it touches (decompress_range); with a file source it fetches from the file
    only the compressed bytes of those blocks.  index=None reads the source once and builds the index."""

    def __init__(self, source, index=None, device=0):
        super().__init__()
        if hasattr(source, "read") and hasattr(source, "seek"):
            self._file, self._view = source, None
        else:
            self._file, self._view = None, _bytes_view(source, "IndexedReader")
        if index is None:
            if self._file is not None:
                self._file.seek(0)
                data = self._file.read()
                if not isinstance(data, (bytes, bytearray, memoryview)):
                    raise TypeError("source.read() must return bytes")
            else:
                data = self._view
            index = build_index(data, device)
        self.records = index if isinstance(index, RecordIndex) else None  # (read_records / readv_records need one)
        self.index = _index_arg(index.index if self.records is not None else index)
        self._device = device
        self._pos = 0

    @property
    def size(self):
        return self.index.size

    def readable(self):
        return True

    def seekable(self):
        return True

    def writable(self):
        return False

    def tell(self):
        return self._pos

    def seek(self, offset, whence=io.SEEK_SET):
        if isinstance(offset, bool) or not isinstance(offset, int):
            raise TypeError(f"offset must be an int, not {type(offset).__name__}")
        if whence == io.SEEK_SET:
            pos = offset
        elif whence == io.SEEK_CUR:
            pos = self._pos + offset
        elif whence == io.SEEK_END:
            pos = self.index.size + offset
        else:
            raise ValueError(f"invalid whence ({whence})")
        if pos < 0:
            raise ValueError(f"negative seek position {pos}")
        self._pos = pos
        return pos

    def _fetch(self, n):
        """the next n decoded bytes (fewer at the end), the position moved behind them"""
        n = max(0, min(n, self.index.size - self._pos))
        if n == 0:
            return b""
        _, _, lo, hi = self.index.span(self._pos, n)
        if self._file is not None:
            self._file.seek(lo)
            comp = self._file.read(hi - lo)
            if not isinstance(comp, (bytes, bytearray, memoryview)):
                raise TypeError("source.read() must return bytes")
            if len(comp) != hi - lo:
                raise EOFError(f"the source holds {len(comp)} of the {hi - lo} bytes from {lo} on that the index names")
        else:
            comp = self._view[lo:hi]
        out = _decode_range(_ctx(9, self._device), comp, self.index, self._pos, n, lo)
        self._pos += len(out)
        return out

    def readv(self, ranges):
        """The decoded bytes of many (offset, length) pairs in one call -> a list of bytes in the order given, each clipped to
        the size; the position does not move.  Every touched block is decoded once (decompress_ranges), and of the source only
        the touched blocks' compressed bytes are fetched and handed over: one seek and read per run of adjacent blocks."""
        sub = _subindex(self.index, ranges)
        parts = []
        for lo, hi in sub.runs.tolist():
            if self._file is not None:
                self._file.seek(lo)
                comp = self._file.read(hi - lo)
                if not isinstance(comp, (bytes, bytearray, memoryview)):
                    raise TypeError("source.read() must return bytes")
                if len(comp) != hi - lo:
                    raise EOFError(f"the source holds {len(comp)} of the {hi - lo} bytes from {lo} on that the index names")
            else:
                comp = self._view[lo:hi]
            parts.append(comp)
        blob, offs, lens = _ctx(9, self._device).decode_ranges(b"".join(parts), sub.entries, sub.ranges, sub.points)
        return _split(blob, offs, lens)

    def readv_records(self, ranges):
        """The records of many (first, count) pairs in one call (decompress_records) -> a list of bytes in the order given; the
        position does not move.  The reader must have been given a RecordIndex.  Of a file source only the hull of the touched
        blocks' compressed bytes is read (bzh_record_spans)."""
        if self.records is None:
            raise ValueError("reading by records needs a RecordIndex (build_record_index) as the reader's index")

        def fetch(lo, hi):
            if self._file is None:
                return self._view[lo:hi]
            self._file.seek(lo)
            comp = self._file.read(hi - lo)
            if not isinstance(comp, (bytes, bytearray, memoryview)):
                raise TypeError("source.read() must return bytes")
            if len(comp) != hi - lo:
                raise EOFError(f"the source holds {len(comp)} of the {hi - lo} bytes from {lo} on that the index names")
            return comp

        return _read_records(self.records, ranges, fetch, self._device)

    def _fetch_comp(self, lo, hi):
        """bytes [lo, hi) of the compressed source"""
        if self._file is None:
            return self._view[lo:hi]
        self._file.seek(lo)
        comp = self._file.read(hi - lo)
        if not isinstance(comp, (bytes, bytearray, memoryview)):
            raise TypeError("source.read() must return bytes")
        if len(comp) != hi - lo:
            raise EOFError(f"the source holds {len(comp)} of the {hi - lo} bytes from {lo} on that the index names")
        return comp

    def search(self, pattern, start=0, end=None, limit=None):
        """The hits of `pattern` that lie wholly inside decoded bytes [start, end) (end None: the size) -> (hits, nhits) as
        search_range; the position does not move.  Of a file source only the span's compressed bytes are read: one seek, one
        read.  Record numbers come when the reader was given a RecordIndex."""
        start = _int_arg(start, "start")
        length = None if end is None else max(0, _int_arg(end, "end") - start)
        return _search_range(self.records if self.records is not None else self.index, self._fetch_comp, pattern, start, length, limit,
                             self._device)

    def grep(self, pattern, limit=None, before=0, after=0):
        """The records that hold a hit of `pattern` -> a list of (record number, bytes), ascending and unique; a match that spans
        a delimiter belongs to the record of its first byte.  `limit` caps the hits looked at.  The reader must have been given
        a RecordIndex; the records are fetched with one readv_records.  `before` / `after`: the records that far in front of and
        behind a hit record come too, clipped to the table."""
        if self.records is None:
            raise ValueError("grep needs a RecordIndex (build_record_index) as the reader's index")
        before, after = _context_arg(before, after, None, "IndexedReader.grep")
        hits, _ = self.search(pattern, limit=limit)
        recs = [int(r) for r in np.unique(hits["record"])]
        if recs and (before or after):
            last, wide = self.records.nrecords - 1, []
            for r in recs:  # ascending: the runs [r - before, r + after] merge into a sorted list without duplicates
                lo = max(r - before, wide[-1] + 1 if wide else 0)
                wide.extend(range(lo, min(r + after, last) + 1))
            recs = wide
        return list(zip(recs, self.readv_records([(r, 1) for r in recs]))) if recs else []

    def matches(self, pattern, limit=None):
        """matches() over the whole indexed source -> (bytes, entries); the position does not move.  Record numbers come when the
        reader was given a RecordIndex."""
        index = self.index
        _, _, _, hi = index.span(0, index.size)
        d = self.records.delim if self.records is not None else None
        got = _ctx(9, self._device).matches_index(self._fetch_comp(0, hi), index.entries, _pattern_arg(pattern), _points_arg(index), d)
        return _limit_matches(got, _limit_arg(limit))

    def read_records(self, first, count):
        """records first .. first + count - 1 as one bytes object (readv_records of one pair)"""
        return self.readv_records([(first, count)])[0]

    def read(self, n=-1):
        if n is None or n < 0:
            n = max(0, self.index.size - self._pos)
        return self._fetch(n)

    def readall(self):
        return self.read(-1)

    def readinto(self, b):
        m = memoryview(b).cast("B")
        out = self._fetch(len(m))
        m[:len(out)] = out
        return len(out)
