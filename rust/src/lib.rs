// =-=-= lib.rs =-=-=
// banzai's public surface over libbzhip.so (MI355X).  Signatures are those of the reference
// crate (lib/lib.rs:84-88 and :141-153); every byte is produced by the HIP library.
// NOTE: the build image has no Rust toolchain, so this crate has never been compiled or run; the same
// calling pattern -- the context pool included -- is executed in C by tests/abi_facade.c (test_rust_facade_twin) and through
// the C ABI by banzai_amd/__init__.py and bnzhip.

use std::collections::HashMap;
use std::convert;
use std::ffi::CStr;
use std::fs;
use std::io;
use std::io::Write;
use std::os::raw::{c_char, c_int};
use std::path;
use std::sync::{Mutex, OnceLock};

#[repr(C)]
struct BzhCtx {
    _private: [u8; 0],
}

extern "C" {
    fn bzh_create(ctx: *mut *mut BzhCtx, device: c_int, level: c_int, max_batch: c_int) -> c_int;
    fn bzh_destroy(ctx: *mut BzhCtx);
    fn bzh_strerror(status: c_int) -> *const c_char;
    fn bzh_last_error(ctx: *const BzhCtx) -> *const c_char;
    fn bzh_stream_begin(ctx: *mut BzhCtx) -> c_int;
    fn bzh_stream_bound(ctx: *const BzhCtx, n: usize) -> usize;
    fn bzh_stream_feed(
        ctx: *mut BzhCtx,
        input: *const u8,
        n: usize,
        eof: c_int,
        out: *mut u8,
        cap: usize,
        out_len: *mut usize,
    ) -> c_int;
    fn bzh_stream_consumed(ctx: *const BzhCtx) -> usize;
    // The decoder (beyond the reference, which has none): `decompress` at the end of this file wraps bzh_decode; the rest is declared
    // for callers that need the device path, the statistics or the scan.  BZH_E_CAP (-4) reports the size needed in *out_len; BZH_E_DATA (-6) is a damaged stream.
    fn bzh_decode(
        ctx: *mut BzhCtx,
        input: *const u8,
        n: usize,
        out: *mut u8,
        cap: usize,
        out_len: *mut usize,
        consumed: *mut usize,
    ) -> c_int;
    #[allow(dead_code)]
    fn bzh_decode_device(
        ctx: *mut BzhCtx,
        d_in: *const std::os::raw::c_void,
        n: usize,
        d_out: *mut std::os::raw::c_void,
        cap: usize,
        out_len: *mut usize,
        consumed: *mut usize,
    ) -> c_int;
    #[allow(dead_code)]
    fn bzh_get_decode_stats(ctx: *const BzhCtx, out: *mut BzhDecodeStats) -> c_int;
    #[allow(dead_code)]
    fn bzh_decode_scan(
        ctx: *mut BzhCtx,
        input: *const u8,
        n: usize,
        bitpos: *mut u64,
        kind: *mut u8,
        max: usize,
        count: *mut usize,
    ) -> c_int;
}

/// `bzh_decode_stats` of include/bzhip.h.
#[repr(C)]
#[allow(dead_code)]
pub struct BzhDecodeStats {
    pub ms_scan: f64,
    pub ms_entropy: f64,
    pub ms_unbwt: f64,
    pub ms_unrle: f64,
    pub ms_crc: f64,
    pub ms_total: f64,
    pub streams: u64,
    pub blocks: u64,
    pub candidates: u64,
    pub candidates_off_chain: u64,
    pub in_bytes: u64,
    pub out_bytes: u64,
}

// A context and the two host buffers an encode works with.  They stay together in the pool: the output buffer is sized by
// bzh_stream_bound (a worst case of a few hundred megabytes for a 100 MB input) and `resize` zero-fills what it adds -- once
// per pooled context, not once per call (per call it cost more than the encode: tests/abi_facade.c measures both).
struct Ctx {
    handle: *mut BzhCtx,
    out: Vec<u8>,
    stage: Vec<u8>,
}

impl Drop for Ctx {
    fn drop(&mut self) {
        unsafe { bzh_destroy(self.handle) }
    }
}

// A context is used by one thread at a time, and may move between threads between calls (include/bzhip.h).
unsafe impl Send for Ctx {}

// Process-wide pool of contexts, keyed by (device, level) -- what banzai_amd/__init__.py keeps in `_contexts`.
// A context owns its workspace arena (56 MB per bzip2 block of a batch: 6.3 GB for a 100 MB input), allocated and
// first-touched on the first encode that needs it; a caller that loops over files through `encode` must not pay that --
// nor `bzh_create` -- per call.  `encode` checks a context OUT of the pool (two threads never share one), and back
// IN when its stream ended cleanly; a context whose stream failed is dropped.  At most POOL_KEEP idle contexts a key.
const POOL_KEEP: usize = 2;
const STAGE: usize = 4 << 20; // small fill_buf slices are coalesced into feeds of this size
static POOL: OnceLock<Mutex<HashMap<(c_int, usize), Vec<Ctx>>>> = OnceLock::new();

fn checkout(device: c_int, level: usize) -> io::Result<Ctx> {
    let pool = POOL.get_or_init(|| Mutex::new(HashMap::new()));
    if let Some(ctx) = pool.lock().unwrap().get_mut(&(device, level)).and_then(|v| v.pop()) {
        return Ok(ctx);
    }
    let mut handle: *mut BzhCtx = std::ptr::null_mut();
    let status = unsafe { bzh_create(&mut handle, device, level as c_int, 0) };
    if status != 0 {
        return Err(to_io_error(std::ptr::null(), status));
    }
    Ok(Ctx { handle, out: Vec::new(), stage: Vec::with_capacity(STAGE) })
}

fn checkin(device: c_int, level: usize, ctx: Ctx) {
    let pool = POOL.get_or_init(|| Mutex::new(HashMap::new()));
    let mut map = pool.lock().unwrap();
    let idle = map.entry((device, level)).or_default();
    if idle.len() < POOL_KEEP {
        idle.push(ctx);
    } // (else: dropped here, bzh_destroy)
}

fn to_io_error(ctx: *const BzhCtx, status: c_int) -> io::Error {
    let text = unsafe {
        let head = CStr::from_ptr(bzh_strerror(status)).to_string_lossy().into_owned();
        if ctx.is_null() {
            head
        } else {
            format!("{}: {}", head, CStr::from_ptr(bzh_last_error(ctx)).to_string_lossy())
        }
    };
    io::Error::new(io::ErrorKind::Other, text)
}

/// bzip2 encode an input stream and write the output to a `BufWriter`
///
/// `level` must be in `1..=9` and describes the block size (`level * 100_000`).
/// Returns the number of input bytes encoded.  Same contract as banzai 0.3.1; the GPU device is
/// taken from `BZHIP_DEVICE` (default 0).
pub fn encode<R, W>(mut reader: R, mut writer: io::BufWriter<W>, level: usize) -> io::Result<usize>
where
    R: io::BufRead,
    W: io::Write,
{
    assert!(1 <= level && level <= 9);

    let device: c_int = std::env::var("BZHIP_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
    let mut ctx = checkout(device, level)?; // (an error below drops it: only a context whose stream ended cleanly goes back)
    let handle = ctx.handle; // (a copy of the raw pointer: the closure below borrows the context's buffers only)
    let status = unsafe { bzh_stream_begin(handle) };
    if status != 0 {
        return Err(to_io_error(handle, status));
    }

    // Pull from the reader as the reference does (fill_buf / consume, lib/rle.rs:43-91).  A BufReader hands
    // out 8 KiB slices by default (bnz/src/main.rs:263); every bzh_stream_feed call is one blocking H2D copy,
    // so small slices are coalesced into a staging buffer of STAGE bytes and fed from there; slices of STAGE
    // bytes or more go straight through.  The library buffers what it must and returns stream bytes as soon
    // as they are final.
    let out = &mut ctx.out; // (the pooled context's buffers: disjoint fields, borrowed until the loop below ends)
    let stage = &mut ctx.stage;
    stage.clear();
    let mut feed = |chunk: &[u8], eof: bool, writer: &mut io::BufWriter<W>| -> io::Result<()> {
        let cap = unsafe { bzh_stream_bound(handle, chunk.len()) };
        if out.len() < cap {
            out.resize(cap, 0);
        }
        let mut out_len = 0usize;
        let status = unsafe {
            bzh_stream_feed(handle, chunk.as_ptr(), chunk.len(), eof as c_int, out.as_mut_ptr(), out.len(), &mut out_len)
        };
        if status != 0 {
            return Err(to_io_error(handle, status));
        }
        writer.write_all(&out[..out_len])
    };
    loop {
        let len = {
            let buf = reader.fill_buf()?;
            if buf.is_empty() {
                feed(&stage[..], true, &mut writer)?; // end of input: whatever is staged, with the eof mark
                break;
            }
            if stage.is_empty() && buf.len() >= STAGE {
                feed(buf, false, &mut writer)?;
            } else {
                stage.extend_from_slice(buf);
                if stage.len() >= STAGE {
                    feed(&stage[..], false, &mut writer)?;
                    stage.clear();
                }
            }
            buf.len()
        };
        reader.consume(len);
    }
    writer.flush()?;
    let consumed = unsafe { bzh_stream_consumed(handle) };
    checkin(device, level, ctx);
    Ok(consumed)
}

/// bzip2 encode a file and write the output to another file (level 9)
///
/// Returns the number of bytes encoded.
pub fn encode_file<I, O>(in_path: I, out_path: O) -> io::Result<usize>
where
    I: convert::AsRef<path::Path>,
    O: convert::AsRef<path::Path>,
{
    let inf = fs::File::open(in_path.as_ref())?;
    let outf = fs::File::create(out_path.as_ref())?;
    // large reads: each fill_buf slice becomes one H2D copy (see encode)
    encode(io::BufReader::with_capacity(16 << 20, inf), io::BufWriter::new(outf), 9)
}

/// Decode one or more complete bzip2 streams lying back to back in `data` (any level, any encoder), as `bzip2 -d` does.
///
/// Beyond banzai 0.3.1, which has no decompressor.  A damaged stream is an `io::Error` that names the kind, the stream,
/// the block and the bit position.  The output is sized from the input, then once more from what the library reports.
pub fn decompress(data: &[u8]) -> io::Result<Vec<u8>> {
    let device: c_int = std::env::var("BZHIP_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
    let ctx = checkout(device, 9)?; // (an error below drops it)
    let handle = ctx.handle;
    let mut cap = data.len() * 6 + 65536;
    let mut out: Vec<u8> = Vec::new();
    let mut status: c_int = 0;
    for _ in 0..2 {
        out.resize(cap, 0);
        let (mut out_len, mut consumed) = (0usize, 0usize);
        status = unsafe { bzh_decode(handle, data.as_ptr(), data.len(), out.as_mut_ptr(), cap, &mut out_len, &mut consumed) };
        if status == -4 {
            cap = out_len; // BZH_E_CAP: the size needed
            continue;
        }
        out.truncate(out_len);
        break;
    }
    if status != 0 {
        return Err(to_io_error(handle, status));
    }
    checkin(device, 9, ctx);
    Ok(out)
}
