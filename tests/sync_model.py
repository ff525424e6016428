"""Shared by tests/test_sync_host.py and tests/test_gpu_sync.py: builds tests/decode_host/sync_host.cpp (the sync points on
the one-lane CPU build of decode_core.h, with AddressSanitizer and UBSan), runs it over streams and reads its report."""
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bzh_sync_point (include/bzhip.h), 288 bytes; banzai_amd._native.SYNC_DTYPE must be the same
POINT_DTYPE = np.dtype([("bit_pos", "<u8"), ("entry", "<u4"), ("group", "<u4"), ("out_pos", "<u4"), ("run", "<u4"),
                        ("run_weight", "<u4"), ("reserved", "<u4"), ("mtf", "u1", (256,))])
assert POINT_DTYPE.itemsize == 288


def build(tmp_dir):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the sync point model"
    exe = os.path.join(str(tmp_dir), "sync_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "sync_host.cpp")])
    return exe


def run(exe, tmp_path, streams, interval):
    """-> ([(blocks, points as an array of POINT_DTYPE, [(point, byte, bit)] caught flips, [(bit_pos, end_bit, bytes of the last
    column, stored crc, stream, level)] of the blocks)] per stream, totals): the model has
    decoded every segment of every block on its own and thrown its damaged points; any sanitizer report, any segment that does
    not join to the serial column and any damage that goes unnoticed fails the run"""
    fin, fout = os.path.join(str(tmp_path), f"sync_cases_{interval}.bin"), os.path.join(str(tmp_path), f"sync_report_{interval}.txt")
    with open(fin, "wb") as f:
        for s in streams:
            f.write(struct.pack("<I", len(s)))
            f.write(s)
    p = subprocess.run([exe, fin, str(interval), fout], capture_output=True, text=True)
    assert p.returncode == 0, f"sync_host exit status {p.returncode}: {p.stderr[-3000:]}"
    out, totals = [], None
    for line in open(fout):
        f = line.split()
        if f[0] == "C":
            assert int(f[1]) == len(out)
            out.append([int(f[2]), [], [], []])
        elif f[0] == "P":
            out[-1][1].append((int(f[3]), int(f[1]), int(f[2]), int(f[4]), int(f[5]), int(f[6]), 0, list(bytes.fromhex(f[7]))))
        elif f[0] == "E":
            out[-1][3].append(tuple(int(x) for x in f[1:]))
        elif f[0] == "D":
            out[-1][2].append((int(f[1]), int(f[2]), int(f[3])))
        elif f[0] == "S":
            totals = dict(zip(("damaged", "ill_formed", "caught", "differ"), map(int, f[1:])))
    assert len(out) == len(streams) and totals is not None
    res = []
    for blocks, pts, flips, ents in out:
        arr = np.zeros(len(pts), dtype=POINT_DTYPE)
        for k, p in enumerate(pts):
            arr[k] = (p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7])
        res.append((blocks, arr, flips, ents))
    return res, totals


def run_heavy(n=99_000, seed=7):
    """an input whose last column is mostly long runs of the front byte: six byte values in runs of seeded lengths, so that RLE2
    run digits are a large share of the symbols and runs straddle group boundaries; one level-1 block"""
    import random
    rng = random.Random(seed)
    d = bytearray()
    while len(d) < n:
        d += bytes([97 + rng.randrange(6)]) * rng.choice([1, 2, 3, 5, 9, 17, 40, 100, 255, 300])
    return bytes(d[:n])
