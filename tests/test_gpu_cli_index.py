"""bnzhip and index files: --index / --interval while compressing, --make-index for an existing .bz2, -d --index --range.  The
argument errors need no device; everything else runs on the GPU, against build_sync_index / build_index of the stream and
slices of the input."""
import bz2
import os
import subprocess

import pytest

from tests import esync_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "banzai_amd", "bnzhip")
ERR_ARGS, ERR_FILESYSTEM, ERR_OUTPUT = 1, 2, 3  # bnz/src/main.rs:11-14; 3 is what -d exits with for a damaged input


@pytest.fixture(scope="module")
def cli(native):
    assert os.path.exists(BIN), "build with `make -C banzai_amd/csrc`"
    return BIN


def run(cli, *args, stdin=None):
    return subprocess.run([cli, *[str(a) for a in args]], input=stdin, capture_output=True)


def test_argument_errors(cli, tmp_path):
    f = tmp_path / "f.bz2"
    f.write_bytes(b"")
    x = tmp_path / "f.bzi"
    for args in (("-d", "--range", "0:1", "-c", f),                               # --range without --index
                 ("-d", "--stream", "--index", x, "--range", "0:1", "-c", f),     # with --stream
                 ("--recover", "--index", x, "--range", "0:1", "-c", f),          # with --recover
                 ("-d", "--index", x, "--range", "0:1", "-c", "-"),               # on standard in
                 ("--index", x, "--range", "0:1", "-c", f),                       # without -d
                 ("-d", "--index", x, "--range", "0:1", f),                       # no --output / --stdout
                 ("-d", "--index", x, "-c", f),                                   # -d --index without a range
                 ("-d", "--index", x, "--range", "5", "-c", f),                   # not <off>:<len>
                 ("-d", "--index", x, "--range", "5:-1", "-c", f),
                 ("-d", "--index", x, "--range", "a:1", "-c", f),
                 ("-d", "--index", x, "--range", "1:99999999999999999999999", "-c", f),
                 ("-d", "--index", x, "--range", "-c", f),
                 ("-d", "--index", x, "-c", f, "--range"),
                 ("--index", "-c", f),                                            # --index needs a path
                 ("--index", x, "--index", x, f),
                 ("--interval", "16", "-c", f),                                   # --interval alone
                 ("--index", x, "--interval", "32768", f),
                 ("--index", x, "--interval", "x", f),
                 ("--index", x, "--interval"),
                 ("-d", "--index", x, "--interval", "16", "--range", "0:1", "-c", f),
                 ("--make-index", x, "-d", f),                                    # --make-index takes nothing else
                 ("--make-index", x, "-c", f),
                 ("--make-index", x, "--index", x, f),
                 ("--make-index", x, "-1", f),
                 ("--make-index", f)):
        r = run(cli, *args)
        assert r.returncode == ERR_ARGS, (args, r.returncode, r.stderr)
    assert not x.exists() and f.read_bytes() == b""
    assert b"--make-index" in run(cli, "--help").stderr


@pytest.fixture(scope="module")
def made(cli, tmp_path_factory):
    """f (350,000 bytes of text), f.bz2 written at level 1 with --index f.bzi --interval 16: made once, never changed"""
    d = tmp_path_factory.mktemp("cli_index")
    data = esync_model.text(350_000, 41)
    f = d / "f"
    f.write_bytes(data)
    r = run(cli, "-1", "-k", "--index", d / "f.bzi", "--interval", "16", f)
    assert r.returncode == 0, r.stderr
    return d, data


@pytest.mark.gpu
def test_index_written_while_compressing(cli, made):
    import banzai_amd
    d, data = made
    stream = (d / "f.bz2").read_bytes()
    r = run(cli, "-1", "-c", d / "f")
    assert r.returncode == 0 and r.stdout == stream and (d / "f").exists()
    blob = (d / "f.bzi").read_bytes()
    ix = banzai_amd.SyncIndex.from_bytes(blob)
    assert ix.to_bytes() == blob == banzai_amd.build_sync_index(stream, 16).to_bytes()
    assert ix.consumed == len(stream) and len(ix) == 4
    # --interval 0: a block index blob; through a pipe, the stream on standard out
    r = run(cli, "-1", "-c", "--index", d / "b.bzi", "--interval", "0", "-", stdin=data)
    assert r.returncode == 0 and r.stdout == stream
    assert (d / "b.bzi").read_bytes() == banzai_amd.build_index(stream).to_bytes()
    # the default interval is 256
    r = run(cli, "-1", "-c", "--index", d / "c.bzi", d / "f")
    assert r.returncode == 0 and r.stdout == stream
    assert (d / "c.bzi").read_bytes() == banzai_amd.build_sync_index(stream, 256).to_bytes()


@pytest.mark.gpu
def test_make_index(cli, made):
    import banzai_amd
    d, data = made
    lib = d / "lib.bz2"
    lib.write_bytes(bz2.compress(data, 1))  # libbz2's stream: other tables, other bits
    r = run(cli, "--make-index", d / "lib.bzi", "--interval", "16", lib)
    assert r.returncode == 0 and r.stdout == b"" and lib.exists(), r.stderr
    assert (d / "lib.bzi").read_bytes() == banzai_amd.build_sync_index(lib.read_bytes(), 16).to_bytes()
    r = run(cli, "--make-index", d / "lib0.bzi", "--interval", "0", lib)
    assert r.returncode == 0 and (d / "lib0.bzi").read_bytes() == banzai_amd.build_index(lib.read_bytes()).to_bytes()
    r = run(cli, "--make-index", d / "lib256.bzi", lib)
    assert r.returncode == 0 and (d / "lib256.bzi").read_bytes() == banzai_amd.build_sync_index(lib.read_bytes(), 256).to_bytes()
    bad = d / "bad.bz2"
    bad.write_bytes(lib.read_bytes()[:5000])
    r = run(cli, "--make-index", d / "bad.bzi", bad)
    assert r.returncode == ERR_OUTPUT and not (d / "bad.bzi").exists() and bad.exists()


@pytest.mark.gpu
def test_ranges(cli, made):
    import banzai_amd
    d, data = made
    ix = banzai_amd.SyncIndex.from_bytes((d / "f.bzi").read_bytes())
    b1 = int(ix.entries["out_off"][1])
    n = len(data)

    def read(*ranges, index=d / "f.bzi", src=d / "f.bz2"):
        args = []
        for off, length in ranges:
            args += ["--range", f"{off}:{length}"]
        return run(cli, "-d", "--index", index, *args, "-c", src)

    for ranges in ([(1000, 300)],                               # inside a block
                   [(b1 - 100, 5000)],                          # across blocks
                   [(b1 - 1, n)],                               # across all the rest
                   [(300_000, 70), (5, 10)],                    # two ranges out of order
                   [(n - 50, 1000)],                            # reaching past the end: clipped
                   [(n, 10)], [(n + 12345, 1 << 40)],           # wholly past the end: no bytes, exit 0
                   [(0, 0)],
                   [(7, 3), (n + 1, 5), (7, 3), (0, n)]):
        r = read(*ranges)
        want = b"".join(data[off:off + length] for off, length in ranges)
        assert r.returncode == 0 and r.stdout == want, (ranges, r.returncode, r.stderr)
    assert (d / "f.bz2").exists()
    # to a file
    out = d / "part"
    r = run(cli, "-d", "--index", d / "f.bzi", "--range", "99990:20", "--output", out, d / "f.bz2")
    assert r.returncode == 0 and out.read_bytes() == data[99990:100010] and (d / "f.bz2").exists()
    # a block index serves as well
    run(cli, "-1", "-c", "--index", d / "blocks.bzi", "--interval", "0", d / "f")
    r = read((b1 - 3, 6), index=d / "blocks.bzi")
    assert r.returncode == 0 and r.stdout == data[b1 - 3:b1 + 3]


@pytest.mark.gpu
def test_index_files_that_are_damaged_or_another_files(cli, made):
    d, data = made
    blob = bytearray((d / "f.bzi").read_bytes())
    for bit in (3, 8 * 12 + 1, 8 * 33, 8 * 200 + 5, 8 * (len(blob) - 1)):  # magic, interval, CRC, an entry, the last point
        b = bytearray(blob)
        b[bit // 8] ^= 1 << (bit % 8)
        (d / "flip.bzi").write_bytes(b)
        r = run(cli, "-d", "--index", d / "flip.bzi", "--range", "0:100", "-c", d / "f.bz2")
        assert r.returncode == ERR_FILESYSTEM and r.stdout == b"", (bit, r.returncode, r.stderr)
    (d / "cut.bzi").write_bytes(blob[:-1])
    assert run(cli, "-d", "--index", d / "cut.bzi", "--range", "0:100", "-c", d / "f.bz2").returncode == ERR_FILESYSTEM
    assert run(cli, "-d", "--index", d / "none.bzi", "--range", "0:100", "-c", d / "f.bz2").returncode == ERR_FILESYSTEM
    # the index of another file: well formed, wrong for the bytes
    other = d / "g"
    other.write_bytes(esync_model.text(350_000, 99))
    assert run(cli, "-1", "-k", "--index", d / "g.bzi", "--interval", "16", other).returncode == 0
    out = d / "never"
    r = run(cli, "-d", "--index", d / "g.bzi", "--range", "150000:100", "--output", out, d / "f.bz2")
    assert r.returncode == ERR_OUTPUT and not out.exists(), (r.returncode, r.stderr)
    # ... and one that names bytes the file does not have
    (d / "short.bz2").write_bytes((d / "f.bz2").read_bytes()[:40_000])
    r = run(cli, "-d", "--index", d / "f.bzi", "--range", "340000:100", "-c", d / "short.bz2")
    assert r.returncode == ERR_OUTPUT and r.stdout == b""
