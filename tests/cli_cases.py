"""The argv table of tests/test_cli_grammar.py: every way `bnzhip` ends before it opens a device, over one fixed scratch
directory.  scripts/record_cli_cases.py runs the table against a given binary and writes tests/golden/cli_grammar.json; the test
runs it against the tree's binary and asks for the same exit status, standard error and standard out, byte for byte.

Only cases that exit 0, 1 or 2 on a machine without a GPU belong here: one that reaches bzh_create exits 3 there and is left out.
The order of the checks is behaviour: where an argv holds two errors, the recorded message says which wins."""
import struct
import zlib

# a record-index envelope ("BZhREC\r\n" | u32 version | u32 delimiter | u64 entries | u64 records | u32 CRC-32 | u32 0 | blob | table)
# of no entries with delimiter TAB and its CRC right: --search refuses the delimiter before it looks at the blob, --grep does not
_REC_TAB = bytearray(b"BZhREC\r\n" + struct.pack("<IIQQII", 1, 9, 0, 0, 0, 0) + bytes(8))
_REC_TAB[32:36] = struct.pack("<I", zlib.crc32(bytes(_REC_TAB)))

FILES = {
    "f.bz2": b"",
    "g.bz2": b"",
    "f.txt": b"hello\nworld\n",
    "bad.bzi": b"junk",
    "rec_bad.bzi": b"BZhREC\r\n" + bytes(32),
    "pats.txt": b"one\n\nthree\n",
    # beyond the junk: a whole block index of no entries (bzh_index_blob_write of nothing) and the envelope above, so that the
    # checks behind a readable index file are reached too
    "empty.bzi": b"BZhIDX\r\n" + struct.pack("<I", 1) + bytes(20),
    "rec_tab.bzi": bytes(_REC_TAB),
}


def make_layout(d):
    """Write FILES into the directory d (a pathlib.Path).  No file is called missing.*."""
    for name, data in FILES.items():
        (d / name).write_bytes(data)


X = ("--index", "bad.bzi")
S = ("--search", "x")
G = ("--grep", "x")

CASES = [
    # ---- the commands and the usage text
    (), ("--help",), ("--info",), ("--version",), ("f.txt", "--help"), ("-d", "--version", "--bogus"),
    ("--output", "--help"),
    # ---- the argument loop: unknown words, clusters, `--`
    ("--bogus",), ("--bogus", "f.txt"), ("-z", "f.txt"), ("-0", "f.txt"), ("-co", "f.bz2"), ("-ce", "x", "f.bz2"), ("-dE", "f.bz2"),
    ("-kw", "f.bz2"), ("-cx", "f.bz2"), ("-cb", "f.bz2"), ("-cA", "1", "f.bz2"), ("-dB", "f.bz2"), ("-kC", "f.bz2"),
    ("-c5", "missing.txt"), ("-dk", "missing.bz2"), ("-kr", "missing.txt"), ("-vc9", "missing.txt"), ("--verbose", "-v", "missing.txt"),
    ("--fast", "--best", "missing.txt"),
    ("--", "--help"), ("--", "-k"), ("--", "-"), ("-d", "--", "-c"), ("--", "f.txt", "g.txt"),
    ("-c", "-c", "missing.txt"), ("--stdout", "-c", "missing.txt"),
    ("-c", "--output", "x", "f.txt"), ("--output", "x", "-c", "f.txt"), ("--output", "x", "--output", "y", "f.txt"),
    ("--output", "-k", "f.txt"), ("--output", "-", "f.txt"), ("--output",), ("--output", "x"), ("--output", "", "f.txt"), ("--output", ""),
    ("f.txt", "--output", "", "-k"), ("-d", "--index", "empty.bzi", "--range", "0:1", "--output", "", "f.bz2"),
    ("-", "f.bz2"), ("f.bz2", "-"), ("-", "-"), ("--grep", "x", "f.bz2", "-"), ("--grep", "x", "-", "f.bz2"),
    ("missing.txt",), ("-k", "missing.txt"), ("-d", "missing.bz2"), ("--recover", "missing.bz2"), ("-d", "--stream", "missing.bz2"),
    ("--make-index", "x.bzi", "missing.bz2"), ("--index", "x.bzi", "missing.txt"),
    ("-d", "f.txt"), ("--recover", "f.txt"), ("-d", "--stream", "f.txt"), ("-d", ".bz2"),
    # ---- the valued options: a bad value, a missing value
    ("--index", "-x", "f.bz2"), ("--index", "", "f.bz2"), ("--index", "a.bzi", "--index", "b.bzi", "f.bz2"),
    ("--make-index", "-k", "f.bz2"), ("--make-index", "a.bzi", "--make-index", "b.bzi", "f.bz2"),
    ("f.bz2", "--index"), ("f.bz2", "--make-index"), ("--make-index", "f.bz2"),
    ("--interval", "32768", "--make-index", "x.bzi", "f.bz2"), ("--interval", "x", "f.bz2"), ("--interval", "", "f.bz2"),
    ("--interval", "-1", "f.bz2"), ("f.bz2", "--interval"),
    ("--grep", "x", "-A", "4294967296", "f.bz2"), ("--grep", "x", "-B", "x", "f.bz2"), ("--grep", "x", "--context", "-1", "f.bz2"),
    ("--grep", "x", "--after-context", "1x", "f.bz2"), ("--grep", "x", "--before-context", "", "f.bz2"),
    ("--grep", "x", "f.bz2", "-A"), ("--grep", "x", "f.bz2", "-B"), ("--grep", "x", "f.bz2", "-C"), ("--grep", "x", "f.bz2", "--context"),
    ("--range", "5", "f.bz2"), ("--range", "1:99999999999999999999999", "f.bz2"), ("--range", "18446744073709551616:1", "f.bz2"),
    ("--range", ":5", "f.bz2"), ("--range", "1:", "f.bz2"), ("--range", "a:1", "f.bz2"), ("--range", "5:-1", "f.bz2"),
    ("--range", "1:2:3", "f.bz2"), ("f.bz2", "--range"), ("-d", "--index", "bad.bzi", "--range", "-c", "f.bz2"),
    ("f.bz2", "--search"), ("f.bz2", "--grep"), ("--search", "x", "f.bz2", "-e"), ("--grep", "x", "f.bz2", "--patterns"),
    ("--grep", "--patterns", "missing.txt", "f.bz2"), ("--grep", "--patterns", "pats.txt", "f.bz2"), ("--patterns", "pats.txt"),
    ("--search", "x", "--patterns", ".", "missing.bz2"),
    # ---- --search and --grep: once, not both, and the word behind them
    ("--search", "a", "--grep", "b", "f.bz2"), ("--grep", "a", "--search", "b", "f.bz2"), ("--search", "a", "--search", "b", "f.bz2"),
    ("--grep", "a", "--grep", "b", "f.bz2"),
    ("--search", "--regex", "x", "f.bz2"), ("--search", "-E", "x", "f.bz2"), ("--grep", "-w", "x", "f.bz2"), ("--grep", "-x", "x", "f.bz2"),
    ("--search", "--word-regexp", "x", "f.bz2"), ("--search", "--line-regexp", "x", "f.bz2"), ("--grep", "--ignore-case", "x", "f.bz2"),
    ("--search", "-e"), ("--grep", "--patterns"), ("--search", "--ignore-case", "f.bz2"), ("--search", "-w", "f.bz2"),
    ("--grep", "-E", "f.bz2"), ("--search", "-x", "-w", "f.bz2"), ("--grep", "-e", "x", "missing.bz2"),
    ("--search", "-o", "missing.bz2"), ("--grep", "--hex", "missing.bz2"),
    # ---- the checks behind the last argument, in their order
    ("f.bz2", "g.bz2"), ("-d", "f.bz2", "g.bz2"), S + ("f.bz2", "g.bz2"), ("f.bz2", "g.bz2", "--index"),
    ("--no-filename", "f.bz2"), ("--no-filename",) + S + ("f.bz2",), ("--no-filename", "f.bz2", "g.bz2"),
    G + ("-o", "f.bz2", "g.bz2"), G + ("-b", "f.bz2", "g.bz2"), G + ("-C", "1", "f.bz2", "g.bz2"), G + ("-A", "1", "f.bz2", "g.bz2"),
    G + ("-B", "0", "f.bz2", "g.bz2"), G + X + ("f.bz2", "g.bz2"), G + ("-o", "-b", "-C", "1") + X + ("f.bz2", "g.bz2"),
    G + ("-b",) + X + ("f.bz2", "g.bz2", "--range"), G + ("--only-matching", "--byte-offset", "f.bz2", "g.bz2"),
    G + ("-w", "-x", "f.bz2"), ("-w", "-x", "f.bz2"), ("-x", "f"), ("-w", "f.bz2"), ("--word-regexp", "--line-regexp"),
    ("-e", "a", "f.bz2"), ("--ignore-case", "f.bz2"), ("-E", "f.bz2"), ("--regex", "f.bz2"), ("--patterns", "f.txt", "f.bz2"),
    G + ("-E", "--hex", "f.bz2"), ("-E", "--hex", "f.bz2"), S + ("-E", "--hex"),
    ("-d",), ("--grep", "a"), ("-k",), ("--hex",),
    ("--hex", "f.bz2"), ("--count", "f.bz2"), ("--invert", "f.bz2"), ("--line-number",) + S + ("f.bz2",), ("--hex", "--invert", "f.bz2"),
    ("-A", "1", "f.bz2"), ("-C", "1") + S + ("f.bz2",), ("-o", "f.bz2"), ("-b",) + S + ("f.bz2",), ("--only-matching", "f.bz2"),
    ("--byte-offset", "f.bz2"), ("--invert", "-A", "1", "-o", "f.bz2"),
    G + ("-o", "--invert", "f.bz2"), G + ("-o", "-A", "1", "f.bz2"), G + ("-o", "--context", "0", "f.bz2"),
    G + ("--range", "1:2", "f.bz2"), G + ("-o", "--invert", "--range", "1:2", "f.bz2"), G + ("--range", "1:2", "-d", "f.bz2"),
    G + ("--range", "1:2") + X + ("f.bz2",),
    S + ("-d", "f.bz2"), S + ("--recover", "f.bz2"), S + ("--stream", "f.bz2"), S + ("--output", "o", "f.bz2"), S + ("-c", "f.bz2"),
    S + ("--make-index", "m.bzi", "f.bz2"), S + ("-1", "f.bz2"), S + ("--best", "f.bz2"), S + ("--interval", "5", "f.bz2"),
    S + ("-r", "f.bz2"), S + ("-k", "missing.bz2"), S + ("-k", "-r", "f.bz2"), S + ("-r", "-k", "missing.bz2"),
    G + ("-d", "f.bz2"), G + ("--recover", "f.bz2"), G + ("--stream", "f.bz2"), G + ("--output", "o", "f.bz2"), G + ("-c", "f.bz2"),
    G + ("--make-index", "m.bzi", "f.bz2"), G + ("-9", "f.bz2"), G + ("--interval", "5", "f.bz2"), G + ("--remove", "f.bz2"),
    G + ("--keep", "missing.bz2"), G + ("-c", "f.bz2", "g.bz2"),
    S + ("--range", "1:2", "--range", "3:4") + X + ("f.bz2",), S + ("--range", "1:2", "f.bz2"), S + ("-d", "--range", "1:2", "f.bz2"),
    S + X + ("-",), S + X + ("--range", "1:2", "--range", "3:4", "-"),
    ("--search", "abc", "--hex", "f.bz2"), ("--search", "zz", "--hex", "f.bz2"), ("--grep", "abc", "--hex", "f.bz2"),
    ("--grep", "0g", "--hex", "f.bz2"), ("--grep", "-e", "abc", "--hex", "f.bz2"), ("--search", "61", "-e", "6", "--hex", "f.bz2"),
    ("--search", "abc", "--hex") + X + ("-",),
    ("--search", "", "f.bz2"), ("--search", "a" * 257, "f.bz2"), ("--grep", "", "f.bz2"), ("--grep", "", "--hex", "f.bz2"),
    ("--search", "a" * 256, "missing.bz2"), ("--grep", "61" * 257, "--hex", "f.bz2"),
    ("--search", "-e", "", "f.bz2"), ("--search", "a", "-e", "b" * 257, "f.bz2"), ("--grep", "a", "--ignore-case", "-e", "", "f.bz2"),
    ("--grep", "-E", "-e", "a" * 4097, "f.bz2"), ("--grep", "-E", "-e", "a", "-e", "", "f.bz2"), ("--grep", "-w", "-e", "b" * 257, "f.bz2"),
    ("--search", "--patterns", "f.txt", "-e", "", "f.bz2"),
    ("--search",) + ("-e", "a") * 65537 + ("f.bz2",),
    ("--grep", "(", "-E", "f.bz2"), ("--search", "(", "-E") + X + ("f.bz2",), ("--grep", "-E", "-e", "a", "-e", "[z-a]", "missing.bz2"),
    ("--grep", "a**", "-E", "f.bz2"), ("--search", "a{2,1}", "--regex", "f.bz2"), ("--grep", ")", "-x", "-E", "f.bz2"),
    ("--search", "(?=a)", "-E", "f.bz2"), ("--grep", "\\1", "-E", "missing.bz2"), ("--grep", "-E", "(", "f.bz2"),
    ("--search", "a", "-w", "-E", "-e", "[", "--ignore-case", "f.bz2", "--count"),
    ("--range", "1:2", "f.bz2"), ("-d", "--range", "0:1", "-c", "f.bz2"), ("-d", "--stream") + X + ("--range", "0:1", "-c", "f.bz2"),
    ("--recover",) + X + ("--range", "0:1", "-c", "f.bz2"), X + ("--range", "0:1", "-c", "f.bz2"), ("-d",) + X + ("--range", "0:1", "-c", "-"),
    ("-d",) + X + ("--range", "0:1", "f.bz2"), ("-d",) + X + ("-c", "f.bz2"), ("--recover",) + X + ("f.bz2",), ("-d", "--stream") + X + ("f.bz2",),
    ("--make-index", "x.bzi", "-d", "f.bz2"), ("--make-index", "x.bzi", "--recover", "f.bz2"), ("--make-index", "x.bzi", "--stream", "f.bz2"),
    ("--make-index", "x.bzi", "-c", "f.bz2"), ("--make-index", "x.bzi", "--output", "o", "f.bz2"), ("--make-index", "x.bzi") + X + ("f.bz2",),
    ("--make-index", "x.bzi", "-1", "f.bz2"), ("--make-index", "x.bzi", "-r", "missing.bz2"),
    ("--interval", "16", "-c", "f.bz2"), ("--interval", "5", "f.txt"), ("-d",) + X + ("--interval", "16", "--range", "0:1", "-c", "f.bz2"),
    ("--interval", "0", "--index", "x.bzi", "missing.txt"), ("--interval", "32767", "--make-index", "x.bzi", "missing.bz2"),
    ("--recover", "-d", "f.bz2"), ("-d", "--stream", "--recover", "f.bz2"), ("--stream", "--recover", "f.bz2"), ("--stream", "f.bz2"),
    ("--stream", "-1", "f.bz2"), ("--recover", "-1", "f.bz2"), ("--recover", "--fast", "--stream", "f.bz2"),
    ("--recover", "--range", "1:2", "-1", "f.bz2"), ("--make-index", "x.bzi", "--range", "1:2", "f.bz2"),
    ("-d", "--range", "1:2", "--interval", "5", "f.bz2"), ("--stream", "--interval", "5", "f.bz2"),
    # ---- the index file and the input, read before a device is opened
    S + ("--index", "missing.bzi", "f.bz2"), S + X + ("f.bz2",), S + ("--index", "rec_bad.bzi", "f.bz2"), S + ("--index", ".", "f.bz2"),
    S + ("--index", "f.bz2", "f.bz2"), S + ("--index", "rec_tab.bzi", "f.bz2"), G + ("--index", "rec_tab.bzi", "f.bz2"),
    S + ("--index", "f.txt", "f.bz2"), S + ("--index", "empty.bzi", "missing.bz2"), S + ("--index", "empty.bzi", "."),
    S + ("--index", "empty.bzi", "--range", "0:1", "missing.bz2"),
    G + ("--index", "missing.bzi", "f.bz2"), G + X + ("f.bz2",), G + ("--index", "rec_bad.bzi", "f.bz2"), G + ("--index", ".", "f.bz2"),
    G + ("--index", "empty.bzi", "missing.bz2"), G + ("--index", "empty.bzi", "."), G + X + ("missing.bz2",),
    S + ("missing.bz2",), G + ("missing.bz2",), G + ("-o", "missing.bz2"), ("--grep", "-w", "-e", "x", "missing.bz2"),
    ("-d", "--index", "missing.bzi", "--range", "0:1", "-c", "f.bz2"), ("-d",) + X + ("--range", "0:1", "-c", "f.bz2"),
    ("-d", "--index", "rec_bad.bzi", "--range", "0:1", "-c", "f.bz2"), ("-d", "--index", "rec_tab.bzi", "--range", "0:1", "-c", "f.bz2"),
    ("-d", "--index", ".", "--range", "0:1", "-c", "f.bz2"), ("-d", "--index", "empty.bzi", "--range", "0:1", "-c", "missing.bz2"),
    ("-d", "--index", "empty.bzi", "--range", "0:1", "--output", "o", "."), ("-d",) + X + ("--range", "0:1", "--output", "o", "missing.bz2"),
    ("-d", "--index", "empty.bzi", "--range", "0:1", "--range", "5:0", "-c", "f.bz2"),
    ("-d", "--index", "empty.bzi", "--range", "0:1", "--output", "o.out", "f.bz2"),
]


def run_case(binary, argv, d):
    """One case in the fresh directory d: -> what the JSON records of it.  `files` names what the run left in d that the layout
    does not hold, or holds otherwise (name -> size; None: removed); it is {} for nearly every case."""
    import subprocess
    make_layout(d)
    r = subprocess.run([binary, *argv], cwd=d, stdin=subprocess.DEVNULL, capture_output=True)
    after = {p.name: p.stat().st_size for p in d.iterdir()}
    files = {n: s for n, s in after.items() if n not in FILES or (d / n).read_bytes() != FILES[n]}
    files.update({n: None for n in FILES if n not in after})
    return {"status": r.returncode, "stderr": r.stderr.decode("latin-1"), "stdout": r.stdout.decode("latin-1"), "files": files}


def label(argv):
    """The key of a case in the JSON: its argv, a long word or a long argv cut short"""
    words = [a if len(a) <= 40 else "%s..[%d]" % (a[:8], len(a)) for a in argv]
    text = " ".join(words)
    return text if len(text) <= 200 else "%s ..[%d words]" % (text[:80], len(argv))
