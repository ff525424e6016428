"""CPU: regular expressions for search and grep without a device, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/regex_host.cpp; nothing is loaded into Python under a sanitizer).  (a) The compile of
banzai_amd/csrc/regex_plan.h against a naive matcher over the harness's own expression trees.  (b) The matchers of
banzai_amd/csrc/regex_core.h, BzrMatcher<true, false> and BzrMatcher<false, false>, thread by thread and tile by tile in the kernels' layout,
both passes of search_tiles and of grep_tiles and the scans between them.  (c) The windows, the hold-back and the finishing window
of search_plan.h's BzmSetWalk and grep_plan.h's BzgWalk with (b) as the device, against brute force per output byte.  And the
program's `hits` mode against Python's `re` (tests/regex_truth.py)."""
import os
import random
import shutil
import subprocess

import pytest

from tests import regex_truth as truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def regex_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the regex model"
    exe = str(tmp_path_factory.mktemp("regex_host") / "regex_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "regex_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20262])
def test_regex_model_against_brute_force(regex_host, seed):
    """(a) 150 seeded lists of one to three random expression trees (literals, escapes, classes with ranges and class escapes,
    negated classes, the dot, groups, alternation, every quantifier form), printed for the compiler and matched on the tree at
    every offset of a seeded text, with two bounds, at spans 256 and 5, with and without folding and DOTALL; the table's
    invariants (row 0 unreached, terminals first, breadth-first order, first[] behind cls[]); min_len, max_len and unbounded of
    known expressions; every refused form with the expression's number and the byte; exactly 65,535 states from exactly 65,536
    NFA positions accepted (256 literal words that share nothing, two of them one alternation) and one state more refused; the
    blow-up (a|b)*a(a|b){16} and nested bounds refused promptly; what folds and what does not ('@' and '`', '[' and '{', 0xC0
    and 0xE0).
    (b) n in {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289} x a set of expressions that fits the LDS bound and one that does
    not (an alternation of 300 words), with and without folding: seeded text; matches of exactly 256 bytes at offset 0, across a
    wave edge, from 4095 to the halo's last byte, ending at byte n - 1; short ones at 15, 1023; the delimiter inside a match;
    x+ over one byte value at spans 256 and 8 with every, three and no hit slots; search and grep, with INVERT; both matcher
    variants wherever the table fits.  The table, the LDS model and every buffer have their exact sizes.
    (c) 300 seeded lists of 1 to 7 blocks of 1 to 9,000 bytes, staging targets from one byte up, long matches that span block
    edges, ranges that cut the longest match so that a shorter one is reported, max above, at and below the count and 0,
    search and grep; order and one hit a start are checked hit by hit.
    A failed comparison or a sanitizer report is a non-zero exit."""
    p = subprocess.run([regex_host, str(seed), "300"], capture_output=True, text=True)
    assert p.returncode == 0, f"regex_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "compile: held" in p.stdout and "matcher: " in p.stdout and "windows: 300 cases held" in p.stdout


EXPRS = [b"[0-9]+", b"err(or)?.*time", b"(abc)+|a{2,3}", b"\\s+", b"[^a]+", b"a+"]
CASES = [(EXPRS[:1], 0, 256), (EXPRS[1:2], truth.FOLD, 256), (EXPRS[2:3], 0, 256), (EXPRS[3:4], 0, 256), (EXPRS[4:5], 0, 256),
         ([b".+"], 0, 16), ([b".+"], truth.DOTALL, 16), (EXPRS[:4], truth.FOLD, 256), ([b"ab|cd", b"a[a-c]", b"abc?"], 0, 256)]


def _text(n, seed):
    r = random.Random(seed)
    words = [b"abc", b"aa", b"a", b"err", b"ERROR", b"error", b"time", b"Time", b" ", b"\n", b"\t ", b"12", b"7", b"x", b"cd", b"ab"]
    out = b""
    while len(out) < n:
        out += r.choice(words)
    return out[:n]


def _program(regex_host, tmp_path, exprs, text, flags, span):
    ef, tf = tmp_path / "exprs", tmp_path / "text"
    ef.write_bytes(b"\n".join(exprs) + b"\n")
    tf.write_bytes(text)
    p = subprocess.run([regex_host, "hits", str(ef), str(tf), str(flags), str(span)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return [tuple(int(v) for v in line.split()) for line in p.stdout.splitlines()]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_hits_against_python_re(regex_host, tmp_path, case):
    """The compiled table under the kernels' own matcher against Python's re, hit by hit: offset, expression, length."""
    exprs, flags, span = CASES[case]
    text = _text(3000, case)
    assert _program(regex_host, tmp_path, exprs, text, flags, span) == truth.hits(exprs, text, flags, span)


def test_a_run_longer_than_a_tile_against_python_re(regex_host, tmp_path):
    """a+ over 4,097 a's: every start reports min(256, what is left)."""
    text = b"a" * 4097
    got = _program(regex_host, tmp_path, [b"a+"], text, 0, 256)
    assert got == truth.hits([b"a+"], text) == [(s, 0, min(256, 4097 - s)) for s in range(4097)]


def test_the_truth_by_bisection_is_the_truth_by_definition():
    """tests/regex_truth.py finds a start's longest match by bisection; held here to one fullmatch an end."""
    text = _text(1500, 99)
    for exprs, flags, span in CASES:
        assert truth.hits(exprs, text, flags, span) == truth.hits_plain(exprs, text, flags, span)
        assert truth.hits(exprs, text, flags, span, 100, 700) == truth.hits_plain(exprs, text, flags, span, 100, 700)
