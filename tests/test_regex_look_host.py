"""CPU: anchors and word boundaries of the device regex without a device, as a stand-alone program with AddressSanitizer and
UBSan (tests/decode_host/look_host.cpp; nothing is loaded into Python under a sanitizer).  (a) The compile of
banzai_amd/csrc/regex_plan.h with assertions admitted against a naive matcher over the harness's own expression trees, the identity
of the plan for lists without assertions, the refusals.  (b) The look-around matcher of banzai_amd/csrc/regex_core.h,
BzrMatcher<true, true> and BzrMatcher<false, true>, thread by thread and tile by tile in the kernels' layout.  (c) The windows of
search_plan.h's BzmSetWalk and grep_plan.h's BzgWalk with (b) as the device, against brute force per output byte.  And the
program's `hits` mode against Python's `re` under re.MULTILINE (tests/regex_look_truth.py)."""
import os
import random
import shutil
import subprocess

import pytest

from tests import regex_look_truth as truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def look_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the look-around model"
    exe = str(tmp_path_factory.mktemp("look_host") / "look_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "look_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20263])
def test_look_model_against_brute_force(look_host, seed):
    """(a) 300 seeded lists of one to three random expression trees with ^ $ \\A \\Z \\b \\B in leading, inner and trailing places
    of their sequences, a fifth of them under the word or the line wrap, printed for the compiler and matched on the tree at every
    offset of a seeded text with two bounds (the assertions see the bytes behind the bound), at spans 256 and 5; lists that came
    out without an assertion compile to the same plan with and without the syntax bit, field by field; ^a, a$, a\\b, \\Aa, a\\Z
    are refused without the bit with today's texts; [\\b], a^*, ^, ^$, \\b, a* under the line wrap, both wraps at once and a^b
    (nothing can match) are refused with it; [xa\\n-]*x[xa\\n-]{14} fits the state bound and crosses it once an assertion makes
    its states name their context.
    (b) n in {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289} x a list that fits the LDS bound and one that does not: seeded
    text, search with record numbers and grep with and without INVERT and with a delimiter that is no 0x0A; ^ab planted at 0, 16,
    1024, 4096, 8192; x+$ at the text's end, in front of a final 0x0A, ending at tile byte 4095, and 256 bytes from 4095 so that
    the byte behind is the tile array's last; a run of one word byte under w+\\b, q\\Z and w$ (the model's unstaged LDS and the
    slack behind the text hold a word byte: read as a neighbour it shows); the two wraps.
    (c) 300 seeded lists of 1 to 7 blocks, staging targets from one byte up, line ends, line starts and long runs on block edges,
    a third of the ranges from a block's first byte to a block's last, the decoded blocks those of the widened range; order,
    record numbers, pattern and length hit by hit; the grep over the same windows.
    A failed comparison or a sanitizer report is a non-zero exit."""
    p = subprocess.run([look_host, str(seed), "300"], capture_output=True, text=True)
    assert p.returncode == 0, f"look_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "compile: held" in p.stdout and "matcher: " in p.stdout and "windows: 300 cases held" in p.stdout


A, W, X = truth.ASSERT, truth.WORD, truth.LINE
CASES = [([b"^[a-z]+"], 0, 256, A), ([b"[0-9]+$"], 0, 256, A), ([b"\\berr(or)?\\b"], truth.FOLD, 256, A), ([b"a\\B."], 0, 256, A),
         ([b"\\A.+", b"x+\\Z"], 0, 16, A), ([b"(^|\\t)time", b"a$\\n^b", b"foo\\b bar"], 0, 256, A), ([b"^.+$"], truth.DOTALL, 24, A),
         ([b"err(or)?", b"[0-9]+", b"a"], 0, 256, W), ([b"[a-z ]+", b"12"], truth.FOLD, 256, X), ([b"\\w+\\b", b"^\\s"], 0, 8, A | W)]
FLOORS = [35, 27, 11, 332, 1, 72, 24, 17, 11, 162]


def _text(n, seed):
    r = random.Random(seed)
    words = [b"abc", b"aa", b"a", b"err", b"ERROR", b"error", b"time", b"Time", b" ", b"\n", b"\t", b"12", b"7", b"x", b"foo bar", b"_", b"-"]
    out = b""
    while len(out) < n:
        out += r.choice(words)
    return out[:n]


def _program(look_host, tmp_path, exprs, text, flags, span, syntax):
    ef, tf = tmp_path / "exprs", tmp_path / "text"
    ef.write_bytes(b"\n".join(exprs) + b"\n")
    tf.write_bytes(text)
    p = subprocess.run([look_host, "hits", str(ef), str(tf), str(flags), str(span), str(syntax)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return [tuple(int(v) for v in line.split()) for line in p.stdout.splitlines()]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_hits_against_python_re(look_host, tmp_path, case):
    """The compiled table under the kernels' own look-around matcher against Python's re, hit by hit: offset, expression, length."""
    exprs, flags, span, syntax = CASES[case]
    text = _text(3000, case)
    want = truth.hits(exprs, text, flags, span, syntax)
    assert len(want) >= FLOORS[case]  # (what the truth gives for these seeds: an empty comparison cannot pass)
    assert _program(look_host, tmp_path, exprs, text, flags, span, syntax) == want


def test_the_truth_by_slices_is_the_truth_by_definition():
    """tests/regex_look_truth.py finds a start's longest match by bisection on a slice that keeps one byte of context at each end;
    held here to one match an end on the whole text."""
    text = _text(1500, 99)
    small = [([b"^ab$"], 0, A), ([b"\\bab\\b", b"ab\\Z", b"\\Aab"], 0, A), ([b"a\\B.", b"^[a-z]+", b"[a-z ]+$"], 0, A)]
    for exprs, flags, syntax in small + [(e, f, y) for e, f, _, y in CASES]:
        assert truth.hits(exprs, text, flags, 24, syntax) == truth.hits_plain(exprs, text, flags, 24, syntax)
        assert truth.hits(exprs, text, flags, 24, syntax, 100, 700) == truth.hits_plain(exprs, text, flags, 24, syntax, 100, 700)
