"""CPU: tests/match_truth.py, the model every test of bzh_match* stands on, held to GNU grep (`grep -a -o -b [-E] [-w|-x]`) on
seeded newline-terminated texts over an alphabet in which every pattern matches often.  Python's `re` is leftmost-first and GNU
grep leftmost-longest, so the model finds the longest match per start itself; this test is what says it does."""
import os
import random
import shutil
import subprocess

from tests import match_truth as mt

ALPHABET = b"aab b1\n"
PATTERNS = [(b"aa", 0), (b"a|ab", 0), (b"ab|abab|b", 0), (b"[0-9]+", 0), (b"[a-c]+b", 0), (b"^a+", 0), (b"b$", 0), (rb"\bab\b", 0),
            (b"a+b?", mt.WORD), (b"a|ab|abb", mt.WORD), (b"[ab]+", mt.WORD), (b"a+b?", mt.LINE), (b"a|ab|abb", mt.LINE), (b"[ab]+", mt.LINE)]
TEXTS = 40


def texts():
    rng = random.Random(22)
    out = []
    for k in range(TEXTS):
        n = 0 if k == 0 else rng.randrange(1, 121)
        t = bytes(rng.choice(ALPHABET) for _ in range(n))
        out.append(t[:-1] + b"\n" if t else t)
    return out


def gnu_matches(gnu, path, expr, syntax):
    mode = ["-w"] if syntax & mt.WORD else ["-x"] if syntax & mt.LINE else []
    p = subprocess.run([gnu, "-a", "-o", "-b", "-E", *mode, "-e", expr.decode(), path], capture_output=True, env=dict(os.environ, LC_ALL="C"))
    assert p.returncode in (0, 1), p.stderr
    out = []
    for line in p.stdout.split(b"\n")[:-1]:
        off, _, what = line.partition(b":")
        out.append((int(off), what))
    return out


def test_model_equals_gnu_grep(tmp_path):
    gnu = shutil.which("grep")
    assert gnu, "GNU grep is needed: the model of the matches is the truth the GPU tests stand on, and grep is what holds it"
    version = subprocess.run([gnu, "--version"], capture_output=True, text=True).stdout
    assert "GNU grep" in version, f"{gnu} is not GNU grep: {version[:80]!r}"
    compared = found = 0
    for k, text in enumerate(texts()):
        path = tmp_path / f"t{k}.txt"
        path.write_bytes(text)
        for expr, syntax in PATTERNS:
            mine = [(s, text[s:s + n]) for s, _, n in mt.select([expr], text, syntax=syntax | mt.ASSERT)]
            theirs = gnu_matches(gnu, str(path), expr, syntax)
            assert mine == theirs, (text, expr, syntax, mine, theirs)
            compared += 1
            found += len(mine)
    assert compared >= 500 and found > 2000, (compared, found)


def test_model_on_the_cases_that_tell_the_rules_apart():
    assert mt.select([b"aa"], b"aaaa") == [(0, 0, 2), (2, 0, 2)]                   # a search has three hits
    assert mt.select([b"a|ab"], b"ab") == [(0, 0, 2)]                              # leftmost-LONGEST: `re` alone takes one byte
    assert mt.select([b"a", b"ab", b"abb"], b"abbab") == [(0, 2, 3), (3, 1, 2)]    # the longest of a start's patterns
    assert mt.select([b"b$"], b"bb\nb") == [(1, 0, 1), (3, 0, 1)]                  # $ sees the real neighbour
    assert mt.select([b"a+"], b"aaaa", span=3) == [(0, 0, 3), (3, 0, 1)]           # a match ends with the span
    assert mt.matches(mt.literal([b"a.", b"b"]), b"a.\nb a.", delim=b"\n") == (b"a.ba.", [(0, 0, 0, 2, 0), (3, 1, 1, 1, 2), (5, 1, 0, 2, 3)])
    assert mt.render(b"xab\nab\n", mt.select([b"ab"], b"xab\nab\n"), True, True) == b"1:1:ab\n2:4:ab\n"
