"""bnzhip's second attempts: every call the CLI makes with a guessed room and repeats with the room the library reports.  One
input of 70,000 lines of 'ab' (210,000 bytes, a few hundred compressed): more rows, lines and matches than the 65,536 entries of
the first room, and more decoded bytes than the first guess of 6 * n + 65,536 for -d and --recover.  The truth is computed from
the text."""
import bz2
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "banzai_amd", "bnzhip")
LINES = 70_000
TEXT = b"ab\n" * LINES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def where(native, tmp_path_factory):
    assert os.path.exists(BIN), "build with `make -C banzai_amd/csrc`"
    d = tmp_path_factory.mktemp("cli_retry")
    stream = bz2.compress(TEXT, 1)
    assert LINES > 65536 and len(TEXT) > 6 * len(stream) + 65536  # (both first guesses are short)
    (d / "a.bz2").write_bytes(stream)
    (d / "b.bz2").write_bytes(stream)
    return d


def run(where, *args):
    p = subprocess.run([BIN, *args], cwd=where, stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert p.returncode == 0, (args, p.returncode, p.stderr[-400:])
    return p.stdout


def test_search_rows(where):
    assert run(where, "--search", "ab", "a.bz2") == b"".join(b"%d\t%d\n" % (3 * k, k) for k in range(LINES))


def test_search_count(where):
    assert run(where, "--search", "ab", "--count", "a.bz2") == b"%d\n" % LINES


def test_grep_line_numbers(where):
    assert run(where, "--grep", "ab", "--line-number", "a.bz2") == b"".join(b"%d:ab\n" % (k + 1) for k in range(LINES))


def test_grep_only_matching_with_offsets(where):
    assert run(where, "--grep", "ab", "-o", "-b", "a.bz2") == b"".join(b"%d:ab\n" % (3 * k) for k in range(LINES))


def test_grep_two_inputs(where):
    want = b"".join(b"%s:%d:ab\n" % (name, k + 1) for name in (b"a.bz2", b"b.bz2") for k in range(LINES))
    assert run(where, "--grep", "ab", "--line-number", "a.bz2", "b.bz2") == want


def test_decode(where):
    assert run(where, "-d", "-c", "a.bz2") == TEXT
    assert (where / "a.bz2").exists()


def test_recover(where):
    assert run(where, "--recover", "-c", "a.bz2") == TEXT
    assert (where / "a.bz2").exists()
