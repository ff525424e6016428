"""bnzhip's argument grammar and its checks, held byte for byte: every argv of tests/cli_cases.py must end with the exit status,
the standard error and the standard out that tests/golden/cli_grammar.json records (and leave the files it records).  The JSON was
written by scripts/record_cli_cases.py from a build of the commit before the CLI was split into options, checks and modes; it is
recorded again only when the table changes, and then from such a build, never from the code under test.  No case reaches a device."""
import json
import os
import pathlib
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import cli_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "banzai_amd", "bnzhip")
with open(os.path.join(ROOT, "tests", "golden", "cli_grammar.json")) as _f:
    GOLDEN = json.load(_f)
LABELS = [cli_cases.label(argv) for argv in cli_cases.CASES]


@pytest.fixture(scope="module")
def answers(native, tmp_path_factory):
    """Every case run once, each in a fresh copy of the layout: label -> what run_case saw"""
    assert os.path.exists(BIN), "build with `make -C banzai_amd/csrc`"
    top = tmp_path_factory.mktemp("cli_grammar")

    def one(k):
        d = pathlib.Path(top, str(k))
        d.mkdir()
        return cli_cases.run_case(BIN, cli_cases.CASES[k], d)
    with ThreadPoolExecutor(8) as pool:
        return dict(zip(LABELS, pool.map(one, range(len(LABELS)))))


def test_the_table_and_the_recording_hold_the_same_cases():
    assert len(set(LABELS)) == len(LABELS) and sorted(LABELS) == sorted(GOLDEN)
    assert len(LABELS) >= 90
    # a recorded case ended before bzh_create: 0, 1 or 2 on a machine without a GPU (3: it reached the device and is left out)
    assert all(g["status"] in (0, 1, 2) for g in GOLDEN.values())


@pytest.mark.parametrize("label", LABELS)
def test_case(answers, label):
    got, want = answers[label], GOLDEN[label]
    assert got["status"] == want["status"], got
    assert got["stderr"] == want["stderr"]
    assert got["stdout"] == want["stdout"]
    assert got["files"] == want["files"]


def first_line(argv):
    g = GOLDEN[cli_cases.label(argv)]
    return g["status"], g["stderr"].split("\n")[0]


def test_the_named_quirks_are_in_the_recording():
    """What the table must hold by name, read from the recording itself (test_case holds the binary to it)"""
    one_input = (1, "Only one input may be specified")
    # the word after --search/--grep that is itself an option is taken as that option
    for word in ("--regex", "-E", "--word-regexp", "--line-regexp"):
        assert first_line(("--search", word, "x", "f.bz2")) == one_input
    no_string = (1, "'--search' and '--grep' require a string, a '-e' or a '--patterns'")
    assert first_line(("--grep", "-w", "x", "f.bz2")) == first_line(("--grep", "-x", "x", "f.bz2")) == no_string  # (--grep takes two inputs)
    assert first_line(("--search", "-e")) == (1, "Argument '-e' requires a string")
    assert first_line(("--grep", "--patterns")) == (1, "Argument '--patterns' requires a file path")
    assert first_line(("--search", "--ignore-case", "f.bz2")) == no_string
    # -e -E -w -x -o -b -A -B -C stand alone; -c5, -dk, -kr cluster
    for argv, f in ((("-co", "f.bz2"), "o"), (("-ce", "x", "f.bz2"), "e"), (("-dE", "f.bz2"), "E"), (("-kw", "f.bz2"), "w"), (("-cx", "f.bz2"), "x"),
                    (("-cb", "f.bz2"), "b"), (("-cA", "1", "f.bz2"), "A"), (("-dB", "f.bz2"), "B"), (("-kC", "f.bz2"), "C")):
        assert first_line(argv) == (1, "Flag '%s' is not valid" % f)
    for argv in (("-c5", "missing.txt"), ("-dk", "missing.bz2"), ("-kr", "missing.txt")):
        assert first_line(argv) == (2, "[filesystem error] cannot open %s: No such file or directory" % argv[-1])
    # `--` ends the options
    assert first_line(("--", "--help")) == (2, "[filesystem error] cannot open --help: No such file or directory")
    assert first_line(("-c", "-c", "missing.txt"))[0] == 2 and first_line(("-c", "--output", "x", "f.txt")) == (1, "Only one output may be specified")
    assert first_line(("--output", "-k", "f.txt")) == (1, "Argument '--output' requires a file path")
    assert first_line(("--index", "a.bzi", "--index", "b.bzi", "f.bz2")) == (1, "'--index' may be given once")
    assert first_line(("--interval", "32768", "--make-index", "x.bzi", "f.bz2"))[1].startswith("Argument '--interval' requires")
    assert first_line(("--range", "1:99999999999999999999999", "f.bz2"))[1].startswith("Argument '--range' requires")
    assert first_line(("--grep", "x", "-A", "4294967296", "f.bz2"))[1].startswith("Arguments '-A', '-B' and '-C' require")
    assert first_line(("--search", "abc", "--hex", "f.bz2"))[1].endswith("an even number of hex digits")
    assert first_line(("--search", "zz", "--hex", "f.bz2"))[1].endswith("requires hex digits")
    assert first_line(("--grep", "--patterns", "pats.txt", "f.bz2")) == (1, "'--patterns': line 2 of pats.txt is empty")
    assert first_line(("--grep", "x", "-w", "-x", "f.bz2")) == (1, "'-w' and '-x' exclude each other")
    assert first_line(("--grep", "x", "-E", "--hex", "f.bz2"))[1].startswith("'-E' and '--hex' exclude each other")
    assert first_line(("--grep", "(", "-E", "f.bz2")) == (1, "error during search: invalid argument: regex: expression 0, byte 0: an unbalanced bracket: ( without )")
    for opt, named in (("-o", "-o"), ("-b", "-b"), ("-C", "-A', '-B' and '-C")):
        argv = ("--grep", "x", opt) + (("1",) if opt == "-C" else ()) + ("f.bz2", "g.bz2")
        assert first_line(argv)[1].startswith("'%s' takes one input" % named)
    assert first_line(("--grep", "x", "--index", "bad.bzi", "f.bz2", "g.bz2"))[1].startswith("'--index' takes one input")
    assert first_line(("--no-filename", "f.bz2")) == (1, "'--no-filename' goes with '--grep'")
    assert first_line(("f.bz2", "g.bz2")) == one_input
    # the three the issue checked by hand
    assert first_line(("--search", "x", "--index", "bad.bzi", "f.bz2")) == (2, "[filesystem error] bad.bzi is not a whole, undamaged index file")
    assert first_line(("--grep", "x", "missing.bz2"))[0] == 2
    assert cli_cases.label(("--search", "x", "f.bz2")) not in GOLDEN  # (it reaches the device)


def test_which_of_two_errors_wins():
    """The order of the checks is behaviour: argv with two errors, and the one that is reported"""
    G, S, X = cli_cases.G, cli_cases.S, cli_cases.X
    for argv, starts in (
            (G + ("-o", "--invert", "--range", "1:2", "f.bz2"), "'-o' writes the matched parts alone"),
            (("-d", "--stream", "--recover", "f.bz2"), "'--recover' and '--decompress' exclude each other"),
            (("f.bz2", "g.bz2", "--index"), "Only one input may be specified"),
            (("--no-filename", "f.bz2", "g.bz2"), "Only one input may be specified"),
            (G + ("-b",) + X + ("f.bz2", "g.bz2", "--range"), "'-b' takes one input"),
            (G + ("-o", "-b", "-C", "1") + X + ("f.bz2", "g.bz2"), "'-o' takes one input"),
            (("-w", "-x", "f.bz2"), "'-w' and '-x' exclude each other"),
            (("--word-regexp", "--line-regexp"), "'-w' and '-x' exclude each other"),
            (("-E", "--hex", "f.bz2"), "'-e', '-E', '--patterns' and '--ignore-case' go with"),
            (S + ("-E", "--hex"), "'-E' and '--hex' exclude each other"),
            (("--hex", "--invert", "f.bz2"), "'--hex' and '--count' go with"),
            (("--invert", "-A", "1", "-o", "f.bz2"), "'--invert' and '--line-number' go with"),
            (G + ("--range", "1:2", "-d", "f.bz2"), "'--grep' takes an input"),
            (S + ("-d", "--range", "1:2", "f.bz2"), "'--search' takes an input"),
            (S + X + ("--range", "1:2", "--range", "3:4", "-"), "'--search' takes one '--range'"),
            (("--search", "abc", "--hex") + X + ("-",), "'--search --index' reads parts of a file"),
            (("--search", "(", "-E") + X + ("f.bz2",), "error during search: invalid argument"),
            (("--recover",) + X + ("--range", "0:1", "-c", "f.bz2"), "'--range' goes with neither"),
            (("--recover", "--range", "1:2", "-1", "f.bz2"), "'--range' needs the '--index'"),
            (("--make-index", "x.bzi", "--range", "1:2", "f.bz2"), "'--range' needs the '--index'"),
            (("--recover", "--fast", "--stream", "f.bz2"), "'--stream' and '--recover' exclude each other"),
            (("--stream", "--interval", "5", "f.bz2"), "'--interval' goes with"),
            (("--patterns", "pats.txt"), "'--patterns': line 2 of pats.txt is empty"),
            (("-d", "--version", "--bogus"), "version alpha"),
            (("-d",) + X + ("--range", "0:1", "--output", "o", "missing.bz2"), "[filesystem error] bad.bzi is not a whole")):
        assert first_line(argv)[1].startswith(starts), (argv, first_line(argv))
