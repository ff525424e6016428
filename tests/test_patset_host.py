"""CPU: search and grep for a set of patterns without a device, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/patset_host.cpp; nothing is loaded into Python under a sanitizer).  (a) The compile of
banzai_amd/csrc/patset_plan.h against a naive matcher.  (b) The matcher of banzai_amd/csrc/patset_core.h thread by thread and
tile by tile in the kernels' layout, both passes of search_tiles and of grep_tiles and the scans between them.  (c) The windows,
the hold-back and the finishing window of search_plan.h's BzmSetWalk and grep_plan.h's BzgWalk with (b) as the device, against
brute force per output byte."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def patset_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the pattern set's model"
    exe = str(tmp_path_factory.mktemp("patset_host") / "patset_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "patset_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20262])
def test_patset_model_against_brute_force(patset_host, seed):
    """(a) Duplicates, duplicates that arise only by folding, a prefix set, a suffix set, all 256 one-byte patterns (256 classes),
    exactly 65,535 states accepted and one more refused, the neighbours that do not fold ('@' and '`', '[' and '{', 0xC0 and 0xE0),
    every refused argument; the table walked at every offset of a text, with two bounds, against the rule.
    (b) n in {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289} x sets of the lengths {1, 2, 4, 5, 17, 255, 256}, with and without
    folding: every length a prefix of the next (short and long at one start), planted at offset 0, ending at byte n - 1, across a
    thread edge (16), a wave edge (1024) and a tile edge (4096), the longest cut by the text's end while its prefixes match; a text
    of one byte value with every, three and no hit slots; the delimiter equal to a pattern byte; search and grep, with INVERT.
    The table and every buffer have their exact sizes.
    (c) 1000 seeded lists of 1 to 7 blocks of 1 to 9,000 bytes, staging targets from one byte up, a short pattern that ends in front
    of a block edge and a long one at the same start that spans it, ranges that cut a match at either end, max above, at and below
    the count and 0, search and grep; order and absence of duplicates are checked hit by hit.
    A failed comparison or a sanitizer report is a non-zero exit."""
    p = subprocess.run([patset_host, str(seed), "1000"], capture_output=True, text=True)
    assert p.returncode == 0, f"patset_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "compile: held" in p.stdout and "matcher: " in p.stdout and "windows: 1000 cases held" in p.stdout
