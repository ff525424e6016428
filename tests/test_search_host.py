"""CPU: the search without a device, as a stand-alone program with AddressSanitizer and UBSan (tests/decode_host/search_host.cpp;
nothing is loaded into Python under a sanitizer).  (a) What one thread of search_tiles does -- banzai_amd/csrc/search_core.h: the
delimiter bits, the filter on the pattern's first bytes, the verify, the delimiters in front of a position -- thread by thread and
tile by tile in the kernel's layout, both passes and the scan between them, against a naive scan.  (b) The windows and the carry
of banzai_amd/csrc/search_plan.h with (a) as the device, against brute force per output byte."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def search_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the search model"
    exe = str(tmp_path_factory.mktemp("search_host") / "search_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "search_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20262])
def test_search_model_against_brute_force(search_host, seed):
    """(a) n in {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289} x plen in {1, 2, 3, 4, 5, 16, 17, 255, 256}: seeded text, a match
    at offset 0, ending at byte n - 1, across a thread edge (16), a wave edge (1024) and a tile edge (4096), a buffer of one byte
    value with every, three and no hit slots, plen > n, the delimiter equal to a pattern byte; every buffer has its exact size.
    (b) 1500 seeded lists of 1 to 7 blocks of 1 to 9,000 bytes, staging targets from one byte up, windows of 1 to 4 blocks, a
    staging buffer allocated anew for every window, matches and delimiters planted on the block edges, max above, at and below
    the hit count and 0, ranges that cut a match at either end.  A failed comparison or a sanitizer report is a non-zero exit."""
    p = subprocess.run([search_host, str(seed), "1500"], capture_output=True, text=True)
    assert p.returncode == 0, f"search_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "raw: " in p.stdout and "windows: 1500 cases held" in p.stdout
