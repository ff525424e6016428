"""CPU: the grep without a device, as a stand-alone program with AddressSanitizer and UBSan (tests/decode_host/grep_host.cpp;
nothing is loaded into Python under a sanitizer).  (a) What one thread, one tile and the scan of grep_tiles / grep_scan do --
banzai_amd/csrc/grep_core.h -- thread by thread and tile by tile in the kernel's layout, the counting pass, the scan and the
gather, against a naive split-and-find.  (b) The windows and the carry of banzai_amd/csrc/grep_plan.h with (a) as the device,
against the same truth."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grep_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the grep model"
    exe = str(tmp_path_factory.mktemp("grep_host") / "grep_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "grep_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20262])
def test_grep_model_against_split_and_find(grep_host, seed):
    """(a) n in {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289} x plen in {1, 2, 3, 4, 5, 16, 17, 255, 256} x invert: seeded text
    of every delimiter density with the pattern planted on the thread, wave and tile edges and at both ends; a delimiter as the
    last byte of a thread, a wave and a tile and as the first of the next; a record over three tiles with its only hit in the
    first, the middle and the last; delimiters only; no delimiter; empty and non-empty tails; a pattern that begins with, ends
    with and is the delimiter; selected output that starts at every residue modulo 16; every buffer has its exact size.
    (b) 600 seeded lists of 1 to 7 blocks of 1 to 9,000 bytes in windows of 1 to 4 blocks, a staging buffer allocated anew for
    every window, records open across several window edges, carries of 1, 511, 512, 513 and 5,000 bytes, the only hit inside
    the carry or across the window edge, rooms above, at and one below the need, zero, and not asked for.  A failed comparison
    or a sanitizer report is a non-zero exit."""
    p = subprocess.run([grep_host, str(seed), "600"], capture_output=True, text=True)
    assert p.returncode == 0, f"grep_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "raw: " in p.stdout and "windows: 600 cases held" in p.stdout
