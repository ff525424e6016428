"""CPU: the grep over many texts in one buffer without a device, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/grep_many_host.cpp; nothing is loaded into Python under a sanitizer).  The virtual-tile plan of
banzai_amd/csrc/grep_many_plan.h and the phases of grep_many_core.h / grep_core.h run thread by thread and tile by tile in the layout of
grep_many_tiles and grep_many_scan, against a naive split-and-find of every segment alone."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grep_many_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the grep-many model"
    exe = str(tmp_path_factory.mktemp("grep_many_host") / "grep_many_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "grep_many_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20263])
def test_grep_many_model_against_split_and_find(grep_many_host, seed):
    """Segment lengths 0, 1, 15, 16, 17, 4095, 4096, 4097 and 8193 in a seeded order, the first start at every residue modulo 16,
    gaps now and then; a wall on a tile edge; 40 segments of 100 bytes in one tile; a gap filled with the needle; a segment of
    delimiters only; a segment without a delimiter over three tiles with its only hit in the first, the middle and the last; a last
    byte that is and is not the delimiter; both senses; the needle cut at every point 1 .. plen - 1 across a wall; plen in
    {1, 2, 16, 17, 256}; rooms at the need, one below, and not asked for; every buffer at its exact size; a segment of 2^44 bytes, whose rows
    are beyond one launch, is counted and refused without a table.  A failed comparison or
    a sanitizer report is a non-zero exit."""
    p = subprocess.run([grep_many_host, str(seed)], capture_output=True, text=True)
    assert p.returncode == 0, f"grep_many_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "shapes: 200 calls held" in p.stdout and "walls: " in p.stdout
