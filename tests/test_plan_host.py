"""CPU: the decoder's host arithmetic (banzai_amd/csrc/decode_plan.h -- tile prefix sums, the window of a range inside an index
entry, the segment list of a batch) against brute force, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/plan_host.cpp).  decode.hip's host side calls the same header, and what it computes there are offsets of
stores on the device: this is where an off-by-one in them is found without one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the decode plan"
    exe = str(tmp_path_factory.mktemp("plan_host") / "plan_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "plan_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20261])
def test_plan_against_brute_force(plan_host, seed):
    """4000 seeded cases of each of the three functions (and the fixed ones: nblock 0 and one off a tile edge, entries of size
    0, ranges that end exactly on a block edge, `off` beyond the total, blocks with no point, all points in one block); a failed
    comparison or a sanitizer report is a non-zero exit status"""
    p = subprocess.run([plan_host, str(seed), "4000"], capture_output=True, text=True)
    assert p.returncode == 0, f"plan_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "4000 cases each" in p.stdout
