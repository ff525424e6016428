"""CPU: the encoder's host arithmetic (banzai_amd/csrc/encode_plan.h -- the job split over lanes, a job's sums, the output words
zeroed before each pack and before the footer, the inputs a batch of a many-streams call opens and closes) against brute force, as
a stand-alone program with AddressSanitizer and UBSan (tests/encode_host/plan_host.cpp).  api.hip's encode drivers call the same
header, and what it computes there decides which words of the output are zero when a kernel ORs bits into them: this is where an
off-by-one in that is found without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the encode plan"
    exe = str(tmp_path_factory.mktemp("encode_plan_host") / "plan_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "encode_host", "plan_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20261])
def test_encode_plan_against_brute_force(plan_host, seed):
    """4000 seeded cases of each of the four functions and the fixed ones (block counts one off a batch edge for one and two
    lanes and batches of one block; batches of 0, 1, 31, 32 and 33 bits at every bit phase with and without a seed word, the
    capacity one word short, exact and one over; empty inputs at the front, in the middle, at the end and nothing but empty
    ones); a failed comparison or a sanitizer report is a non-zero exit status"""
    p = subprocess.run([plan_host, str(seed), "4000"], capture_output=True, text=True)
    assert p.returncode == 0, f"plan_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "4000 cases each" in p.stdout
