"""CPU: the chain walk of bzh_decode_many (banzai_amd/csrc/decode_many_plan.h -- one chain per input over one scan, batches
across inputs, the slice bound on what a wavefront reports, output placement with gaps behind failed inputs) against a
restatement that judges every input alone and knows no batches, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/many_host.cpp).  decode.hip's decode_many_run drives the same text; the GPU is only where its results
come from."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def many_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the walk"
    exe = str(tmp_path_factory.mktemp("many_host") / "many_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "many_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20261])
def test_walk_against_inputs_judged_alone(many_host, seed):
    """1500 seeded worlds and the fixed ones -- every damage alone and in every input (cut mid-block with the next input
    directly behind, an end one bit behind the slice, cut inside the footer, block and stream CRC, bad magic, empty and short
    slices, a level above the context's in the first and in the second stream, a lost magic), inputs of 0 to 3 streams,
    magics inside payloads and in gaps, every input failed, no input at all -- each walked in batches of 1, 2, 3, 4, 5, 7,
    8, 16 and 1000 candidates, so that a batch edge falls at every position of every chain.  Status, out_len and consumed
    equal the input's judged alone; the output is packed, a failed input's gap is what it had placed.  A failed comparison
    or a sanitizer report is a non-zero exit status."""
    p = subprocess.run([many_host, str(seed), "1500"], capture_output=True, text=True)
    assert p.returncode == 0, f"many_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "1500 cases held" in p.stdout
