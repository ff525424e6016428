"""CPU: what bzh_recover and bzh_recover_stream decide on the host, as stand-alone programs with AddressSanitizer and UBSan.
The walk (banzai_amd/csrc/decode_recover_plan.h: candidates, the shadow of a kept block, the verdict, flags that wait for a
footer a batch later) against a restatement that makes one pass over all candidates and knows no batches
(tests/decode_host/recover_host.cpp); the per-word rule of the gather kernel (banzai_amd/csrc/recover_gather.h: descriptor
search, two-word funnel, tail mask) and the check of an untrusted report against a bit-by-bit copy
(tests/decode_host/gather_host.cpp).  decode.hip and recover.hip compile the same text; the GPU is only where the walk's
results come from and where the rule runs a thread a word."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path_factory, name):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build"
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", name + ".cpp")])
    return exe


@pytest.fixture(scope="module")
def recover_host(tmp_path_factory):
    return _build(tmp_path_factory, "recover_host")


@pytest.fixture(scope="module")
def gather_host(tmp_path_factory):
    return _build(tmp_path_factory, "gather_host")


@pytest.mark.parametrize("seed", [1, 20261])
def test_walk_against_one_pass_over_all_candidates(recover_host, seed):
    """1500 seeded worlds and the fixed ones -- 0 to 4 streams of 0 to 4 blocks; magics of both kinds inside kept payloads and
    inside lost ones; loose footers and loose blocks in foreign bytes; a lost magic; a lost stream header, the first and a later
    one; a lost, truncated or CRC-wrong footer; each loss kind in every position beside every footer damage; a block above the
    context's level, as the walk checks it and as the kernel reports it; a block above its stream's level but within the
    context's (kept, not STREAM_OK); everything lost; nothing at all; a kept block planted inside a lost one -- each walked in
    batches of 1, 2, 3, 4, 5, 7, 8, 16 and 1000 candidates and with room for everything, for exactly everything, for one byte
    less and for nothing.  Entries byte for byte, statistics, the total and `over` equal the restatement's; every kept item of
    a batch has its entry.  A failed comparison or a sanitizer report is a non-zero exit status."""
    p = subprocess.run([recover_host, str(seed), "1500"], capture_output=True, text=True)
    assert p.returncode == 0, f"recover_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "1500 cases held" in p.stdout


@pytest.mark.parametrize("seed", [1, 20261])
def test_gather_rule_against_a_bit_by_bit_copy(gather_host, seed):
    """Single blocks of every source residue 0-31 x destination residue 0-31 x 1-130 bits, the source ending with the block's
    last bit; 400 seeded lists of 1-40 blocks of 81 bits and more with gaps and lost entries between them, the first at bit 0
    and the last in the last bits of the buffer now and then; the search once per 64 words and once per word.  The words equal
    a bit-by-bit copy, guard words around them are untouched, source and output are heap arrays of exactly their size; the
    report check accepts what is well formed and names the entry of each of the four things it refuses."""
    p = subprocess.run([gather_host, str(seed), "400"], capture_output=True, text=True)
    assert p.returncode == 0, f"gather_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "400 lists held" in p.stdout
