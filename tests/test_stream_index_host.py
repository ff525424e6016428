"""CPU: the host side of an index that is written while its stream is (banzai_amd/csrc/stream_index.h), as a stand-alone program
with AddressSanitizer and UBSan (tests/decode_host/stream_index_host.cpp): the rebase of a streaming pass's entries and sync points
into stream coordinates and the take, against a stream laid out once in absolute coordinates; and the index files of the C ABI
(bzh_index_blob_write / _read are these functions) on random and damaged blobs held in buffers of their exact size."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stream_index_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the stream index arithmetic"
    exe = str(tmp_path_factory.mktemp("stream_index_host") / "stream_index_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "stream_index_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20263])
def test_rebase_take_and_blobs_against_the_restatement(stream_index_host, seed):
    """2000 seeded streams of 1 to 9 passes -- passes with no final block, every phase 0..31 (the program insists on having seen
    all 32), streams that begin above bit 2^32, takes after some passes and one at the end, takes with an array one short --
    and 201 seeded blobs of 0 to 300 entries and 0 to 4,000 points at intervals 0, 1, 256 and others: round trip, BZH_E_CAP with
    both counts, every truncation, every header bit and 64 body bits flipped, random bytes behind either magic; a failed
    comparison or a sanitizer report is a non-zero exit status"""
    p = subprocess.run([stream_index_host, str(seed), "2000"], capture_output=True, text=True)
    assert p.returncode == 0, f"stream_index_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "2000 rebase cases and 201 blob cases held" in p.stdout
