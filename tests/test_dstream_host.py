"""CPU: the resumable chain walk and the feed loop of bzh_dstream_* (banzai_amd/csrc/decode_stream_plan.h -- a sliding window of
the input, undecided items that wait for more bytes, staging room, tail moves, growing rooms) against a restatement that walks
the whole buffer once and knows no windows, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/dstream_host.cpp).  decode.hip's DStreamDev drives the same text; the GPU is only where its results come
from."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dstream_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the walk"
    exe = str(tmp_path_factory.mktemp("dstream_host") / "dstream_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "dstream_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20261])
def test_walk_against_the_whole_buffer_walked_once(dstream_host, seed):
    """30 seeded worlds of 1-5 streams of 0-6 blocks with magics inside payloads, empty streams, no tail / a foreign tail / a
    tail that is a prefix of "BZh9", and one defect of every kind (a field outside the format, a randomised block, block and
    stream CRC, an end in four equal bytes, too many bytes for the level, a cut at a seeded bit, a damaged stream header, a
    lost magic, a level above the context's in the first and in a later stream, an empty and a 1-3 byte input): each fed byte
    by byte and in one piece through every pair of a window target of 16, 64, 200 and 100,000 bytes and a staging target of 1,
    50 and 100,000 bytes with a cap of 1, 7 and 1 MiB, and split in two at every byte with the rooms, caps and batch sizes
    (1, 2, 3, 1000 candidates) taking turns.  Output, consumed, status and the named item equal the restatement's; on an error
    the bytes handed out are a prefix of the true output and the next feed is a call sequence error; no feed with input or
    pending output does nothing.  The fake device holds a real window and a real staging buffer, sized exactly, and checks
    every byte of the window against the input before every scan and batch.  The program itself fails unless the runs moved a
    tail, grew a window, grew a staging buffer, redid a block, made a footer wait for what follows it and met a magic that
    straddles two scans.  A failed comparison or a sanitizer report is a non-zero exit status."""
    p = subprocess.run([dstream_host, str(seed), "30"], capture_output=True, text=True)
    assert p.returncode == 0, f"dstream_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "30 cases held" in p.stdout
