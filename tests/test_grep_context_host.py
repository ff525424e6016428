"""CPU: the grep with context records without a device, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/grep_ctx_host.cpp; nothing is loaded into Python under a sanitizer).  (a) The phases of
banzai_amd/csrc/grep_ctx_core.h -- pass one, the scan of the distances, pass two, the sums, the gather -- thread by thread and tile
by tile in the kernels' layout against a naive split-find-dilate.  (b) The windows, the pending records and the tail of
banzai_amd/csrc/grep_ctx_plan.h with (a) as the device, against the same truth."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grep_ctx_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the context grep's model"
    exe = str(tmp_path_factory.mktemp("grep_ctx_host") / "grep_ctx_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "grep_ctx_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20263])
def test_context_model_against_split_find_dilate(grep_ctx_host, seed):
    """(a) n in {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289} x (before, after) in {(0,0), (1,0), (0,1), (1,1), (2,3), (16,16),
    (17,0), (0,17), (5000,5000)} x invert x delimiter densities from none to delimiters only (16 records a thread); a primary as
    the last and as the first record of a tile with the context reaching one and two tiles on and back; a record longer than one
    and than two tiles as context; two primaries whose contexts overlap, touch and leave one record between them, with the group
    count; a primary at record 0 and at the last record; a primary tail and a tail that is after-context; 300 and 700 tiles, so
    that a scan thread owns several and contexts cross the chunk edges; with (0, 0) the same inputs through grep_core.h's phases.
    (b) 600 seeded lists of 1 to 7 blocks in windows of 1 to 4 blocks: pending records across one and several window edges, a
    window without a delimiter between two with, before above the records of a window, the only primary being the tail, every
    uint32_t reach, rooms above, at and one below the need, zero, and not asked for; the pending records behind every window and
    pending_peak against a count of their own.  A failed comparison or a sanitizer report is a non-zero exit."""
    p = subprocess.run([grep_ctx_host, str(seed), "600"], capture_output=True, text=True)
    assert p.returncode == 0, f"grep_ctx_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "raw: " in p.stdout and "windows: 600 cases held" in p.stdout
