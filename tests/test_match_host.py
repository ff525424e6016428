"""CPU: the matched parts alone (bzh_match*) without a device, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/match_host.cpp; nothing is loaded into Python under a sanitizer).  (a) The phases of
banzai_amd/csrc/match_core.h -- pass one with the matchers' longest1, the scan of the tiles' maps, the counting pass, the sums, the
gather -- thread by thread and tile by tile in the kernels' layout against a ten-line greedy loop.  (b) The windows and the cursor
of banzai_amd/csrc/match_plan.h with (a) as the device, against the same truth."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def match_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the matches' model"
    exe = str(tmp_path_factory.mktemp("match_host") / "match_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "match_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20263])
def test_match_model_against_the_greedy_loop(match_host, seed):
    """(a) n in {0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8192, 12289} x one string, a set with a pattern that is a
    prefix of another, an automaton with spans 256 and 1 x three densities; a run of one byte over three tiles searched for two of
    it, begun at an even and at an odd offset (every tile open, both parities across both edges); the same for a 256-byte pattern
    (entries up to 255); a match that spans a tile edge and is selected, one that is dropped because the cursor lies inside it;
    a tile entered at 255; 300 and 700 tiles with dense stretches across a scan thread's chunk edge and a chunk with no constant
    tile; entered_tiles and open_tiles non-zero where claimed and zero on a sparse text.  (b) 600 seeded lists of 1 to 7 blocks in
    windows of 1 to 4 blocks: a cursor beyond a window's end, held-back starts dropped and selected, a dense run across several
    window edges, rooms above, at and one below the need, zero, and not asked for.  A failed comparison or a sanitizer report is a
    non-zero exit."""
    p = subprocess.run([match_host, str(seed), "600"], capture_output=True, text=True)
    assert p.returncode == 0, f"match_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "raw: " in p.stdout and "windows: 600 cases held" in p.stdout
