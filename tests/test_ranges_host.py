"""CPU: the host arithmetic of a call over many ranges (banzai_amd/csrc/decode_plan.h -- bzp_spans, which is bzh_index_spans and the
output layout of bzh_decode_ranges; bzp_block_pieces and bzp_pieces, the tables unrle_walk_pieces stores by; bzp_segments
over a list of entries) against brute force per output byte, as a stand-alone program with AddressSanitizer and UBSan
(tests/decode_host/ranges_host.cpp).  What these compute are destinations of stores on the device.  And what unrle_walk_pieces
does with those tables, thread by thread in the kernel's layout, from the text it shares with the kernel -- decode_core.h's
bzd_ur_emit and bzd_piece_cut -- against the serial expansion (tests/decode_host/pieces_host.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sanitizer_build(tmp_path_factory, name):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the ranges plan"
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", name + ".cpp")])
    return exe


@pytest.fixture(scope="module")
def ranges_host(tmp_path_factory):
    return sanitizer_build(tmp_path_factory, "ranges_host")


@pytest.fixture(scope="module")
def pieces_host(tmp_path_factory):
    return sanitizer_build(tmp_path_factory, "pieces_host")


@pytest.mark.parametrize("seed", [1, 20262])
def test_ranges_plan_against_brute_force(ranges_host, seed):
    """3000 seeded cases: synthetic indexes of 0 to 11 blocks, many of them of 1 byte, tiles with no output, 0 to 64 ranges that
    overlap, repeat, are empty, lie behind the total or end at 2^64 - 1 and beyond, batches of 1 to 5 blocks; a failed comparison
    or a sanitizer report is a non-zero exit status"""
    p = subprocess.run([ranges_host, str(seed), "3000"], capture_output=True, text=True)
    assert p.returncode == 0, f"ranges_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "3000 cases each" in p.stdout


def test_pieces_walk_against_the_serial_expansion(pieces_host):
    """300 seeded blocks of 1 to 12,287 bytes behind the inverse BWT, half of them run-heavy so that their tiles exceed the
    stage, 0 to 69 pieces each (and the fixed ones: a block of one byte, exactly one tile, one byte more, 1,100 pieces over
    unstaged tiles): every piece holds the bytes of the serial expansion, every output byte is written once, and the stage
    and the output, allocated at their exact sizes, are never left"""
    p = subprocess.run([pieces_host, "7", "300"], capture_output=True, text=True)
    assert p.returncode == 0, f"pieces_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "300 seeded blocks held" in p.stdout
