"""CPU: reads by record number without a device, as stand-alone programs with AddressSanitizer and UBSan.  The host arithmetic
(banzai_amd/csrc/decode_records_plan.h -- the table check, bzq_spans, which is bzh_record_spans, and the walk of bzh_decode_records
over its batches: the queries it sends to unrle_select, the pieces, the running output offsets) against brute force per output
byte (tests/decode_host/records_host.cpp).  And what unrle_count and unrle_select do, thread by thread in the kernels' layout,
from the text they share with the kernels -- decode_core.h's bzd_ur_count and bzd_ur_select -- against the serial expansion
(tests/decode_host/count_host.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sanitizer_build(tmp_path_factory, name):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the records plan"
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", name + ".cpp")])
    return exe


@pytest.fixture(scope="module")
def records_host(tmp_path_factory):
    return sanitizer_build(tmp_path_factory, "records_host")


@pytest.fixture(scope="module")
def count_host(tmp_path_factory):
    return sanitizer_build(tmp_path_factory, "count_host")


@pytest.mark.parametrize("seed", [1, 20262])
def test_records_plan_against_brute_force(records_host, seed):
    """3000 seeded cases: synthetic indexes of 0 to 11 blocks, many of 1 byte, tiles with no output, delimiters at a block's last
    byte and at the next block's first, none at all and every byte one, 0 to 40 ascending ranges with empty and adjacent ones,
    ones behind D and lengths up to 2^64 - 1, batches of 1 to 5 blocks; every list that does not ascend is refused and the range
    named; a failed comparison or a sanitizer report is a non-zero exit status"""
    p = subprocess.run([records_host, str(seed), "3000"], capture_output=True, text=True)
    assert p.returncode == 0, f"records_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "3000 cases held" in p.stdout


def test_count_and_select_against_the_serial_expansion(count_host):
    """120 seeded blocks of 1 to 12,287 bytes behind the inverse BWT, half of them run-heavy, and the fixed ones (the count byte
    equal to the delimiter, a run whose count byte opens the next thread and the next tile, count bytes 0 and 255, a block of one
    byte, exactly one tile and one byte more, every k of a 259-byte run): every tile's count, every k of every tile, the
    last-byte flag; the arrays have their exact sizes"""
    p = subprocess.run([count_host, "7", "120"], capture_output=True, text=True)
    assert p.returncode == 0, f"count_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "120 seeded blocks held" in p.stdout
