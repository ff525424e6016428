"""CPU: how the library cuts its workspaces (banzai_amd/csrc/batch.h -- the carver, layout_batch, the views of borrowed arrays;
decode_plan.h -- the decoder's tables; encode_plan.h -- the plan's two workspaces), as a stand-alone program with
AddressSanitizer and UBSan (tests/workspace_host/layout_host.cpp).  The library lays its device memory out with the same text:
an array that overlaps its neighbour, or a borrowed array too small for its borrower, is found here without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def layout_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the workspace layouts"
    exe = str(tmp_path_factory.mktemp("workspace_host") / "layout_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined,pointer-overflow",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "workspace_host", "layout_host.cpp")])
    return exe


def test_workspace_layouts(layout_host):
    """Levels 1..9.  layout_batch at B in {1, 2, 8, 9, 16, 17, 112, 576}: every array 256-byte aligned, inside the arena, clear of
    the next, the same in a measuring pass (null base: no pointer formed) and a real one; every view of a borrowed array within
    its lender at both MTF tile sizes, its need worked out from the kernels' indexing; the two lanes of max_batch 1, 2, 3 and
    576 disjoint and inside the arena ensure_lanes asks for; the same for the decoder's tables (B 1 and 576), the plan's
    workspace (n 1, 4095, 4096, 4097, 2^20; extra 0 and 1000) and the many-inputs workspace (1, 2 and 1000 inputs, empty ones
    among them).  A failed comparison or a sanitizer report is a non-zero exit status."""
    p = subprocess.run([layout_host], capture_output=True, text=True)
    assert p.returncode == 0, f"layout_host exit status {p.returncode}: {p.stdout[-500:]} {p.stderr[-3000:]}"
    assert "held at levels 1..9" in p.stdout
