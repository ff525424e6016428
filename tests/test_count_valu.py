"""scripts/count_valu.py on a listing small enough to count by hand: kernels, the compiler's loop comments (a nested loop, a
block without a label, a block laid out behind its loop) and the parts of the source by the line table."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = """\
__global__ void k()
{
    // part: front
    a();
    for (;;) {
        // part: body
        b();
        // part: tail
        c();
    }
    // part: -
    d();
}
"""

LISTING = """\
\t.text
\t.file\t1 "/somewhere" "k.hip"
\t.file\t2 "/somewhere" "helpers.h"
_Z5otherv:                              ; @_Z5otherv
; %bb.0:
\tv_mov_b32_e32 v0, 0
\ts_endpgm
.Lfunc_end0:
_Z1kv:                                  ; @_Z1kv
; %bb.0:
\t.loc\t1 4 5
\tv_mov_b32_e32 v0, 0
\ts_mov_b32 s0, 0
.LBB1_1:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB1_2 Depth 2
\t.loc\t1 7 9
\tv_add_u32_e32 v0, 1, v0
\tds_read_b32 v1, v0
\t.loc\t2 90 3
\tv_or_b32_dpp v1, v1, v1 row_shr:1
.LBB1_2:                                ;   Parent Loop BB1_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\t.loc\t1 9 9
\tv_lshrrev_b32_e32 v2, 1, v1
\tglobal_store_short v2, v1, s[2:3]
\ts_cbranch_execnz .LBB1_2
; %bb.3:                                ;   in Loop: Header=BB1_1 Depth=1
\tv_add_u32_e32 v0, 2, v0
\ts_cbranch_scc1 .LBB1_5
.LBB1_4:
\t.loc\t1 12 5
\tv_mov_b32_e32 v3, 0
\ts_endpgm
.LBB1_5:                                ;   in Loop: Header=BB1_1 Depth=1
\t.loc\t1 7 9
\tds_write_b32 v0, v1
\ts_branch .LBB1_1
.Lfunc_end1:
"""


def test_counts_loops_and_parts(tmp_path):
    (tmp_path / "k.hip").write_text(SOURCE)
    (tmp_path / "k.s").write_text(LISTING)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "count_valu.py"), str(tmp_path / "k.s"), "--kernel", "_Z1kv",
                          "--source", str(tmp_path / "k.hip")], check=True, capture_output=True, text=True).stdout
    lines = [" ".join(l.split()) for l in out.splitlines()]
    assert "_Z1kv: v_ 6, ds_ 2" in lines
    assert not any("_Z5otherv" in l for l in lines)
    assert "loop BB1_1 depth 1 own v_ 3 ds_ 2 total v_ 4 ds_ 2" in lines
    assert "loop BB1_2 depth 2 own v_ 1 ds_ 0 total v_ 1 ds_ 0" in lines
    # the helper's instruction stays with `body`; the block without its own line stays with `tail`; the block behind the loop
    # comes back to `body`; the instructions outside every loop are in no part
    assert "body in BB1_1 v_ 2 ds_ 2" in lines
    assert "tail in BB1_2 v_ 1 ds_ 0" in lines
    assert "tail in BB1_1 v_ 1 ds_ 0" in lines
    assert not any(l.startswith("front") for l in lines)
