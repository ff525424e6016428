"""The inverse-RLE1 edge suite on the CPU (tests/unrle_paths_model.py, tests/unrle_cases.py): the model's constants are the kernels',
its layout is the one the kernels' per-thread text is laid out by (tests/decode_host/unrle_host.cpp --layout, built with
-fsanitize=address,undefined) on every case and on seeded random blocks, every case reaches the edges it was built for, every
declared edge has a case, every stream is one that libbz2 reads as bz2_handbuilt.unrle reads its block, and each deliberately
wrong variant of the model is told from the truth by a case of the family built for it.  No GPU, no library under test."""
import bz2
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import bz2_handbuilt
from tests import unrle_cases as uc
from tests import unrle_paths_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "banzai_amd", "csrc", "decode.hip")).read()
    m = re.search(r"constexpr uint32_t UR_THREADS = (\d+), UR_ITEMS = (\d+), UR_TILE = UR_THREADS \* UR_ITEMS, UR_STAGE = (\d+);", text)
    assert m, "the constexpr line of the unrle kernels has changed: tests/unrle_paths_model.py restates it"
    assert (um.UR_THREADS, um.UR_ITEMS, um.UR_STAGE) == tuple(int(v) for v in m.groups())
    assert um.UR_TILE == um.UR_THREADS * um.UR_ITEMS and um.WAVE == 64 * um.UR_ITEMS
    assert "f1 - f0 < UR_THREADS / 64" in text and um.PIECE_WAVES == um.UR_THREADS // 64
    assert "const bool staged = tile_total <= UR_STAGE;" in text and "if (tile_total > UR_STAGE) {" in text
    assert "(uint32_t)((0 - (uintptr_t)g) & 3u)" in text  # ur_copy_out's head
    core = open(os.path.join(ROOT, "banzai_amd", "csrc", "decode_core.h")).read()
    assert "constexpr uint32_t BZD_UR_ITEMS = %d;" % um.UR_ITEMS in core


# ---- the model against the layout the kernels' text is run by --------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the layout"
    exe = str(tmp_path_factory.mktemp("unrle_layout") / "unrle_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "unrle_host.cpp")])
    return exe


def same_as_host(exe, tmp_path, blocks):
    fin, fout = str(tmp_path / "blocks.bin"), str(tmp_path / "layout.bin")
    with open(fin, "wb") as f:
        for b in blocks:
            f.write(struct.pack("<I", len(b)))
            f.write(b)
    p = subprocess.run([exe, "--layout", fin, fout], capture_output=True, text=True)
    assert p.returncode == 0, f"unrle_host --layout exit status {p.returncode}: {p.stderr[-3000:]}"
    d = np.fromfile(fout, dtype=np.uint32).astype(np.int64)
    at = 0
    for k, b in enumerate(blocks):
        r = um.analyse(b, obase=k % 4)
        T, end, bsize = d[at:at + 3]
        at += 3
        assert (T, end, bsize) == (r["T"], r["end"][2], r["bsize"]), (k, len(b))
        tl = d[at:at + 2 * T].reshape(T, 2)
        at += 2 * T
        th = d[at:at + 3 * um.UR_THREADS * T].reshape(T, um.UR_THREADS, 3)
        at += 3 * um.UR_THREADS * T
        assert tl[:, 0].tolist() == [t["toff"] for t in r["tiles"]] and tl[:, 1].tolist() == [t["total"] for t in r["tiles"]], (k, len(b))
        for j, what in enumerate(("state", "outn", "off")):
            assert np.array_equal(th[:, :, j], r["threads"][what]), (k, len(b), what)
        # the thread that writes endstate is the one that holds the last byte, and the host's end state is its own
        assert r["end"][:2] == ((len(b) - 1) // um.UR_TILE, ((len(b) - 1) % um.UR_TILE) // um.UR_ITEMS)
        want, closed = bz2_handbuilt.unrle(b)
        assert r["out"] == want and (end != 4) == closed, (k, len(b))
    assert at == d.size


@pytest.mark.parametrize("family", list(uc.FAMILIES))
def test_model_is_the_host_layout_on_every_case(layout_host, tmp_path, family):
    same_as_host(layout_host, tmp_path, sorted({uc.case(n)[1] for n in uc.FAMILIES[family]}))


def test_model_is_the_host_layout_on_random_blocks(layout_host, tmp_path):
    rng = random.Random(2027)
    blocks = []
    for k in range(2000):
        n = rng.choice((1, 2, 3, 15, 16, 17, 31, 33, 64, 100, 255, 1023, 1024, 1025)) if k % 50 else rng.randrange(4000, 13000)
        stick = rng.randrange(1, 5)
        b = bytearray()
        for i in range(n):
            b.append(b[-1] if i and rng.randrange(5) < stick else rng.choice((0, 1, 4, 5, 255)))
        blocks.append(bytes(b))
    assert sum(not bz2_handbuilt.unrle(b)[1] for b in blocks) > 100  # blocks that end in state 4 are among them
    same_as_host(layout_host, tmp_path, blocks)


# ---- the case list -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(uc.FAMILIES))
def test_every_case_reaches_its_edges(family):
    for name in uc.FAMILIES[family]:
        (_, x, level, want, extras), rec = uc.analysed(name)
        assert uc.unmet(rec, want) == [], name
        truth, closed = uc.truth(name)
        assert rec["out"] == truth and rec["bsize"] == len(truth) and (rec["end"][2] != 4) == closed, name
        assert len(x) <= 5 * um.UR_TILE or family in ("chain", "stale"), name
        if "delim" in extras:
            pos = [i for i, v in enumerate(truth) if v == extras["delim"]]
            assert rec["count"] == len(pos) == int(rec["tcount"].sum()) and rec["last"] == truth.endswith(bytes([extras["delim"]])), name
            assert [rec["select"](k + 1) for k in range(len(pos))] == pos, name
        for w in rec["windows"] + rec["pieces"]:  # the cuts of a window or a piece tile its bytes
            assert sum(c["thi"] - c["tlo"] for c in w["cuts"]) == w["hi"] - w["lo"], name


def test_every_edge_has_a_case_and_every_want_is_declared():
    declared = [e for fam in uc.EDGES.values() for e in fam]
    assert len(declared) == len(set(declared))
    wanted = {}
    for name in uc.NAMES:
        for w in uc.case(name)[3]:
            wanted.setdefault(w, []).append(name)
    assert sorted(set(declared) - set(wanted)) == [], "declared and never built"
    assert sorted(set(wanted) - set(declared)) == [], "built and never declared"
    assert set(uc.EDGES) == set(uc.FAMILIES)


@pytest.mark.parametrize("family", list(uc.FAMILIES))
def test_streams_are_what_libbz2_reads(family):
    """every case framed: Python's bz2 accepts it and gives bz2_handbuilt.unrle's bytes; a block that ends in four equal bytes
    without a count is refused"""
    state4 = 0
    for name in uc.FAMILIES[family]:
        s = uc.stream(name)
        truth, closed = uc.truth(name)
        if closed:
            assert bz2.decompress(s) == truth, name
        else:
            state4 += 1
            with pytest.raises(Exception):
                bz2.decompress(s)
    assert (state4 > 0) == (family == "ends")


# ---- sensitivity: a wrong layout is told from the truth by the cases built for its edge ------------------------------------------
CAUGHT_BY = {  # variant -> (family, the wanted edge whose cases must tell it)
    "no_wave_carry": ("seams", "seam:wave:"),
    "chain_le": ("constant", "stretch:"),
    "chain_one_wave": ("chain", "chain:tiles_over:"),
    "no_prev": ("seams", "seam:thread:"),
    "stale_behind_n": ("ends", "behind_n"),
    "count_eq_run": ("seams", "count:again"),
    "stage_one_more": ("staging", "tile_total:"),
    "head_residue": ("copyout", "copy:head:"),
    "count_is_delim": ("records", "rec:count_value_not_counted"),
    "end_from_full_thread": ("ends", "end_state:"),
}


def signature(name, variant):
    """what a decoder that worked by this layout would hand back: bytes (and with them size and CRC), the state behind the block
    (status -6 or not), the delimiter count with the last-byte flag, and the positions a read by record number selects"""
    c, rec = uc.analysed(name, variant)
    sig = [rec["out"], rec["bsize"], rec["end"][2] == 4]
    if "delim" in c[4]:
        sig += [rec["count"], rec["last"], tuple(rec["tcount"].tolist()), tuple(rec["select"](k + 1) for k in range(min(rec["count"], 600)))]
    return sig


def test_the_variants_are_all_here():
    assert set(CAUGHT_BY) == set(um.VARIANTS)


@pytest.mark.parametrize("variant", list(um.VARIANTS))
def test_a_wrong_variant_is_caught(variant):
    family, edge = CAUGHT_BY[variant]
    names = [n for n in uc.FAMILIES[family] if any(w.startswith(edge) for w in uc.case(n)[3])]
    assert names
    caught = [n for n in names if signature(n, variant) != signature(n, None)]
    assert caught, (variant, um.VARIANTS[variant])
    # and the right layout is the truth on the same cases: what differs is the variant's doing
    for n in caught[:5]:
        assert signature(n, None)[0] == uc.truth(n)[0]
