"""CPU: the rules by which the encoder writes sync points (tests/esync_model.py, the serial form of sync_emit.hip's) give the
points the decoder's recorder reports for the same block (tests/sync_model.py: the sanitizer build of decode_core.h)."""
import random

import pytest

from tests import esync_model, sync_model

INPUTS = {
    "text": lambda: esync_model.text(90_000),
    "run_heavy": lambda: sync_model.run_heavy(),
    "random": lambda: random.Random(5).randbytes(60_000),  # 256 names
    "one_name": lambda: b"a" * 50_000,                     # RLE1 leaves under a thousand bytes: fewer symbols than one group, no point
    "short": lambda: esync_model.text(3_000),              # fewer groups than an interval of 256; some at 1 and 7
}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("esync_model")
    return sync_model.build(tmp), tmp


@pytest.fixture(scope="module")
def blocks(oracle):
    """per input: (its level-1 stream, the last column of its only block)"""
    out = {}
    for name, make in INPUTS.items():
        data = make()
        rle, _, consumed = oracle.rle_one(data, 1)
        assert consumed == len(data), name  # one block
        last, _, _ = oracle.bwt(bytes(rle))
        out[name] = (oracle.encode(data, 1), bytes(last))
    return out


@pytest.mark.parametrize("interval", [1, 7])
def test_encoder_rules_give_the_decoders_points(model, blocks, interval):
    exe, tmp = model
    names = list(blocks)
    want, _ = sync_model.run(exe, tmp, [blocks[k][0] for k in names], interval)
    kinds = []
    for name, (nblocks, wpts, _, _) in zip(names, want):
        assert nblocks == 1
        got = esync_model.points(blocks[name][1], interval, kinds)
        assert len(got) == len(wpts) and (len(got) > 0 or name == "one_name"), (name, interval)
        for k, (group, out_pos, run, weight, mtf) in enumerate(got):
            w = wpts[k]
            assert (group, out_pos, run, weight) == (int(w["group"]), int(w["out_pos"]), int(w["run"]), int(w["run_weight"])), (name, k)
            assert mtf == w["mtf"].tolist(), (name, k)
    if interval == 1:
        assert {"none", "mid", "head"} <= set(kinds)  # points inside a run's digits and behind its last one both occur


@pytest.mark.parametrize("TL", [2048, 4096, 64])
def test_tile_form_gives_the_serial_points(blocks, TL):
    """the kernel's way to a point -- tile by offset, head by count, keys raised inside the tile -- against the serial walk;
    tiles of 64 bytes put tiles without a head, runs across many tiles and trailing empty tiles into every input"""
    for name, (_, last) in blocks.items():
        if TL == 64 and name in ("text", "random"):
            last = last[:20_000]  # (the tile form is quadratic in the names: a part of the column is as good for tiny tiles)
        for interval in ((1, 7) if name != "random" else (7,)):
            assert esync_model.points_by_tiles(last, interval, TL) == esync_model.points(last, interval), (name, interval, TL)


@pytest.mark.parametrize("TL", [2048, 4096, 64])
def test_lane_form_gives_the_serial_points(blocks, TL):
    """the kernel's steps lane for lane (64 lanes in lock step, the tile behind its margin in LDS) against the serial walk"""
    for name, (_, last) in blocks.items():
        if name in ("text", "random"):
            last = last[:12_000]
        for interval in (1, 7):
            assert esync_model.points_by_lanes(last, interval, TL) == esync_model.points(last, interval), (name, interval, TL)
