"""bzh_encode_many* without a device: the declared surface, the Python wrapper's argument checks, and the output bound
held against the oracle's streams for adversarial inputs."""
import os

import numpy as np
import pytest

from tests.test_abi import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANY = ("bzh_encode_many_device", "bzh_encode_many", "bzh_encode_many_bound", "bzh_plan_many_device")


def test_header_declares_many_entry_points():
    syms = header_symbols()
    for name in MANY:
        assert name in syms, name


def test_encode_many_validates_without_a_device():
    import banzai_amd
    for bad in (0, 10, -1, "9", 9.0, True):
        with pytest.raises(ValueError):
            banzai_amd.encode_many([b"abc"], bad)
    for item in ("text", 5, None, [1, 2], object()):
        with pytest.raises(TypeError):
            banzai_amd.encode_many([b"abc", item], 9)
    assert banzai_amd.encode_many([], 9) == []
    assert banzai_amd.encode_many(iter(()), 1) == []


def _adversarial(seed):
    rng = np.random.default_rng(seed)
    out = [b"", b"a", bytes(range(256)), bytes(range(256)) * 700]
    out.append(rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes())
    for run in (4, 255, 256):
        # runs of exactly `run` bytes, each byte unlike its neighbours: the RLE1 worst cases
        vals = rng.permutation(np.tile(np.arange(256, dtype=np.uint8), 8))
        out.append(b"".join(bytes([v]) * run for v in vals[: 120_000 // run]))
    out.append(rng.integers(0, 256, 1000, dtype=np.uint8).tobytes() + b"\x07" * 5000)
    return out


def _align4(n):
    return (n + 3) & ~3


@pytest.mark.parametrize("level", [1, 9])
def test_bound_covers_oracle_streams(native, oracle, level):
    items = _adversarial(level)
    sizes = [len(oracle.encode(x, level)) for x in items]
    for x, s in zip(items, sizes):  # single inputs
        assert native.encode_many_bound(level, [len(x)]) >= _align4(s)
    # lists: the back-to-back layout with its alignment
    assert native.encode_many_bound(level, [len(x) for x in items]) >= sum(_align4(s) for s in sizes)
    tiny = [len(x) for x in items[:2]] * 5000  # ten thousand tiny inputs: a few kB each, not a block's worth
    assert native.encode_many_bound(level, tiny) <= 5000 * len(tiny)


def test_bound_rejects_a_bad_level(native):
    for bad in (0, 10, -1):
        assert native.encode_many_bound(bad, [1, 2, 3]) == 0
    assert native.encode_many_bound(9, []) == 0
    assert native.encode_many_bound(9, [0]) >= 14
