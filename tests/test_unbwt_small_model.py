"""CPU: the NumPy model of the LDS inverse BWT (tests/unbwt_small_model.py: the kernel's phases, its 16-bit indices) against
libbz2's serial walk (bz2_handbuilt.inverse_column) -- on the BWT of something and on columns that are no BWT of anything, where
the last byte is L[T^n(ptr)] and not L[ptr]."""
import random

import numpy as np
import pytest

from tests import bz2_handbuilt, unbwt_small_model as model

BOUND = model.SMALL_MAX


def columns(n, rng):
    """random, one-byte-alphabet, periodic, two-byte and no-BWT columns of n bytes, each with a few origin pointers"""
    nprng = np.random.default_rng(n)
    cols = [nprng.integers(0, 256, n, dtype=np.uint8).tobytes(), b"\x07" * n, (b"ab" * n)[:n], (bytes(range(5)) * n)[:n],
            nprng.integers(0, 2, n, dtype=np.uint8).tobytes(), (b"ab" * (n // 4 + 1) + b"ba" * (n // 4 + 1))[:n]]
    for col in cols:
        for ptr in sorted({0, n - 1, rng.randrange(n)}):
            yield col, ptr


def check(n, rng):
    for col, ptr in columns(n, rng):
        assert model.inverse(col, ptr) == bz2_handbuilt.inverse_column(col, ptr), (n, ptr, col[:16])


def test_bound_matches_the_library(native):
    assert model.SMALL_MAX == native.decode_many_small_max()


def test_every_length_up_to_130():
    rng = random.Random(1)
    for n in range(1, 131):
        check(n, rng)


@pytest.mark.parametrize("n", sorted({p + d for p in (256, 512, 1024, 2048, 4096, 8192) for d in (-1, 0, 1) if p + d <= BOUND}
                                     | {BOUND - 1, BOUND, 511 * 8 + 1, 64 * 8, 64 * 8 + 1}))
def test_around_powers_of_two_and_at_the_bound(n):
    check(n, random.Random(n))


def test_the_last_byte_is_not_the_one_at_the_origin_pointer():
    """columns whose walk closes a cycle that does not divide n: the model must differ from 'S[n-1] = L[ptr]' there"""
    seen = 0
    for col, ptr in ((b"ab" * 500 + b"ba" * 500, 1), (b"ab" * 500 + b"ba" * 500, 1999), (b"ba" * 2048 + b"a", 7),
                     (bytes(range(256)) + bytes(range(255, -1, -1)) * 20, 5000)):
        want = bz2_handbuilt.inverse_column(col, ptr)
        assert model.inverse(col, ptr) == want
        seen += want[-1] != col[ptr]
    assert seen >= 2
