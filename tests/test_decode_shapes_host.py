"""CPU: the decoder's serial front on blocks no encoder writes (tests/decode_shapes.py: code lengths up to 20, incomplete codes,
selectors beyond the last group, MTF positions up to 255, long runs, last columns that are no BWT of anything), through the
sanitizer build of tests/test_decode_host.py.  The expected bytes come from the construction; libbz2 and the strict decoder
are held to them as well."""
import bz2

import pytest

from tests import bz2_handbuilt, decode_shapes
from tests.test_decode_host import bzd_host, run_cases  # noqa: F401  (the fixture: one sanitizer build a session)

FORMAT = 3


def test_cases_reach_their_edges():
    """what each block really holds, so that a case cannot silently stop reaching the edge it is there for"""
    c = decode_shapes.accepted()
    for name in ("lengths_1_to_20", "lengths_20_to_1", "lengths_all_20", "one_byte_long_code", "runs"):
        assert c[name].longest_code == 20, name
    assert c["lengths_10_and_11"].longest_code == 11 and c["lengths_5_and_6"].longest_code == 6
    assert c["lengths_1_to_20"].positions >= {18} and c["lengths_20_to_1"].zero_runs  # the 20-bit codes: position 18 + EOB, RUNA / RUNB
    assert c["one_byte_short_code"].nblock == 1 and c["one_byte_short_code"].nsyms == 2
    assert c["six_tables"].selector_slots == {0, 1, 2, 3, 4, 5} and c["six_tables_one_used"].selector_slots == {0}
    assert c["two_tables_alternating"].selector_slots == {0, 1}
    for name, extra, total in (("selectors_1_extra", 1, None), ("selectors_100_extra", 100, None), ("selectors_18002", None, 18002),
                               ("selectors_18003", None, 18003), ("selectors_32767", None, 32767)):
        b = c[name]
        assert b.nsel == (total if total else b.groups + extra) and b.nsel > b.groups >= 2, name
    assert c["mtf_edges"].positions >= set(decode_shapes.EDGE_POSITIONS)
    b = c["mtf_always_255"]
    assert b.nsyms == 10_241 and b.positions == set(range(1, 256)) and b.nblock == 10_240
    b = c["runs"]
    assert set(b.zero_runs) >= set(decode_shapes.EDGE_RUNS) and b.runs_across_groups >= 1
    b = c["run_900000"]
    assert b.zero_runs == [900_000] and b.nsyms == 20 and len(b.stream) == 40 and b.level == 9
    assert {b.level for b in c.values()} == {1, 9}
    for name, b in c.items():
        assert b.nsel >= b.groups == (b.nsyms + 49) // 50 and len(b.expected) >= 1, name


def test_accepted_blocks(bzd_host, oracle, tmp_path):
    c = decode_shapes.accepted()
    res = run_cases(bzd_host, tmp_path, [b.stream for b in c.values()])
    libbz2_refused, oracle_refused = [], []
    for (name, b), (kind, consumed, got) in zip(c.items(), res):
        assert kind == 0, (name, kind)
        assert consumed == len(b.stream), name
        assert got == b.expected, name
        try:
            assert bz2.decompress(b.stream) == b.expected, name
        except (OSError, ValueError):
            libbz2_refused.append(name)
        try:
            assert oracle.decode(b.stream) == b.expected, name
        except oracle.DecodeError:
            oracle_refused.append(name)
    assert set(libbz2_refused) <= set(decode_shapes.LIBBZ2_MAY_REFUSE), libbz2_refused
    assert oracle_refused == sorted(decode_shapes.ORACLE_REFUSES), oracle_refused


def test_refused_blocks(bzd_host, oracle, tmp_path):
    c = decode_shapes.refused()
    res = run_cases(bzd_host, tmp_path, list(c.values()))  # (a sanitizer report fails run_cases)
    for (name, s), (kind, _, _) in zip(c.items(), res):
        assert kind == FORMAT, (name, kind)
        with pytest.raises((OSError, ValueError)):
            bz2.decompress(s)
        with pytest.raises(oracle.DecodeError) as e:
            oracle.decode(s)
        assert e.value.status == -3, name


def test_oversubscribed_table_that_no_selector_names(bzd_host, oracle, tmp_path):
    """The one divergence from libbz2, kept on purpose: a table with more codes than its lengths hold is refused even where no
    selector names it.  libbz2 accepts that unused-table form (it never checks a table); this decoder and the strict one build and
    check every table up front."""
    b = decode_shapes.oversubscribed_unused_table()
    assert bz2.decompress(b.stream) == b.expected
    assert run_cases(bzd_host, tmp_path, [b.stream])[0][0] == FORMAT
    with pytest.raises(oracle.DecodeError) as e:
        oracle.decode(b.stream)
    assert e.value.status == -3


def doubling_walk(col, ptr, nmax):
    """the inverse transform as bwt.hip computes it (unbwt_init / unbwt_round / unbwt_emit), round for round, for a block of a
    batch whose longest block has nmax bytes: P = T^m squared every round, X[m + r] = P[X[r]], n + 1 values of X"""
    n = len(col)
    P = sorted(range(n), key=col.__getitem__)  # the stable radix pass: T
    X = [ptr] + [None] * n
    m = 1
    while m <= nmax:  # the host's loop: one launch a round, P and P2 swapped behind each
        P2 = None
        if m <= n:
            if 2 * m <= n:
                P2 = [P[P[r]] for r in range(n)]
            for r in range(min(m, n + 1 - m)):
                X[m + r] = P[X[r]]
        P = P2
        m <<= 1
    return bytes(col[X[i + 1]] for i in range(n))


def test_doubling_walk_ends_where_the_serial_walk_ends():
    """the rule of the device's inverse transform against libbz2's serial walk, on columns that are no BWT of anything and at
    block lengths around the powers of two (where the number of rounds changes)"""
    import random
    rng = random.Random(5)
    odd_end = 0
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000):
        for alphabet in (1, 2, 3, 200):
            col = bytes(rng.randrange(alphabet) for _ in range(n))
            for ptr in {0, n // 2, n - 1}:
                want = bz2_handbuilt.inverse_column(col, ptr)
                odd_end += want[-1] != col[ptr]
                for nmax in (n, n + 1, 2 * n + 3):
                    assert doubling_walk(col, ptr, nmax) == want, (n, alphabet, ptr, nmax)
    assert odd_end > 20  # blocks whose last byte is not the one at the origin pointer: what a true BWT never has
