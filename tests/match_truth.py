"""What bzh_match* has to return -- the matched parts alone, grep -o -- by Python's `re` on bytes: the reference of every test
of the matches, itself held to GNU grep by tests/test_match_truth.py.

THE RULE, over the whole text: for a start s that holds a match, L(s) is the length of the LONGEST match there of at most `span`
bytes, assertions seeing the real neighbours (tests/regex_look_truth.py: a candidate t[s:e] holds iff the expression, followed
by a look-ahead that pins the end, matches at s; `re` alone is leftmost-FIRST and `endpos` hides the neighbours).  A cursor walks
from 0: the next match is at the lowest s >= cursor that holds one, and the cursor becomes s + L(s).

`re.search(text, cursor)` names the lowest start at or behind the cursor at which ANY match exists, whatever the alternative the
engine prefers, and sees the real bytes in front of the cursor; L(s) is then found by bisection as in regex_look_truth.hits.  A
start whose only matches are longer than `span` holds none."""
import bisect
import re

from tests.regex_look_truth import ASSERT, FOLD, LINE, WORD, _flags, _left, wrapped  # noqa: F401


def literal(pats):
    """byte strings as expressions"""
    return [re.escape(p) for p in pats]


def longest_at(ws, f, text, s, span=256):
    """-> (L, pattern) of the start s, (0, None) where it holds no match of at most `span` bytes"""
    n = len(text)
    end = min(n, s + span)
    s0 = max(s - 1, 0)
    piece = text[s0:min(end + 1, n)]
    at, tail = s - s0, (1 if end < n else 0)
    room = len(piece) - at
    if not any(_left(w, f, tail, room - 1).match(piece, at) for w in ws):
        return 0, None
    a, b = 1, end - s
    while a < b:
        k = (a + b + 1) // 2
        if any(_left(w, f, tail, room - k).match(piece, at) for w in ws):
            a = k
        else:
            b = k - 1
    who = [j for j, w in enumerate(ws) if _left(w, f, room - a, room - a).match(piece, at)]
    assert who and a >= 1
    return a, who[0]


def select(exprs, text, flags=0, span=256, syntax=ASSERT):
    """-> [(off, pattern, len)]: the non-overlapping leftmost-longest matches"""
    f = _flags(flags)
    ws = [wrapped(e, syntax) for e in exprs]
    some = re.compile(b"|".join(b"(?:" + w + b")" for w in ws), f)
    out, cursor = [], 0
    while cursor < len(text):
        m = some.search(text, cursor)
        if m is None:
            break
        s = m.start()
        length, who = longest_at(ws, f, text, s, span)
        if length:
            out.append((s, who, length))
            cursor = s + length
        else:
            cursor = s + 1
    return out


def matches(exprs, text, flags=0, span=256, syntax=ASSERT, delim=None):
    """-> (bytes, [(off, record, pattern, len, out_off)]) as bzh_match* returns them; delim None: record 0"""
    delims = [k for k, b in enumerate(text) if delim is not None and b == delim[0]]
    out, rows = bytearray(), []
    for s, who, length in select(exprs, text, flags, span, syntax):
        rows.append((s, bisect.bisect_left(delims, s), who, length, len(out)))
        out += text[s:s + length]
    return bytes(out), rows


def rows_of(entries):
    return [tuple(int(e[k]) for k in ("off", "record", "pattern", "len", "out_off")) for e in entries]


def render(text, found, line_number=False, byte_offset=False):
    """what grep -o [-n] [-b] writes for the matches `found` = select(...) of a newline-terminated text"""
    newlines = [k for k, b in enumerate(text) if b == 0x0A]
    out = bytearray()
    for s, _, length in found:
        if line_number:
            out += b"%d:" % (bisect.bisect_left(newlines, s) + 1)
        if byte_offset:
            out += b"%d:" % s
        out += text[s:s + length] + b"\n"
    return bytes(out)
