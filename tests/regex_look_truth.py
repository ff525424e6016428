"""What a search for regular expressions WITH ASSERTIONS has to report, by Python's `re` on bytes under re.MULTILINE -- the
reference of every look-around test.  tests/regex_truth.py cannot serve: it bounds a match with `endpos`, which makes $ and \\b
true at the bound.

THE RULE: a start s (lo <= s < hi) is live if some expression matches t[s:e] for some s < e <= min(hi, s + span), its assertions
seeing the REAL neighbours t[s - 1] and t[e] (the text's two ends where there are none); its hit is the largest such e, and the
lowest-numbered expression that matches exactly t[s:e].  One hit a start.

A candidate t[s:e] holds iff (?:expr)(?=[\\s\\S]{k}\\Z) matches at s, k the bytes left to the true end (hits_plain).  Every
assertion sees one byte, so the same holds on a slice that keeps one byte in front of s and one byte behind the last end that is
tried, with k counted inside the slice: the slice's ends are true ends exactly where the text's are (hits)."""
import re

FOLD, DOTALL, NO_LDS = 1, 2, 4
ASSERT, WORD, LINE = 1, 2, 4
WORD_BYTES = b"[0-9A-Za-z_]"


def wrapped(expr, syntax=ASSERT):
    if syntax & WORD:
        return b"(?<!" + WORD_BYTES + b")(?:" + expr + b")(?!" + WORD_BYTES + b")"
    if syntax & LINE:
        return b"^(?:" + expr + b")$"
    return expr


def _flags(flags):
    return re.MULTILINE | (re.IGNORECASE if flags & FOLD else 0) | (re.DOTALL if flags & DOTALL else 0)


_cache = {}


def _left(expr, f, least, most):
    """`expr` with between `least` and `most` bytes left behind it up to the end of what is searched"""
    key = (expr, f, least, most)
    if key not in _cache:
        _cache[key] = re.compile(b"(?:" + expr + b")(?=[\\s\\S]{%d,%d}\\Z)" % (least, most), f)
    return _cache[key]


def hits(exprs, text, flags=0, span=256, syntax=ASSERT, lo=0, hi=None):
    """-> [(off, pattern, len)] ascending by off.  One slice a start, the longest end by bisection: "some match of at least k
    bytes that ends at or in front of the bound" is one call of the engine."""
    n = len(text)
    hi = n if hi is None else min(hi, n)
    f = _flags(flags)
    ws = [wrapped(e, syntax) for e in exprs]
    out = []
    for s in range(lo, hi):
        end = min(hi, s + span)
        s0 = max(s - 1, 0)
        piece = text[s0:min(end + 1, n)]
        at, tail = s - s0, (1 if end < n else 0)  # (the byte behind `end`, if there is one, is context only)
        room = len(piece) - at                     # bytes of the slice from s on
        if not any(_left(w, f, tail, room - 1).match(piece, at) for w in ws):
            continue
        a, b = 1, end - s  # a match of at least a bytes exists; none above b
        while a < b:
            k = (a + b + 1) // 2
            if any(_left(w, f, tail, room - k).match(piece, at) for w in ws):
                a = k
            else:
                b = k - 1
        who = [j for j, w in enumerate(ws) if _left(w, f, room - a, room - a).match(piece, at)]
        assert who and a >= 1
        out.append((s, who[0], a))
    return out


def hits_plain(exprs, text, flags=0, span=256, syntax=ASSERT, lo=0, hi=None):
    """the same by the definition on the whole text, one match an end: slow, kept to hold hits() to it"""
    n = len(text)
    hi = n if hi is None else min(hi, n)
    f = _flags(flags)
    ws = [wrapped(e, syntax) for e in exprs]
    out = []
    for s in range(lo, hi):
        for e in range(min(hi, s + span), s, -1):
            who = [j for j, w in enumerate(ws) if _left(w, f, n - e, n - e).match(text, s)]
            if who:
                out.append((s, who[0], e - s))
                break
    return out


def records_of(found, text, invert=False, delim=b"\n"):
    """-> the records of `text` in which a hit of `found` starts (or, inverted, none does), delimiters included"""
    live = {h[0] for h in found}
    out, start = [], 0
    while start < len(text):
        end = text.find(delim, start)
        end = len(text) if end < 0 else end + 1
        if any(s in live for s in range(start, end)) != invert:
            out.append(text[start:end])
        start = end
    return out


def records(exprs, text, flags=0, span=256, syntax=ASSERT, invert=False, delim=b"\n"):
    return records_of(hits(exprs, text, flags, span, syntax), text, invert, delim)
