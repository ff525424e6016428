"""What a search for regular expressions has to report, by Python's `re` -- the reference of every regex test.

THE RULE: a start s (lo <= s < hi) is live if some expression matches a prefix of t[s : min(hi, s + span)]; its hit is the largest
end e with a full match of t[s:e], and the lowest-numbered expression that matches exactly t[s:e].  One hit a start."""
import re

FOLD, DOTALL, NO_LDS = 1, 2, 4


def compiled(exprs, flags=0):
    f = (re.IGNORECASE if flags & FOLD else 0) | (re.DOTALL if flags & DOTALL else 0)
    return [re.compile(b"(?:" + e + b")", f) for e in exprs]


_tail = {}


def _with_tail(expr, f, rest):
    """`expr` followed by at most `rest` bytes up to the end of the searched range"""
    key = (expr, f, rest)
    if key not in _tail:
        _tail[key] = re.compile(b"(?:" + expr + b")(?![\\s\\S]{%d})" % (rest + 1), f)
    return _tail[key]


def hits(exprs, text, flags=0, span=256, lo=0, hi=None):
    """-> [(off, pattern, len)] ascending by off.  The longest end is found by bisection: "some match of at least k bytes" is
    one call of the engine, which backtracks through every way to match until the bytes left behind it are few enough."""
    hi = len(text) if hi is None else min(hi, len(text))
    f = (re.IGNORECASE if flags & FOLD else 0) | (re.DOTALL if flags & DOTALL else 0)
    res = compiled(exprs, flags)
    out = []
    for s in range(lo, hi):
        end = min(hi, s + span)
        if not any(r.match(text, s, end) for r in res):
            continue
        a, b = 1, end - s  # a match of at least a bytes exists; none above b
        while a < b:
            k = (a + b + 1) // 2
            if any(_with_tail(e, f, end - s - k).match(text, s, end) for e in exprs):
                a = k
            else:
                b = k - 1
        who = [j for j, r in enumerate(res) if r.fullmatch(text, s, s + a)]
        assert who and a >= 1
        out.append((s, who[0], a))
    return out


def hits_plain(exprs, text, flags=0, span=256, lo=0, hi=None):
    """the same by the definition, one fullmatch an end: slow, kept to hold hits() to it"""
    hi = len(text) if hi is None else min(hi, len(text))
    res = compiled(exprs, flags)
    out = []
    for s in range(lo, hi):
        end = min(hi, s + span)
        if not any(r.match(text, s, end) for r in res):
            continue
        for e in range(end, s, -1):
            who = [j for j, r in enumerate(res) if r.fullmatch(text, s, e)]
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


def records(exprs, text, flags=0, span=256, invert=False, delim=b"\n"):
    return records_of(hits(exprs, text, flags, span), text, invert, delim)
