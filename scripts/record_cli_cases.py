#!/usr/bin/env python3
"""Record tests/golden/cli_grammar.json: what a given `bnzhip` answers to every argv of tests/cli_cases.py.

    python scripts/record_cli_cases.py <path/to/bnzhip> [out.json]

Run it against a build of the commit BEFORE a change to the CLI, never against the code under test, and on a machine
without a GPU: a case that exits with anything but 0, 1 or 2 there has reached the device and does not belong in the table."""
import json
import os
import pathlib
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cli_cases  # noqa: E402


def record(binary):
    with tempfile.TemporaryDirectory() as top:
        def one(k):
            d = pathlib.Path(top, str(k))
            d.mkdir()
            return cli_cases.run_case(binary, cli_cases.CASES[k], d)
        with ThreadPoolExecutor(8) as pool:
            got = list(pool.map(one, range(len(cli_cases.CASES))))
    out, bad = {}, []
    for argv, res in zip(cli_cases.CASES, got):
        key = cli_cases.label(argv)
        assert key not in out, "two cases with the label %r" % key
        out[key] = res
        if res["status"] not in (0, 1, 2):
            bad.append((key, res["status"], res["stderr"]))
    return out, bad


if __name__ == "__main__":
    binary = os.path.abspath(sys.argv[1])
    dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "cli_grammar.json")
    out, bad = record(binary)
    for key, status, err in bad:
        print("exit %d, reaches the device, take it out: %s\n    %s" % (status, key, err.strip()), file=sys.stderr)
    if bad:
        sys.exit(1)
    with open(dest, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(out), dest))
