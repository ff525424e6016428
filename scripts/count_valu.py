#!/usr/bin/env python3
"""Static vector-ALU and LDS instruction counts of compiled kernels: per kernel, per loop and per marked part of the source.

    hipcc <the Makefile's flags> --cuda-device-only -S -gline-tables-only -Rpass-analysis=kernel-resource-usage \
          mtf.hip -o mtf.s 2> mtf.remarks
    scripts/count_valu.py mtf.s [--kernel mtf_walk_par] [--source mtf.hip] [--remarks mtf.remarks]

An instruction is a line of the device assembly whose mnemonic begins `v_` (vector ALU, what a kernel bound by instruction
issue pays for) or `ds_` (LDS); nothing else is told apart and no instruction is named.

Loops are the compiler's own: every basic block of the listing carries a comment that names the header of the innermost
loop around it (`=>This Loop Header`, `in Loop: Header=BBn_m Depth=d`, `Parent Loop BBn_m`), and a block without a label is
announced by `; %bb.N:`.  A loop's `own` figures are the blocks whose innermost loop it is, `total` adds the loops nested
in it.

Parts: with --source, comment lines `// part: NAME` in that file cut it into parts (`// part: -` ends the last one), and
every instruction goes to the part of the source line the compiler's line table (-gline-tables-only: `.loc`) gives it -- so
a block that the compiler lays out elsewhere, or an instruction the scheduler moves, stays with the code it came from.  An
instruction from an inlined helper (a line outside every part, or of another file) goes to the part of the last
instruction before it that had one.  The line table changes no instruction: the totals are those of the build without it.
"""
import argparse
import collections
import os
import re
import sys

FUNC = re.compile(r"^([A-Za-z_][\w$.]*):\s*; @")
END = re.compile(r"^\.Lfunc_end")
LABEL = re.compile(r"^(?:\.L(BB\d+_\d+)|; %bb\.(\d+)):(.*)$")
CONT = re.compile(r"^\s+;(.*)$")
HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
INLOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
FILE = re.compile(r'^\s+\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"')
LOC = re.compile(r"^\s+\.loc\s+(\d+)\s+(\d+)")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
MARK = re.compile(r"^\s*// part: (\S+)")


def kind(mnemonic):
    if mnemonic.startswith("v_"):
        return "v"
    if mnemonic.startswith("ds_"):
        return "ds"
    return None


def source_parts(path):
    """-> [(first line, name or None)] in line order"""
    marks = []
    for no, line in enumerate(open(path), 1):
        m = MARK.match(line)
        if m:
            marks.append((no, None if m.group(1) == "-" else m.group(1)))
    return marks


def part_of(marks, line):
    name = None
    for first, n in marks:
        if first > line:
            break
        name = n
    return name


def parse(lines, source, marks):
    """-> {kernel: dict(total=Counter, loops={header: dict(depth, parent, own=Counter)}, parts={(loop, part): Counter})}"""
    kernels = collections.OrderedDict()
    files = {}
    cur = None
    i = 0
    while i < len(lines):
        line = lines[i]
        m = FILE.match(line)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3))
            i += 1
            continue
        m = FUNC.match(line)
        if m:
            cur = dict(total=collections.Counter(), loops=collections.OrderedDict(), parts=collections.OrderedDict(), loop=None, part=None)
            kernels[m.group(1)] = cur
            i += 1
            continue
        if cur is None:
            i += 1
            continue
        if END.match(line):
            cur = None
            i += 1
            continue
        m = LOC.match(line)
        if m:
            if source and files.get(int(m.group(1))) == source:
                p = part_of(marks, int(m.group(2)))
                if p:
                    cur["part"] = p
            i += 1
            continue
        m = LABEL.match(line)
        if m:
            # the block's comment may run on over the following lines
            text = m.group(3)
            while i + 1 < len(lines) and CONT.match(lines[i + 1]):
                i += 1
                text += lines[i]
            name = m.group(1)
            h = HEADER.search(text)
            if h and name:
                parents = PARENT.findall(text)
                parent = max(parents, key=lambda p: int(p[1]))[0] if parents else None
                cur["loops"].setdefault(name, dict(depth=int(h.group(1)), parent=None, own=collections.Counter()))["parent"] = parent
                cur["loop"] = name
            else:
                il = INLOOP.search(text)
                cur["loop"] = il.group(1) if il else None
                if il and il.group(1) not in cur["loops"]:  # (a block laid out in front of its header)
                    cur["loops"][il.group(1)] = dict(depth=int(il.group(2)), parent=None, own=collections.Counter())
            i += 1
            continue
        m = INSN.match(line)
        if m:
            k = kind(m.group(1))
            if k:
                cur["total"][k] += 1
                if cur["loop"]:
                    cur["loops"][cur["loop"]]["own"][k] += 1
                if cur["part"] and cur["loop"]:
                    cur["parts"].setdefault((cur["loop"], cur["part"]), collections.Counter())[k] += 1
        i += 1
    return kernels


def totals(loops):
    tot = {h: collections.Counter(l["own"]) for h, l in loops.items()}
    for h in sorted(loops, key=lambda h: -loops[h]["depth"]):
        p = loops[h]["parent"]
        if p in tot:
            tot[p].update(tot[h])
    return tot


def resources(path, want):
    """the VGPR / scratch / LDS figures of -Rpass-analysis=kernel-resource-usage, per kernel"""
    out, name = collections.OrderedDict(), None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            out[name] = []
        elif name is not None:
            out[name].append("%s %s" % (m.group(1), m.group(2)))
    return {k: v for k, v in out.items() if want in k}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="", help="only kernels whose (mangled) name contains this")
    ap.add_argument("--source", help="the source file whose `// part: NAME` comments cut the kernels into parts")
    ap.add_argument("--remarks", help="the compiler's stderr of the same build: prints the resource line of every kernel listed")
    a = ap.parse_args()
    marks = source_parts(a.source) if a.source else []
    kernels = parse(open(a.asm).read().splitlines(), os.path.basename(a.source) if a.source else None, marks)
    for name, k in kernels.items():
        if a.kernel not in name:
            continue
        print("%s: v_ %d, ds_ %d" % (name, k["total"]["v"], k["total"]["ds"]))
        tot = totals(k["loops"])
        depth = {h: l["depth"] for h, l in k["loops"].items()}
        for h, l in k["loops"].items():
            print("  %sloop %-10s depth %d  own v_ %4d ds_ %3d   total v_ %4d ds_ %3d" %
                  ("  " * (l["depth"] - 1), h, l["depth"], l["own"]["v"], l["own"]["ds"], tot[h]["v"], tot[h]["ds"]))
        if k["parts"]:
            print("  parts of %s (by the line table), per innermost loop:" % a.source)
            byname = collections.OrderedDict()
            for (loop, part), c in sorted(k["parts"].items(), key=lambda kv: [n for _, n in marks].index(kv[0][1])):
                if depth.get(loop, 0) >= 2:
                    byname.setdefault(part, collections.Counter()).update(c)
                print("    %-28s in %-10s v_ %4d ds_ %3d" % (part, loop, c["v"], c["ds"]))
            print("  parts, summed over the loops of depth 2 and more:")
            for part, c in byname.items():
                print("    %-28s v_ %4d ds_ %3d" % (part, c["v"], c["ds"]))
    if a.remarks:
        for name, rows in resources(a.remarks, a.kernel).items():
            print("%s: %s" % (name, ", ".join(rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
