#!/usr/bin/env python3
"""Static instruction counts of one kernel in a `hipcc -S` listing, and of its loader loop.

    python3 tools/isa_count.py LISTING.s KERNEL_SUBSTRING [MARKER_REGEX]

Counts VALU, SALU, VMEM, LDS and lane-move (v_readlane / v_writelane: SGPR spill traffic through
VGPR lanes) instructions of the first kernel whose symbol contains KERNEL_SUBSTRING.  The loader
loop is the largest loop (a backward branch and its target label) that contains an instruction
matching MARKER_REGEX (default: a non-temporal global load, the cached kernel's stream loads) and
no buffer load (the probers' record loads); every candidate loop is listed."""
import re
import sys


def classify(op):
    if op.startswith(("v_readlane", "v_writelane")):
        return "lane"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return None


def count(lines):
    c = {"valu": 0, "salu": 0, "vmem": 0, "lds": 0, "lane": 0}
    for ln in lines:
        k = classify(ln.split()[0]) if ln.split() else None
        if k:
            c[k] += 1
    c["valu"] += c["lane"]   # lane moves are VALU instructions; "lane" is the part of them
    return c


def main():
    path, sub = sys.argv[1], sys.argv[2]
    marker = re.compile(sys.argv[3] if len(sys.argv) > 3 else r"^global_load\S*\s.*\bnt\b")
    text = open(path).read().split("\n")
    start = next(i for i, l in enumerate(text) if re.match(r"^\S+:", l) and sub in l and not l.startswith("."))
    end = next(i for i in range(start, len(text)) if text[i].strip().startswith("s_endpgm"))
    body = [l.strip() for l in text[start:end + 1]]
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\S+):", l))}
    print(text[start].rstrip(":"))
    print("  whole kernel:", count([l for l in body if not l.endswith(":")]))
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"^s_c?branch\S*\s+(\.LBB\S+)", l)
        if m and labels.get(m.group(1), 1 << 30) < i:
            seg = body[labels[m.group(1)]:i + 1]
            if any(marker.search(x) for x in seg) and not any(x.startswith("buffer_load") for x in seg):
                loops.append((len(seg), m.group(1), seg))
    for n, lab, seg in sorted(loops, key=lambda t: -t[0]):
        print(f"  loop {lab} ({n} lines):", count(seg))
    if loops:
        n, lab, seg = max(loops, key=lambda t: t[0])
        first = next(j for j, x in enumerate(seg) if marker.search(x))
        print(f"  loader loop = {lab}; from its first stream load to the back-edge:", count(seg[first:]))


if __name__ == "__main__":
    main()
