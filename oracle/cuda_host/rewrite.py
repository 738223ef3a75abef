#!/usr/bin/env python3
"""Rewrite the kernel launches of a CUDA C file for the host execution layer (cuda_host.h).

    rewrite.py IN.cu OUT.cpp

Every `kernel<<<grid, block>>>(args);` becomes
`cuda_host::launch(grid, block, HAS_BARRIER, [&]{ kernel(args); });`, where HAS_BARRIER says
whether a __global__ function of that name calls __syncthreads().  The file is handled as bytes
(its comments need not be UTF-8).  A `//` comment whose last byte is a backslash would splice
the next line into the comment for a byte-oriented compiler; such lines get a full stop.
Nothing else changes, and the output is a build product: it is written next to the other
reference binaries and never committed.
"""
import re
import sys

LAUNCH = re.compile(
    r"([A-Za-z_]\w*)(\s*<[\w\s,]+>)?\s*<<<\s*([^,<>]+?)\s*,\s*([^<>]+?)\s*>>>\s*\((.*?)\)\s*;", re.S)
KERNEL = re.compile(r"__global__\s+(?:void\s+)?([A-Za-z_]\w*)\s*\(")


def rewrite(text):
    lines = text.split("\n")
    spliced = 0
    for i, line in enumerate(lines):
        body = line.rstrip("\r")
        if body.endswith("\\") and "//" in body:
            lines[i] = body + " ."
            spliced += 1
    text = "\n".join(lines)

    barrier = {}
    heads = list(KERNEL.finditer(text))
    for k, m in enumerate(heads):
        end = heads[k + 1].start() if k + 1 < len(heads) else len(text)
        barrier[m.group(1)] = barrier.get(m.group(1), False) or "__syncthreads" in text[m.end():end]

    launches = []

    def sub(m):
        name, targs, grid, block, args = m.group(1), m.group(2) or "", m.group(3), m.group(4), m.group(5)
        if name not in barrier:
            raise SystemExit("rewrite.py: launch of an unknown kernel %r" % name)
        launches.append(name)
        return "cuda_host::launch(%s, %s, %s, [&]{ %s%s(%s); });" % (
            grid, block, "true" if barrier[name] else "false", name, targs.strip(), args)

    text = LAUNCH.sub(sub, text)
    if "<<<" in text:
        raise SystemExit("rewrite.py: a launch was not rewritten")
    return text, launches, barrier, spliced


def main(argv):
    src, dst = argv[1], argv[2]
    with open(src, "rb") as f:
        text = f.read().decode("latin-1")
    text, launches, barrier, spliced = rewrite(text)
    with open(dst, "wb") as f:
        f.write(text.encode("latin-1"))
    print("rewrite.py: %d launches of %d kernels (%s with a barrier), %d comment lines closed" % (
        len(launches), len(barrier), ", ".join(sorted(k for k, v in barrier.items() if v)), spliced))


if __name__ == "__main__":
    main(sys.argv)
