#!/usr/bin/env python3
"""Instruction classes of every loop of one kernel in a hipcc --save-temps .s file, over the loop's whole text
range (header label .. backward branch) and per basic block inside it, so that the count of each path through
the loop (k_pix5: waves 0..3, waves 4..7, the edge and interior copies) can be read off.

Usage: tools/isa_loop_paths.py file.s <kernel-substring> [min_loop_len]
valu counts every v_* instruction (f64, lane reads and v_mfma included; the last two are also given alone).
"""
import re
import sys
from collections import Counter

from isa_loops import classify


def stats(seg):
    c = Counter(classify(x.split()[0]) for x in seg)
    mf = sum(x.startswith("v_mfma") for x in seg)
    lg = sum(x.startswith("s_waitcnt") and "lgkmcnt" in x for x in seg)
    nop = sum(x.startswith("s_nop") for x in seg)
    return (f"n={len(seg):4d} valu={c['valu'] + c['valu64'] + c['lane']:3d} (f64 {c['valu64']}, mfma {mf}) ds={c['lds']:2d} "
            f"salu={c['salu']:2d} vmem={c['vmem']} wait={c['wait']:2d} (lgkmcnt {lg}) s_nop={nop} branch={c['branch']}")


def main():
    path, kname = sys.argv[1], sys.argv[2]
    minlen = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    lines = open(path).read().split("\n")
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and kname in l.split(":")[0]), None)
    if start is None:
        sys.exit("kernel not found")
    labpos, labat, ins = {}, {}, []
    for l in lines[start + 1:]:
        if ".Lfunc_end" in l:
            break
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            labpos[m.group(1)] = len(ins)
            labat[len(ins)] = m.group(1)
            continue
        s = l.strip()
        if s and not s.startswith((";", ".")):
            ins.append(s)
    for i, s in enumerate(ins):
        p = s.split()
        if not (p[0].startswith(("s_cbranch", "s_branch")) and p[1] in labpos and labpos[p[1]] <= i):
            continue
        a = labpos[p[1]]
        if i + 1 - a < minlen:
            continue
        print(f"loop {p[1]}: {stats(ins[a:i + 1])}")
        cuts = sorted({a, i + 1} | {k for k in labat if a < k <= i}
                      | {k + 1 for k in range(a, i) if ins[k].split()[0].startswith(("s_cbranch", "s_branch"))})
        for b0, b1 in zip(cuts, cuts[1:]):
            last = ins[b1 - 1].split()
            to = f" -> {last[0]} {last[1]}" if last[0].startswith(("s_cbranch", "s_branch")) else ""
            print(f"    {labat.get(b0, ''):12s} {stats(ins[b0:b1])}{to}")


if __name__ == "__main__":
    main()
