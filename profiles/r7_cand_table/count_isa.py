#!/usr/bin/env python3
"""Count the instructions of one kernel in a `hipcc -S` listing, block by block.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm -pragma-unroll-threshold=1000000 \
          --cuda-device-only -S nucleoatac_amd/csrc/natac_api.hip -o natac_api.s
    python profiles/r7_cand_table/count_isa.py natac_api.s 'natac_candidates_pairedILb1EE'

Prints the kernel's register / scratch / occupancy lines, then one line per basic block (label, instruction classes, and the
label a trailing backward branch returns to: such a block closes a loop).  The sweep's four-pair trip is the loop whose body holds
64 ds_read and 128 v_fma_f64 / v_mul_f64 of the bilinear form; everything else is "outside the loop".
"""
import re
import sys
from collections import Counter, OrderedDict


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if key in l and l.rstrip().split(";")[0].rstrip().endswith(":") and not l.startswith("\t"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("\t.amdhsa_kernel") or ".Lfunc_end" in lines[i] and lines[i].endswith(":"))
    blocks = OrderedDict()
    cur = "entry"
    blocks[cur] = []
    for l in lines[start + 1:end]:
        s = l.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", s)
            if m:
                cur = m.group(1)
                blocks[cur] = []
            continue
        blocks[cur].append(s)
    for l in lines[end:]:
        if re.search(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy|SGPRBlocks|NumSgprs|LDSByteSize|codeLenInByte)", l):
            print(l.strip())
        if l.startswith("\t.section") and ".text" in l and key not in l:
            break
    order = list(blocks)
    total = Counter()
    print("%-12s %6s %6s %6s %6s %6s %6s %6s  %s" % ("block", "valu", "lds", "vmem", "smem", "salu", "wait", "all", "notes"))
    for name, ins in blocks.items():
        c = Counter(classify(i.split()[0]) for i in ins)
        ops = Counter(i.split()[0] for i in ins)
        total.update(c)
        note = ""
        for i in ins:
            m = re.match(r"s_cbranch\S*\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", i)
            if m:
                tgt = m.group(1) or m.group(2)
                if tgt in order and order.index(tgt) <= order.index(name):
                    note += " loop->" + tgt
        f64 = sum(v for k, v in ops.items() if k in ("v_fma_f64", "v_mul_f64", "v_add_f64", "v_pk_fma_f64"))
        if f64:
            note += " fp64=%d" % f64
        print("%-12s %6d %6d %6d %6d %6d %6d %6d %s" % (name, c["valu"], c["lds"], c["vmem"], c["smem"], c["salu"], c["wait"], len(ins), note))
        if "-v" in sys.argv and "loop->" in note:
            for k, v in sorted(ops.items(), key=lambda kv: -kv[1]):
                print("      %-28s %d" % (k, v))
    print("%-12s %6d %6d %6d %6d %6d %6d %6d" % ("total", total["valu"], total["lds"], total["vmem"], total["smem"], total["salu"], total["wait"], sum(total.values())))


if __name__ == "__main__":
    main()
