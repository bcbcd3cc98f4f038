#!/usr/bin/env python3
"""Instruction counts of k_lk_iter's rolled row loops, and the resources of the LK kernels, from the
gfx950 assembly of mdx_lk.hip (the Makefile's flags plus --cuda-device-only -S).

Usage: python3 scripts/lk_rowloop_count.py mdx_lk.s [G UW DF ...]   (default: 4 56 1  8 112 1)

A row loop is an innermost loop (the compiler's "Inner Loop Header" / "in Loop: Header=" block
annotations) that holds LDS-DMA loads (buffer_load ... lds).  Counts are per ROW: the loop's
instructions divided by the rows it holds (its LDS-DMA loads / 3).  The fused body is told from the
exact one by its v_pk_fma_f32.  Resources come from the code object metadata at the end of the file.
"""
import re
import sys

CLASSES = ("VALU", "LDS", "LDS-DMA", "SALU", "branch", "s_nop", "s_waitcnt")


def functions(lines):
    name, start = None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN3mdx\w+):", l)
        if m:
            name, start = m.group(1), i
        elif l.startswith(".Lfunc_end") and name:
            yield name, lines[start:i]
            name = None


def klass(op, line):
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("buffer_") or op.startswith("global_") or op.startswith("flat_"):
        return "LDS-DMA" if line.rstrip().endswith(" lds") else "VMEM"
    if op.startswith("v_"):
        return "VALU"
    return "other"


def inner_loops(body):
    """{header label: [instruction lines]} of the innermost loops"""
    loops, cur = {}, None
    for i, l in enumerate(body):   # the headers first: a loop's blocks may be laid out ahead of its header
        if "This Inner Loop Header" in l:
            j = i
            while j >= 0 and not re.match(r"^\.LBB\d+_\d+:", body[j]):
                j -= 1
            if j >= 0:
                loops[body[j].split(":")[0]] = []
    i = 0
    while i < len(body):
        l = body[i]
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", l) or re.match(r"^(; %bb\.\d+):(.*)", l)
        if m:
            note = m.group(2)
            # a header's annotation may continue on the following comment-only lines
            j = i + 1
            while j < len(body) and re.match(r"^\s+; ", body[j]) and "Loop" in body[j]:
                note += body[j]
                j += 1
            if "This Inner Loop Header" in note:
                cur = m.group(1)
            else:
                h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
                cur = ".L" + h.group(1) if h and ".L" + h.group(1) in loops else None
        elif cur is not None:
            s = l.strip()
            mm = re.match(r"^([a-z_0-9]+)", s)
            if mm and not s.startswith((";", ".")):
                loops[cur].append(s)
        i += 1
    return loops


def main():
    lines = open(sys.argv[1]).read().split("\n")
    want = [int(x) for x in sys.argv[2:]] or [4, 56, 1, 8, 112, 1]
    shapes = [tuple(want[i:i + 3]) for i in range(0, len(want), 3)]
    for name, body in functions(lines):
        m = re.match(r"_ZN3mdx9k_lk_iterILi(\d+)ELi(\d+)ELb([01])E", name)
        if not m or tuple(int(x) for x in m.groups()) not in shapes:
            continue
        print("k_lk_iter<%s, %s, %s>" % (m.group(1), m.group(2), "true" if m.group(3) == "1" else "false"))
        for ins in inner_loops(body).values():
            c = {}
            for s in ins:
                k = klass(s.split()[0], s)
                c[k] = c.get(k, 0) + 1
            if not c.get("LDS-DMA"):
                continue
            rows = c["LDS-DMA"] / 3.0
            fused = any(s.startswith("v_pk_fma_f32") for s in ins)
            nonvec = sum(c.get(k, 0) for k in ("SALU", "branch", "s_nop", "s_waitcnt"))
            print("  %s body, %g rows per trip, per row: " % ("fused" if fused else "exact", rows) +
                  "  ".join("%s %g" % (k, c.get(k, 0) / rows) for k in CLASSES) +
                  "  | non-vector %g" % (nonvec / rows))
    print("resources: VGPRs, SGPRs, spilled SGPRs (to VGPR lanes) / VGPRs, scratch B, LDS B, waves per SIMD (by VGPRs and LDS)")
    text = "\n".join(lines)
    meta = text[text.find("amdhsa.kernels:"):]
    for ent in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        def f(key):
            mm = re.search(r"\n    \.%s:\s+(\S+)" % key, ent)
            return mm.group(1) if mm else "?"
        name = f("name")
        mm = re.match(r"_ZN3mdx\d+(k_lk_iter|k_lk_A_rows|k_lk_A)I((?:L[ib]\d+E)+)E", name)
        if not mm:
            continue
        targs = re.findall(r"L([ib])(\d+)E", mm.group(2))
        targs = ", ".join(("true" if v == "1" else "false") if t == "b" else v for t, v in targs)
        vg = int(f("vgpr_count"))
        lds = int(f("group_segment_fixed_size"))
        occ = min(8, 512 // (((vg + 7) // 8) * 8)) if vg else 8     # 512 VGPRs per lane and SIMD, blocks of 8
        if lds:
            occ = min(occ, (160 * 1024 // lds) // 4)                # one-wave workgroups, 160 KB per CU, 4 SIMDs
        print("  %-30s v%-4s s%-4s spills %s/%s  scratch %s  lds %s  waves %d" % (
            "%s<%s>" % (mm.group(1), targs), vg, f("sgpr_count"), f("sgpr_spill_count"), f("vgpr_spill_count"),
            f("private_segment_fixed_size"), f("group_segment_fixed_size"), occ))


if __name__ == "__main__":
    main()
