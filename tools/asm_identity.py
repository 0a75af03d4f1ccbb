#!/usr/bin/env python3
"""Do two builds of one translation unit compile to the same kernels?  (no GPU)

  hipcc -O3 -std=c++17 --offload-arch=gfx950 [per-file flags of capi.build_library] --cuda-device-only -S -o old.s csrc/<file>.hip   (parent)
  ... the same on the branch -> new.s
  tools/asm_identity.py old.s new.s ['new demangled name=old demangled name' ...]

Per kernel of new.s (renamed through the table; the parameter list may be left out): IDENTICAL / DIFFERENT instruction stream -- comment lines,
assembler directives and symbol names dropped, basic-block labels renumbered in order of appearance -- and the resource counts of both.
Exit status 1 when a kernel differs, has no partner, or a kernel of old.s is left over.
"""
import re
import subprocess
import sys

KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    res = {}  # mangled name -> {key: value}, from the metadata note
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        blk = "  - .agpr_count" + blk
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        res[name] = {k: int(re.search(r"%s:\s+(\d+)" % re.escape(k), blk).group(1)) for k in KEYS}
    out = {}
    for name in res:
        body = text.split("\n%s:" % name, 1)[1].split("\n.Lfunc_end", 1)[0]
        labels, lines = {}, []
        for ln in body.splitlines():
            ln = ln.split(";", 1)[0].strip()
            if not ln or (ln.startswith(".") and not ln.startswith(".LBB")):
                continue
            ln = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), ln)
            lines.append(re.sub(r"_Z\w+", "SYM", ln))
        out[name] = (lines, res[name])
    demangled = subprocess.run(["c++filt"] + list(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^void ", "", d): out[m] for d, m in zip(demangled, out)}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    table = dict(a.split("=", 1) for a in sys.argv[3:])
    bad = 0
    for name, (lines, res) in new.items():
        short = name.split("(", 1)[0]
        want = table.get(name, table.get(short, name))
        partner = [k for k in old if k == want or k.split("(", 1)[0] == want]
        if len(partner) != 1:
            print("NO PARTNER  %s (looked for %s)" % (short, want))
            bad += 1
            continue
        olines, ores = old.pop(partner[0])
        same = lines == olines and res == ores
        bad += not same
        print("%s  %s <- %s  %d/%d lines  vgpr %d/%d agpr %d/%d sgpr %d/%d scratch %d/%d lds %d/%d" % (
            ("IDENTICAL" if same else "DIFFERENT"), short, partner[0].split("(", 1)[0], len(lines), len(olines),
            *[v for k in KEYS for v in (res[k], ores[k])]))
    for k in old:
        print("LEFT OVER   %s (in the old file only)" % k.split("(", 1)[0])
    sys.exit(1 if bad or old else 0)


if __name__ == "__main__":
    main()
