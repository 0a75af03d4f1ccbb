"""diagnostic (no GPU): vector loads of a kernel that sit exposed on a dependent chain, from the compiler's own assembly
   (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S [-mllvm -amdgpu-sched-strategy=max-ilp] file.hip -o file.s):
   python tools/asm_exposed_loads.py file.s '<kernel symbol or a substring of it>' [-n N] [--from LINE] [--to LINE] [--counts]

Two lists per kernel:
  EXPOSED  every global_load / flat_load whose first covering `s_waitcnt vmcnt(k)` follows within N instructions (default 8): nothing
           of note is issued between the request and the wait, so the wavefront sits out the whole memory round trip.  A wait covers
           a load when at most k vector-memory operations were issued behind the load (gfx9 counts loads and stores in one counter
           and returns loads in order).  The scan follows the text: labels are walked through, a conditional branch is walked past
           (fall-through side), an unconditional branch or s_endpgm ends it.
  UNIFORM  every vector load off a scalar base whose vector offset is lane-invariant (the offset register was last written, walking
           the text backwards, by a v_mov_b32 of an immediate or a scalar register): a batch-uniform word fetched through the vector
           memory path -- behind a fence or an LDS store the compiler can no longer prove the block unclobbered and does not use
           a scalar load.  Loads with a per-lane address (state, goals, per-joint constants) never show up here.
A load can be in both lists.  Each line: line number in the .s file, the last label in front of it, the instruction, and for EXPOSED the
number of instructions up to the wait and the wait itself.  Exit status 0 always: the lists are read by a person."""
import argparse
import re
import sys

VMEM = ("global_", "flat_", "buffer_", "scratch_")
LOAD = re.compile(r"^(global|flat)_load_")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


def kernel_symbols(lines):
    return [m.group(1) for l in lines for m in [re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", l)] if m and not l.startswith(".L")]


def body(lines, name):
    syms = [s for s in kernel_symbols(lines) if name in s]
    exact = [s for s in syms if s == name]
    syms = exact or syms
    if len(syms) != 1:
        sys.exit(f"'{name}' matches {len(syms)} symbols: {syms[:8]}")
    start = next(i for i, l in enumerate(lines) if l.startswith(syms[0] + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".size") and syms[0] in lines[i])
    return syms[0], start, end


def instructions(lines, start, end):
    """(line number, label in front, text) of every instruction; labels and unconditional ends are kept as markers"""
    out, label = [], ""
    for i in range(start + 1, end):
        l = lines[i].split(";")[0].strip()
        if not l or l.startswith("."):
            if l.endswith(":"):
                label = l[:-1]
            continue
        if l.endswith(":"):
            label = l[:-1]
            continue
        out.append((i + 1, label, l))
    return out


def wait_covers(text, behind):
    """does this s_waitcnt cover a load with `behind` vector-memory operations issued after it"""
    if not text.startswith("s_waitcnt"):
        return False
    m = VMCNT.search(text)
    if m:
        return int(m.group(1)) <= behind
    return bool(re.match(r"s_waitcnt\s+(0|0x0)\s*$", text))  # the bare all-counters form


def regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return [int(m.group(1))] if m else []


def writes(text, reg):
    parts = text.replace(",", " ").split()
    if len(parts) < 2 or not parts[0].startswith(("v_", "ds_read", "global_load", "flat_load", "buffer_load", "scratch_load")):
        return False
    return reg in regs(parts[1])


def invariant(ins, k, reg):
    """the immediate or scalar register VGPR `reg`, read by instruction k, was last written from by a plain move; None: anything else"""
    for j in range(k - 1, -1, -1):
        t = ins[j][2]
        if writes(t, reg):
            p = t.replace(",", " ").split()
            return p[2] if p[0] == "v_mov_b32_e32" and len(p) == 3 and not p[2].startswith("v") else None
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("-n", type=int, default=8)
    ap.add_argument("--from", dest="lo", type=int, default=0, help="only loads at or behind this line of the .s file")
    ap.add_argument("--to", dest="hi", type=int, default=1 << 30, help="only loads in front of this line")
    ap.add_argument("--counts", action="store_true", help="the three counts only, not the lists")
    a = ap.parse_args()
    lines = open(a.asm).read().split("\n")
    sym, start, end = body(lines, a.kernel)
    ins = instructions(lines, start, end)
    exposed, uniform, nload = [], [], 0
    for k, (ln, label, t) in enumerate(ins):
        if not LOAD.match(t) or not (a.lo <= ln < a.hi):
            continue
        nload += 1
        behind = 0
        for d in range(1, a.n + 1):
            if k + d >= len(ins):
                break
            u = ins[k + d][2]
            if wait_covers(u, behind):
                exposed.append((ln, label, t, d, u))
                break
            if u.startswith(VMEM):
                behind += 1
            if u.startswith(("s_branch", "s_endpgm", "s_setpc")):
                break
        p = t.replace(",", " ").split()
        if len(p) >= 4 and re.match(r"s\[\d+:\d+\]$", p[3]):  # global_load vdst, voffset, s[base:base+1]
            src = [invariant(ins, k, r) for r in regs(p[2])]
            if all(v is not None for v in src):
                uniform.append((ln, label, t, "voffset = " + src[0]))
        elif len(p) >= 3 and regs(p[2]):  # address pair built from scalars
            src = [invariant(ins, k, r) for r in regs(p[2])]
            if all(v is not None for v in src):
                uniform.append((ln, label, t, "address = " + ":".join(src)))
    if a.counts:
        print(f"{sym}: {nload} global / flat loads, EXPOSED {len(exposed)}, UNIFORM {len(uniform)}")
        return
    print(f"{sym}: {nload} global / flat loads in lines {max(a.lo, start + 1)}..{min(a.hi, end)}")
    print(f"EXPOSED (covering wait within {a.n} instructions): {len(exposed)}")
    for ln, label, t, d, u in exposed:
        print(f"  {ln:7d} {label:14s} {t:60s} +{d} {u}")
    print(f"UNIFORM (scalar base, lane-invariant offset): {len(uniform)}")
    for ln, label, t, src in uniform:
        print(f"  {ln:7d} {label:14s} {t:60s} {src}")


if __name__ == "__main__":
    main()
