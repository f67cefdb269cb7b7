#!/usr/bin/env python3
"""List a kernel's memory instructions and s_waitcnt in program order, from gfx950 assembly.

The assembly comes from the kernels file compiled with the Makefile's flags plus
`--cuda-device-only -S` (and -DKPART=n to compile one launcher part only):

  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -DKPART=1 \\
        ffmpeg-hybrid_amd/csrc/vp9hip_kernels.hip -o k1.s
  tools/isa_mem.py k1.s 'k_lfIh3GeoILi1ELi1EE'            # every kernel whose symbol holds the text
  tools/isa_mem.py k1.s k_lf --wide --summary

Per kernel it prints one line per vector / flat / global memory instruction, scalar load, LDS
access group and s_waitcnt, with the line number of the listing, and collapses runs of equal LDS
accesses (`ds_write_b32 x4`). --wide keeps only accesses of 8 bytes and more plus the waits
between them (the tile chunks); --no-lds drops the LDS accesses and the waits that name no vmcnt.
--summary prints per-kernel counts: flat, global and scalar
accesses, and `vmcnt waits inside a run`: the s_waitcnt vmcnt(..) that stand between two wide
global / flat accesses of the same kind (load or store) with no barrier or LDS access between
them, which is how a serialised round trip shows.
No GPU is needed.
"""
import argparse
import re
import sys

MEM = re.compile(r"^\s+((?:flat|global|buffer|scratch)_\w+|s_load_\w+|s_buffer_load_\w+|ds_\w+|s_waitcnt\b.*|s_barrier)\b")
WIDE = re.compile(r"_(dwordx2|dwordx3|dwordx4|b64|b96|b128)\b")


def kernels(path):
    """symbol -> [(line number, text)] for every .amdhsa kernel body in the listing."""
    out, cur, name = {}, None, None
    for n, line in enumerate(open(path, errors="replace"), 1):
        m = re.match(r"^(_Z\w+):\s", line + " ")
        if m and "; @" in line:
            name, cur = m.group(1), []
            out[name] = cur
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end") or line.lstrip().startswith(".section"):
                cur = None
                continue
            cur.append((n, line.rstrip("\n")))
    return out


def events(body):
    ev = []
    for n, line in body:
        m = MEM.match(line)
        if not m:
            continue
        text = line.split(";")[0].strip()
        op = text.split()[0]
        if op == "s_waitcnt":
            ev.append((n, "wait", text))
        elif op == "s_barrier":
            ev.append((n, "barrier", text))
        elif op.startswith("ds_"):
            ev.append((n, "lds", op))
        elif op.startswith("s_"):
            ev.append((n, "sload", text))
        else:
            kind = "store" if "store" in op else "atomic" if "atomic" in op else "load"
            ev.append((n, kind, text))
    return ev


def summary(ev):
    c = {"flat": 0, "global": 0, "scalar loads": 0, "vmcnt waits": 0, "vmcnt waits inside a run": 0}
    last_kind, pending = None, 0        # pending: vmcnt waits seen since the last wide access of last_kind
    for n, kind, text in ev:
        op = text.split()[0]
        if kind in ("load", "store", "atomic"):
            c["flat" if op.startswith("flat") else "global"] += 1
            if kind != "atomic" and WIDE.search(op):
                if last_kind == kind:
                    c["vmcnt waits inside a run"] += pending
                last_kind, pending = kind, 0
        elif kind == "sload":
            c["scalar loads"] += 1
        elif kind == "wait":
            if "vmcnt" in text:
                c["vmcnt waits"] += 1
                pending += 1
        elif kind in ("lds", "barrier"):
            last_kind, pending = None, 0
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("match", help="text the kernel's (mangled) symbol must hold")
    ap.add_argument("--wide", action="store_true", help="only accesses of 8 bytes and more, and the waits")
    ap.add_argument("--no-lds", action="store_true", help="leave out LDS accesses and the waits that name no vmcnt")
    ap.add_argument("--summary", action="store_true", help="counts only")
    a = ap.parse_args()
    ks = {k: v for k, v in kernels(a.asm).items() if a.match in k}
    if not ks:
        sys.exit("no kernel symbol holds %r" % a.match)
    for name, body in ks.items():
        ev = events(body)
        print("== %s" % name)
        if not a.summary:
            run = None                  # [first line, op, count] of a run of equal LDS accesses
            def flush():
                nonlocal run
                if run:
                    print("%7d  %s%s" % (run[0], run[1], " x%d" % run[2] if run[2] > 1 else ""))
                run = None
            for n, kind, text in ev:
                if a.no_lds and (kind == "lds" or (kind == "wait" and "vmcnt" not in text)):
                    continue
                if kind == "lds":
                    if a.wide:
                        text = "ds_*"
                    if run and run[1] == text:
                        run[2] += 1
                    else:
                        flush()
                        run = [n, text, 1]
                    continue
                if a.wide and kind in ("load", "store") and not WIDE.search(text.split()[0]):
                    continue
                if a.wide and kind == "sload":
                    continue
                flush()
                print("%7d  %s" % (n, text))
            flush()
        for k, v in summary(ev).items():
            print("   %-26s %d" % (k, v))


if __name__ == "__main__":
    main()
