#!/usr/bin/env python3
"""Per instantiation of the residual kernels (k_resid, k_resid_dev, k_resid_multi): mean per
launch of each PMC counter and of the kernel-trace duration in tools/profile.sh output.
Usage: resid_pmc.py DIR   (the prof_TAG directory that tools/profile.sh TAG wrote)"""
import csv
import glob
import os
import sys
from collections import defaultdict


def inst(name):
    """"void k_resid_dev<8, 1, unsigned char, M32, short>(RJob const*, ...)" without "void" and arguments."""
    n = name.strip()
    if n.startswith("void "):
        n = n[5:]
    return n.split("(")[0].strip()


def main(d):
    acc = defaultdict(lambda: defaultdict(list))
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            acc[inst(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            acc[inst(r["Kernel_Name"])]["duration_us"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, cs in sorted(acc.items()):
        if not k.startswith("k_resid"):
            continue
        print(k)
        for c, v in sorted(cs.items()):
            print("  %-24s n=%-5d mean=%.4g total=%.4g" % (c, len(v), sum(v) / len(v), sum(v)))


if __name__ == "__main__":
    main(sys.argv[1])
