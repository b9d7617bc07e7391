"""Winograd weight-gradient GEMM launches of the LAST training step in a
rocprofv3 kernel trace, split into single-owner launches (one m-split of a
plain grid: every output tile has one writer) and accumulating ones, with the
zero-fills and inverse transforms of the same step.

A Winograd point GEMM is batched over the 144 points of F(4x2x4), so its grid
carries splits * 144 workgroups along z (x3_wgrad_tr_kernel<0, false>,
x3_wgrad_kernel, conv_wgrad_kernel) or tiles * splits * 144 along x
(x3_wgrad64_kernel: 64 -> 64 layers, one tile); the unbatched 1x1x1 / direct
weight gradients never reach a multiple of 144 there (their split counts are
powers of two or capped by 1024 / tiles).  The stream-K form
(x3_wgrad_tr_kernel<0, true>) always accumulates.
Usage: wgrad_owner_table.py run_kernel_trace.csv[.gz]"""
import csv
import gzip
import sys

POINTS = 144

f = sys.argv[1]
rows = list(csv.DictReader(gzip.open(f, "rt") if f.endswith(".gz") else open(f)))
ends = [int(r["End_Timestamp"]) for r in rows if "sgd_update_kernel" in r["Kernel_Name"]]
lo, hi = ends[-2], ends[-1]
sel = sorted((r for r in rows if int(r["Start_Timestamp"]) >= lo and int(r["End_Timestamp"]) <= hi),
             key=lambda r: int(r["Start_Timestamp"]))


def blocks(r):
    return tuple(int(r[f"Grid_Size_{a}"]) // max(int(r[f"Workgroup_Size_{a}"]), 1) for a in "XYZ")


def short(r):
    return r["Kernel_Name"].split("(")[0].replace("void ", "").replace("m3d::", "")


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


single, accum, other = [], [], {}
for r in sel:
    n, g = short(r), blocks(r)
    if n.startswith("x3_wgrad_tr_kernel<0, true>"):
        accum.append((n, g, us(r), "stream-K"))
    elif n.startswith(("x3_wgrad_tr_kernel", "x3_wgrad_kernel", "conv_wgrad_kernel")):
        if g[2] % POINTS == 0:
            s = g[2] // POINTS
            (single if s == 1 else accum).append((n, g, us(r), f"splits {s}"))
        else:
            other[n] = other.get(n, 0) + 1
    elif n.startswith("x3_wgrad64_kernel"):
        if g[0] % POINTS == 0:
            s = g[0] // POINTS
            (single if s == 1 else accum).append((n, g, us(r), f"tiles x splits {s}"))
        else:
            other[n] = other.get(n, 0) + 1

print(f"step window {(hi - lo) / 1e6:.2f} ms, {len(sel)} dispatches")
for title, ls in (("single-owner Winograd weight-gradient GEMMs", single),
                  ("accumulating Winograd weight-gradient GEMMs", accum)):
    print(f"--- {title}: n = {len(ls)}, {sum(l[2] for l in ls) / 1e3:.3f} ms")
    for n, g, d, how in ls:
        print(f"{d:9.1f} us  {'x'.join(map(str, g)):>14s}  {how:<18s} {n[:60]}")
for key in ("fillBufferAligned", "wino_wgrad_out_kernel", "wino_grad_kernel"):
    ls = [us(r) for r in sel if key in r["Kernel_Name"]]
    print(f"--- {key}: n = {len(ls)}, {sum(ls) / 1e3:.3f} ms")
print("--- weight-gradient launches that are no Winograd point GEMM (not counted): "
      + ", ".join(f"{k[:40]} x{v}" for k, v in sorted(other.items())))
