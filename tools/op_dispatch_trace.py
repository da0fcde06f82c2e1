#!/usr/bin/env python3
"""The dispatches of the Lorentz operator and tracer launchers, for comparing two builds of libswmhd.so (SWMHD_LIBRARY).

    rocprofv3 --kernel-trace --stats -d DIR -o ops --output-format csv -- python tools/op_dispatch_trace.py
    python tools/op_dispatch_trace.py --summarize DIR --out sequence.json

The first form makes a fixed list of calls through swmhd_amd.operators -- the cases of the operator sections of
tests/launch_plan_check.cpp that the Python layer can reach (no caller's edge_cols, no 1.6 M-row grid), fp64 unless stated -- then one
step (three tracer stages) of a 65 x 17 model with three tracers and of a three-member ensemble of it.  The second form reads the kernel
trace and writes the library's own kernels (k_*) as the sequence of (kernel, grid, workgroup) in dispatch order."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, B = "Periodic", "Bounded"
# (form, Nx, Ny, (topology x, y), rows, kernel, strict, dtype)
CALLS = [
    ("jacobian", 4096, 4096, (P, P), None, "auto", False, "f64"),
    ("divergence", 4096, 4096, (P, P), None, "auto", False, "f64"),
    ("jacobian", 16384, 2048, (P, P), None, "auto", False, "f64"),
    ("divergence", 16384, 2048, (P, P), None, "auto", False, "f64"),
    ("jacobian", 1415, 1414, (P, P), None, "auto", False, "f64"),
    ("jacobian", 1414, 1414, (P, P), None, "auto", False, "f64"),
    ("divergence", 1300, 800, (B, B), None, "auto", False, "f64"),
    ("divergence", 1300, 800, (P, B), None, "auto", False, "f64"),
    ("divergence", 1300, 800, (B, P), None, "auto", False, "f64"),
    ("divergence", 1284, 800, (B, B), (5, 790), "auto", False, "f64"),
    ("divergence", 1284, 800, (B, B), (5, 790), "auto", False, "f32"),
    ("divergence", 18752, 48, (B, B), None, "auto", False, "f64"),
    ("divergence", 18751, 48, (B, B), None, "auto", False, "f64"),
    ("divergence", 18750, 48, (B, B), None, "auto", False, "f64"),
    ("divergence", 18749, 48, (B, B), None, "auto", False, "f64"),
    ("divergence", 18752, 47, (B, B), None, "auto", False, "f64"),
    ("divergence", 255, 4096, (B, B), None, "auto", False, "f64"),
    ("divergence", 1300, 800, (B, B), None, "tile", False, "f64"),
    ("divergence", 1300, 800, (B, B), None, "march", False, "f64"),
    ("divergence", 1300, 800, (B, B), None, "auto", True, "f64"),
    ("divergence", 4096, 4096, (P, P), (7, 7), "auto", False, "f64"),
    # forced variants, one size per form
    ("jacobian", 1000, 900, (P, P), None, "tile", False, "f64"),
    ("jacobian", 1000, 900, (P, P), None, "march", False, "f64"),
    ("jacobian", 1000, 900, (P, P), None, "auto", True, "f64"),
    ("divergence", 1000, 800, (P, P), None, "tile", False, "f64"),
    ("divergence", 1000, 800, (P, P), None, "march", False, "f64"),
    ("divergence", 1000, 800, (P, P), None, "auto", True, "f64"),
]


def run():
    import numpy as np
    import torch
    import swmhd_amd as S
    torch.cuda.set_device(0)
    for form, Nx, Ny, topo, rows, kernel, strict, dt in CALLS:
        tdt = torch.float64 if dt == "f64" else torch.float32
        g = S.RectilinearGrid(size=(Nx, Ny), x=(0, 0.37 * Nx), y=(0, 0.41 * Ny), halo=(3, 3), topology=(topo[0], topo[1], "Flat"))
        A, h = S.Field(g, dtype=tdt), S.Field(g, dtype=tdt)
        A.data.normal_(); h.data.uniform_(1.0, 1.3)
        fn = S.lorentz_force_func if form == "jacobian" else S.div_lorentz
        fn(g, {"A": A, "h": h}, strict=strict, rows=rows, kernel=kernel)
        torch.cuda.synchronize()
    g = S.RectilinearGrid(size=(65, 17), x=(-5, 5), y=(-5, 5))
    names = ("c0", "c1", "c2")
    state = {"h": lambda X, Y: np.ones_like(X), "A": lambda X, Y: 0.1 * np.exp(-(X ** 2 + Y ** 2))}
    dye = {n: (lambda X, Y, k=k: np.tanh((1 + 0.25 * k) * Y)) for k, n in enumerate(names)}
    m = S.ShallowWaterModel(g, tracers=names)
    m.set(**state, **dye)
    m.time_step(0.001); m.synchronize()
    e = S.ShallowWaterEnsemble(g, 3, tracers=names)
    e.set(**state, **dye)
    e.time_step(0.001); e.synchronize()
    print("op_dispatch_trace: calls made", flush=True)


def summarize(raw, out):
    import csv, glob, re
    files = sorted(glob.glob(os.path.join(raw, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"no *kernel_trace.csv under {raw}")
    rows = []
    for fn in files:
        for r in csv.DictReader(open(fn)):
            m = re.search(r"(k_\w+)(<.*>)?", r["Kernel_Name"])
            if m and "swmhd::" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), m.group(0), [int(r[f"Grid_Size_{d}"]) for d in "XYZ"],
                             [int(r[f"Workgroup_Size_{d}"]) for d in "XYZ"]))
    rows.sort(key=lambda r: r[0])
    seq = [[k, g, w] for _, k, g, w in rows]
    with open(out, "w") as f:
        json.dump({"tool": "tools/op_dispatch_trace.py under rocprofv3 --kernel-trace --stats", "dispatches": len(seq), "sequence": seq}, f, indent=0)
        f.write("\n")
    print(f"{len(seq)} dispatches of the library's kernels -> {out}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--summarize", metavar="DIR", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    summarize(a.summarize, a.out) if a.summarize else run()
