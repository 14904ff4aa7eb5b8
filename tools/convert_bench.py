#!/usr/bin/env python3
"""What a layout conversion costs (gs_gaussians_buffer_create_converted) next to the plain extraction of the
same records (gs_gaussians_buffer_create_from_selection, the 224-byte copy: the nearest existing kernel and the yardstick).
A tools/synth scene of 1 M and of 10 M Gaussians is uploaded as SH f32 / rot-scale and turned into SH f16 / cov f16
(144-byte records) and into SH none / cov f16 (32-byte records), with no selection and with a random 30 % selection.

Every call is blocking (scan, count to the host, allocation, one kernel, synchronise), so the host clock around it is the
call's time; the three calls alternate inside every repeat, the result is destroyed outside the timed window, the first
`--warmup` repeats are dropped and the median of the rest is reported with the spread (min .. max).  GB/s = (records read +
records written) / time: selected records x (224 + destination record size).  One JSON line per workload and a table.

The `decompose` rows (gs_gaussians_buffer_create_decomposed) are measured the same way in the same run: the
scene as SH f16 / cov f16 (144-byte records) decomposed into SH f16 / rot-scale (144-byte records), alternating with the
conversion f32 / rot-scale -> f16 / f16 of the same selection, the baseline; `x` = time / the baseline's time.

    python tools/convert_bench.py [--iters 15] [--warmup 3] [--workloads 1m,10m] [--rows convert,decompose]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKLOADS = {"1m": 1_000_000, "10m": 10_000_000}
SRC = (0, 0)
TARGETS = [("copy f32/rot-scale (yardstick)", None), ("-> f16/f16", (1, 2)), ("-> none/f16", (3, 2))]


def measure(stream, calls, count, iters, warmup):
    """calls: (label, source pod, destination pod, fn); they alternate inside every repeat.  Returns one row per call."""
    ts = {label: [] for label, _, _, _ in calls}
    for _ in range(warmup + iters):
        for label, _, _, fn in calls:
            stream.synchronize()
            t0 = time.perf_counter()
            out = fn()                       # blocking: returns after the kernel has finished
            ts[label].append((time.perf_counter() - t0) * 1e3)
            assert out.len() == count
            out.destroy()
    rows = []
    for label, spod, dpod, _ in calls:
        t = np.array(ts[label][warmup:])
        moved = count * (spod.size + dpod.size)
        rows.append(dict(call=label, count=int(count), dst_bytes=dpod.size, ms=float(np.median(t)), ms_min=float(t.min()),
                         ms_max=float(t.max()), gbps=moved / (float(np.median(t)) * 1e-3) / 1e9))
    return rows


def run(gs, name, n, iters, warmup, row_sets):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    spod = gs.GaussianPod(*SRC)
    g = synth.scene(n)
    n = len(g)
    buf = gs.GaussiansBuffer.new_with_pods(dev, spod, spod.from_gaussian(g))
    del g
    sel = gs.Selection(dev, n)
    sel.upload(stream, np.random.default_rng(1).random(n) < 0.3)
    count30 = sel.count(stream)
    rows = []
    masks = (("all", None, n), ("30 %", sel, count30))
    if "convert" in row_sets:
        for mask_name, s, count in masks:
            calls = []
            for label, dst in TARGETS:
                if dst is None:
                    calls.append((label, spod, spod, lambda s=s: buf.extract(stream, s)))
                else:
                    calls.append((label, spod, gs.GaussianPod(*dst), lambda s=s, d=gs.GaussianPod(*dst): buf.convert(stream, d, s)))
            rows += [dict(r, mask=mask_name) for r in measure(stream, calls, count, iters, warmup)]
    if "decompose" in row_sets:
        half, out = gs.GaussianPod(1, 2), gs.GaussianPod(1, 0)
        cov = buf.convert(stream, half)
        for mask_name, s, count in masks:
            calls = [("baseline: f32/rot-scale -> f16/f16", spod, half, lambda s=s: buf.convert(stream, half, s)),
                     ("decompose: f16/f16 -> f16/rot-scale", half, out, lambda s=s: cov.decompose(stream, 1, s))]
            base, dec = measure(stream, calls, count, iters, warmup)
            rows += [dict(base, mask=mask_name), dict(dec, mask=mask_name, x=dec["ms"] / base["ms"])]
        cov.destroy()
    sel.destroy(); buf.destroy(); stream.close()
    return dict(workload=name, n=n, iters=iters, warmup=warmup, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="1m,10m")
    ap.add_argument("--rows", default="convert,decompose")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    results = []
    for name in a.workloads.split(","):
        results.append(run(gs, name, WORKLOADS[name], a.iters, a.warmup, a.rows.split(",")))
        print(json.dumps(results[-1]), flush=True)
    print("| scene | mask | call | records | ms (min .. max) | GB/s | x baseline |")
    print("|---|---|---|---|---|---|---|")
    for res in results:
        for r in res["rows"]:
            print("| %s | %s | %s | %d | %.3f (%.3f .. %.3f) | %.0f | %s |" % (res["workload"], r["mask"], r["call"], r["count"], r["ms"],
                                                                            r["ms_min"], r["ms_max"], r["gbps"],
                                                                            "%.2f" % r["x"] if "x" in r else ""))


if __name__ == "__main__":
    main()
