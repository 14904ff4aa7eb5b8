#!/usr/bin/env python3
"""What simplifying costs (gs_gaussians_buffer_create_simplified): the blocking call at 1 M and 10 M synthetic
Gaussians, SH f32 / rot-scale in and out, at the two cell sizes that merge about 4 : 1 and about 32 : 1 (found by bisection
on K), next to two baselines on the same buffer in the same run: gs_gaussians_buffer_create_converted of the same records
(to SH f16 / cov f16: the streaming gather) and gs_select_neighbors with the same radius and no cap (the shared grid front
plus its traversal).  Wall time per call with the stream synchronised behind it, after warm-up calls, median over the
iterations, the rows timed once more in the opposite order and the smaller median kept.  One JSON line per workload and
ratio.

    python tools/simplify_bench.py [--iters 15] [--workloads 1m,10m]

The split into the grid front and the merge kernels comes from a kernel trace of a run of its own (a tracer slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/simplify_bench.py --workloads 1m --only simplify
    python tools/simplify_bench.py --kernel-stats DIR/.../trace_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import neighbor_bench as nb  # noqa: E402

UMAX = 0xFFFFFFFF
WORKLOADS = {"1m": 1_000_000, "10m": 10_000_000}
RATIOS = (4.0, 32.0)
FRONT_KERNELS = nb.KEY_KERNELS + ("k_nb_gather",)


def pick_cell(buf, stream, n, ratio, extent):
    """the cell size whose K is n / ratio within 5 %, by bisection on a logarithmic scale"""
    lo, hi = extent * 2.0 ** -12, extent
    cell, K = hi, 1
    for _ in range(24):
        cell = float(np.sqrt(lo * hi))
        out = buf.simplify(stream, cell)
        K = len(out)
        out.destroy()
        if abs(K * ratio / n - 1.0) < 0.05:
            break
        if K * ratio > n:
            lo = cell
        else:
            hi = cell
    return cell, K


def run(gs, name, n, iters, only):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod, small = gs.GaussianPod(0, 0), gs.GaussianPod(1, 2)
    g = synth.scene(n)
    pos = np.asarray(g["pos"], np.float32)
    extent = float((pos.max(axis=0) - pos.min(axis=0)).max())
    rows = np.asarray(pod.from_gaussian(g)).reshape(n, pod.size)
    buf = gs.GaussiansBuffer.new_with_pods(dev, pod, rows)
    sel = gs.Selection(dev, n)
    out_rows = []
    for ratio in RATIOS:
        cell, K = pick_cell(buf, stream, n, ratio, extent)

        def simplify():
            buf.simplify(stream, cell).destroy()

        def convert():
            buf.convert(stream, small).destroy()

        def neighbors():
            sel.select_neighbors(stream, buf, cell, 0, UMAX)
            stream.synchronize()

        fns = dict(simplify=simplify) if only == "simplify" else dict(simplify=simplify, convert=convert, select_neighbors=neighbors)
        ms = {k: nb._median_ms(fn, iters) for k, fn in fns.items()}
        again = {k: nb._median_ms(fns[k], iters) for k in reversed(list(fns))}
        ms = {k: min(ms[k], again[k]) for k in ms}
        row = dict(workload=name, n=n, pod_bytes=pod.size, iters=iters, ratio_asked=ratio, cell_size=cell, cell_over_extent=cell / extent, K=K,
                   ratio=n / max(K, 1), out_bytes=K * pod.size)
        for k, v in ms.items():
            row[k + "_ms"] = v
        row["out_GBps"] = K * pod.size / (ms["simplify"] * 1e-3) / 1e9
        row["in_plus_out_GBps"] = (n + K) * pod.size / (ms["simplify"] * 1e-3) / 1e9
        for k in ("convert", "select_neighbors"):
            if k in ms:
                row["simplify_x_" + k] = ms["simplify"] / ms[k]
        out_rows.append(row)
    sel.destroy(); buf.destroy(); stream.close()
    return out_rows


def kernel_split(path):
    """rocprofv3's kernel_stats.csv of a run with --only simplify -> total kernel time by group and per kernel"""
    rows = list(csv.DictReader(open(path)))
    out = dict(total_ms={}, kernels={})
    for r in rows:
        short = r["Name"].replace("void gs::", "").split("(")[0].split("<")[0]
        group = ("front" if any(k in short for k in FRONT_KERNELS) else "merge" if "k_sm_merge" in short else
                 "long" if "k_sm_long" in short else "count" if "k_sm_count" in short else None)
        if group:
            ms = float(r["TotalDurationNs"]) / 1e6
            out["total_ms"][group] = out["total_ms"].get(group, 0.0) + ms
            k = out["kernels"].setdefault(short, dict(calls=0, total_ms=0.0))
            k["calls"] += int(r["Calls"])
            k["total_ms"] += ms
    for k in out["kernels"].values():
        k["avg_ms"] = k["total_ms"] / k["calls"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--workloads", default="1m,10m")
    ap.add_argument("--only", default=None, choices=(None, "simplify"), help="time only the simplify call (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="summarise a rocprofv3 kernel_stats.csv instead of running")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_split(a.kernel_stats)), flush=True)
        return
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        for row in run(gs, name, WORKLOADS[name], a.iters, a.only):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
