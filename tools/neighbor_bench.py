#!/usr/bin/env python3
"""What neighbour counts cost (gs_gaussians_buffer_neighbor_counts, gs_select_neighbors): both calls at
1 M (SH none) and 10 M (SH3 f32) synthetic Gaussians with a radius at which the median count is about 8 and cap = 16, next
to gs_select_attribute on the same buffer — the yardstick: one streaming pass over the first cache line of every record.
The radius is picked on the host: a first guess from the 8th-nearest-neighbour distance in a subsample, scaled by the
sampling fraction, then corrected from the median of the downloaded counts.  At 1 M the counts are timed once more with ONE
Gaussian added at 1000 x the extent of the scene (`outlier_ms`, `outlier_x`): the sort does the same work and only the
bounding box grows, so a ratio far above 1 would mean that the grid's resolution depends on the extent.  `counts_sparse` is the same call with a third of the radius (an expected count of 8 / 27: the floater regime, where most
queries find nothing).  Wall time per call
with the stream synchronised behind it, after warm-up calls, median over the iterations.  One JSON line per workload.

    python tools/neighbor_bench.py [--iters 20] [--workloads 1m,10m] [--calls counts,select,sparse]

The split into key build + sort and gather + count comes from a kernel trace of a run of its own (a tracer slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/neighbor_bench.py --workloads 1m --calls counts --no-outlier --radius R
    python tools/neighbor_bench.py --kernel-stats DIR/.../trace_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKLOADS = {
    "1m": dict(n=1_000_000, sh=3, cov=0),
    "10m": dict(n=10_000_000, sh=0, cov=0),
}
WARMUP = 3
TARGET, CAP = 8, 16
KEY_KERNELS = ("k_nb_bbox_partial", "k_bbox_final", "k_nb_keys", "k_sort_", "k_scan_")
COUNT_KERNELS = ("k_nb_gather", "k_nb_count", "k_nb_select")


def _median_ms(fn, iters):
    ts = []
    for _ in range(iters + WARMUP):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[WARMUP:]))


def first_radius(pos, rng):
    """8th-nearest-neighbour distance among a subsample, scaled to the full density (uniform in the small)"""
    n = len(pos)
    m = min(n, 50_000)
    sub = pos[rng.choice(n, m, replace=False)].astype(np.float64)
    q = sub[:256]
    d2 = ((q[:, None, :] - sub[None, :, :]) ** 2).sum(axis=2)
    r = float(np.median(np.sqrt(np.partition(d2, TARGET, axis=1)[:, TARGET])))
    return r * (m / n) ** (1.0 / 3.0)


def pick_radius(buf, stream, pos):
    r = first_radius(pos, np.random.default_rng(1))
    med = 0.0
    for _ in range(6):
        plane = buf.neighbor_counts(stream, r, 4 * CAP)
        med = float(np.median(np.asarray(plane.download(stream, np.uint32))[:buf.len()]))
        plane.release()
        if TARGET - 1 <= med <= TARGET + 1:
            break
        r *= (TARGET / max(med, 0.5)) ** (1.0 / 3.0)
    return r, med


def run(gs, wl, name, iters, calls, outlier, radius=None):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod = gs.GaussianPod(wl["sh"], wl["cov"])
    g = synth.scene(wl["n"])
    n = len(g)
    rows = np.asarray(pod.from_gaussian(g)).reshape(n, pod.size)
    buf = gs.GaussiansBuffer.new_with_pods(dev, pod, rows)
    pos = np.asarray(g["pos"], np.float32)
    r, med = pick_radius(buf, stream, pos) if radius is None else (radius, None)
    plane = gs.Buffer(dev, size=4 * (n + 1))
    out = gs.Selection(dev, n)

    def counts(b=buf):
        b.neighbor_counts(stream, r, CAP, out=plane)
        stream.synchronize()

    def select():
        out.select_neighbors(stream, buf, r, 0, 2)
        stream.synchronize()

    def select_attribute():
        out.select_attribute(stream, buf, gs.ATTR_DIST2, 0.0, 1.0)
        stream.synchronize()

    def counts_sparse():      # the floater regime: most Gaussians have no neighbour at all
        buf.neighbor_counts(stream, r / 3.0, CAP, out=plane)
        stream.synchronize()

    fns = dict(select_attribute=select_attribute)
    if "counts" in calls:
        fns["counts"] = counts
    if "sparse" in calls:
        fns["counts_sparse"] = counts_sparse
    if "select" in calls:
        fns["select"] = select
    ms = {k: _median_ms(fn, iters) for k, fn in fns.items()}
    # once more in the opposite order: clocks and caches must not favour a row
    again = {k: _median_ms(fns[k], iters) for k in reversed(list(fns))}
    ms = {k: min(ms[k], again[k]) for k in ms}
    row = dict(workload=name, n=n, pod_bytes=pod.size, iters=iters, radius=r, median_count=med, cap=CAP)
    for k, v in ms.items():
        row[k + "_ms"] = v
        row[k + "_x_select_attribute"] = v / ms["select_attribute"]
    if outlier and "counts" in calls:
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        far = rows[:1].copy()
        far[0, :12] = (hi + 1000.0 * float((hi - lo).max())).astype(np.float32).view(np.uint8)
        with_far = gs.GaussiansBuffer.new_with_pods(dev, pod, np.concatenate([rows, far]))
        a = _median_ms(counts, iters)
        b = _median_ms(lambda: counts(with_far), iters)
        a, b = min(a, _median_ms(counts, iters)), min(b, _median_ms(lambda: counts(with_far), iters))
        row.update(without_outlier_ms=a, outlier_ms=b, outlier_x=b / a)
        with_far.destroy()
    plane.release(); out.destroy(); buf.destroy(); stream.close()
    return row


def kernel_split(path):
    """rocprofv3's kernel_stats.csv of a run with --calls counts -> average kernel time per call, by group"""
    rows = list(csv.DictReader(open(path)))
    calls = max(int(r["Calls"]) for r in rows if "k_nb_count" in r["Name"])
    out = dict(calls=calls, keys_and_sort_ms=0.0, gather_and_count_ms=0.0, kernels={})
    for r in rows:
        short = r["Name"].replace("void gs::", "").split("(")[0].split("<")[0]
        group = "keys_and_sort_ms" if any(k in short for k in KEY_KERNELS) else "gather_and_count_ms" if any(k in short for k in COUNT_KERNELS) else None
        if group:
            ms = float(r["TotalDurationNs"]) / 1e6 / calls
            out[group] += ms
            out["kernels"][short] = out["kernels"].get(short, 0.0) + ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--workloads", default="1m,10m")
    ap.add_argument("--calls", default="counts,select,sparse")
    ap.add_argument("--no-outlier", action="store_true")
    ap.add_argument("--radius", type=float, default=None, help="the radius of an earlier run instead of picking one (a kernel trace then holds the timed calls alone)")
    ap.add_argument("--kernel-stats", default=None, help="summarise a rocprofv3 kernel_stats.csv instead of running")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_split(a.kernel_stats)), flush=True)
        return
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        print(json.dumps(run(gs, WORKLOADS[name], name, a.iters, a.calls.split(","), not a.no_outlier and name == "1m", a.radius)), flush=True)


if __name__ == "__main__":
    main()
