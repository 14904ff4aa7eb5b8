#!/usr/bin/env python3
"""What the nearest neighbours cost (gs_gaussians_buffer_knn, gs_select_knn, gs_knn_summary): the calls at
1 M (SH3 f32) and 10 M (SH none) synthetic Gaussians for k = 3 and k = 8, at the radius with a median neighbour count of
about 8 (picked as tools/neighbor_bench.py picks it), next to gs_select_neighbors with max_count = UINT32_MAX on the same
buffer in the same run — the yardstick: the identical front and the identical traversal with no cap, so the ratio prices the
top-k bookkeeping.  knn_auto is timed end to end (its stats() call, every pass, every count) with the number of passes it
took.  Wall time per call with the stream synchronised behind it, after warm-up calls, median over the iterations, the rows
timed once more in the opposite order and the smaller median kept.  One JSON line per workload and k; no figure is gated.

    python tools/knn_bench.py [--iters 15] [--workloads 1m,10m] [--ks 3,8]
"""
import argparse
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


def run(gs, wl, name, iters, ks, radius=None):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod = gs.GaussianPod(wl["sh"], wl["cov"])
    g = synth.scene(wl["n"])
    n = len(g)
    rows = np.asarray(pod.from_gaussian(g)).reshape(n, pod.size)
    buf = gs.GaussiansBuffer.new_with_pods(dev, pod, rows)
    r, med = nb.pick_radius(buf, stream, np.asarray(g["pos"], np.float32)) if radius is None else (radius, None)
    out = gs.Selection(dev, n)
    out_rows = []
    for k in ks:
        dist2, index = gs.Buffer(dev, size=4 * k * n), gs.Buffer(dev, size=4 * k * n)
        passes = []

        def neighbors():
            out.select_neighbors(stream, buf, r, 0, UMAX)
            stream.synchronize()

        def knn():
            buf.knn(stream, k, r, dist2_out=dist2)
            stream.synchronize()

        def knn_indices():
            buf.knn(stream, k, r, dist2_out=dist2, index_out=index)
            stream.synchronize()

        def knn_auto():
            d, i, _, p = buf.knn_auto(stream, k)
            passes.append(p)
            d.release(); i.release()

        def select_knn():
            out.select_knn(stream, dist2, k, gs.KNN_MEAN_DIST, 0.0, r)
            stream.synchronize()

        def summary():
            gs.knn_summary(stream, dist2, n, k, gs.KNN_MEAN_DIST)

        fns = dict(select_neighbors=neighbors, knn=knn, knn_indices=knn_indices, knn_auto=knn_auto, select_knn=select_knn,
                   knn_summary=summary)
        ms = {name_: nb._median_ms(fn, iters) for name_, fn in fns.items()}
        again = {name_: nb._median_ms(fns[name_], iters) for name_ in reversed(list(fns))}
        ms = {name_: min(ms[name_], again[name_]) for name_ in ms}
        knn()
        s = gs.knn_summary(stream, dist2, n, k, gs.KNN_KTH_DIST2)
        row = dict(workload=name, n=n, pod_bytes=pod.size, iters=iters, k=k, radius=r, median_count=med, points=s.points,
                   complete=s.complete, knn_auto_passes=int(np.median(passes)))
        for name_, v in ms.items():
            row[name_ + "_ms"] = v
        for name_ in ("knn", "knn_indices", "knn_auto"):
            row[name_ + "_x_select_neighbors"] = ms[name_] / ms["select_neighbors"]
        out_rows.append(row)
        dist2.release(); index.release()
    out.destroy(); buf.destroy(); stream.close()
    return out_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--workloads", default="1m,10m")
    ap.add_argument("--ks", default="3,8")
    ap.add_argument("--radius", type=float, default=None, help="the median-8 radius of an earlier run instead of picking one")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        for row in run(gs, nb.WORKLOADS[name], name, a.iters, [int(k) for k in a.ks.split(",")], a.radius):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
