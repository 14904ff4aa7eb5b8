#!/usr/bin/env python3
"""What the nearest neighbours between two buffers cost (gs_gaussians_buffer_knn_between, gs_gaussians_buffer_pair_sums,
GaussiansBuffer.align_to): knn_to at 1 M against 1 M (SH none) and 10 M against 10 M (SH f32) synthetic
Gaussians for k = 1 and k = 8.  The two scans are the same synthetic scene, the query side under a small rigid offset
(a rotation of 0.05 degrees about the scene's centre and a shift of a quarter of the radius, given as its model
transform).  The radius is the one with a median neighbour count of about 8 (picked as tools/neighbor_bench.py picks it).
The yardstick, in the same run: gs_gaussians_buffer_knn of the target alone with the same k and radius — the same
traversal, so the ratio prices the second sort and the reads from two sets of arrays.  pair_sums is timed on the k = 1
index plane, align_to end to end (every search, sum, fit and its two planes) with its iteration count.  Wall time per
call with the stream synchronised behind it, after warm-up calls, median over the iterations, the rows timed once more in
the opposite order and the smaller median kept.  One JSON line per workload and k; no figure is gated.

    python tools/align_bench.py [--iters 15] [--workloads 1m,10m] [--ks 1,8]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import neighbor_bench as nb  # noqa: E402


def offset_pod(gs, centre, radius):
    """x -> R (x - c) + c + t: 0.05 degrees about an oblique axis through c, t = a quarter of the radius along x"""
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    half = math.radians(0.05) / 2
    w, (x, y, z) = math.cos(half), math.sin(half) * axis
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    t = centre - R @ centre + np.array([0.25 * radius, 0.0, 0.0])
    return gs.model_transform_pod(tuple(t), (x, y, z, w), (1.0, 1.0, 1.0))


def run(gs, wl, name, iters, ks, radius=None):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod = gs.GaussianPod(wl["sh"], wl["cov"])
    g = synth.scene(wl["n"])
    n = len(g)
    rows = np.asarray(pod.from_gaussian(g)).reshape(n, pod.size)
    target = gs.GaussiansBuffer.new_with_pods(dev, pod, rows)
    query = gs.GaussiansBuffer.new_with_pods(dev, pod, rows)
    pos = np.asarray(g["pos"], np.float32)
    r, med = nb.pick_radius(target, stream, pos) if radius is None else (radius, None)
    mt = offset_pod(gs, pos[np.isfinite(pos).all(axis=1)].astype(np.float64).mean(axis=0), r)
    out_rows = []
    for k in ks:
        dist2, index = gs.Buffer(dev, size=4 * k * n), gs.Buffer(dev, size=4 * k * n)
        first, first_d2 = gs.Buffer(dev, size=4 * n), gs.Buffer(dev, size=4 * n)
        query.knn_to(stream, target, 1, r, model_transform=mt, dist2_out=first_d2, index_out=first)
        stream.synchronize()
        reports = []

        def knn():
            target.knn(stream, k, r, dist2_out=dist2, index_out=index)
            stream.synchronize()

        def knn_to():
            query.knn_to(stream, target, k, r, model_transform=mt, dist2_out=dist2, index_out=index)
            stream.synchronize()

        def pair_sums():
            query.pair_sums(stream, target, first, 1, model_transform=mt)

        def align_to():
            reports.append(query.align_to(stream, target, r, model_transform=mt)[1])

        fns = dict(knn=knn, knn_to=knn_to, pair_sums=pair_sums, align_to=align_to)
        ms = {name_: nb._median_ms(fn, iters) for name_, fn in fns.items()}
        again = {name_: nb._median_ms(fns[name_], iters) for name_ in reversed(list(fns))}
        ms = {name_: min(ms[name_], again[name_]) for name_ in ms}
        knn_to()
        s = gs.knn_summary(stream, dist2, n, k, gs.KNN_KTH_DIST2)
        sums = query.pair_sums(stream, target, first, 1, model_transform=mt)
        rep = reports[-1]
        row = dict(workload=name, n_q=n, n_t=n, pod_bytes=pod.size, iters=iters, k=k, radius=r, median_count=med, points=s.points,
                   complete=s.complete, pairs=sums.pairs, rms=sums.rms, align_iterations=len(rep.iterations), align_stopped=rep.stopped,
                   align_first_rms=rep.iterations[0][1], align_last_rms=rep.iterations[-1][1])
        for name_, v in ms.items():
            row[name_ + "_ms"] = v
        row["knn_to_x_knn"] = ms["knn_to"] / ms["knn"]
        out_rows.append(row)
        dist2.release(); index.release(); first.release(); first_d2.release()
    query.destroy(); target.destroy(); stream.close()
    return out_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--workloads", default="1m,10m")
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--radius", type=float, default=None, help="the median-8 radius of an earlier run instead of picking one")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        for row in run(gs, nb.WORKLOADS[name], name, a.iters, [int(k) for k in a.ks.split(",")], a.radius):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
