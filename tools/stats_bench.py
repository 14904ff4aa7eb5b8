#!/usr/bin/env python3
"""What the read side of the editor costs (gs_gaussians_buffer_stats / _histogram, gs_select_attribute):
the statistics of all nine attributes, a 256-bin histogram of the opacity (colour class: the first 16 bytes of a record), a
256-bin histogram of SIZE2 (covariance class: one more line per record) and a range select on DIST2 (position class), at
1 M (SH none) and 10 M (SH3 f32) Gaussians with every Gaussian selected, next to gs_select_sphere on the same buffer — the
yardstick: a kernel that touches the same first cache line of every record.  Wall time per call with the stream
synchronised behind it (the statistics and the histograms are blocking calls and include their result copy), after warm-up
calls, median over the iterations; `x_sphere` is the ratio to gs_select_sphere.  One JSON line per workload.

    python tools/stats_bench.py [--iters 30] [--workloads 1m,10m]
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

WORKLOADS = {
    "1m": dict(n=1_000_000, sh=3, cov=0),
    "10m": dict(n=10_000_000, sh=0, cov=0),
}
WARMUP = 5


def _median_ms(fn, iters):
    ts = []
    for _ in range(iters + WARMUP):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[WARMUP:]))


def run(gs, wl, name, iters):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod = gs.GaussianPod(wl["sh"], wl["cov"])
    g = synth.scene(wl["n"])
    n = len(g)
    buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pod.from_gaussian(g))
    mt = gs.model_transform_pod()
    sel, out = gs.Selection(dev, n), gs.Selection(dev, n)
    sel.fill(stream)
    st = buf.stats(stream, sel, mt)
    center = tuple(float(v) for v in st.centroid)
    radius = float(np.sqrt(st.max[gs.ATTR_SIZE2])) + 0.25 * float(np.max(st.max[:3] - st.min[:3]))
    size_hi = float(np.nextafter(st.max[gs.ATTR_SIZE2], np.float32(np.inf)))

    def sphere():
        out.select_sphere(stream, buf, mt, center, radius)
        stream.synchronize()

    def select_dist2():
        out.select_attribute(stream, buf, gs.ATTR_DIST2, 0.0, radius * radius, model_transform=mt, ref=center)
        stream.synchronize()

    calls = dict(select_sphere=sphere,
                 stats=lambda: buf.stats(stream, sel, mt, center),
                 histogram_opacity=lambda: buf.histogram(stream, gs.ATTR_OPACITY, 0.0, 1.0, 256, sel),
                 histogram_size2=lambda: buf.histogram(stream, gs.ATTR_SIZE2, 0.0, size_hi, 256, sel),
                 select_dist2=select_dist2)
    ms = {k: _median_ms(fn, iters) for k, fn in calls.items()}
    # once more in the opposite order: clocks and caches must not favour a row
    again = {k: _median_ms(calls[k], iters) for k in reversed(list(calls))}
    ms = {k: min(ms[k], again[k]) for k in ms}
    row = dict(workload=name, n=n, pod_bytes=pod.size, iters=iters, selected=int(st.count))
    for k, v in ms.items():
        row[k + "_ms"] = v
        row[k + "_x_sphere"] = v / ms["select_sphere"]
    sel.destroy(); out.destroy(); buf.destroy(); stream.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--workloads", default="1m,10m")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        print(json.dumps(run(gs, WORKLOADS[name], name, a.iters)), flush=True)


if __name__ == "__main__":
    main()
