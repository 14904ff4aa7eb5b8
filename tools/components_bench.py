#!/usr/bin/env python3
"""What the clusters cost (gs_gaussians_buffer_components, gs_select_components, gs_select_connected): the
three calls at 1 M (SH3 f32) and 10 M (SH none) synthetic Gaussians, at the radius with a median neighbour count of about 8
(picked as tools/neighbor_bench.py picks it) and at a third of it, next to gs_select_neighbors with max_count = UINT32_MAX
on the same buffer in the same run — the yardstick: the identical front and the identical traversal with no cap, no
atomics and no finalise.  Wall time per call with the stream synchronised behind it, after warm-up calls, median over the
iterations, the rows timed once more in the opposite order and the smaller median kept.  One JSON line per workload and
radius.

    python tools/components_bench.py [--iters 15] [--workloads 1m,10m]

The split into the shared front, link and finalise comes from a kernel trace of a run of its own (a tracer slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/components_bench.py --workloads 1m --calls components --radius R
    python tools/components_bench.py --kernel-stats DIR/.../trace_kernel_stats.csv
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
FRONT_KERNELS = nb.KEY_KERNELS + ("k_nb_gather",)


def run(gs, wl, name, iters, calls, radius=None):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod = gs.GaussianPod(wl["sh"], wl["cov"])
    g = synth.scene(wl["n"])
    n = len(g)
    rows = np.asarray(pod.from_gaussian(g)).reshape(n, pod.size)
    buf = gs.GaussiansBuffer.new_with_pods(dev, pod, rows)
    r8, med = nb.pick_radius(buf, stream, np.asarray(g["pos"], np.float32)) if radius is None else (radius, None)
    labels, sizes, info = gs.Buffer(dev, size=4 * n), gs.Buffer(dev, size=4 * n), gs.Buffer(dev, size=16)
    out, seeds = gs.Selection(dev, n), gs.Selection(dev, n)
    seeds.select_range(stream, n // 2, 1)
    out_rows = []
    for what, r in (("median8", r8), ("third", r8 / 3.0)):
        def neighbors():
            out.select_neighbors(stream, buf, r, 0, UMAX)
            stream.synchronize()

        def components():
            buf.components(stream, r, labels_out=labels, sizes_out=sizes, info_out=info)
            stream.synchronize()

        def select_components():
            out.select_components(stream, buf, r, 1, 19)
            stream.synchronize()

        def select_connected():
            out.select_connected(stream, buf, r, seeds)
            stream.synchronize()

        fns = dict(select_neighbors=neighbors)
        for k, fn in (("components", components), ("select_components", select_components), ("select_connected", select_connected)):
            if k in calls:
                fns[k] = fn
        ms = {k: nb._median_ms(fn, iters) for k, fn in fns.items()}
        again = {k: nb._median_ms(fns[k], iters) for k in reversed(list(fns))}
        ms = {k: min(ms[k], again[k]) for k in ms}
        components()
        i = np.asarray(info.download(stream, np.uint32))[:4].view(gs.COMPONENTS_INFO_DTYPE)[0]
        row = dict(workload=name, n=n, pod_bytes=pod.size, iters=iters, radius_kind=what, radius=r, median_count=med if what == "median8" else None,
                   points=int(i["points"]), components=int(i["components"]), largest=int(i["largest"]))
        for k, v in ms.items():
            row[k + "_ms"] = v
            row[k + "_x_select_neighbors"] = v / ms["select_neighbors"]
        out_rows.append(row)
    for b in (labels, sizes, info):
        b.release()
    out.destroy(); seeds.destroy(); buf.destroy(); stream.close()
    return out_rows


def kernel_split(path):
    """rocprofv3's kernel_stats.csv of a run with --calls components -> average kernel time per call of the link kernel, by group"""
    rows = list(csv.DictReader(open(path)))
    calls = max(int(r["Calls"]) for r in rows if "k_cc_link" in r["Name"])
    out = dict(link_calls=calls, total_ms={}, kernels={})
    for r in rows:
        short = r["Name"].replace("void gs::", "").split("(")[0].split("<")[0]
        group = ("front" if any(k in short for k in FRONT_KERNELS) else "link" if "k_cc_link" in short else
                 "finalise" if "k_cc_finalise" in short else "planes_and_info" if "k_cc_" in short else
                 "count_and_select" if "k_nb_" in short else None)
        if group:
            ms = float(r["TotalDurationNs"]) / 1e6
            out["total_ms"][group] = out["total_ms"].get(group, 0.0) + ms
            out["kernels"][short] = dict(calls=int(r["Calls"]), total_ms=ms, avg_ms=ms / int(r["Calls"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--workloads", default="1m,10m")
    ap.add_argument("--calls", default="components,select_components,select_connected")
    ap.add_argument("--radius", type=float, default=None, help="the median-8 radius of an earlier run instead of picking one")
    ap.add_argument("--kernel-stats", default=None, help="summarise a rocprofv3 kernel_stats.csv instead of running")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_split(a.kernel_stats)), flush=True)
        return
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        for row in run(gs, nb.WORKLOADS[name], name, a.iters, a.calls.split(","), a.radius):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
