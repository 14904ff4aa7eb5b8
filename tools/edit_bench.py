#!/usr/bin/env python3
"""What an edit costs (gs_gaussians_buffer_edit): one edit plus the first frame after it against the frame
alone, at 1 M (SH none, 1080p) and 10 M (SH3 f32, 1080p), for 0.1 % / 10 % / 100 % of the Gaussians selected, for a
colour edit (the mirror keeps its spatial order: repack + block bounds) and a transform edit (the next frame sorts the
order again).  Wall time per iteration with the stream synchronised behind every frame, median over the iterations; the
edit alone (kernel only, synchronised) is listed too.  One JSON line per workload.

    python tools/edit_bench.py [--iters 15] [--workloads 1m,10m]
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
    "1m": dict(n=1_000_000, sh=3, cov=0, sh_deg=0),
    "10m": dict(n=10_000_000, sh=0, cov=0, sh_deg=3),
}
SHARES = [0.001, 0.1, 1.0]


def run(gs, wl, name, iters, W=1920, H=1080):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod = gs.GaussianPod(wl["sh"], wl["cov"])
    g = synth.scene(wl["n"])
    n = len(g)
    buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pod.from_gaussian(g))
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=wl["sh_deg"]), gs.model_transform_pod()
    img = gs.Buffer(dev, size=W * H * 16)
    r = gs.Renderer(dev)
    sel = gs.Selection(dev, n)
    # edits that give the scene back after two applications, so that every iteration renders a like frame
    t = 0.001
    edits = {"color": [gs.edit(color=gs.color_exposure(0.05)), gs.edit(color=gs.color_exposure(-0.05))],
             "transform": [gs.edit(transform=gs.model_transform_pod(pos=(t, 0, 0), rot=(0, 0, np.sin(0.005), np.cos(0.005)))),
                           gs.edit(transform=gs.model_transform_pod(pos=(-t, 0, 0), rot=(0, 0, -np.sin(0.005), np.cos(0.005))))]}

    def frame():
        r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False)
        stream.synchronize()

    for _ in range(20):
        frame()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        frame()
        ts.append((time.perf_counter() - t0) * 1e3)
    out = dict(workload=name, n=n, width=W, height=H, iters=iters, frame_ms=float(np.median(ts)), cases=[])
    rng = np.random.default_rng(1)
    for share in SHARES:
        sel.upload(stream, rng.random(n) < share if share < 1.0 else np.ones(n, bool))
        for kind, pair in edits.items():
            both, alone = [], []
            for k in range(iters + 2):
                stream.synchronize()
                t0 = time.perf_counter()
                buf.edit(stream, sel, pair[k & 1])
                frame()
                both.append((time.perf_counter() - t0) * 1e3)
            for k in range(iters + 2):
                stream.synchronize()
                t0 = time.perf_counter()
                buf.edit(stream, sel, pair[k & 1])
                stream.synchronize()
                alone.append((time.perf_counter() - t0) * 1e3)
            frame()
            out["cases"].append(dict(share=share, kind=kind, edit_plus_frame_ms=float(np.median(both[2:])),
                                     edit_ms=float(np.median(alone[2:])),
                                     over_frame_ms=float(np.median(both[2:])) - out["frame_ms"]))
    sel.destroy(); r.destroy(); img.release(); buf.destroy(); stream.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--workloads", default="1m,10m")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        print(json.dumps(run(gs, WORKLOADS[name], name, a.iters)), flush=True)


if __name__ == "__main__":
    main()
