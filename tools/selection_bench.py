#!/usr/bin/env python3
"""What selection frames cost (gs_render_frame_sel): four kinds of frame of one renderer in alternating
blocks, at 1 M (SH none, 1080p) and 10 M (SH3 f32, 1080p):

    a  no selection                      (gs_render_frame)
    b  an EMPTY hide selection           (the cost of the mask path)
    c  a crop box hiding about half      (whole 1024-blocks of the spatially ordered mirror are skipped)
    d  tint on about half

Per block: the wall time per pipelined frame, then a timed block (HIP events on the launch stream) for the preprocess
stage (stage 1) and the whole frame.  One JSON line per workload, with b/a and c/a, the share of fully hidden blocks of c
and the ratio of its preprocess time to a's.

    python tools/selection_bench.py [--frames 50] [--reps 3] [--workloads 1m,10m]
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
KINDS = ["a", "b", "c", "d"]


def run(gs, wl, name, frames, reps, W=1920, H=1080):
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
    empty, crop, half = gs.Selection(dev, n), gs.Selection(dev, n), gs.Selection(dev, n)
    # the crop: everything on one side of the median x is hidden
    lo, hi = g["pos"].min(axis=0).astype(np.float64), g["pos"].max(axis=0).astype(np.float64)
    hi[0] = float(np.median(g["pos"][:, 0]))
    crop.select_box(stream, buf, mt, gs.box_from_bounds(lo - 1.0, hi))
    crop.invert(stream)
    half.upload(stream, np.arange(n) % 2 == 0)
    hidden = crop.download(stream)
    order = buf.download_order(stream)
    blocks = hidden[order][: n // 1024 * 1024].reshape(-1, 1024)
    kw = dict(a={}, b=dict(hide=empty), c=dict(hide=crop), d=dict(tint=half, tint_rgba=(1.0, 0.5, 0.0, 0.5)))
    r = gs.Renderer(dev)
    for kind in KINDS:           # settle: sizing, sort and round feedback
        for _ in range(20):
            r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[kind])
        r.wait_frame()
    res = {k: dict(wall=[], pre=[], frame=[]) for k in KINDS}
    for _ in range(reps):
        for kind in KINDS:
            for _ in range(5):   # (c follows frames with twice its pairs and b follows c: let the history settle)
                r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[kind])
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[kind])
            stream.synchronize()
            res[kind]["wall"].append((time.perf_counter() - t0) * 1e3 / frames)
            flags = r.wait_frame().flags
            r.set_timing(True)
            r.reset_stats()
            for _ in range(frames):
                r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[kind])
            st = r.stats()
            r.set_timing(False)
            k = max(st.timed_frames, 1)
            res[kind]["pre"].append(st.stage_ms[1] / k)
            res[kind]["frame"].append(sum(st.stage_ms[i] for i in range(8)) / k)
            res[kind]["flags"] = flags
    med = {kind: {k: float(np.median(v)) for k, v in res[kind].items() if k != "flags"} for kind in KINDS}
    out = dict(workload=name, n=n, width=W, height=H, frames=frames, reps=reps, rounds=r.sort_info().rounds,
               hidden_share=float(hidden.mean()), hidden_block_share=float(blocks.all(axis=1).mean()),
               ms={kind: med[kind] for kind in KINDS}, last_flags={kind: res[kind]["flags"] for kind in KINDS},
               b_over_a=med["b"]["wall"] / med["a"]["wall"], c_over_a=med["c"]["wall"] / med["a"]["wall"],
               d_over_a=med["d"]["wall"] / med["a"]["wall"],
               b_pre_over_a=med["b"]["pre"] / med["a"]["pre"] if med["a"]["pre"] else None,
               c_pre_over_a=med["c"]["pre"] / med["a"]["pre"] if med["a"]["pre"] else None)
    for s in (empty, crop, half):
        s.destroy()
    r.destroy(); img.release(); buf.destroy(); stream.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="1m,10m")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        print(json.dumps(run(gs, WORKLOADS[name], name, a.frames, a.reps)), flush=True)


if __name__ == "__main__":
    main()
