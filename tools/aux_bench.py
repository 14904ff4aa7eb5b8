#!/usr/bin/env python3
"""What the depth / pick planes cost (gs_render_frame_aux): plain and aux frames of one renderer in
alternating blocks, at 1 M (SH none, 1080p: one round) and 10 M (SH3 f32, 1080p: the renderer's two rounds).  Per block:
the wall time per pipelined frame, then a timed block (HIP events on the launch stream) for the blend stage (stage 7;
in a two-round frame it spans round 1's blend, the round-2 selection and sorts, and round 2's blend) and the whole frame.
One JSON line per workload.

    python tools/aux_bench.py [--frames 50] [--reps 3] [--workloads 1m,10m]
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


def run(gs, wl, name, frames, reps, W=1920, H=1080):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod = gs.GaussianPod(wl["sh"], wl["cov"])
    buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pod.from_gaussian(synth.scene(wl["n"])))
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=wl["sh_deg"]), gs.model_transform_pod()
    img = gs.Buffer(dev, size=W * H * 16)
    depth = gs.Buffer(dev, size=W * H * 4)
    pick = gs.Buffer(dev, size=W * H * 4)
    r = gs.Renderer(dev)
    kw = {False: {}, True: dict(depth_device_ptr=depth.device_ptr(), pick_device_ptr=pick.device_ptr())}
    for aux in (False, True):           # settle: sizing, round feedback
        for _ in range(20):
            r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[aux])
        r.wait_frame()
    res = {False: dict(wall=[], blend=[], frame=[]), True: dict(wall=[], blend=[], frame=[])}
    for _ in range(reps):
        for aux in (False, True):
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[aux])
            stream.synchronize()
            res[aux]["wall"].append((time.perf_counter() - t0) * 1e3 / frames)
            r.wait_frame()
            r.set_timing(True)
            r.reset_stats()
            for _ in range(frames):
                r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[aux])
            st = r.stats()
            r.set_timing(False)
            k = max(st.timed_frames, 1)
            res[aux]["blend"].append(st.stage_ms[7] / k)
            res[aux]["frame"].append(sum(st.stage_ms[i] for i in range(8)) / k)
    si = r.sort_info()
    med = {a: {k: float(np.median(v)) for k, v in res[a].items()} for a in res}
    out = dict(workload=name, n=wl["n"], width=W, height=H, rounds=si.rounds, frames=frames, reps=reps,
               plain_ms=med[False], aux_ms=med[True],
               blend_ratio=med[True]["blend"] / med[False]["blend"] if med[False]["blend"] else None,
               frame_ratio=med[True]["wall"] / med[False]["wall"] if med[False]["wall"] else None)
    r.destroy(); img.release(); depth.release(); pick.release(); buf.destroy(); stream.close()
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
