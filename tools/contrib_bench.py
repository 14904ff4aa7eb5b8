#!/usr/bin/env python3
"""What contribution frames cost (gs_render_frame_contrib, gs_select_contribution), on the bench's 1 M
(SH none) and 10 M (SH3 f32) scenes at 1080p, every frame pinned to one round (a contribution frame always takes one).

  (a) the plain single-round frame of this build against another build of the library (--ref-lib: tools/build_rev.sh
      <parent>), alternating child processes, one build per process (the switch GS3D_LIB is read when the package loads);
  (b) contribution frames against plain frames of one renderer in alternating blocks of one process;
  (c) the blend stage alone (HIP events on the launch stream, stage 7) for both;
  (d) gs_select_contribution against gs_select_attribute (GS_ATTR_OPACITY) on the same n.

Every figure is the median of `reps` blocks (>= 15) after a warm-up; the spread (min .. max of the blocks) is printed
with it.  One JSON line per workload.

    python tools/contrib_bench.py [--frames 20] [--reps 15] [--workloads 1m,10m] [--ref-lib build/ab/libgs3d_hip_<rev>.so] [--ab-pairs 3]
"""
import argparse
import json
import os
import subprocess
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
    "100k": dict(n=100_000, sh=3, cov=0, sh_deg=0),
}


def _stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=len(v))


def _upload(gs, synth, dev, stream, wl, chunk=1_000_000):
    pod = gs.GaussianPod(wl["sh"], wl["cov"])
    buf = gs.GaussiansBuffer.new_empty(dev, pod, wl["n"])
    for first in range(0, wl["n"], chunk):
        cnt = min(chunk, wl["n"] - first)
        buf.update_range_with_pod(stream, first, pod.from_gaussian(synth.scene(cnt, first=first)))
    return buf


def run(gs, wl, name, frames, reps, plain_only=False, W=1920, H=1080):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    buf = _upload(gs, synth, dev, stream, wl)
    n = wl["n"]
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=wl["sh_deg"]), gs.model_transform_pod()
    img = gs.Buffer(dev, size=W * H * 16)
    r = gs.Renderer(dev)
    r.set_rounds(0)
    kinds = [False] if plain_only else [False, True]
    c = None if plain_only else gs.Contributions.new(dev, stream, n)
    kw = {False: {}, True: dict(contributions=c)}
    for k in kinds:           # settle: sizing, sort feedback
        for _ in range(20):
            r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[k])
        r.wait_frame()
    res = {k: dict(wall=[], blend=[], frame=[]) for k in kinds}
    for _ in range(reps):
        for k in kinds:
            if k:
                c.clear(stream)
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[k])
            stream.synchronize()
            res[k]["wall"].append((time.perf_counter() - t0) * 1e3 / frames)
            r.wait_frame()
            r.set_timing(True)
            r.reset_stats()
            for _ in range(frames):
                r.render(stream, buf, gt, mt, cam, img.device_ptr(), check=False, **kw[k])
            st = r.stats()
            r.set_timing(False)
            t = max(st.timed_frames, 1)
            res[k]["blend"].append(st.stage_ms[7] / t)
            res[k]["frame"].append(sum(st.stage_ms[i] for i in range(8)) / t)
    fr = r.wait_frame()
    out = dict(workload=name, n=n, width=W, height=H, rounds=r.sort_info().rounds, frames=frames, reps=reps,
               visible=int(fr.visible), pairs=int(fr.pairs), lib=os.environ.get("GS3D_LIB", "this build"),
               plain_ms={k: _stat(v) for k, v in res[False].items()})
    if not plain_only:
        out["contrib_ms"] = {k: _stat(v) for k, v in res[True].items()}
        out["blend_ratio"] = out["contrib_ms"]["blend"]["median"] / out["plain_ms"]["blend"]["median"]
        out["frame_ratio"] = out["contrib_ms"]["wall"]["median"] / out["plain_ms"]["wall"]["median"]
        rec = c.download(stream)
        out["contributions_per_frame"] = int(rec["hits"].astype(np.uint64).sum()) // (2 * frames)
        # (d) the select ops: `batch` enqueues per timed block
        sel = gs.Selection(dev, n)
        batch = 20
        sel_ms = dict(contribution=[], attribute=[])
        for which in ("contribution", "attribute", "contribution", "attribute"):      # warm-up
            c.select(stream, sel, gs.CONTRIB_SUM, 0.0, 1.0) if which == "contribution" else \
                sel.select_attribute(stream, buf, gs.ATTR_OPACITY, 0.0, 0.1)
        for _ in range(reps):
            for which in ("contribution", "attribute"):
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(batch):
                    if which == "contribution":
                        c.select(stream, sel, gs.CONTRIB_SUM, 0.0, 1.0)
                    else:
                        sel.select_attribute(stream, buf, gs.ATTR_OPACITY, 0.0, 0.1)
                stream.synchronize()
                sel_ms[which].append((time.perf_counter() - t0) * 1e3 / batch)
        out["select_ms"] = {k: _stat(v) for k, v in sel_ms.items()}
        sel.destroy()
        c.release()
    r.destroy(); img.release(); buf.destroy(); stream.close()
    return out


def ab_plain(name, frames, reps, ref_lib, pairs):
    """(a): plain frames of the reference build and of this build, alternating child processes"""
    sides = {"ref": [], "this": []}
    for _ in range(pairs):
        for side in ("ref", "this"):
            env = dict(os.environ)
            env.pop("GS3D_LIB", None)
            if side == "ref":
                env["GS3D_LIB"] = os.path.abspath(ref_lib)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--workloads", name, "--frames", str(frames),
                                  "--reps", str(reps)], env=env, stdout=subprocess.PIPE, text=True, check=True)
            sides[side].append(json.loads(res.stdout.strip().splitlines()[-1])["plain_ms"])
    return {side: {k: [p[k]["median"] for p in v] for k in ("wall", "blend", "frame")} for side, v in sides.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--workloads", default="1m,10m")
    ap.add_argument("--ref-lib", default=None, help="another build of libgs3d_hip.so for (a)")
    ap.add_argument("--ab-pairs", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true", help="(child of (a)) plain frames only")
    a = ap.parse_args()
    if not a.plain_only and a.ref_lib:
        # before this process opens the device: one process with the GPU open at a time
        ab = {name: ab_plain(name, a.frames, a.reps, a.ref_lib, a.ab_pairs) for name in a.workloads.split(",")}
    else:
        ab = {}
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        out = run(gs, WORKLOADS[name], name, a.frames, a.reps, plain_only=a.plain_only)
        if name in ab:
            out["plain_ab_process_medians_ms"] = ab[name]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
