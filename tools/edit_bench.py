#!/usr/bin/env python3
"""What an edit costs (gs_gaussians_buffer_edit): one edit plus the first frame after it against the frame
alone, at 1 M (SH none, 1080p) and 10 M (SH3 f32, 1080p), for 0.1 % / 10 % / 100 % of the Gaussians selected, for a
colour edit (the mirror keeps its spatial order: repack + block bounds) and a transform edit (the next frame sorts the
order again).  Wall time per iteration with the stream synchronised behind every frame, median over the iterations; the
edit alone (kernel only, synchronised) is listed too.  One JSON line per workload.

The history rows at the same scene sizes and shares: `snapshot` of the selection (blocking: scan, allocation
and gather), `restore` and `exchange` of that snapshot (one launch, synchronised), `concat` of the selection into a new
buffer (blocking scan, allocation, copy, synchronised), each as ms and as GB/s of the bytes it must move — the selected
records read and written once, twice for an exchange — next to a device-to-device hipMemcpyAsync of the same records
(count x pod size read and written) as the yardstick.

    python tools/edit_bench.py [--iters 15] [--workloads 1m,10m] [--rows edit,history]
"""
import argparse
import ctypes as C
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


def _median_ms(fn, iters, after=None):
    ts = []
    for _ in range(iters + 2):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        if after is not None:
            after(out)
    return float(np.median(ts[2:]))


def history_rows(gs, dev, stream, buf, sel, share, iters):
    """snapshot / restore / exchange / concat of `sel` and the device-to-device copy of the same bytes"""
    lib = gs._capi.load()
    memcpy = lib.hipMemcpyAsync          # the runtime the library is linked to
    memcpy.argtypes, memcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p], C.c_int
    D2D = 3                              # hipMemcpyDeviceToDevice
    stream.synchronize()
    snap = buf.snapshot(stream, sel)
    count, nbytes = snap.count, snap.count * buf.pod.size
    a, b = gs.Buffer(dev, size=max(nbytes, 16)), gs.Buffer(dev, size=max(nbytes, 16))
    dev.synchronize()

    def copy():
        assert memcpy(b.device_ptr(), a.device_ptr(), nbytes, D2D, stream.native()) == 0
        stream.synchronize()

    def restore(exchange):
        buf.restore(stream, snap, exchange=exchange)
        stream.synchronize()

    def concat():
        out, _ = gs.GaussiansBuffer.concat(stream, [buf], [sel])
        stream.synchronize()
        return out

    ms = dict(copy=_median_ms(copy, iters),
              snapshot=_median_ms(lambda: buf.snapshot(stream, sel), iters, after=lambda o: o.destroy()),
              restore=_median_ms(lambda: restore(False), iters),
              exchange=_median_ms(lambda: restore(True), iters),
              concat=_median_ms(concat, iters, after=lambda o: o.destroy()))
    moved = dict(copy=2 * nbytes, snapshot=2 * nbytes, restore=2 * nbytes, exchange=4 * nbytes, concat=2 * nbytes)
    row = dict(share=share, count=count, record_bytes=nbytes, snapshot_bytes=snap.nbytes)
    for k, v in ms.items():
        row[k + "_ms"] = v
        row[k + "_gbps"] = moved[k] / (v * 1e-3) / 1e9
    snap.destroy(); a.release(); b.release()
    return row


def run(gs, wl, name, iters, rows, W=1920, H=1080):
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
    out = dict(workload=name, n=n, width=W, height=H, iters=iters, frame_ms=float(np.median(ts)), cases=[], history=[])
    rng = np.random.default_rng(1)
    for share in SHARES:
        sel.upload(stream, rng.random(n) < share if share < 1.0 else np.ones(n, bool))
        if "history" in rows:
            out["history"].append(history_rows(gs, dev, stream, buf, sel, share, iters))
        for kind, pair in edits.items() if "edit" in rows else ():
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
    ap.add_argument("--rows", default="edit,history", help="edit: the edit cases; history: snapshot / restore / exchange / concat")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    for name in a.workloads.split(","):
        print(json.dumps(run(gs, WORKLOADS[name], name, a.iters, a.rows.split(","))), flush=True)


if __name__ == "__main__":
    main()
