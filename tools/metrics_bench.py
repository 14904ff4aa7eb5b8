#!/usr/bin/env python3
"""What measuring a picture costs: gs_image_compare with and without GS_COMPARE_SSIM, with and without
the two planes, at 1920x1080 and 3840x2160, next to the plain device-to-host copy of the two images that any host metric
pays before it computes anything.

The call is blocking, so the host clock around it is the call's time (two launches, the 176-byte result, one
synchronise); the first `--warmup` repeats are dropped and the median of the rest is reported with the spread.  A compare
must read 2 x 16 B x W x H bytes: the table gives that over the call's time as GB/s and as a share of the 8.0 TB/s the
HBM is specified for (about 6.3 TB/s is what a plain copy kernel reaches).  So that a repeat does not find the previous
repeat's images in the 256 MiB Infinity Cache, the calls rotate through enough image pairs to hold more than 512 MiB.
The copy is gs_buffer_download of both images into pageable host memory, measured in the same run.  One JSON line per
size and a table.

    python tools/metrics_bench.py [--iters 15] [--warmup 3] [--sizes 1920x1080,3840x2160]
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

HBM_SPEC_BPS = 8.0e12


def _timed(fn, stream):
    stream.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run(gs, w, h, iters, warmup):
    dev = gs.Device(0)
    stream = dev.create_stream()
    rng = np.random.default_rng(5)
    a = rng.random((h, w, 4), dtype=np.float32)
    b = (a + np.float32(0.02) * rng.standard_normal((h, w, 4), dtype=np.float32)).astype(np.float32)
    read_bytes = 2 * 16 * w * h
    npairs = max(2, -(-(512 << 20) // read_bytes))
    pairs = [(gs.Buffer(dev, data=a), gs.Buffer(dev, data=b)) for _ in range(npairs)]
    err, ssim = gs.Buffer(dev, size=w * h * 4), gs.Buffer(dev, size=w * h * 4)
    turn = [0]

    def compare(with_ssim, planes):
        pa, pb = pairs[turn[0] % npairs]
        turn[0] += 1
        return gs.image_compare(dev, stream, pa.device_ptr(), pb.device_ptr(), w, h, ssim=with_ssim,
                                err_plane_ptr=err.device_ptr() if planes else None,
                                ssim_plane_ptr=ssim.device_ptr() if planes and with_ssim else None)

    def copy():
        pa, pb = pairs[turn[0] % npairs]
        turn[0] += 1
        return pa.download(stream, np.float32), pb.download(stream, np.float32)

    calls = [("compare, no SSIM", lambda: compare(False, False)), ("compare, no SSIM, error plane", lambda: compare(False, True)),
             ("compare, SSIM", lambda: compare(True, False)), ("compare, SSIM, both planes", lambda: compare(True, True)),
             ("device-to-host copy of the two images", copy)]
    ts = {label: [] for label, _ in calls}
    last = {}
    # one call after the other, each with its own warm-up: a compare that follows the 4 - 16 ms copy finds the device idle
    # (interleaved, the compare behind the copy took 0.1 ms longer at 4K than the next one, which also writes a plane)
    for label, fn in calls:
        for _ in range(warmup + iters):
            ms, out = _timed(fn, stream)
            ts[label].append(ms)
            last[label] = out
    m = last["compare, SSIM"]
    assert m.finite == w * h and m.raw[:128] == last["compare, no SSIM"].raw[:128]
    rows = []
    for label, _ in calls:
        t = np.array(ts[label][warmup:])
        ms = float(np.median(t))
        rows.append(dict(call=label, ms=ms, ms_min=float(t.min()), ms_max=float(t.max()), gbps=read_bytes / (ms * 1e-3) / 1e9,
                         hbm_share=read_bytes / (ms * 1e-3) / HBM_SPEC_BPS))
    for pa, pb in pairs:
        pa.release(); pb.release()
    err.release(); ssim.release(); stream.close()
    return dict(width=w, height=h, read_bytes=read_bytes, pairs=npairs, iters=iters, warmup=warmup, psnr=m.psnr(), ssim=m.ssim, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    results = []
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        results.append(run(gs, w, h, a.iters, a.warmup))
        print(json.dumps(results[-1]), flush=True)
    print("| size | call | ms, median of %d (min .. max) | GB/s of the 2 x 16 B x W x H read | share of 8.0 TB/s |" % a.iters)
    print("|---|---|---|---|---|")
    for res in results:
        for r in res["rows"]:
            share = "" if r["call"].startswith("device-to-host") else "%.1f %%" % (100 * r["hbm_share"])      # the copy is PCIe's
            print("| %dx%d | %s | %.3f (%.3f .. %.3f) | %.1f | %s |" % (res["width"], res["height"], r["call"], r["ms"], r["ms_min"],
                                                                     r["ms_max"], r["gbps"], share))


if __name__ == "__main__":
    main()
