#!/usr/bin/env python3
"""What saving costs: gs_gaussians_buffer_export_ply / _export_spz_decompressed / _write next to the five-step
host path of the same build — gs_gaussians_buffer_create_from_selection, gs_gaussians_buffer_download_gaussians,
gs_gaussian_to_ply or gs_spz_encode_decompressed, gs_ply_write — for a tools/synth scene of 1 M and of 10 M Gaussians uploaded as
SH f32 / rot-scale, with no selection and with a random 30 % selection.

Every call is blocking, so the host clock around it is the call's time; the calls alternate inside every repeat, the first
`--warmup` repeats are dropped and the median of the rest is reported with the spread (min .. max).  The ceiling of the PLY
export is the device-to-host copy of its output: the rate of a plain copy of as many bytes from device memory into pageable
host memory (gs_buffer_download) is measured in the same run, and the PLY rows report the bytes delivered per second next
to it.  The gzip member (gs_gaussians_buffer_export_spz: zlib on one host thread) is timed with `--gzip-iters` repeats and
reported as a share of the call.  One JSON line per workload and a table.

    python tools/export_bench.py [--iters 15] [--warmup 2] [--gzip-iters 3] [--workloads 1m,10m]
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

WORKLOADS = {"1m": 1_000_000, "10m": 10_000_000}
PLY_RECORD = 248


def _timed(fn, stream):
    stream.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run(gs, name, n, iters, warmup, gzip_iters):
    import synth
    dev = gs.Device(0)
    stream = dev.create_stream()
    pod = gs.GaussianPod(0, 0)
    g = synth.scene(n)
    n = len(g)
    buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pod.from_gaussian(g))
    del g
    sel = gs.Selection(dev, n)
    sel.upload(stream, np.random.default_rng(1).random(n) < 0.3)
    count30 = sel.count(stream)
    opt = gs.spz_options()

    def host_pods(s):
        part = buf.extract(stream, s)
        gg = part.download_gaussians(stream)
        part.destroy()
        return gs.gaussian_to_ply(gg)

    def host_ply(s):
        return gs.PlyGaussians(host_pods(s)).write_to()

    def host_spz(s):
        part = buf.extract(stream, s)
        gg = part.download_gaussians(stream)
        part.destroy()
        return gs.SpzGaussians.write_gaussians_decompressed(gg, opt)

    def device_spz(s):
        # the payload bytes, as host_spz returns them (GaussiansBuffer.export_spz would also decode them into an SpzGaussians)
        return gs._sized_call(gs._L.gs_gaussians_buffer_export_spz_decompressed, buf._h, stream._h, s._h if s is not None else None, 0,
                              C.byref(opt))

    rows = []
    for mask_name, s, count in (("all", None, n), ("30 %", sel, count30)):
        # the ceiling: a plain device-to-host copy of the PLY bytes into pageable memory
        raw = gs.Buffer(dev, size=count * PLY_RECORD)
        copy_ms = []
        for _ in range(warmup + max(3, iters // 3)):
            copy_ms.append(_timed(lambda: raw.download(stream, np.uint8), stream)[0])
        raw.release()
        copy_gbps = count * PLY_RECORD / (float(np.median(copy_ms[warmup:])) * 1e-3) / 1e9
        calls = [("export_ply on the device", lambda s=s: buf.export_ply(stream, s).pods, count * PLY_RECORD),
                 ("host path: extract, download, to_ply", lambda s=s: host_pods(s), count * PLY_RECORD),
                 ("write(PLY) on the device", lambda s=s: buf.write(stream, gs.GaussiansSource.Ply, s), count * PLY_RECORD),
                 ("five-step host path, PLY file image", lambda s=s: host_ply(s), count * PLY_RECORD),
                 ("export_spz_decompressed on the device", lambda s=s: device_spz(s), None),
                 ("five-step host path, SPZ payload", lambda s=s: host_spz(s), None)]
        ts = {label: [] for label, _, _ in calls}
        sizes = {}
        for _ in range(warmup + iters):
            for label, fn, _ in calls:
                ms, out = _timed(fn, stream)
                ts[label].append(ms)
                sizes[label] = out.nbytes if isinstance(out, np.ndarray) else len(out)
                del out
        for a, b in ((0, 1), (2, 3), (4, 5)):
            assert sizes[calls[a][0]] == sizes[calls[b][0]], (calls[a][0], sizes)
        for label, _, ply_bytes in calls:
            t = np.array(ts[label][warmup:])
            row = dict(mask=mask_name, call=label, count=int(count), bytes=int(sizes[label]), ms=float(np.median(t)),
                       ms_min=float(t.min()), ms_max=float(t.max()))
            if ply_bytes:
                row["delivered_gbps"] = ply_bytes / (row["ms"] * 1e-3) / 1e9
                row["copy_gbps"] = copy_gbps
            rows.append(row)
        if gzip_iters:
            t = np.array([_timed(lambda: buf.write(stream, gs.GaussiansSource.Spz, s), stream)[0] for _ in range(gzip_iters)])
            payload_ms = float(np.median(ts[calls[4][0]][warmup:]))
            rows.append(dict(mask=mask_name, call="write(SPZ): payload + gzip member", count=int(count), ms=float(np.median(t)),
                             ms_min=float(t.min()), ms_max=float(t.max()), gzip_share=1.0 - payload_ms / float(np.median(t))))
    sel.destroy(); buf.destroy(); stream.close()
    return dict(workload=name, n=n, iters=iters, warmup=warmup, gzip_iters=gzip_iters, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gzip-iters", type=int, default=3)
    ap.add_argument("--workloads", default="1m,10m")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    results = []
    for name in a.workloads.split(","):
        results.append(run(gs, name, WORKLOADS[name], a.iters, a.warmup, a.gzip_iters))
        print(json.dumps(results[-1]), flush=True)
    print("| scene | mask | call | records | ms (min .. max) | PLY GB/s delivered (plain copy) | gzip share |")
    print("|---|---|---|---|---|---|---|")
    for res in results:
        for r in res["rows"]:
            rate = "%.1f (%.1f)" % (r["delivered_gbps"], r["copy_gbps"]) if "delivered_gbps" in r else ""
            share = "%.0f %%" % (100 * r["gzip_share"]) if "gzip_share" in r else ""
            print("| %s | %s | %s | %d | %.1f (%.1f .. %.1f) | %s | %s |" % (res["workload"], r["mask"], r["call"], r["count"], r["ms"],
                                                                          r["ms_min"], r["ms_max"], rate, share))


if __name__ == "__main__":
    main()
