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

--rows deflate (or all) adds the fast gzip member of DESIGN.md §3.15: write(SPZ, fast), Buffer.gzip_fast of the payload
resident on the device and the host encoder gs_gzip_fast, next to write(SPZ) — zlib, this build's untouched path — of the
same run, with the speed-up, the member's size over zlib's and the call's time over a plain device-to-host copy of as many
bytes as the member has.  The kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/export_bench.py --rows deflate --workloads 10m --iters 3 --gzip-iters 0

    python tools/export_bench.py [--iters 15] [--warmup 2] [--gzip-iters 3] [--workloads 1m,10m] [--rows export|deflate|all]
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


def deflate_rows(gs, dev, stream, buf, mask_name, s, count, payload, iters, warmup, gzip_iters):
    """The fast gzip member next to zlib's in the same run: write(SPZ, fast), Buffer.gzip_fast of the payload
    resident on the device and the host encoder gs_gzip_fast, alternating inside every repeat; write(SPZ) — zlib on one host
    thread, this build's untouched path — is the baseline (`gzip_iters` repeats); the yardstick is a plain device-to-host
    copy of as many bytes as the fast member has."""
    resident = gs.Buffer(dev, data=np.frombuffer(payload, np.uint8))
    calls = [("write(SPZ, fast): payload + member on the device", lambda: buf.write(stream, gs.GaussiansSource.Spz, s, fast=True)),
             ("Buffer.gzip_fast of the resident payload", lambda: resident.gzip_fast(stream)),
             ("host gs_gzip_fast of the payload", lambda: gs.gzip_fast(payload))]
    ts = {label: [] for label, _ in calls}
    sizes = {}
    for _ in range(warmup + iters):
        for label, fn in calls:
            ms, out = _timed(fn, stream)
            ts[label].append(ms)
            sizes[label] = len(out)
            del out
    assert len(set(sizes.values())) == 1, sizes
    member = sizes[calls[0][0]]
    resident.release()
    raw = gs.Buffer(dev, size=member)
    copy_ms = [_timed(lambda: raw.download(stream, np.uint8), stream)[0] for _ in range(warmup + iters)]
    raw.release()
    copy = float(np.median(copy_ms[warmup:]))
    zl, zl_bytes = [], 0
    for _ in range(gzip_iters):
        ms, out = _timed(lambda: buf.write(stream, gs.GaussiansSource.Spz, s), stream)
        zl.append(ms)
        zl_bytes = len(out)
        del out
    rows = []
    if zl:
        rows.append(dict(mask=mask_name, call="write(SPZ): payload + zlib member (baseline)", count=int(count), bytes=int(zl_bytes),
                         ms=float(np.median(zl)), ms_min=float(min(zl)), ms_max=float(max(zl)), payload_bytes=len(payload)))
    for label, _ in calls:
        t = np.array(ts[label][warmup:])
        row = dict(mask=mask_name, call=label, count=int(count), bytes=int(member), ms=float(np.median(t)), ms_min=float(t.min()),
                   ms_max=float(t.max()), payload_bytes=len(payload), copy_ms=copy, over_copy=float(np.median(t)) / copy)
        if zl:
            row["speedup_over_zlib"] = float(np.median(zl)) / row["ms"]
            row["size_over_zlib"] = member / zl_bytes
        rows.append(row)
    return rows


def run(gs, name, n, iters, warmup, gzip_iters, which="all"):
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
    if which == "deflate":
        rows = []
        for mask_name, s, count in (("all", None, n), ("30 %", sel, count30)):
            payload = gs._sized_call(gs._L.gs_gaussians_buffer_export_spz_decompressed, buf._h, stream._h, s._h if s is not None else None, 0,
                                     C.byref(opt))
            rows += deflate_rows(gs, dev, stream, buf, mask_name, s, count, payload, iters, warmup, gzip_iters)
        sel.destroy(); buf.destroy(); stream.close()
        return dict(workload=name, n=n, iters=iters, warmup=warmup, gzip_iters=gzip_iters, rows=rows)

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
        if which == "all":
            rows += deflate_rows(gs, dev, stream, buf, mask_name, s, count, device_spz(s), iters, warmup, gzip_iters)
    sel.destroy(); buf.destroy(); stream.close()
    return dict(workload=name, n=n, iters=iters, warmup=warmup, gzip_iters=gzip_iters, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gzip-iters", type=int, default=3)
    ap.add_argument("--workloads", default="1m,10m")
    ap.add_argument("--rows", default="export", choices=("export", "deflate", "all"),
                    help="export: the rows of DESIGN.md 3.13; deflate: the fast gzip member of 3.15 next to zlib's; all: both")
    a = ap.parse_args()
    import wgpu_3dgs_core_amd as gs
    results = []
    for name in a.workloads.split(","):
        results.append(run(gs, name, WORKLOADS[name], a.iters, a.warmup, a.gzip_iters, a.rows))
        print(json.dumps(results[-1]), flush=True)
    if a.rows != "export":
        print("| scene | mask | call | records | member bytes (of payload) | ms (min .. max) | x zlib time | size / zlib | time / plain copy of the member |")
        print("|---|---|---|---|---|---|---|---|---|")
        for res in results:
            for r in res["rows"]:
                if "payload_bytes" not in r:
                    continue
                print("| %s | %s | %s | %d | %d (%.4f) | %.1f (%.1f .. %.1f) | %s | %s | %s |" % (
                    res["workload"], r["mask"], r["call"], r["count"], r["bytes"], r["bytes"] / r["payload_bytes"], r["ms"], r["ms_min"], r["ms_max"],
                    "%.0f" % r["speedup_over_zlib"] if "speedup_over_zlib" in r else "", "%.4f" % r["size_over_zlib"] if "size_over_zlib" in r else "",
                    "%.2f (copy %.1f ms)" % (r["over_copy"], r["copy_ms"]) if "over_copy" in r else ""))
        if a.rows == "deflate":
            return
    print("| scene | mask | call | records | ms (min .. max) | PLY GB/s delivered (plain copy) | gzip share |")
    print("|---|---|---|---|---|---|---|")
    for res in results:
        for r in res["rows"]:
            if "payload_bytes" in r:
                continue
            rate = "%.1f (%.1f)" % (r["delivered_gbps"], r["copy_gbps"]) if "delivered_gbps" in r else ""
            share = "%.0f %%" % (100 * r["gzip_share"]) if "gzip_share" in r else ""
            print("| %s | %s | %s | %d | %.1f (%.1f .. %.1f) | %s | %s |" % (res["workload"], r["mask"], r["call"], r["count"], r["ms"],
                                                                          r["ms_min"], r["ms_max"], rate, share))


if __name__ == "__main__":
    main()
