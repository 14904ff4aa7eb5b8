#!/usr/bin/env python3
"""Render an Inria-style .ply (or an .spz) with the MI355X path and write a PPM — the counterpart of the
reference's examples/read_ply.rs / read_spz.rs followed by one frame of the viewer.
usage: python examples/render_ply.py tests/golden/model.ply out.ppm [--size 960x540] [--eye 0,0,4]
       [--mode splat|ellipse|point] [--pod ShHalf/Cov3dHalf]          (needs a GPU: there is no CPU fallback)
       [--depth depth.pgm] [--pick X,Y]   the frame's depth plane (expected depth, 16-bit PGM) / the Gaussian under a pixel
       [--stats]                          count, bounds and centroid from gs_gaussians_buffer_stats"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_3dgs_core_amd as gs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--size", default="960x540")
    ap.add_argument("--eye", default="0,0,4")
    ap.add_argument("--target", default="0,0,0")
    ap.add_argument("--mode", default="splat", choices=["splat", "ellipse", "point"])
    ap.add_argument("--pod", default="ShSingle/Cov3dRotScale")
    ap.add_argument("--depth", help="write the expected depth (depth / alpha) as a 16-bit PGM, near = dark")
    ap.add_argument("--pick", help="X,Y: print the index and record of the Gaussian picked at that pixel (median contributor)")
    ap.add_argument("--crop", nargs=6, type=float, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="hide what lies outside this axis-aligned box (a device selection: the data is left alone)")
    ap.add_argument("--stats", action="store_true",
                    help="print count, bounds and centroid of the Gaussians (of those the crop keeps), computed on the device")
    args = ap.parse_args()
    sh, cov = args.pod.split("/")
    pod = getattr(gs, "GaussianPodWith%s%sConfigs" % (sh, cov))
    W, H = (int(v) for v in args.size.split("x"))
    dev = gs.Device(0)
    stream = dev.create_stream()
    # the device-side load path: the file's records cross PCIe as they are; from_ply / from_spz and the
    # pack to the POD layout run in one kernel (gs_gaussians_buffer_create_from_ply / _from_spz)
    if args.scene.endswith(".spz"):
        buf = gs.GaussiansBuffer.new_from_spz(dev, pod, open(args.scene, "rb").read())
    else:
        buf = gs.GaussiansBuffer.new_from_ply(dev, pod, gs.PlyGaussians.read_from_file(args.scene))
    img = gs.Buffer(dev, size=W * H * 16)
    cam = gs.camera_look_at(tuple(float(v) for v in args.eye.split(",")), tuple(float(v) for v in args.target.split(",")),
                            (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    mode = {"splat": gs.DISPLAY_SPLAT, "ellipse": gs.DISPLAY_ELLIPSE, "point": gs.DISPLAY_POINT}[args.mode]
    r = gs.Renderer(dev)
    aux = args.depth or args.pick
    depth = gs.Buffer(dev, size=W * H * 4) if aux else None
    pick = gs.Buffer(dev, size=W * H * 4) if aux else None
    hide = None
    if args.crop:
        hide = gs.Selection(dev, len(buf))
        hide.select_box(stream, buf, gs.model_transform_pod(), gs.box_from_bounds(args.crop[:3], args.crop[3:]))
        hide.invert(stream)
        print("crop: %d of %d Gaussians hidden" % (hide.count(stream), len(buf)))
    if args.stats:
        kept = None
        if hide is not None:
            kept = gs.Selection(dev, len(buf))
            kept.combine(stream, "set", hide)
            kept.invert(stream)
        s = buf.stats(stream, kept)
        lo, hi = s.bounds
        print("stats: %d Gaussians, bounds (%.4g, %.4g, %.4g) .. (%.4g, %.4g, %.4g), centroid (%.4g, %.4g, %.4g)"
              % ((s.count,) + tuple(lo) + tuple(hi) + tuple(s.centroid)))
    r.render(stream, buf, gs.gaussian_transform_pod(1.0, mode, 3, False, 3.0), gs.model_transform_pod(), cam,
             img.device_ptr(), depth_device_ptr=depth.device_ptr() if aux else None,
             pick_device_ptr=pick.device_ptr() if aux else None, hide=hide)
    rgba = img.download(stream, np.float32).reshape(H, W, 4)
    st = r.stats()
    rgb8 = (np.clip(rgba[..., :3], 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    with open(args.out, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (W, H))
        f.write(rgb8.tobytes())
    print("%d Gaussians, %d visible, %d (tile, Gaussian) pairs -> %s" % (len(buf), st.visible, st.pairs, args.out))
    if args.depth:
        alpha = rgba[..., 3]
        z = np.where(alpha > 0.0, depth.download(stream, np.float32).reshape(H, W) / np.maximum(alpha, 1e-30), 0.0)
        seen = alpha > 0.0
        lo, hi = (float(z[seen].min()), float(z[seen].max())) if seen.any() else (0.0, 1.0)
        q = np.where(seen, (z - lo) / max(hi - lo, 1e-30) * 65534.0 + 1.0, 0.0)   # 0 = nothing there
        with open(args.depth, "wb") as f:
            f.write(b"P5\n%d %d\n65535\n" % (W, H))
            f.write(np.clip(q, 0, 65535).astype(">u2").tobytes())
        print("depth %.4g .. %.4g -> %s" % (lo, hi, args.depth))
    if args.pick:
        x, y = (int(v) for v in args.pick.split(","))
        i = int(pick.download(stream, np.uint32).reshape(H, W)[y, x])
        if i == gs.PICK_NONE:
            print("pick (%d, %d): nothing" % (x, y))
        else:
            # the one record, through a non-owning view of the buffer's memory
            view = gs.Buffer.from_raw(dev, buf.buffer().device_ptr() + i * pod.size, pod.size)
            rec = view.download(stream)
            view.release()
            print("pick (%d, %d): Gaussian %d" % (x, y, i), pod.into_gaussian(rec)[0])


if __name__ == "__main__":
    main()
