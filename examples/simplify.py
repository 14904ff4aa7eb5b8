#!/usr/bin/env python3
"""Write a level-of-detail pyramid of a scene: three simplified copies (gs_gaussians_buffer_create_simplified, DESIGN.md
§3.17) whose cell size doubles from a given fraction of the scene's extent — all on the device; each level is downloaded
once, as its file.
usage: python examples/simplify.py tests/golden/model.ply out_prefix [--fraction 0.01] [--ext ply] [--pod ShSingle/Cov3dRotScale]
       [--report-quality] [--views 12] [--radius 4] [--height 0.5] [--target 0,0,0] [--size 640x360] [--fast-save]
                                                                                   (needs a GPU: there is no CPU fallback)
       writes out_prefix_lod1.<ext>, _lod2, _lod3 with cells of fraction, 2 fraction and 4 fraction of the largest side of the
       bounding box of the positions (gs_gaussians_buffer_stats).
       --report-quality: prints each level's count, bytes on the device and PSNR / SSIM against the full scene over an orbit of
       views, compared where the images are (gs_image_compare); no image is downloaded.  A report, not a test."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_3dgs_core_amd as gs  # noqa: E402

LEVELS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out_prefix")
    ap.add_argument("--fraction", type=float, default=0.01)
    ap.add_argument("--ext", default="ply", choices=("ply", "spz"))
    ap.add_argument("--pod", default="ShSingle/Cov3dRotScale")
    ap.add_argument("--report-quality", action="store_true")
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--height", type=float, default=0.5)
    ap.add_argument("--target", default="0,0,0")
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--fast-save", action="store_true")
    args = ap.parse_args()
    sh, cov = args.pod.split("/")
    pod = getattr(gs, "GaussianPodWith%s%sConfigs" % (sh, cov))
    dev = gs.Device(0)
    stream = dev.create_stream()
    if args.scene.endswith(".spz"):
        buf = gs.GaussiansBuffer.new_from_spz(dev, pod, open(args.scene, "rb").read())
    else:
        buf = gs.GaussiansBuffer.new_from_ply(dev, pod, gs.PlyGaussians.read_from_file(args.scene))
    n = len(buf)
    st = buf.stats(stream)
    extent = float(max(st.max[a] - st.min[a] for a in (gs.ATTR_X, gs.ATTR_Y, gs.ATTR_Z)))
    if not np.isfinite(extent) or extent <= 0.0:
        sys.exit("the scene has no extent: nothing to simplify")
    levels = []
    for k in range(LEVELS):
        cell = args.fraction * extent * 2 ** k
        # a covariance layout cannot be saved as it is: a rotation + scale pod of the same SH config can, and every layout is a
        # valid target of the merge
        out_pod = gs.GaussianPod(pod.sh, gs.COV3D_ROT_SCALE)
        lod = buf.simplify(stream, cell, out_pod)
        path = "%s_lod%d.%s" % (args.out_prefix, k + 1, args.ext)
        lod.write_to_file(path, stream, fast=args.fast_save)
        levels.append((cell, lod, path))
        print("level %d: cell %.6g (%.4g of the extent): %d -> %d Gaussians (%.1f : 1), %d bytes on the device -> %s" % (
            k + 1, cell, cell / extent, n, len(lod), n / max(len(lod), 1), len(lod) * out_pod.size, path))
    if args.report_quality:
        W, H = (int(v) for v in args.size.split("x"))
        target = tuple(float(v) for v in args.target.split(","))
        img, img2 = gs.Buffer(dev, size=W * H * 16), gs.Buffer(dev, size=W * H * 16)
        r_full, r_lod = gs.Renderer(dev), gs.Renderer(dev)
        gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()

        def camera(k):
            a = 2.0 * np.pi * k / args.views
            eye = (target[0] + args.radius * np.sin(a), target[1] + args.height, target[2] + args.radius * np.cos(a))
            return gs.camera_look_at(eye, target, (0, 1, 0), float(np.deg2rad(60.0)), W, H)

        for k, (cell, lod, path) in enumerate(levels):
            psnr, ssim = [], []
            for v in range(args.views):
                r_full.render(stream, buf, gt, mt, camera(v), img.device_ptr())
                r_lod.render(stream, lod, gt, mt, camera(v), img2.device_ptr())
                m = gs.image_compare(dev, stream, img.device_ptr(), img2.device_ptr(), W, H, ssim=True)
                psnr.append(m.psnr())
                ssim.append(m.ssim)
            finite = [p for p in psnr if np.isfinite(p)]
            print("level %d: %d Gaussians, %d bytes: mean over %d views PSNR %s dB (%d views unchanged)  SSIM %.6f" % (
                k + 1, len(lod), len(lod) * lod.pod.size, args.views, "%.2f" % np.mean(finite) if finite else "inf",
                len(psnr) - len(finite), float(np.mean(ssim))))


if __name__ == "__main__":
    main()
