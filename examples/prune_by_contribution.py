#!/usr/bin/env python3
"""Prune a scene by what its Gaussians do to the pictures: accumulate the per-Gaussian contribution scores
(gs_render_frame_contrib) over an orbit of views, select the Gaussians whose summed blending weight
stays below a threshold, extract the others and write them — all on the device; the scene is downloaded once, as the
pruned file.
usage: python examples/prune_by_contribution.py tests/golden/model.ply pruned.ply [--views 24] [--radius 4] [--height 0.5]
       [--size 640x360] [--threshold 0.5] [--pod ShSingle/Cov3dRotScale] [--report-quality] [--fast-save]
                                                                                   (needs a GPU: there is no CPU fallback)
       threshold: in units of "fully covered pixels", summed over all views (1.0 = the weight of one opaque pixel in one view);
       0 removes exactly the Gaussians no view blended.
       --report-quality: renders the orbit's views again from the original and from the pruned buffer and prints PSNR and
       SSIM per view and their means (gs_image_compare); no image is downloaded.
       --fast-save: an .spz result is deflated on the device (Huffman only, no zlib; every .spz reader opens
       it); a .ply result is the same either way."""
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
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--height", type=float, default=0.5)
    ap.add_argument("--target", default="0,0,0")
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--pod", default="ShSingle/Cov3dRotScale")
    ap.add_argument("--report-quality", action="store_true")
    ap.add_argument("--fast-save", action="store_true")
    args = ap.parse_args()
    sh, cov = args.pod.split("/")
    pod = getattr(gs, "GaussianPodWith%s%sConfigs" % (sh, cov))
    W, H = (int(v) for v in args.size.split("x"))
    dev = gs.Device(0)
    stream = dev.create_stream()
    if args.scene.endswith(".spz"):
        buf = gs.GaussiansBuffer.new_from_spz(dev, pod, open(args.scene, "rb").read())
    else:
        buf = gs.GaussiansBuffer.new_from_ply(dev, pod, gs.PlyGaussians.read_from_file(args.scene))
    n = len(buf)
    target = tuple(float(v) for v in args.target.split(","))
    img = gs.Buffer(dev, size=W * H * 16)
    scores = gs.Contributions.new(dev, stream, n)
    r = gs.Renderer(dev)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()

    def camera(k):
        a = 2.0 * np.pi * k / args.views
        eye = (target[0] + args.radius * np.sin(a), target[1] + args.height, target[2] + args.radius * np.cos(a))
        return gs.camera_look_at(eye, target, (0, 1, 0), float(np.deg2rad(60.0)), W, H)

    for k in range(args.views):
        r.render(stream, buf, gt, mt, camera(k), img.device_ptr(), contributions=scores)      # accumulates; never clears
    low = gs.Selection(dev, n)
    if args.threshold > 0.0:
        scores.select(stream, low, gs.CONTRIB_SUM, 0.0, args.threshold)
    else:
        scores.select(stream, low, gs.CONTRIB_HITS, 0.0, 0.0)
    removed = low.count(stream)
    kept = buf.extract(stream, low, invert=True)
    kept.write_to_file(args.out, stream, fast=args.fast_save)
    rec = scores.download(stream)
    print("%d Gaussians, %d views: %d never blended, %d below %g -> %d kept -> %s" % (
        n, args.views, int((rec["hits"] == 0).sum()), removed, args.threshold, len(kept), args.out))
    if args.report_quality:
        # what the pruning cost: every view of the orbit from both buffers, compared where the images are (gs_image_compare,
        # DESIGN.md §3.14); only the 176-byte record of each view comes back
        img2 = gs.Buffer(dev, size=W * H * 16)
        psnr, ssim = [], []
        for k in range(args.views):
            r.render(stream, buf, gt, mt, camera(k), img.device_ptr())
            r.render(stream, kept, gt, mt, camera(k), img2.device_ptr())
            m = gs.image_compare(dev, stream, img.device_ptr(), img2.device_ptr(), W, H, ssim=True)
            psnr.append(m.psnr())
            ssim.append(m.ssim)
            print("view %2d: PSNR %s dB  SSIM %.6f  %d of %d pixels differ, max |d| %.4g" % (
                k, "inf" if m.identical or np.isinf(psnr[-1]) else "%.2f" % psnr[-1], ssim[-1], m.differing, m.pixels, float(m.max_abs[:3].max())))
        finite = [p for p in psnr if np.isfinite(p)]
        print("mean over %d views: PSNR %s dB (%d views unchanged)  SSIM %.6f" % (
            args.views, "%.2f" % np.mean(finite) if finite else "inf", len(psnr) - len(finite), float(np.mean(ssim))))


if __name__ == "__main__":
    main()
