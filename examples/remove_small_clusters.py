#!/usr/bin/env python3
"""Remove the small clusters of a scene: the connected components of the neighbour graph within a radius
(gs_gaussians_buffer_components, gs_select_components) — the floater clumps whose members have plenty of
neighbours each and survive every neighbour-count threshold.  Everything runs on the device; the scene is downloaded once,
as the cleaned file.
usage: python examples/remove_small_clusters.py tests/golden/model.ply cleaned.ply [--radius 0.05] [--min-size 50]
       [--pod ShSingle/Cov3dRotScale] [--fast-save]                                 (needs a GPU: there is no CPU fallback)
       radius: two Gaussians closer than this belong to one cluster; min-size: every cluster with fewer Gaussians goes."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_3dgs_core_amd as gs  # noqa: E402


def info_of(buf, stream, radius):
    labels, sizes, info = buf.components(stream, radius)
    rec = np.asarray(info.download(stream, np.uint32))[:4].view(gs.COMPONENTS_INFO_DTYPE)[0]
    for b in (labels, sizes, info):
        b.release()
    return "%d points in %d clusters, the largest of %d (label %d)" % (rec["points"], rec["components"], rec["largest"], rec["largest_label"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--min-size", type=int, default=50)
    ap.add_argument("--pod", default="ShSingle/Cov3dRotScale")
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
    print("before: %d Gaussians, %s" % (n, info_of(buf, stream, args.radius)))
    small = gs.Selection(dev, n)
    if args.min_size > 1:
        small.select_components(stream, buf, args.radius, max_size=args.min_size - 1)
    removed = small.count(stream)
    kept = buf.extract(stream, small, invert=True)      # (a Gaussian without a finite position is no point and stays)
    print("after:  %d Gaussians, %s" % (len(kept), info_of(kept, stream, args.radius)))
    kept.write_to_file(args.out, stream, fast=args.fast_save)
    print("%d Gaussians in clusters smaller than %d within %g removed -> %s" % (removed, args.min_size, args.radius, args.out))


if __name__ == "__main__":
    main()
