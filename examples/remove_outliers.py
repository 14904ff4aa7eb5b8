#!/usr/bin/env python3
"""Remove the statistical outliers of a scene (gs_gaussians_buffer_knn, gs_knn_summary, gs_select_knn): the
Gaussians whose mean distance to their k nearest neighbours lies above mean + sigma x std over the scene — the floater filter
of PCL / Open3D, which needs no radius guess.  Everything runs on the device; the scene is downloaded once, as the cleaned
file.  It also prints the median distance to the k-th neighbour: the radius to start from with select_neighbors,
components (examples/remove_small_clusters.py) or simplify.
usage: python examples/remove_outliers.py tests/golden/model.ply cleaned.ply [--k 8] [--sigma 2.0]
       [--pod ShSingle/Cov3dRotScale] [--fast-save]                                 (needs a GPU: there is no CPU fallback)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_3dgs_core_amd as gs  # noqa: E402


def median_kth_distance(dev, stream, dist2, n, k):
    """the median over the complete rows of the distance to the k-th neighbour, found on the device: a bisection on the bit
    pattern of d2 (the order of the bits is the order of the values) with select_knn + count, 31 small calls and no download"""
    s = gs.knn_summary(stream, dist2, n, k, gs.KNN_KTH_DIST2)
    if not s.complete:
        return float("nan")
    sel = gs.Selection(dev, n)
    lo, hi = int(np.float32(s.min).view(np.uint32)), int(np.float32(s.max).view(np.uint32))
    while lo < hi:      # the smallest value with at least half of the complete rows at or below it
        mid = (lo + hi) // 2
        sel.select_knn(stream, dist2, k, gs.KNN_KTH_DIST2, 0.0, float(np.uint32(mid).view(np.float32)))
        if 2 * sel.count(stream) >= s.complete:
            hi = mid
        else:
            lo = mid + 1
    sel.destroy()
    return float(np.sqrt(np.float64(np.uint32(lo).view(np.float32))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=2.0)
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
    n = buf.len()
    dist2, index, radius, passes = buf.knn_auto(stream, args.k)
    s = gs.knn_summary(stream, dist2, n, args.k, gs.KNN_MEAN_DIST)
    print("%d Gaussians, %d with a finite position, %d with %d neighbours within %g (%d passes)" % (n, s.points, s.complete, args.k, radius, passes))
    print("mean distance to the %d nearest: mean %g, std %g, min %g, max %g" % (args.k, s.mean, s.std, s.min, s.max))
    print("median distance to neighbour %d: %g  <- a radius for select_neighbors / components / simplify" %
          (args.k, median_kth_distance(dev, stream, dist2, n, args.k)))
    dist2.release(); index.release()
    outliers = gs.Selection(dev, n)
    threshold, _ = outliers.select_statistical_outliers(stream, buf, k=args.k, sigma=args.sigma)
    removed = outliers.count(stream)
    kept = buf.extract(stream, outliers, invert=True)      # (a Gaussian without a finite position is no point and stays)
    kept.write_to_file(args.out, stream, fast=args.fast_save)
    print("%d Gaussians with a mean distance above %g (mean + %g std) removed, %d kept -> %s" % (removed, threshold, args.sigma, kept.len(), args.out))


if __name__ == "__main__":
    main()
