#!/usr/bin/env python3
"""Align one scan onto another and merge them without the doubled layer (gs_gaussians_buffer_knn_between,
gs_gaussians_buffer_pair_sums, gs_rigid_fit).  ICP (GaussiansBuffer.align_to) finds the transform that
brings scan A onto scan B, iterating on A's model transform without touching a record; the transform is baked into A with
one edit (SH rotated); the Gaussians of A that then have a counterpart in B within the overlap radius are dropped
(Selection.select_near, extract inverted) and the rest is concatenated behind B in B's layout.  The Chamfer distance
between the scans is printed before and after.  Everything runs on the device; the result is downloaded once, as the file.
--subsample K: a random selection of about one Gaussian of A in K is the query set of the ICP; --first N: the first N are
(a range selection).  The overlap select and the Chamfer distances always take all of A.
usage: python examples/align_scans.py a.ply b.ply merged.ply --radius 0.1 [--overlap 0.02] [--scale] [--subsample 4]
       [--first N] [--iterations 32] [--pod ShSingle/Cov3dRotScale] [--fast-save]   (needs a GPU: there is no CPU fallback)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_3dgs_core_amd as gs  # noqa: E402


def load(dev, pod, path):
    if path.endswith(".spz"):
        return gs.GaussiansBuffer.new_from_spz(dev, pod, open(path, "rb").read())
    return gs.GaussiansBuffer.new_from_ply(dev, pod, gs.PlyGaussians.read_from_file(path))


def show(title, ch):
    print("%s: A -> B mean %g (%d without a neighbour), B -> A mean %g (%d without), Chamfer %g" %
          (title, ch.mean_to, ch.incomplete_to, ch.mean_from, ch.incomplete_from, ch.distance))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("out")
    ap.add_argument("--radius", type=float, required=True, help="the largest distance at which a Gaussian of A is paired with one of B")
    ap.add_argument("--overlap", type=float, default=None, help="a Gaussian of A this close to one of B is dropped (default: radius / 4)")
    ap.add_argument("--scale", action="store_true", help="fit a uniform scale too")
    ap.add_argument("--subsample", type=int, default=1)
    ap.add_argument("--first", type=int, default=None)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--pod", default="ShSingle/Cov3dRotScale")
    ap.add_argument("--fast-save", action="store_true")
    args = ap.parse_args()
    sh, cov = args.pod.split("/")
    pod = getattr(gs, "GaussianPodWith%s%sConfigs" % (sh, cov))
    dev = gs.Device(0)
    stream = dev.create_stream()
    a, b = load(dev, pod, args.a), load(dev, pod, args.b)
    overlap = args.overlap if args.overlap is not None else args.radius / 4
    print("A: %d Gaussians, B: %d" % (a.len(), b.len()))
    show("before", a.chamfer_to(stream, b, args.radius))

    queries = None
    if args.first is not None or args.subsample > 1:
        queries = gs.Selection(dev, a.len())
        if args.first is not None:
            queries.select_range(stream, 0, min(args.first, a.len()))
        else:
            queries.upload(stream, np.random.default_rng(0).random(a.len()) < 1.0 / args.subsample)
        print("%d of A's Gaussians are queries of the ICP" % queries.count(stream))
    pod_ab, report = a.align_to(stream, b, args.radius, queries=queries, scale=args.scale, max_iterations=args.iterations)
    for it, (pairs, rms) in enumerate(report.iterations):
        print("iteration %2d: %d pairs, RMS %g" % (it + 1, pairs, rms))
    print("stopped: %s; position %s, rotation (xyzw) %s, scale %g" %
          (report.stopped, [round(v, 6) for v in pod_ab.pos], [round(v, 6) for v in pod_ab.rot], pod_ab.scale[0]))
    # the same transform as a model transform of A's frames would do for viewing; for the merge it is baked
    a.edit(stream, None, gs.edit(transform=pod_ab, rotate_sh=True))
    show("after", a.chamfer_to(stream, b, args.radius))

    doubled = gs.Selection(dev, a.len())
    doubled.select_near(stream, a, b, overlap)
    dropped = doubled.count(stream)
    rest = a.extract(stream, doubled, invert=True)
    merged, counts = gs.GaussiansBuffer.concat(stream, [b, rest], pod=b.pod)
    merged.write_to_file(args.out, stream, fast=args.fast_save)
    print("%d Gaussians of A within %g of B dropped; %d of B + %d of A -> %s" % (dropped, overlap, counts[0], counts[1], args.out))


if __name__ == "__main__":
    main()
