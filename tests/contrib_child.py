"""Child process of tests/test_gpu_contrib.py — NOT collected by pytest.

    python tests/contrib_child.py OUT.npy

Renders scene A (tests/contrib_np.py) as a contribution frame in the three display modes, in a FRESH process — the
GS3D_BLEND_GROUPS switch is read once per process — and writes the three record arrays, stacked, to OUT.npy.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    import contrib_np
    import gpu_child
    import helpers
    with gpu_child.child_rig() as (gs, ob, dev, stream):      # (ob: only its look-at helper — the camera is the oracle's, bit for bit)
        W, H = contrib_np.SCENE_A_SIZE
        pod = gs.GaussianPod(gs.SH_NONE, gs.COV3D_ROT_SCALE)
        pods = pod.from_gaussian(contrib_np.scene_a())
        buf = gs.GaussiansBuffer.new_with_pods(dev, pod, pods)
        n = buf.len()
        cam = helpers.copy_camera(helpers.default_camera(ob, W, H), gs.Camera)
        mt = gs.model_transform_pod((0, 0, 0), (0, 0, 0, 1), (1, 1, 1))
        img = gs.Buffer(dev, size=W * H * 16)
        out = []
        for mode in (0, 1, 2):
            gt = gs.gaussian_transform_pod(1.0, mode, 0, False, 3.0)
            c = gs.Contributions.new(dev, stream, n)
            r = gs.Renderer(dev)
            r.render(stream, buf, gt, mt, cam, img.device_ptr(), contributions=c)
            out.append(c.download(stream).copy())
            r.destroy()
            c.release()
        np.save(sys.argv[1], np.stack(out))
        img.release()
        buf.destroy()
    print("contrib_child OK")


if __name__ == "__main__":
    main()
