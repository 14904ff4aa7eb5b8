"""The depth and pick planes of a frame (gs_render_frame_aux) for the tests that render them: the poisoned
targets, the depth plane's definition on the oracle, and the float64 witness of the pick plane."""
import numpy as np

from helpers import POISON

POISON_DEPTH = np.float32(np.nan)
POISON_PICK = np.uint32(0xDEADBEEF)


class Planes:
    """an RGBA target and the two aux planes of one image, poisoned"""

    def __init__(self, gs, device, W, H):
        self.W, self.H = W, H
        self.img = gs.Buffer(device, data=np.full(H * W * 4, POISON))
        self.depth = gs.Buffer(device, data=np.full(H * W, POISON_DEPTH, dtype=np.float32))
        self.pick = gs.Buffer(device, data=np.full(H * W, POISON_PICK, dtype=np.uint32))

    def poison(self, stream, image=False):
        if image:       # a target that one renderer fills frame after frame
            self.img.write(stream, 0, np.full(self.H * self.W * 4, POISON))
        self.depth.write(stream, 0, np.full(self.H * self.W, POISON_DEPTH, dtype=np.float32))
        self.pick.write(stream, 0, np.full(self.H * self.W, POISON_PICK, dtype=np.uint32))
        stream.synchronize()

    def render(self, r, stream, buf, gt, mt, cam, band=None, threshold=0.5, check=True):
        fr = r.render(stream, buf, gt, mt, cam, self.img.device_ptr(), band=band, check=check,
                      depth_device_ptr=self.depth.device_ptr(), pick_device_ptr=self.pick.device_ptr(),
                      pick_threshold=threshold)
        stream.synchronize()
        return fr

    def get(self, stream):
        return (self.img.download(stream, np.float32).reshape(self.H, self.W, 4).copy(),
                self.depth.download(stream, np.float32).reshape(self.H, self.W).copy(),
                self.pick.download(stream, np.uint32).reshape(self.H, self.W).copy())

    def release(self):
        for b in (self.img, self.depth, self.pick):
            b.release()


def oracle_depth(ob, proj, sidx, ranges, ocam, ogt, band=None):
    """the depth plane's definition: the oracle blend's R channel with r := z', g = b = 0, background 0"""
    p = proj.copy()
    p["r"] = p["depth"]
    p["g"] = 0.0
    p["b"] = 0.0
    cam0 = ob.Camera.from_buffer_copy(bytes(ocam))
    cam0.background[:] = [0.0, 0.0, 0.0]
    return ob.blend(p, sidx, ranges, cam0, band=band, gt=ogt)[..., 0]


def pick_witness(proj, sidx, ranges, W, H, tiles_x, tcut64, rel=1e-5):
    """float64 walk of every pixel's tile list (splat mode): the first splat whose step takes T to <= tcut; also
    whether any decision up to there lies within `rel` of its boundary.  Returns (pick, ambiguous)."""
    NONE = 0xFFFFFFFF
    pick = np.full((H, W), NONE, dtype=np.uint64)
    amb = np.zeros((H, W), bool)
    p = {k: proj[k].astype(np.float64) for k in ("mx", "my", "ca", "cb", "cc", "opacity")}
    for t in range(ranges.shape[0]):
        s, e = int(ranges[t, 0]), int(ranges[t, 1])
        if e <= s:
            continue
        tx, ty = t % tiles_x, t // tiles_x
        xs = np.arange(tx * 16, min(tx * 16 + 16, W))
        ys = np.arange(ty * 16, min(ty * 16 + 16, H))
        if not len(xs) or not len(ys):
            continue
        px, py = np.meshgrid(xs + 0.5, ys + 0.5)
        px, py = px.ravel(), py.ravel()
        T = np.ones(px.shape)
        live = np.ones(px.shape, bool)
        got = np.full(px.shape, NONE, dtype=np.uint64)
        am = np.zeros(px.shape, bool)
        for j in range(s, e):
            g = int(sidx[j])
            dx, dy = p["mx"][g] - px, p["my"][g] - py
            a, b, c = p["ca"][g] * dx * dx, p["cb"][g] * dx * dy, p["cc"][g] * dy * dy
            power = a + b + c
            scale = np.abs(a) + np.abs(b) + np.abs(c)
            alpha = np.minimum(0.99, p["opacity"][g] * np.exp(power))
            act = live & (power <= 0.0) & (alpha >= 1.0 / 255.0)
            am |= live & ((np.abs(power) <= rel * scale) | (np.abs(alpha - 1.0 / 255.0) <= rel / 255.0))
            Tn = T * (1.0 - alpha)
            am |= act & ((np.abs(Tn - 1e-4) <= rel * 1e-4) | (np.abs(Tn - tcut64) <= rel * tcut64))
            fin = act & (Tn < 1e-4)
            blend = act & ~fin
            hit = blend & (Tn <= tcut64) & (got == NONE)
            got[hit] = g
            T = np.where(blend, Tn, T)
            live &= ~fin & (got == NONE)
            if not live.any():
                break
        pick[py.astype(int), px.astype(int)] = got
        amb[py.astype(int), px.astype(int)] = am
    return pick, amb
