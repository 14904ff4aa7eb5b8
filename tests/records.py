"""What the record tests share: rows of bytes and where two sets of them differ, a selection from a mask, the select ops in
numpy, and the one edit (tests/edit_np.py restates it) that the edit, snapshot, statistics and neighbour tests apply."""
import numpy as np

import edit_np

f32 = np.float32
SELECT_OPS = ["set", "or", "and", "andnot", "xor"]      # gs.SEL_SET .. gs.SEL_XOR are their indices
Q = np.array([0.3, -0.5, 0.2, 0.7])
Q = tuple((Q / np.linalg.norm(Q)).astype(f32))
POS, SCALE = (0.5, -0.25, 1.5), 1.25
# a non-trivial colour matrix (column-major 3 x 4): mixes the channels, pushes some results below 0 and above 1
COLOR = np.array([1.3, 0.1, -0.2, -0.4, 0.9, 0.3, 0.2, -0.1, 1.6, -0.15, 0.05, 0.1], f32)
OPACITY = (1.7, -0.2)


def sample_edit(gs, flags):
    e = gs.edit(transform=gs.model_transform_pod(pos=POS, rot=Q, scale=(SCALE,) * 3), color=COLOR, opacity=OPACITY)
    e.flags = flags
    return e


def edited_pods(gs, sh, cov, pods, mask, flags):
    """what sample_edit(gs, flags) makes of the selected records, by the restatement"""
    return edit_np.apply_edit(sh, cov, pods, mask, flags, pos=POS, rot=Q, scale=(SCALE,) * 3, color=COLOR, opacity=OPACITY,
                              D=gs.sh_rotation_matrices(Q))


def rows(a, nb):
    return np.asarray(a).reshape(-1, nb)


def buffer_rows(buf, stream):
    return np.asarray(buf.download(stream)).reshape(buf.len(), buf.pod.size)


def diff(got, want, nb):
    """for an assertion's message: how many records of nb bytes differ, and where the first one does"""
    if got.size != want.size:
        return "%d bytes, want %d" % (got.size, want.size)
    got, want = rows(got, nb), rows(want, nb)
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad) == 0:
        return ""
    return "%d records differ; first %d at bytes %s" % (len(bad), bad[0], np.flatnonzero(got[bad[0]] != want[bad[0]])[:12].tolist())


def first_difference(got, want, rec=None):
    """for an assertion's message: the first byte at which two byte strings differ (and its record, of rec bytes)"""
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    m = min(len(a), len(b))
    bad = np.flatnonzero(a[:m] != b[:m])
    at = bad[0] if len(bad) else ("none" if len(a) == len(b) else m)
    where = " (record %d, byte %d)" % (at // rec, at % rec) if rec and len(bad) else ""
    return "%d bytes, want %d; %d differ, first difference at byte %s%s" % (len(a), len(b), len(bad), at, where)


def selection_from_mask(gs, device, stream, mask):
    """a device selection holding the mask; None (everything) for no mask"""
    if mask is None:
        return None
    sel = gs.Selection(device, len(mask))
    sel.upload(stream, mask)
    return sel


def np_op(d, s, op):
    """dst = dst op src on bool or word arrays; op is a name of SELECT_OPS or its gs.SEL_* integer"""
    op = SELECT_OPS[op] if isinstance(op, (int, np.integer)) else op
    return {"set": s, "or": d | s, "and": d & s, "andnot": d & ~s, "xor": d ^ s}[op]
