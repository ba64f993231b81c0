"""Golden values of the mask-level video metrics: runs the REFERENCE's own evaluation/video_metrics/f_boundary.py and jaccard.py
(read-only checkout at /root/reference, loaded by path, unmodified) on small synthetic mask pairs and stores the masks with what
those functions return.
Build container only:  python tests/golden/make_goldens_vidmetrics.py   -> tests/golden/video_metrics_tiny.json

Stand-ins: `np.bool = bool` where numpy no longer has it, and a `skimage.morphology` shell (skimage is not in this image) whose
disk(r) is x^2 + y^2 <= r^2 and whose binary_dilation(img, fp) is scipy.ndimage.binary_dilation(img, structure=fp, border_value=0).
So the boundary rule (seg2bmap), the radius rule, the precision / recall / F branches and J are pinned to executed reference code;
the dilation is pinned to scipy: PARITY UNPINNED against skimage.

Per case: the two masks, bound_th as passed, the radius `disk` received, the reference's seg2bmap of both masks, the F of
db_eval_boundary, and the J of db_eval_iou on the plain masks (J) and on the stacked (~m, m) pairs of evaluate_vid.py:55-57 (J2).
Masks are bit-packed (np.packbits, hex).

Asserted, so that the fixture pins what it is meant to pin: at least three cases have 0.1 < F < 0.9 with precision and recall both
strictly between 0 and 1; each of the branches n_fg = 0 < n_gt, n_gt = 0 < n_fg and n_fg = n_gt = 0 occurs, the last one with an
all-foreground mask (an empty boundary map); one case has both boundaries non-empty and F = 0 (the masks are further apart than
the radius).  (A 2-pixel shift on the 96 x 160 canvas would give F = 1: the default radius there is 2.)"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np

from tests import maskmetric_cases as C

REF_DIR = "/root/reference/evaluation/video_metrics"
RADII = []                                                # what `disk` was called with


def _disk(radius):
    RADII.append(float(radius))
    r = int(radius)
    assert r == radius
    v = np.arange(-r, r + 1)
    return (v[:, None] ** 2 + v[None, :] ** 2 <= r * r).astype(np.uint8)


def _binary_dilation(image, footprint=None):
    from scipy.ndimage import binary_dilation
    return binary_dilation(image, structure=footprint, border_value=0)


def load_reference():
    if not hasattr(np, "bool"):
        np.bool = bool
    for name, attrs in (("skimage", {}), ("skimage.morphology", dict(disk=_disk, binary_dilation=_binary_dilation))):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        if name == "skimage":
            mod.__path__ = []
        sys.modules[name] = mod                           # stays: db_eval_boundary imports it when it is called
    mods = []
    for fname in ("f_boundary", "jaccard"):
        spec = importlib.util.spec_from_file_location("ref_" + fname, os.path.join(REF_DIR, fname + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def squares(h, w, boxes):
    m = np.zeros((h, w), bool)
    for y0, x0, y1, x1 in boxes:
        m[y0:y1, x0:x1] = True
    return m


def make_cases():
    """[(name, pred, gt, bound_th)]"""
    cases = []
    p, g = C.pair(96, 160, 7, shift=(3, 5))
    cases.append(("shift_default_radius", p, g, 0.008))
    cases.append(("shift_radius_4", p, g, 4))
    p, g = C.pair(64, 100, 11, shift=(-6, 11))
    cases.append(("shift_radius_9", p, g, 9))
    p, g = C.pair(37, 70, 13, shift=(4, -7))
    cases.append(("ragged_radius_5", p, g, 5))
    g = C.blobs(48, 80, 17)
    cases.append(("pred_empty", np.zeros_like(g), g, 3))
    cases.append(("gt_empty", g, np.zeros_like(g), 3))
    cases.append(("full_against_empty", np.ones((48, 80), bool), np.zeros((48, 80), bool), 3))
    cases.append(("both_empty", np.zeros((48, 80), bool), np.zeros((48, 80), bool), 0.008))
    cases.append(("identical", g, g.copy(), 0.008))
    cases.append(("far_apart", squares(48, 80, [(5, 5, 15, 15)]), squares(48, 80, [(28, 50, 40, 70)]), 3))
    cases.append(("radius_0", squares(20, 33, [(3, 3, 12, 20)]), squares(20, 33, [(3, 4, 12, 21)]), 0))
    return [(n, np.asarray(p) != 0, np.asarray(g) != 0, th) for n, p, g, th in cases]


def main():
    fb, jc = load_reference()
    out, partial, branches, far = [], 0, set(), False
    for name, pred, gt, th in make_cases():
        h, w = pred.shape
        del RADII[:]
        F = float(fb.db_eval_boundary(pred.copy(), gt.copy(), th))
        assert len(RADII) == 2 and RADII[0] == RADII[1]
        radius = int(RADII[0])
        bp, bg = fb.seg2bmap(pred.copy()).astype(bool), fb.seg2bmap(gt.copy()).astype(bool)
        J = float(jc.db_eval_iou(pred.copy(), gt.copy()))
        J2 = float(jc.db_eval_iou(np.stack((~pred, pred), axis=-1), np.stack((~gt, gt), axis=-1)))
        n_fg, n_gt = int(bp.sum()), int(bg.sum())
        if n_fg and n_gt:
            prec = (bp & _binary_dilation(bg, _disk(radius))).sum() / n_fg
            rec = (bg & _binary_dilation(bp, _disk(radius))).sum() / n_gt
            partial += 0.1 < F < 0.9 and 0 < prec < 1 and 0 < rec < 1
            far |= F == 0
        else:
            branches.add((n_fg > 0, n_gt > 0))
            if name == "full_against_empty":
                assert pred.all() and n_fg == 0
        print(f"{name:24s} {h}x{w} radius {radius} n_fg {n_fg} n_gt {n_gt} F {F:.4f} J {J:.4f} J2 {J2:.4f}")
        out.append(dict(name=name, height=h, width=w, bound_th=th, radius=radius, pred=C.pack(pred), gt=C.pack(gt),
                        bmap_pred=C.pack(bp), bmap_gt=C.pack(bg), F=F, J=J, J2=J2))
    assert partial >= 3, partial
    assert branches == {(False, True), (True, False), (False, False)}, branches
    assert far
    with open(os.path.join(HERE, "video_metrics_tiny.json"), "w") as fh:
        json.dump({"cases": out}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
