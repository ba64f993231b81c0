"""The mask-metric rules of include/phnet_hip.h (phnet_mask_metrics, rules 1-4) restated in numpy / scipy, and the cases the CPU
and GPU tests share.  `counts(pred, gt, radius)` is what the kernel is held to, all seven integers; the CPU test holds this file
to the reference's executed seg2bmap / db_eval_boundary / db_eval_iou through tests/golden/video_metrics_tiny.json.  The dilation
the fixture pins is scipy.ndimage.binary_dilation with the disk as footprint (`dilate_scipy`): PARITY UNPINNED against skimage,
which is not installed.  `counts` uses the same set by its definition (`dilate`: nearest set pixel within the radius), which costs
the same at every radius."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_metrics_tiny.json")


def disk(radius: int) -> np.ndarray:
    """rule 3: the offsets (dy, dx) with dx^2 + dy^2 <= radius^2, bool [2 r + 1, 2 r + 1] (skimage.morphology.disk)."""
    v = np.arange(-radius, radius + 1)
    return v[:, None] ** 2 + v[None, :] ** 2 <= radius * radius


def boundary_map(mask: np.ndarray) -> np.ndarray:
    """rules 1 and 2 on one [H, W] mask -> bool [H, W]."""
    s = np.asarray(mask) != 0
    h, w = s.shape
    b = np.zeros((h, w), bool)
    b[:-1, :-1] = (s[:-1, :-1] ^ s[:-1, 1:]) | (s[:-1, :-1] ^ s[1:, :-1]) | (s[:-1, :-1] ^ s[1:, 1:])
    b[-1, :-1] = s[-1, :-1] ^ s[-1, 1:]
    b[:-1, -1] = s[:-1, -1] ^ s[1:, -1]
    return b


def dilate_scipy(b: np.ndarray, radius: int) -> np.ndarray:
    """rule 3 as the fixture pins it: scipy's binary_dilation with the disk as footprint.  Its cost grows with the footprint (seconds
    at radius 64 on a small canvas), so the tests use it at small radii and `dilate` everywhere else."""
    from scipy.ndimage import binary_dilation
    return binary_dilation(b, structure=disk(radius), border_value=0)


def dilate(b: np.ndarray, radius: int) -> np.ndarray:
    """rule 3 on one [H, W] bit image, by its definition: a pixel is set iff the NEAREST set pixel of `b` lies within dx^2 + dy^2 <=
    radius^2 - the exact feature transform (scipy's distance_transform_edt returns the nearest set pixel's indices; the squared
    distance is then integer arithmetic).  The CPU test holds this equal to `dilate_scipy`."""
    from scipy.ndimage import distance_transform_edt
    b = np.asarray(b, bool)
    if not b.any():
        return np.zeros_like(b)
    iy, ix = distance_transform_edt(~b, return_distances=False, return_indices=True)
    yy, xx = np.mgrid[0:b.shape[0], 0:b.shape[1]]
    return (iy.astype(np.int64) - yy) ** 2 + (ix.astype(np.int64) - xx) ** 2 <= radius * radius


def counts(pred: np.ndarray, gt: np.ndarray, radius: int) -> np.ndarray:
    """rule 4: pred, gt [.., H, W] of any integer type -> int64 [.., 7]."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape and pred.ndim >= 2
    lead = pred.shape[:-2]
    out = np.zeros((int(np.prod(lead, dtype=np.int64)), 7), np.int64)
    for k, (p, g) in enumerate(zip(pred.reshape((-1,) + pred.shape[-2:]), gt.reshape((-1,) + gt.shape[-2:]))):
        p, g = p != 0, g != 0
        bp, bg = boundary_map(p), boundary_map(g)
        out[k] = (p.sum(), g.sum(), (p & g).sum(), bp.sum(), bg.sum(), (bp & dilate(bg, radius)).sum(), (bg & dilate(bp, radius)).sum())
    return out.reshape(lead + (7,))


# ---------------------------------------------------------------------------------------------- the fixture
def pack(mask: np.ndarray) -> str:
    """[H, W] bool -> hex text of np.packbits (row-major, most significant bit first)."""
    return np.packbits(np.asarray(mask, bool).reshape(-1)).tobytes().hex()


def unpack(text: str, h: int, w: int) -> np.ndarray:
    return np.unpackbits(np.frombuffer(bytes.fromhex(text), np.uint8))[:h * w].reshape(h, w).astype(bool)


@functools.lru_cache(maxsize=None)
def fixture_cases():
    """[dict(name, pred, gt bool [H, W], radius, bound_th, bmap_pred, bmap_gt, F, J, J2)] as the reference computed them."""
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    cases = []
    for c in doc["cases"]:
        h, w = c["height"], c["width"]
        cases.append(dict(name=c["name"], radius=c["radius"], bound_th=c["bound_th"], F=c["F"], J=c["J"], J2=c["J2"],
                          **{k: unpack(c[k], h, w) for k in ("pred", "gt", "bmap_pred", "bmap_gt")}))
    return cases


# ---------------------------------------------------------------------------------------------- generated cases
def blobs(h: int, w: int, seed: int, n_blobs: int = 6, n_strokes: int = 4, borders: bool = True) -> np.ndarray:
    """u8 [H, W]: random ellipses, thin diagonal strokes and (borders) a blob cut by each of the four image borders."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    centres = [(rng.integers(0, h), rng.integers(0, w)) for _ in range(n_blobs)]
    if borders:
        centres += [(0, w // 3), (h - 1, 2 * w // 3), (h // 3, 0), (2 * h // 3, w - 1)]
    for cy, cx in centres:
        ry, rx = rng.integers(2, max(3, h // 6)), rng.integers(2, max(3, w // 8))
        m |= ((yy - cy) * rx) ** 2 + ((xx - cx) * ry) ** 2 <= (ry * rx) ** 2
    for _ in range(n_strokes):
        x0, slope, thick = rng.integers(0, w), rng.choice([-2, -1, 1, 2]), rng.integers(1, 3)
        m |= np.abs(xx - (x0 + slope * yy)) < thick
    return m.astype(np.uint8)


def pair(h: int, w: int, seed: int, shift=(3, 5)) -> tuple:
    """(pred, gt): gt the blobs of `seed`, pred the same blobs moved by `shift` = (dy, dx) plus a few of its own."""
    gt = blobs(h, w, seed)
    pred = np.zeros_like(gt)
    dy, dx = shift
    src = gt[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)]
    pred[max(0, dy):max(0, dy) + src.shape[0], max(0, dx):max(0, dx) + src.shape[1]] = src
    pred |= blobs(h, w, seed + 1000, n_blobs=2, n_strokes=1, borders=False)
    return pred, gt


def edge_columns(h: int, w: int) -> tuple:
    """A foreground column at x = W - 1 in pred and at x = 0 in gt (and a short bar each): a dilation that wrapped from one row's
    end into the next row's start would match them."""
    pred, gt = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    pred[:, w - 1] = 1
    gt[:, 0] = 1
    pred[h // 2, max(0, w - 4):] = 1
    gt[h // 3, :min(w, 3)] = 1
    return pred, gt
