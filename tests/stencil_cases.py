"""The neighbourhood ops of the training augmentation (csrc/augment_stencil.hip; rule 7 of include/phnet_hip.h): a restatement in numpy -
int64 where the kernel computes in int32 - and the cases.  It stands on tests/augment_cases.py, which it imports and does not copy: rules
1 - 6, the colour and dropout restatements, the epilogue and the frames of the two earlier shapes.

`staged(frames, flip2, table, stencil, t)` gives B of frame t, the image the staging launch writes; `augment(...)` the augmented 8-bit
clip: a frame with a neighbourhood op is rules 1 - 3 and 6 on B (the warp of augment_cases with a neutral table), every other frame is
augment_cases.augment's.  PARITY UNPINNED against imgaug / cv2: this file restates the project's own rules;
tests/test_augment_stencil_cpu.py holds it to scipy.ndimage, which is independent of the kernel.

Shapes (T, H, W), the smallest at which each thing can go wrong with the kernel's 64 x 16 tile: the two of augment_cases; 70 x 150, more
than one tile each way with ragged last tiles (22 columns, 6 rows); 5 x 7, smaller than a tile and than the 9-tap radius, so a reflection
wraps more than once; 1 x 9, H = 1."""
import functools

import numpy as np

from phnet_amd.libs.dataset.openlane import augment as A
from tests import augment_cases as AC

COLS = 40
SHAPES = dict(AC.SHAPES, ragged=(1, 70, 150), small=(2, 5, 7), flat=(1, 1, 9))
TILE_W, TILE_H = 64, 16


# ------------------------------------------------------------------------------------------------------------ the restatement
def reflect101(i, n):
    """r(i, n) of rule 7 on an integer array."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)                                                                  # numpy: non-negative
    return np.where(m < n, m, p - m)


def row(stencil_row):
    """The clamps of the kernels on one stencil row -> dict(edge, e [3,3], kind, k, weights)."""
    r = [int(v) for v in stencil_row]
    kind = r[10] if r[10] in (1, 2, 3) else 0
    k = 0 if kind == 0 else min(max(r[11], 3), 9 if kind == 3 else 5) | 1
    out = dict(edge=r[0] != 0, e=np.clip(np.array(r[1:10], np.int64), -65536, 65536).reshape(3, 3), kind=kind, k=k, weights=None)
    if kind == 1:
        out["weights"] = np.clip(np.array(r[12:12 + k * k], np.int64), 0, 65536).reshape(k, k)
    elif kind == 3:
        out["weights"] = np.clip(np.array(r[12:12 + k], np.int64), 0, 256)
    return out


def active(stencil_row):
    s = row(stencil_row)
    return s["edge"] or s["kind"] != 0


def edge_filter(C, e):
    """E of rule 7 on C int64 [H, W, 3] with e int64 [3, 3]."""
    H, W, _ = C.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    acc = np.zeros_like(C)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            acc += e[dy + 1, dx + 1] * C[reflect101(ys + dy, H), reflect101(xs + dx, W)]
    return np.clip((acc + 2048) >> 12, 0, 255)


def blur(D, s):
    """B of rule 7 on D int64 [H, W, 3] with the clamped row s."""
    H, W, _ = D.shape
    kind, k = s["kind"], s["k"]
    R = k // 2
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == 1:
        acc = np.zeros_like(D)
        for j in range(k):
            for i in range(k):
                acc += s["weights"][j, i] * D[reflect101(ys + j - R, H), reflect101(xs + i - R, W)]
        return np.clip((acc + 2048) >> 12, 0, 255)
    if kind == 2:
        taps = [D[np.clip(ys + j - R, 0, H - 1), np.clip(xs + i - R, 0, W - 1)] for j in range(k) for i in range(k)]
        return np.sort(np.stack(taps), axis=0)[(k * k) // 2]
    if kind == 3:
        g = s["weights"]
        hsum = sum(g[i] * D[ys, reflect101(xs + i - R, W)] for i in range(k))        # nothing is rounded between the passes
        acc = sum(g[j] * hsum[reflect101(ys + j - R, H), xs] for j in range(k))
        assert acc.max() < 2 ** 31 - 32768                                           # the kernel's int32 holds it
        return np.clip((acc + 32768) >> 16, 0, 255)
    return D


def staged(frames, flip2, table, stencil, t):
    """B of frame t, u8 [H, W, 3]: flip, rule 4, the edge filter, rule 5, the blur."""
    _, H, W, _ = frames.shape
    p, s, info = AC._row(table[t]), row(stencil[t]), AC.new_info()
    src = frames[t][:, ::-1] if flip2[t] != 0 else frames[t]
    C = AC.colour(src.reshape(-1, 3).astype(np.int64), p, info).reshape(H, W, 3)
    E = edge_filter(C, s["e"]) if s["edge"] else C
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    D = AC.dropout(E.reshape(-1, 3), p, t, xs.ravel(), ys.ravel(), H, W, info).reshape(H, W, 3)
    B = blur(D, s)
    assert B.min() >= 0 and B.max() <= 255
    return B.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _neutral_table():
    return A.AugmentParams.identity(1).numpy()["table"]


def augment(frames, flip2, inv, table, stencil):
    """frames u8 [T, H, W, 3] -> the augmented u8 [T, H, W, 3] by rules 1 - 7; stencil None: augment_cases.augment."""
    out, _ = AC.augment(frames, flip2, inv, table)
    if stencil is None:
        return out
    for t in range(frames.shape[0]):
        if active(stencil[t]):
            B = staged(frames, flip2, table, stencil, t)
            out[t] = AC.augment(B[None], np.zeros(1, np.int32), inv[t:t + 1], _neutral_table())[0][0]
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def frames(shape):
    """The frames of augment_cases for its two shapes, seeded random bytes for the others; read-only."""
    if shape in AC.SHAPES:
        return AC.frames(shape)
    T, H, W = SHAPES[shape]
    f = np.random.default_rng({"ragged": 13, "small": 14, "flat": 15}[shape]).integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    f.setflags(write=False)
    return f


def _blur(kind, k, weights=None):
    return dict(kind=kind, k=k) if weights is None else dict(kind=kind, k=k, weights=weights)


# name -> one dict for every frame, or a list of dicts (the first T are used)
PARAM_SETS = {
    "edge": dict(edge=dict(weights=A.edge_kernel(0.15))),
    "directed_edge": dict(edge=dict(weights=A.directed_edge_kernel(0.2, 0.37))),
    "motion3": dict(blur=_blur("motion", 3, A.motion_kernel(3, 25.0, 0.4))),
    "motion5": dict(blur=_blur("motion", 5, A.motion_kernel(5, 130.0, -0.6))),
    "motion5_dropout": dict(blur=_blur("motion", 5, A.motion_kernel(5, 200.0, 0.1)), dropout=dict(mode="pixel", p=0.2, per_channel=False, seed=31)),
    "median3": dict(blur=_blur("median", 3)),
    "median5": dict(blur=_blur("median", 5)),
    "gauss3": dict(blur=_blur("gaussian", 3, np.array([0.25, 0.5, 0.25]))),
    "gauss5": dict(blur=_blur("gaussian", 5, A.gaussian_kernel(1.0))),
    "gauss7": dict(blur=_blur("gaussian", 7, A.gaussian_kernel(2.2))),
    "gauss9": dict(blur=_blur("gaussian", 9, A.gaussian_kernel(2.9))),
    "everything": dict(flip=True, perm=(1, 2, 0), mul=1.07, add=-6, value=9, edge=dict(weights=A.directed_edge_kernel(0.18, 0.8)),
                       dropout=dict(mode="pixel", p=0.05, per_channel=True, seed=2 ** 63 + 11), blur=_blur("median", 5),
                       rotate=4.1, scale=1.08, translate=(-0.04, 0.07)),
    "mixed": [dict(value=-7, dropout=dict(mode="pixel", p=0.04, per_channel=True, seed=99), rotate=-3.3, scale=0.92, translate=(0.06, -0.03)),
              dict(flip=True, edge=dict(weights=A.edge_kernel(0.2)), rotate=2.0),
              dict(dropout=dict(mode="coarse", p=0.3, per_channel=False, seed=77, grid=(3, 5)), blur=_blur("gaussian", 9, A.gaussian_kernel(3.0)))],
}
SINGLE_OPS = tuple(n for n in PARAM_SETS if n not in ("everything", "mixed", "motion5_dropout"))


def build(shape, spec):
    T, H, W = SHAPES[shape]
    return A.AugmentParams.build(spec[:T] if isinstance(spec, list) else [spec] * T, H, W, stencil=True)


@functools.lru_cache(maxsize=None)
def params(shape, name):
    """The AugmentParams (host, with a stencil table) of a parameter set for a shape."""
    return build(shape, PARAM_SETS[name])


@functools.lru_cache(maxsize=None)
def expected(shape, name):
    """The augmented u8 of a parameter set on the frames of a shape, by the restatement; read-only."""
    p = params(shape, name).numpy()
    out = augment(frames(shape), p["flip2"], p["inv"], p["table"], p["stencil"])
    out.setflags(write=False)
    return out


# a table no host code would build: an unknown kind behind an edge filter of +-2^31, k below and above every allowed size, weights +-2^31
WILD_SHAPE = (4, 19, 70)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def wild_stencil():
    s = np.zeros((4, COLS), np.int64)
    s[0, 0], s[0, 1:10], s[0, 10], s[0, 11] = 7, [I32_MAX, I32_MIN] * 4 + [I32_MAX], 77, 1000
    s[1, 10], s[1, 11], s[1, 12:37] = 2, -3, I32_MIN
    s[2, 10], s[2, 11], s[2, 12:37] = 3, 1000, I32_MAX
    s[3, 0], s[3, 10], s[3, 11], s[3, 12:37] = I32_MIN, 1, 1000, [I32_MIN, I32_MAX, 1, 0, 4095] * 5
    s[3, 5] = 4096                                                                    # the edge filter is on: the identity
    s[:, 37:] = I32_MAX                                                               # the columns that should be zero
    return s.astype(np.int32)
