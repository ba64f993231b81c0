"""Camera pixel formats  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE: numpy statements of the NV12 / YUYV -> 8-bit RGB rule of
phnet_preprocess_yuv (include/phnet_hip.h) in int64, and seeded random surfaces whose padding is poisoned.

The rule, per source pixel (row r of the uncropped frame, column x), csc = [y0, m row-major (rows R, G, B; columns Y, U, V)]:
    c = clip((m[c][0] (Y - y0) + m[c][1] (U - 128) + m[c][2] (V - 128) + 2^19) >> 20, 0, 255)       (the shift floors)
NV12: Y = surface[r, x], (U, V) = surface[surface_rows + (r >> 1), 2 (x >> 1) + {0, 1}];  YUYV: Y = surface[r, 2 x],
(U, V) = surface[r, 4 (x >> 1) + {1, 3}].  Chroma is replicated."""
import numpy as np

GEOMETRIES = {            # name: (src_h, src_w, crop, out_h, out_w, {format: (pitch, surface_rows)})
    "a": (98, 134, 13, 64, 160, {"nv12": (192, 104), "yuyv": (320, None)}),          # W0/2 odd, odd crop, padded both ways
    "b": (64, 160, 0, 64, 160, {"nv12": (None, None), "yuyv": (None, None)}),        # tight; identity resize
    "c": (1280, 1920, 480, 320, 800, {"nv12": (2048, 1280), "yuyv": (3840, None)}),  # the workload
    "d": (98, 134, 13, 64, 160, {"nv12": (137, 100), "yuyv": (271, None)}),          # odd pitch: nothing is aligned, byte loads only
}
MATRICES = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]


def _convert(Y, U, V, csc):
    csc = np.asarray(csc, np.int64)
    y, u, v = Y.astype(np.int64) - csc[0], U.astype(np.int64) - 128, V.astype(np.int64) - 128
    m = csc[1:].reshape(3, 3)
    rgb = [(m[c, 0] * y + m[c, 1] * u + m[c, 2] * v + (1 << 19)) >> 20 for c in range(3)]
    return np.clip(np.stack(rgb, axis=-1), 0, 255).astype(np.uint8)


def convert_triples(Y, U, V, csc):
    """The fixed-point rule on arrays of (Y, U, V) -> uint8 [..., 3]."""
    return _convert(np.asarray(Y), np.asarray(U), np.asarray(V), csc)


def nv12_to_rgb(surface, H0, W0, pitch, surface_rows, csc):
    """surface uint8 [..., surface_rows*3//2, pitch] -> RGB uint8 [..., H0, W0, 3]."""
    assert surface.shape[-2:] == (surface_rows * 3 // 2, pitch)
    r, x = np.arange(H0)[:, None], np.arange(W0)[None, :]
    Y = surface[..., :H0, :W0]
    U = surface[..., surface_rows + (r >> 1), 2 * (x >> 1)]
    V = surface[..., surface_rows + (r >> 1), 2 * (x >> 1) + 1]
    return _convert(Y, U, V, csc)


def yuyv_to_rgb(surface, H0, W0, pitch, surface_rows, csc):
    """surface uint8 [..., H0, pitch] -> RGB uint8 [..., H0, W0, 3] (surface_rows: unused, YUYV surfaces have H0 rows)."""
    assert surface.shape[-2:] == (H0, pitch)
    r, x = np.arange(H0)[:, None], np.arange(W0)[None, :]
    Y = surface[..., r, 2 * x]
    U = surface[..., r, 4 * (x >> 1) + 1]
    V = surface[..., r, 4 * (x >> 1) + 3]
    return _convert(Y, U, V, csc)


TO_RGB = {"nv12": nv12_to_rgb, "yuyv": yuyv_to_rgb}


def layout(fmt, H0, W0, pitch=None, surface_rows=None):
    """(pitch, surface_rows, frame_shape) with the defaults of ClipPreprocessor filled in."""
    pitch = (W0 if fmt == "nv12" else 2 * W0) if pitch is None else pitch
    surface_rows = H0 if surface_rows is None else surface_rows
    return pitch, surface_rows, ((surface_rows * 3 // 2, pitch) if fmt == "nv12" else (H0, pitch))


def padding_mask(fmt, H0, W0, pitch, surface_rows):
    """bool [frame_shape]: True on every byte no pixel of the H0 x W0 image owns."""
    _, _, shape = layout(fmt, H0, W0, pitch, surface_rows)
    pad = np.ones(shape, bool)
    if fmt == "nv12":
        pad[:H0, :W0] = False
        pad[surface_rows:surface_rows + H0 // 2, :W0] = False
    else:
        pad[:H0, :2 * W0] = False
    return pad


def poison(surfaces, fmt, H0, W0, pitch, surface_rows, phase=0):
    """Overwrite the padding of uint8 [T, *frame_shape] in place with alternating 0 / 255 (phase 1: 255 / 0)."""
    pad = padding_mask(fmt, H0, W0, pitch, surface_rows)
    pattern = (((np.indices(pad.shape).sum(0) + phase) & 1) * 255).astype(np.uint8)
    surfaces[:, pad] = pattern[pad]
    return surfaces


def random_surfaces(fmt, T, H0, W0, pitch=None, surface_rows=None, seed=0, extremes=True):
    """uint8 [T, *frame_shape]: seeded random bytes; with `extremes` frames 0 and 1 are Y in {0, 255} bands of 5 rows with
    U, V in {0, 255} (blocks of 8 columns x 6 rows, the two chroma channels out of step), which saturates both ends of every
    channel; the padding is poisoned to alternating 0 / 255."""
    pitch, surface_rows, shape = layout(fmt, H0, W0, pitch, surface_rows)
    r = np.random.default_rng(seed)
    s = r.integers(0, 256, (T, *shape), dtype=np.uint8)
    if extremes:
        rows, cols = np.arange(H0)[:, None], np.arange(W0)[None, :]
        for t in range(min(T, 2)):
            Y = ((((rows // 5) + t) & 1) * 255 + 0 * cols).astype(np.uint8)
            U = (((cols // 8 + rows // 6 + t) & 1) * 255).astype(np.uint8)
            V = (((cols // 8 + rows // 6 + (rows // 12) + 1) & 1) * 255).astype(np.uint8)
            if fmt == "nv12":
                s[t, :H0, :W0] = Y
                s[t, surface_rows:surface_rows + H0 // 2, 0:W0:2] = U[::2, ::2]
                s[t, surface_rows:surface_rows + H0 // 2, 1:W0:2] = V[::2, ::2]
            else:
                s[t, :, 0:2 * W0:2] = Y
                s[t, :, 1:2 * W0:4] = U[:, ::2]
                s[t, :, 3:2 * W0:4] = V[:, ::2]
    return poison(s, fmt, H0, W0, pitch, surface_rows)
