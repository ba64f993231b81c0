"""Camera pixel formats without a GPU: the colour matrices of `yuv_matrix` against the tables worked out from BT.601 / BT.709,
the fixed-point conversion rule against the float64 formula, the surface geometry and validation of ClipPreprocessor, and the
argument checks of phnet_preprocess_yuv through the built library (they precede every launch)."""
import ctypes

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor, yuv_matrix
from tests import pixfmt_cases as C

TABLES = {
    ("bt601", False): (16, [[1220945, 0, 1673555], [1220945, -410793, -852458], [1220945, 2115221, 0]]),
    ("bt601", True): (0, [[1048576, 0, 1470104], [1048576, -360853, -748826], [1048576, 1858077, 0]]),
    ("bt709", False): (16, [[1220945, 0, 1879825], [1220945, -223607, -558796], [1220945, 2215014, 0]]),
    ("bt709", True): (0, [[1048576, 0, 1651297], [1048576, -196424, -490864], [1048576, 1945738, 0]]),
}
K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


@pytest.fixture(scope="module")
def built():
    from phnet_amd import build
    return build.build(verbose=False)


@pytest.mark.parametrize("standard,full", C.MATRICES)
def test_yuv_matrix_equals_the_tables(standard, full):
    m = yuv_matrix(standard, full)
    y0, rows = TABLES[(standard, full)]
    assert m.dtype == np.int32 and m.shape == (10,)
    assert m.tolist() == [y0] + [v for row in rows for v in row]
    with pytest.raises(ValueError):
        yuv_matrix("bt2020", full)


@pytest.mark.parametrize("standard,full", C.MATRICES)
def test_fixed_point_conversion_is_within_one_lsb_of_float64(standard, full):
    """All 256 Y x (U, V) in {0, 3, ..., 255}^2 against clip(floor(float64 formula + 0.5)): <= 1 LSB, <= 0.2 % of the samples differ
    (the 20-bit coefficients are off by <= 2^-21 each, the operands are < 256: the sums differ by < 4e-4, which moves a rounding
    only next to a half)."""
    Y, U, V = np.meshgrid(np.arange(256), np.arange(0, 256, 3), np.arange(0, 256, 3), indexing="ij")
    got = C.convert_triples(Y, U, V, yuv_matrix(standard, full)).astype(np.int64)
    kr, kb = K[standard]
    kg = 1.0 - kr - kb
    y0, sy, sc = (0.0, 1.0, 1.0) if full else (16.0, 255.0 / 219.0, 255.0 / 224.0)
    y, u, v = sy * (Y - y0), sc * (U - 128.0), sc * (V - 128.0)
    want = np.stack([y + 2 * (1 - kr) * v,
                     y - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v,
                     y + 2 * (1 - kb) * u], axis=-1)
    want = np.clip(np.floor(want + 0.5), 0, 255).astype(np.int64)
    diff = np.abs(got - want)
    print(f"{standard} full={full}: max {int(diff.max())} LSB, {100.0 * float((diff > 0).mean()):.4f} % differ")
    assert diff.max() <= 1
    assert float((diff > 0).mean()) <= 0.002


def test_grey_and_range_end_points():
    y = np.arange(256)
    mid = np.full(256, 128)
    for standard in ("bt601", "bt709"):
        rgb = C.convert_triples(y, mid, mid, yuv_matrix(standard, True))
        assert np.array_equal(rgb, np.repeat(y[:, None], 3, axis=1).astype(np.uint8))     # full range: (Y,128,128) -> (Y,Y,Y)
    lim = yuv_matrix("bt601", False)
    assert C.convert_triples([16, 235], [128, 128], [128, 128], lim).tolist() == [[0, 0, 0], [255, 255, 255]]
    assert C.convert_triples([0, 255], [128, 128], [128, 128], lim).tolist() == [[0, 0, 0], [255, 255, 255]]   # foot / head room clamps


def test_numpy_converters_read_the_documented_bytes():
    """nv12_to_rgb / yuyv_to_rgb on surfaces built pixel by pixel: chroma of the 2x2 / 2x1 cell, padding never read."""
    H0, W0 = 6, 10
    csc = yuv_matrix("bt709", False)
    r = np.random.default_rng(5)
    Y = r.integers(0, 256, (H0, W0))
    for fmt, pitch, srows, ch in (("nv12", 16, 8, H0 // 2), ("yuyv", 24, None, H0)):
        U, V = r.integers(0, 256, (ch, W0 // 2)), r.integers(0, 256, (ch, W0 // 2))
        pitch, srows, shape = C.layout(fmt, H0, W0, pitch, srows)
        s = np.zeros((1, *shape), np.uint8)
        for i in range(H0):
            for j in range(W0):
                if fmt == "nv12":
                    s[0, i, j] = Y[i, j]
                    s[0, srows + i // 2, 2 * (j // 2)], s[0, srows + i // 2, 2 * (j // 2) + 1] = U[i // 2, j // 2], V[i // 2, j // 2]
                else:
                    s[0, i, 2 * j] = Y[i, j]
                    s[0, i, 4 * (j // 2) + 1], s[0, i, 4 * (j // 2) + 3] = U[i, j // 2], V[i, j // 2]
        rows = np.arange(H0)[:, None] // (2 if fmt == "nv12" else 1)
        want = C.convert_triples(Y, U[rows, np.arange(W0)[None, :] // 2], V[rows, np.arange(W0)[None, :] // 2], csc)
        a = C.TO_RGB[fmt](C.poison(s.copy(), fmt, H0, W0, pitch, srows, 0), H0, W0, pitch, srows, csc)
        b = C.TO_RGB[fmt](C.poison(s.copy(), fmt, H0, W0, pitch, srows, 1), H0, W0, pitch, srows, csc)
        assert np.array_equal(a[0], want) and np.array_equal(b[0], want)
        assert int(C.padding_mask(fmt, H0, W0, pitch, srows).sum()) == s[0].size - (H0 * W0 * 3 // 2 if fmt == "nv12" else H0 * W0 * 2)


def test_frame_shape_and_validation_need_no_gpu():
    mk = lambda **kw: ClipPreprocessor(64, 160, device="cpu", **kw)                       # noqa: E731  (tables only: no launch)
    assert mk(src_h=98, src_w=134, crop_size=13).frame_shape == (98, 134, 3)
    assert mk(src_h=98, src_w=134, crop_size=13).pixel_format == "rgb"
    assert mk(src_h=98, src_w=134, crop_size=13, pixel_format="nv12").frame_shape == (147, 134)
    assert mk(src_h=98, src_w=134, crop_size=13, pixel_format="nv12", pitch=192, surface_rows=104).frame_shape == (156, 192)
    assert mk(src_h=98, src_w=134, crop_size=13, pixel_format="yuyv").frame_shape == (98, 268)
    assert mk(src_h=97, src_w=134, crop_size=13, pixel_format="yuyv", pitch=320).frame_shape == (97, 320)   # 4:2:2: any height
    assert ClipPreprocessor(320, 800, device="cpu", pixel_format="nv12", pitch=2048).frame_shape == (1920, 2048)
    for bad in (dict(pixel_format="i420"), dict(pixel_format="nv12", src_w=133), dict(pixel_format="yuyv", src_w=133),
                dict(pixel_format="nv12", src_h=97), dict(pixel_format="nv12", pitch=133), dict(pixel_format="yuyv", pitch=267),
                dict(pixel_format="nv12", surface_rows=96), dict(pixel_format="nv12", surface_rows=99),
                dict(pixel_format="yuyv", surface_rows=104), dict(pitch=512), dict(surface_rows=104),
                dict(pixel_format="nv12", matrix="bt2020")):
        with pytest.raises(ValueError):
            mk(**{"src_h": 98, "src_w": 134, "crop_size": 13, **bad})
    pre = mk(src_h=98, src_w=134, crop_size=13, pixel_format="nv12", pitch=192, surface_rows=104)
    with pytest.raises(RuntimeError):
        pre(torch.zeros((3, 156, 192), dtype=torch.uint8))                                 # no CPU path
    with pytest.raises(RuntimeError):
        pre(torch.zeros((3, 156, 192), dtype=torch.float32))
    for shape in ((3, 147, 192), (3, 156, 134), (3, 98, 134, 3), (156, 192)):
        with pytest.raises(ValueError):
            pre(torch.zeros(shape, dtype=torch.uint8))


def _yuv_call(lib, T=0, H0=98, W0=134, crop=13, layout=0, fmt=0, stride=None, pitch=192, chroma=None, ptr=None):
    chroma = pitch * H0 if chroma is None else chroma
    stride = (chroma + pitch * (H0 // 2) if fmt == 0 else pitch * H0) if stride is None else stride
    return lib.phnet_preprocess_yuv(ptr, ptr, None, ptr, ptr, ptr, ptr, T, H0, W0, crop, 64, 160, 0, layout, fmt, stride, pitch, chroma,
                                    ptr, ptr, ptr, None)


def test_yuv_entry_validates_before_any_launch(built):
    """Shape checks come first, then T == 0 is a no-op: with T = 0 a bad geometry is -1 and a good one 0, no GPU involved."""
    lib = _lib.lib()
    names = {n: (r, a) for n, r, a in _lib.declared_functions()}
    _, args = names["phnet_preprocess_yuv"]
    assert len(args) == 23 and args[16] is ctypes.c_int64 and args[18] is ctypes.c_int64 and args[15] is ctypes.c_int32
    assert lib.phnet_abi_version() == 1
    assert _yuv_call(lib) == 0                                        # T = 0
    assert _yuv_call(lib, fmt=1, pitch=320) == 0
    assert _yuv_call(lib, W0=133) == -1                               # odd W0
    assert _yuv_call(lib, W0=133, fmt=1, pitch=320) == -1
    assert _yuv_call(lib, H0=97) == -1                                # odd H0, NV12 only
    assert _yuv_call(lib, H0=97, fmt=1, pitch=320) == 0
    assert _yuv_call(lib, pitch=133) == -1                            # pitch < W0
    assert _yuv_call(lib, pitch=134) == 0
    assert _yuv_call(lib, fmt=1, pitch=267) == -1                     # pitch < 2 W0
    assert _yuv_call(lib, chroma=192 * 98 - 1) == -1                  # the UV plane inside the Y plane
    assert _yuv_call(lib, fmt=1, pitch=320, chroma=0) == 0            # YUYV: ignored
    assert _yuv_call(lib, fmt=2) == -1 and _yuv_call(lib, fmt=-1) == -1
    assert _yuv_call(lib, layout=2) == -1
    assert _yuv_call(lib, crop=98) == -1 and _yuv_call(lib, crop=-1) == -1
    assert _yuv_call(lib, stride=192 * 98) == -1                      # frames that would overlap
    assert _yuv_call(lib, T=-1) == -1
    assert _yuv_call(lib, T=1) == -1                                  # null pointers
    # host-side arguments with everything else in place: a zero std and a matrix that would overflow int32 (checked before the launch)
    csc = (ctypes.c_int32 * 10)(*yuv_matrix("bt601", False).tolist())
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.0, 0.2)
    fake = ctypes.c_void_p(256)                                       # never dereferenced: the call returns before launching
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)                     # noqa: E731
    call = lambda c, s: lib.phnet_preprocess_yuv(fake, fake, None, fake, fake, fake, fake, 1, 98, 134, 13, 64, 160, 0, 0, 0,       # noqa: E731
                                                 192 * 147, 192, 192 * 98, p(c), p(mean), p(s), None)
    assert call(csc, std) == -1
    big = (ctypes.c_int32 * 10)(16, 1 << 23, 1 << 22, 0, 0, 0, 0, 0, 0, 0)
    assert call(big, (ctypes.c_float * 3)(0.2, 0.2, 0.2)) == -1
