"""Lane overlay, the part that needs no GPU: phnet_lane_draw (csrc/lane_draw.hip) is declared, exported and refuses bad
arguments before any launch; the resources the compiler gives its kernels; the numpy restatement the GPU tests compare against
(tests/overlay_cases.py) agrees with the project's own statements of the same rules - oracle.culane_cpu.raster_lane for the
coverage, Python's int() for the point mapping, tests/pixfmt_cases.py for the colour conversion; and the Python surface."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import culane_cpu
from phnet_amd import _lib
from phnet_amd import build as hip_build
from phnet_amd.libs.dataset.openlane.preprocess import yuv_matrix
from tests import overlay_cases as OC
from tests import pixfmt_cases as PC

ERR_ARG = -1
N_ARGS = 25


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


def test_symbol_is_declared_and_exported(built):
    names = {n: a for n, _, a in _lib.declared_functions(_lib.HEADER)}
    assert len(names["phnet_lane_draw"]) == N_ARGS
    exported = set(os.popen(f"nm -D --defined-only {_lib.SO_PATH}").read().split())
    assert "phnet_lane_draw" in exported
    assert built.phnet_abi_version() == 1


def test_lane_draw_validates_without_a_gpu(built):
    """Every refusal comes before any launch (no device is touched: this runs on a machine without one).  Non-null pointers are
    made-up addresses - a call that got past the checks would try to launch."""
    p = 0x1000
    csc = (ctypes.c_int32 * 10)(*[int(v) for v in yuv_matrix("bt601", False)])
    csc_p = ctypes.cast(csc, ctypes.c_void_p)

    def draw(points=p, count=p, lanes_num=p, slot=None, track_id=None, F=3, L=4, S=72, sx=160.0, sy=64.0, oy=0.0, out_h=64, out_w=160,
             lane_width=12, src=None, fmt=0, stride=0, pitch=0, chroma=0, csc=None, palette=p, alpha=256, label=p, overlay=p):
        return built.phnet_lane_draw(points, count, lanes_num, slot, track_id, F, L, S, sx, sy, oy, out_h, out_w, lane_width, src, fmt,
                                     stride, pitch, chroma, csc, palette, alpha, label, overlay, None)

    for key in ("points", "count", "lanes_num"):                               # null required pointers
        assert draw(**{key: None}) == ERR_ARG, key
    assert draw(points=p + 4) == ERR_ARG                                        # points are read as (x, y) pairs
    assert draw(label=None, overlay=None) == ERR_ARG                            # no output requested
    assert draw(palette=None) == ERR_ARG                                        # an overlay needs its colours
    assert draw(track_id=p) == ERR_ARG                                          # track_id without slot
    for key, bads in (("F", (0, -1, 1 << 31, 1 << 40)), ("L", (0, -1, 65)), ("S", (1, 0, -1, 257)), ("out_h", (0, -1, 4097)),
                      ("out_w", (0, -1, 4097)), ("lane_width", (0, -1, 257)), ("alpha", (-1, 257)), ("fmt", (-1, 4))):
        for bad in bads:
            assert draw(**{key: bad}) == ERR_ARG, (key, bad)
    assert draw(F=(1 << 31) // (2 * 8), out_h=64, out_w=160) == ERR_ARG         # F * tiles = 2^31: the grid cannot hold it
    for key in ("sx", "sy", "oy"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert draw(**{key: bad}) == ERR_ARG, (key, bad)
    # sources.  rgb 64x160: rows of 480 bytes; nv12: 64 luma rows + 32 chroma rows of 160 bytes; yuyv: rows of 320 bytes
    rgb = dict(src=p, fmt=1, stride=64 * 480, pitch=480)
    nv12 = dict(src=p, fmt=2, stride=96 * 160, pitch=160, chroma=64 * 160, csc=csc_p)
    yuyv = dict(src=p, fmt=3, stride=64 * 320, pitch=320, csc=csc_p)
    for good in (rgb, nv12, yuyv):
        assert draw(**{**good, "src": None}) == ERR_ARG                         # a format without frames
        assert draw(**{**good, "pitch": good["pitch"] - 1}) == ERR_ARG
        assert draw(**{**good, "stride": good["stride"] - 1}) == ERR_ARG        # frames would overlap
        assert draw(**{**good, "label": p, "overlay": None, "stride": 0}) == ERR_ARG   # checked whichever output is asked for
    assert draw(**{**nv12, "chroma": 64 * 160 - 1}) == ERR_ARG
    for good in (nv12, yuyv):
        assert draw(**{**good, "csc": None}) == ERR_ARG
        assert draw(**good, out_w=159) == ERR_ARG                               # odd sizes for subsampled formats
    assert draw(**nv12, out_h=63) == ERR_ARG
    wild = (ctypes.c_int32 * 10)(16, *([1 << 23] * 9))                          # a coefficient outside 24 bits
    assert draw(**{**nv12, "csc": ctypes.cast(wild, ctypes.c_void_p)}) == ERR_ARG
    # a source whose frame spans >= 2^31 bytes: 4096 rows of a pitch of 2^20 bytes
    big = 1 << 20
    assert draw(src=p, fmt=1, out_h=4096, out_w=4096, pitch=big, stride=4096 * big) == ERR_ARG
    assert draw(src=p, fmt=3, out_h=4096, out_w=4096, pitch=big, stride=4096 * big, csc=csc_p) == ERR_ARG
    assert draw(src=p, fmt=2, out_h=4096, out_w=4096, pitch=big, stride=6144 * big, chroma=4096 * big, csc=csc_p) == ERR_ARG
    from phnet_amd import hip_ops as K
    assert (K.LANE_DRAW_MAX_SIZE, K.LANE_DRAW_MAX_WIDTH, K.LANE_DRAW_COORD_BOUND) == (4096, 256, OC.COORD_BOUND)
    header = open(_lib.HEADER).read()
    assert "outside [-8192, 8192]" in header and "PARITY UNPINNED against cv2.line" in header


def test_draw_kernels_compile_without_scratch_or_spills(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/lane_draw.hip: the eight instances (four sources x wide / byte stores) of one kernel,
    no scratch, no spilled registers."""
    src = os.path.join(hip_build.CSRC, "lane_draw.hip")
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "lane_draw.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == 8 and all("lane_draw_kernel" in n for n in names), names
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", out.stderr)]
        assert len(vals) == 8 and not any(vals), (key, vals)
    print("VGPRs:", re.findall(r" VGPRs: (\d+)", out.stderr), "occupancy:", re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr))


SEGMENT_SETS = {                     # integer poly-lines on a 40 x 56 image
    "diagonal": [(3, 4), (20, 30), (50, 35)],
    "single point": [(10, 10), (10, 10)],
    "axis-parallel": [(5, 8), (30, 8), (30, 33), (30, 8)],
    "leaves the image": [(-40, 20), (25, -30), (90, 15), (30, 70), (-5, 45)],
    "all outside": [(-30, -30), (-10, -50)],
    "repeats": [(12, 12), (12, 12), (40, 20), (40, 20), (13, 37)],
}


@pytest.mark.parametrize("lane_width", [1, 2, 5, 12, 31])
def test_coverage_equals_raster_lane(lane_width):
    """Rule 2 of the restatement on one lane == oracle.culane_cpu.raster_lane on the same integer segments."""
    H, W = 40, 56
    for name, pts in SEGMENT_SETS.items():
        pix = np.asarray(pts, dtype=np.int64)
        segs = [(*a, *b) for a, b in zip(pts[:-1], pts[1:])]
        want = culane_cpu.raster_lane(segs, H, W, lane_width)
        got = OC.cover(pix, H, W, lane_width)
        assert np.array_equal(got, want), (name, lane_width)
    assert OC.cover(np.asarray(SEGMENT_SETS["diagonal"]), H, W, lane_width).any()
    assert not OC.cover(np.asarray([(3, 4)]), H, W, lane_width).any()           # one survivor draws nothing


def test_point_mapping_equals_python_int():
    """Rule 1 == int(np.float64(np.float32(x)) * size [+ offset]) on a sweep with negative products (a negative scale, a negative
    offset), values just below an integer, and the values the rule skips."""
    below = [np.nextafter(np.float32(k / 160.0), np.float32(0)) for k in range(1, 160, 7)]
    xs = np.asarray([0.5, 1.0, 1e-6, 0.999999, 37.0 / 53.0, 2.5, 50.0, 51.2, 51.21] + below + list(np.linspace(0.001, 1.3, 97)),
                    dtype=np.float32)
    for sx, sy, oy in ((160.0, 64.0, 0.0), (1920.0, 800.0, 480.0), (53.0, 45.0, -8.0), (-160.0, 64.0, -70.5), (4096.0, 33.3, 0.25)):
        xy = np.stack([xs, xs[::-1]], axis=1)
        want = []
        for x, y in xy:
            px, py = int(np.float64(np.float32(x)) * sx), int(np.float64(np.float32(y)) * sy + oy)
            if abs(px) <= OC.COORD_BOUND and abs(py) <= OC.COORD_BOUND:
                want.append((px, py))
        got = OC.map_points(xy, sx, sy, oy)
        assert got.tolist() == [list(p) for p in want], (sx, sy, oy)
        assert len(want) > 50
    assert any(int(np.float64(x) * 160.0) != int(round(float(x) * 160.0)) for x in below)      # truncation, not rounding, is what is tested
    skipped = np.asarray([(0.0, 0.5), (-0.1, 0.5), (0.5, 0.0), (0.5, -1.0), (np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf),
                          (1e30, 0.5), (8194.0 / 160.0, 0.5)], dtype=np.float32)
    assert len(OC.map_points(skipped, 160.0, 64.0, 0.0)) == 0
    assert OC.map_points(np.asarray([(8192.0 / 160.0, 0.5)], dtype=np.float32), 160.0, 64.0, 0.0).tolist() == [[8192, 32]]


@pytest.mark.parametrize("fmt", ["nv12", "yuyv"])
def test_source_conversion_equals_pixfmt_cases(fmt):
    """Rule 5's source pixel (the folded form the kernel computes) == the numpy conversion of tests/pixfmt_cases.py, on random
    and saturating surfaces with padded pitch / surface rows, for both standards and both ranges."""
    H, W, _, _, _, layouts = PC.GEOMETRIES["a"]
    pitch, rows = layouts[fmt]
    pitch, rows, _ = PC.layout(fmt, H, W, pitch, rows)
    surf = PC.random_surfaces(fmt, 3, H, W, pitch, rows, seed=5)
    for standard, full in PC.MATRICES:
        csc = yuv_matrix(standard, full)
        assert np.array_equal(OC.source_rgb(fmt, surf, H, W, pitch, rows, csc), PC.TO_RGB[fmt](surf, H, W, pitch, rows, csc)), (standard, full)


def test_restatement_order_value_and_blend():
    """Rules 3-5 of the restatement on the literal frames: the lane lying on another owns every pixel of it; values follow
    track ids; alpha = 256 replaces, alpha = 0 keeps the source, 128 is the rounded mean."""
    P, count, num = OC.adversarial_frames()
    H, W = 37, 53
    geo = dict(out_hw=(H, W), sx=W, sy=H + 8, oy=-8, lane_width=5)
    ref = OC.draw_reference(P, count, num, **geo)["label_map"]
    assert not (ref[0] == 1).any() and (ref[0] == 3).any() and (ref[0] == 2).any() and (ref[0] == 4).any()
    assert not ref[3].any() and set(np.unique(ref[4])) == {0, 3, 4} and set(np.unique(ref[2])) == {0, 1, 2, 3}
    slot = np.tile(np.array([3, 2, 1, 0], dtype=np.int32), (5, 1))
    ids = np.tile(np.array([509, 255, 0, 254], dtype=np.int32), (5, 1))
    tracked = OC.draw_reference(P, count, num, slot=slot, track_id=ids, **geo)["label_map"]
    assert set(np.unique(tracked[0])) == {0, 255, 1} and [OC.lane_value(k, slot[0], ids[0]) for k in range(4)] == [254, 255, 1, 1]
    from phnet_amd.overlay import default_palette
    pal = default_palette()
    src = np.random.default_rng(0).integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    full = OC.draw_reference(P, count, num, src_rgb=src, palette=pal, alpha=256, **geo)["overlay"]
    none = OC.draw_reference(P, count, num, src_rgb=src, palette=pal, alpha=0, **geo)["overlay"]
    half = OC.draw_reference(P, count, num, src_rgb=src, palette=pal, alpha=128, **geo)["overlay"]
    assert np.array_equal(none, src) and np.array_equal(full, np.where((ref > 0)[..., None], pal[ref], src))
    assert np.array_equal(half[ref > 0], ((src[ref > 0].astype(int) + pal[ref][ref > 0] + 1) >> 1).astype(np.uint8))


def test_surface_exists_and_refuses_to_run_without_a_gpu():
    """render= defaults to None in the four signatures; the renderer has no CPU path; the palette is fixed."""
    from phnet_amd import hip_ops as K
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    from phnet_amd.libs.models import Router4OL, Router4OLV2
    from phnet_amd.overlay import LaneRenderer, default_palette
    from phnet_amd.stream import LaneStream, LaneStreamV2
    for fn in (LaneStream.__init__, LaneStreamV2.__init__, Router4OL.RouterOL.open_stream, Router4OLV2.RouterOL.open_stream):
        assert inspect.signature(fn).parameters["render"].default is None, fn
    pal = default_palette()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8 and not pal[0].any()
    assert len({tuple(c) for c in pal[1:]}) == 255 and (0, 0, 0) not in {tuple(c) for c in pal[1:]}
    assert np.array_equal(pal, default_palette()) and pal[1].tolist() == [255, 0, 0] and pal[2].tolist() == [0, 255, 77]
    pts, count, num = OC.random_lanes(2, 4, 8, seed=1)
    pl = dict(points=torch.from_numpy(pts), count=torch.from_numpy(count), lanes_num=torch.from_numpy(num))
    r = LaneRenderer((37, 53), sx=53, sy=37, oy=0)
    with pytest.raises(RuntimeError):
        r.render(pl)
    with pytest.raises(RuntimeError):
        K.lane_draw(pl["points"], pl["count"], pl["lanes_num"], (37, 53), 53.0, 37.0, 0.0)
    for bad in (dict(lane_width=0), dict(lane_width=257), dict(alpha=257), dict(label_map=False), dict(src_format="nv12")):
        with pytest.raises(ValueError):
            LaneRenderer((37, 53), sx=53, sy=37, oy=0, **bad)
    with pytest.raises(ValueError):
        LaneRenderer((4097, 53), sx=53, sy=37, oy=0)
    pre = ClipPreprocessor(64, 160, src_h=48, src_w=80, crop_size=16, device="cpu", pixel_format="nv12", pitch=96, surface_rows=52)
    r = LaneRenderer.for_preprocessor(pre, overlay=True, alpha=128)
    assert (r.out_h, r.out_w, r.sx, r.sy, r.oy) == (48, 80, 80.0, 32.0, 16.0)
    assert (r.src_format, r.pitch, r.chroma_offset, r.frame_shape) == ("nv12", 96, 52 * 96, pre.frame_shape)
    assert r.csc == [int(v) for v in yuv_matrix("bt601", False)]
