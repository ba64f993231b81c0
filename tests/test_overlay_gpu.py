"""Lane overlay on the MI355X (csrc/lane_draw.hip, phnet_amd/overlay.py): the kernel against the numpy restatement of its rules
(tests/overlay_cases.py draw_reference), then the stream and clip surfaces of both model families.

Everything the kernel computes is integer arithmetic on exactly specified inputs, so EVERY comparison is bit for bit
(np.array_equal); there is no tolerance in this file.  Output buffers are pre-filled with 0xA5, so an element the kernel does not
write shows."""
import numpy as np
import pytest
import torch

from phnet_amd.libs.dataset.openlane.preprocess import yuv_matrix
from tests import overlay_cases as OC
from tests import pixfmt_cases as PC
from tests import polyline_cases as C
from tests import synth
from tests.test_polylines_gpu import _build_v1, _build_v2, _tiny_v1

pytestmark = pytest.mark.gpu

POISON = 0xA5


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _geo(H, W):
    """Points of tests/overlay_cases.py: x in image widths, y with 8 rows above the image (y < 8 / (H + 8) leaves at the top)."""
    return dict(sx=float(W), sy=float(H + 8), oy=-8.0)


def _palette():
    from phnet_amd.overlay import default_palette
    return default_palette()


def _draw(pts, count, num, hw, geo, width, label=True, overlay=True, out=None, **kw):
    """hip_ops.lane_draw on numpy inputs -> numpy outputs; the output buffers are poisoned (or `out`, as it stands)."""
    from phnet_amd import hip_ops as K
    F, (H, W) = pts.shape[0], hw
    dev = "cuda"
    if out is None:
        out = dict(label_map=torch.full((F, H, W), POISON, dtype=torch.uint8, device=dev) if label else None,
                   overlay=torch.full((F, H, W, 3), POISON, dtype=torch.uint8, device=dev) if overlay else None)
    for key in ("slot", "track_id", "src"):
        if kw.get(key) is not None:
            kw[key] = torch.from_numpy(np.ascontiguousarray(kw[key])).to(dev)
    got = K.lane_draw(torch.from_numpy(pts).to(dev), torch.from_numpy(count).to(dev), torch.from_numpy(num).to(dev), hw, geo["sx"], geo["sy"],
                      geo["oy"], width, palette=torch.from_numpy(_palette()).to(dev) if overlay else None,
                      label_map=out["label_map"], overlay=out["overlay"], **kw)
    assert all(got[k] is None or got[k].data_ptr() == out[k].data_ptr() for k in got)
    return {k: None if v is None else v.cpu().numpy() for k, v in got.items()}, out


def _same(got, want, what):
    for key in ("label_map", "overlay"):
        if got[key] is None:
            continue
        bad = got[key] != want[key]
        assert not bad.any(), (what, key, int(bad.sum()), np.argwhere(bad)[:5].tolist())


# ---------------------------------------------------------------------------------------------------------------- the kernel
SIZES = {
    # (H, W): [(L, S, lane_width, seed)]  - F = 3 each.  37x53: no dimension a multiple of the tile or of 4 (byte stores, ragged tiles);
    # L = 64, S = 72 there puts thousands of segments on one tile (the LDS list is flushed several times); S = 256 fills every thread
    (37, 53): [(64, 72, 2, 1), (4, 5, 256, 2), (1, 2, 31, 100), (4, 72, 12, 4), (2, 256, 5, 5), (64, 72, 31, 6)],
    (64, 128): [(64, 72, 12, 7), (4, 5, 1, 8), (1, 72, 31, 9), (4, 2, 256, 10), (3, 256, 2, 11)],      # aligned: dword stores
    (33, 4096): [(4, 72, 12, 12), (64, 5, 31, 13), (1, 2, 256, 100)],                                  # the limits
    (4096, 8): [(4, 72, 12, 15), (64, 2, 2, 16), (1, 5, 256, 17)],
}


@pytest.mark.parametrize("hw", list(SIZES), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_kernel_equals_the_restatement_on_random_lanes(hw):
    """Label map and overlay (on black, alpha 256) on seeded random lanes: every L, S and width of the list above."""
    _gpu()
    H, W = hw
    lanes = 0
    for L, S, width, seed in SIZES[hw]:
        pts, count, num = OC.random_lanes(3, L, S, seed, reach=1.0 if max(H, W) < 1024 else 0.5)
        want = OC.draw_reference(pts, count, num, hw, lane_width=width, palette=_palette(), **_geo(H, W))
        got, _ = _draw(pts, count, num, hw, _geo(H, W), width)
        _same(got, want, (hw, L, S, width))
        lanes += int((want["label_map"] > 0).any(axis=(1, 2)).sum())
        assert (want["label_map"] > 0).any(), (L, S, width)
        print(f"{H}x{W} L={L} S={S} width={width}: {int((want['label_map'] > 0).sum())} lane pixels, values {np.unique(want['label_map'])[:8]}")
    assert lanes >= len(SIZES[hw])


@pytest.mark.parametrize("hw", [(37, 53), (64, 128)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("width", [1, 5, 12])
def test_kernel_equals_the_restatement_on_the_adversarial_frames(hw, width):
    """The literal frames of overlay_cases.adversarial_frames: crossing and coinciding lanes (order), lanes that leave the image
    and come back, far end points, skipped points, counts 0 and 1, lanes_num 0 and L, identical consecutive points."""
    _gpu()
    H, W = hw
    pts, count, num = OC.adversarial_frames()
    want = OC.draw_reference(pts, count, num, hw, lane_width=width, palette=_palette(), **_geo(H, W))
    got, _ = _draw(pts, count, num, hw, _geo(H, W), width)
    _same(got, want, (hw, width))
    assert not (want["label_map"][0] == 1).any() and (want["label_map"][0] == 3).any()      # the lane on top owns the shared pixels
    assert not want["label_map"][3].any() and not got["overlay"][3].any()                     # lanes_num = 0: a zero map, black


@pytest.mark.parametrize("L,S,seed", [(4, C.S_MAIN, 21), (8, C.S_ODD, 22)])
def test_kernel_draws_what_lane_points_writes(L, S, seed):
    """polyline_cases.random_frames rows through hip_ops.lane_points, its four tensors straight into the draw (the device-side
    hand-over of the stream step), at the reference's geometry scaled down: 64 x 160, crop 16."""
    _gpu()
    from phnet_amd import hip_ops as K
    kept, num = C.random_frames(24, L, S, seed)
    pl = K.lane_points(kept.cuda(), num.cuda(), C.head(S).prior_ys.cuda())
    hw, geo = (64, 160), dict(sx=160.0, sy=48.0, oy=16.0)
    got = K.lane_draw(pl["points"], pl["count"], pl["lanes_num"], hw, lane_width=3, label_map=True, overlay=False, **geo)
    want = OC.draw_reference(pl["points"].cpu().numpy(), pl["count"].cpu().numpy(), pl["lanes_num"].cpu().numpy(), hw, lane_width=3, **geo)
    assert np.array_equal(got["label_map"].cpu().numpy(), want["label_map"]) and got["overlay"] is None
    assert (want["label_map"] > 0).any() and int(want["label_map"].max()) > 1


SOURCES = [        # fmt, (H, W), pitch, surface_rows
    ("rgb", (37, 53), None, None), ("rgb", (64, 128), None, None),
    ("nv12", (38, 54), 70, 44), ("nv12", (64, 128), 192, 72), ("nv12", (64, 128), 131, 64),       # byte path; dword path; odd pitch
    ("yuyv", (37, 54), 121, None), ("yuyv", (64, 128), 320, None), ("yuyv", (64, 128), 258, None),
]


@pytest.mark.parametrize("fmt,hw,pitch,rows", SOURCES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_overlay_on_camera_frames(fmt, hw, pitch, rows):
    """Overlay on packed RGB, NV12 (pitch > width, surface_rows > height) and YUYV (padded pitch) frames with poisoned padding:
    bt601 and bt709 in both ranges, alpha 0, 1, 128, 255, 256, and the three output choices."""
    _gpu()
    H, W = hw
    F, L, S, width = 3, 4, 9, 7
    lanes, count, num = OC.random_lanes(F, L, S, seed=31)
    geo = _geo(H, W)
    if fmt == "rgb":
        surf = np.random.default_rng(32).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
        kw, matrices = dict(src=surf, src_format="rgb"), [None]
    else:
        pitch, rows, _ = PC.layout(fmt, H, W, pitch, rows)
        surf = PC.random_surfaces(fmt, F, H, W, pitch, rows, seed=32)
        kw = dict(src=surf, src_format=fmt, pitch=pitch, chroma_offset=rows * pitch if fmt == "nv12" else 0)
        matrices = PC.MATRICES
    runs = [(m, a, True, True) for m, a in zip(matrices, (128, 255, 1, 256))] + [(matrices[0], a, True, True) for a in (0, 1, 128, 255, 256)] \
        + [(matrices[-1], 128, False, True), (matrices[-1], 128, True, False)]
    for matrix, alpha, label, overlay in runs:
        csc = None if matrix is None else yuv_matrix(*matrix)
        rgb = OC.source_rgb(fmt, surf, H, W, pitch, rows, csc)
        want = OC.draw_reference(lanes, count, num, hw, lane_width=width, src_rgb=rgb, palette=_palette(), alpha=alpha, **geo)
        got, _ = _draw(lanes, count, num, hw, geo, width, label=label, overlay=overlay, alpha=alpha, csc=csc, **dict(kw))
        assert (got["label_map"] is None) == (not label) and (got["overlay"] is None) == (not overlay)
        _same(got, want, (fmt, hw, matrix, alpha, label, overlay))
        if overlay and alpha == 0:
            assert np.array_equal(got["overlay"], rgb)
    assert (want["label_map"] > 0).any() and not (want["label_map"] > 0).all()


def test_every_pixel_is_written_once_and_nothing_is_stale():
    """0xA5-filled buffers, one set of lanes; then ANOTHER set into the same buffers without clearing: both equal the restatement
    (no pixel keeps the poison or a lane of the first draw), on the byte path and on the dword path."""
    _gpu()
    for hw in ((37, 53), (64, 128)):
        H, W = hw
        first, second = OC.random_lanes(3, 4, 72, seed=41), OC.random_lanes(3, 4, 72, seed=42)
        got, bufs = _draw(*first, hw, _geo(H, W), 12)
        _same(got, OC.draw_reference(*first, hw, lane_width=12, palette=_palette(), **_geo(H, W)), ("first", hw))
        got, _ = _draw(*second, hw, _geo(H, W), 12, out=bufs)
        want = OC.draw_reference(*second, hw, lane_width=12, palette=_palette(), **_geo(H, W))
        _same(got, want, ("second", hw))
        assert (OC.draw_reference(*first, hw, lane_width=12, **_geo(H, W))["label_map"] != want["label_map"]).any()


def test_track_ids_choose_the_values():
    """slot + track_id with ids 0, 1, 254, 255, 509 (and -1): v = 1 + (id - 1) mod 254, 255 for a lane without an identity."""
    _gpu()
    hw = (37, 53)
    pts, count, num = OC.adversarial_frames()
    slot = np.tile(np.array([3, 2, 1, 0], dtype=np.int32), (5, 1))
    slot[1] = (0, 1, 2, -1)                                                       # a slot outside [0, L): no identity
    ids = np.array([[509, 255, 0, 254], [1, 254, 255, 7], [-1, 509, 1, 2], [1, 1, 1, 1], [254, 255, 509, 0]], dtype=np.int32)
    want = OC.draw_reference(pts, count, num, hw, lane_width=5, slot=slot, track_id=ids, palette=_palette(), **_geo(*hw))
    got, _ = _draw(pts, count, num, hw, _geo(*hw), 5, slot=slot, track_id=ids)
    _same(got, want, "tracks")
    assert set(np.unique(want["label_map"][0])) == {0, 1, 255} and set(np.unique(want["label_map"][1])) >= {1, 254, 255}
    assert [OC.lane_value(k, slot[4], ids[4]) for k in range(4)] == [255, 1, 1, 254]


@pytest.mark.parametrize("width", [1, 12, 31])
def test_label_map_agrees_with_the_evaluators_raster(width):
    """One lane: label_map > 0 == the bit mask hip_ops.lane_raster (the CULane evaluator's canvas) makes of the same integer
    segments and width."""
    _gpu()
    from phnet_amd import hip_ops as K
    hw = (64, 160)
    H, W = hw
    pts, count, num = OC.random_lanes(1, 1, 72, seed=50 + width)
    count[:], num[:] = 72, 1
    got, _ = _draw(pts, count, num, hw, _geo(H, W), width, overlay=False)
    pix = OC.map_points(pts[0, 0], **_geo(H, W))
    assert len(pix) > 8
    segs = np.concatenate([pix[:-1], pix[1:], np.zeros((len(pix) - 1, 1), dtype=np.int64)], axis=1).astype(np.int32)
    words = K.lane_raster(torch.from_numpy(segs).cuda(), 1, H, W, width).cpu().numpy()[0]
    bits = ((words[:, :, None].astype(np.int64) >> np.arange(32)) & 1).reshape(H, -1)[:, :W].astype(bool)
    assert bits.any() and np.array_equal(got["label_map"][0] > 0, bits)


# ---------------------------------------------------------------------------------------------------------------- streams, clips
def _build(family):
    return _build_v1(_tiny_v1(), conf_threshold=0.3) if family == "v1" else _build_v2(_tiny_v2())


def _tiny_v2():
    from oracle import phnet_cpu_v2 as O2
    return O2.GeometryV2(img_h=64, img_w=160)


def _run_streams(model, s, plain, frames_per_step):
    """Both streams over the same frames with torch's sync debug mode at "error" -> per step (out, out_plain, polylines, tracks,
    rendered), cloned on the device."""
    probe = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    steps = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        for frames in frames_per_step:
            out = [x.clone() for x in s.step(frames)]
            steps.append((out, [x.clone() for x in plain.step(frames)], {k: v.clone() for k, v in s.polylines.items()},
                          {k: v.clone() for k, v in s.tracks.items()}, {k: None if v is None else v.clone() for k, v in s.rendered.items()}))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert honoured, "torch.cuda.set_sync_debug_mode('error') did not flag .item()"
    return steps


def _check_steps(steps, r, src_rgb_of=None):
    """Each step's `rendered` == draw_reference of that step's own polylines / tracks; the step's three tensors == the plain
    stream's.  Returns the number of frames that show a lane."""
    shown = 0
    for t, (out, out_plain, pl, tracks, rendered) in enumerate(steps):
        for a, b, name in zip(out, out_plain, ("kept_rows", "num", "anchors")):
            assert torch.equal(a, b), (t, name)
        want = OC.draw_reference(pl["points"].cpu().numpy(), pl["count"].cpu().numpy(), pl["lanes_num"].cpu().numpy(), (r.out_h, r.out_w),
                                 r.sx, r.sy, r.oy, r.lane_width, slot=pl["slot"].cpu().numpy(), track_id=tracks["track_id"].cpu().numpy(),
                                 src_rgb=None if src_rgb_of is None else src_rgb_of(t), palette=r.palette, alpha=r.alpha)
        _same({k: None if v is None else v.cpu().numpy() for k, v in rendered.items()}, want, f"step {t}")
        shown += int((want["label_map"] > 0).any(axis=(1, 2)).sum())
    return shown


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_stream_renders_inside_the_captured_step(family):
    """open_stream(polylines=True, track=True, render=r, graph=True), B = 2, 5 frames: `rendered` (label map + 50/50 overlay on
    black, colours by track) is the restatement of each step's own polylines and tracks; kept_rows / num / anchors are
    bit-identical to a stream opened without render=; no synchronising copy occurs in a step."""
    from phnet_amd.overlay import LaneRenderer
    model = _build(family)
    g, B, T = (_tiny_v1() if family == "v1" else _tiny_v2()), 2, 5
    hw = (g.img_h, g.img_w)
    clips = torch.stack([synth.make_clip(g, T, seed=42 + b) for b in range(B)]).cuda()
    r = LaneRenderer(hw, sx=g.img_w, sy=g.img_h, oy=0, lane_width=5, alpha=128, label_map=True, overlay=True)
    with pytest.raises(ValueError):
        model.open_stream(streams=B, frame_hw=hw, graph=False, render=r)            # render= needs polylines=True
    s = model.open_stream(streams=B, frame_hw=hw, graph=True, polylines=True, track=True, render=r)
    plain = model.open_stream(streams=B, frame_hw=hw, graph=True, polylines=True, track=True)
    assert plain.rendered is None and s.graph is not None
    static = {k: v.data_ptr() for k, v in s.rendered.items()}
    steps = _run_streams(model, s, plain, [clips[:, t] for t in range(T)])
    assert {k: v.data_ptr() for k, v in s.rendered.items()} == static             # the graph's static outputs
    assert tuple(s.rendered["label_map"].shape) == (B, *hw) and tuple(s.rendered["overlay"].shape) == (B, *hw, 3)
    assert _check_steps(steps, r) > 0


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_stream_overlays_the_raw_nv12_frame(family):
    """The same with raw= NV12 surfaces of 48 x 80 (pitch 96, 52 surface rows, crop 16) and a renderer made by for_preprocessor:
    the overlay is drawn on the converted camera frame at the camera's resolution; with no lanes it IS the converted frame."""
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    from phnet_amd.overlay import LaneRenderer
    model = _build(family)
    g, B, T = (_tiny_v1() if family == "v1" else _tiny_v2()), 2, 5
    hw = (g.img_h, g.img_w)
    H0, W0, pitch, rows = 48, 80, 96, 52
    pre = ClipPreprocessor(*hw, src_h=H0, src_w=W0, crop_size=16, pixel_format="nv12", pitch=pitch, surface_rows=rows, matrix="bt709")
    r = LaneRenderer.for_preprocessor(pre, lane_width=3, alpha=256, label_map=True, overlay=True)
    surf = PC.random_surfaces("nv12", T * B, H0, W0, pitch, rows, seed=61).reshape(T, B, *pre.frame_shape)
    frames = torch.from_numpy(surf).cuda()
    s = model.open_stream(streams=B, frame_hw=hw, graph=True, raw=pre, polylines=True, track=True, render=r)
    plain = model.open_stream(streams=B, frame_hw=hw, graph=True, raw=pre, polylines=True, track=True)
    steps = _run_streams(model, s, plain, [frames[t] for t in range(T)])
    csc = yuv_matrix("bt709", False)
    rgb = OC.source_rgb("nv12", surf.reshape(T * B, *pre.frame_shape), H0, W0, pitch, rows, csc).reshape(T, B, H0, W0, 3)
    _check_steps(steps, r, src_rgb_of=lambda t: rgb[t])
    assert tuple(s.rendered["overlay"].shape) == (B, H0, W0, 3)
    none = {k: (torch.zeros_like(v) if k == "lanes_num" else v) for k, v in s.polylines.items()}
    empty = r.render(none, frames=frames[T - 1], tracks=s.tracks)
    assert np.array_equal(empty["overlay"].cpu().numpy(), rgb[T - 1]) and not bool(empty["label_map"].any())
    other = LaneRenderer((H0, W0), sx=W0, sy=H0 - 16, oy=16, overlay=True)
    with pytest.raises(ValueError):                                                # a renderer for other frames than the stream takes
        model.open_stream(streams=B, frame_hw=hw, graph=False, raw=pre, polylines=True, render=other)


def test_clips_render_like_their_frames():
    """The clip path: render on the polylines of infer_points_device with leading dimensions [B,T] == frame-by-frame calls, and
    == the restatement; out= writes into the caller's buffers."""
    from phnet_amd.overlay import LaneRenderer
    g, B, T = _tiny_v1(), 2, 3
    model = _build_v1(g, conf_threshold=0.3)
    clips = torch.stack([synth.make_clip(g, T, seed=50 + b) for b in range(B)]).cuda()
    with torch.no_grad():
        rows, nums, anchors, pl = model.infer_points_device(clips)
    hw = (g.img_h, g.img_w)
    r = LaneRenderer(hw, sx=g.img_w, sy=g.img_h, oy=0, lane_width=5, label_map=True, overlay=True)
    bufs = r.buffers((B, T), "cuda")
    got = r.render(pl, out=bufs)
    assert tuple(got["label_map"].shape) == (B, T, *hw) and tuple(got["overlay"].shape) == (B, T, *hw, 3)
    assert got["label_map"].data_ptr() == bufs["label_map"].data_ptr() and got["overlay"].data_ptr() == bufs["overlay"].data_ptr()
    flat = {k: v.reshape(B * T, *v.shape[2:]).cpu().numpy() for k, v in pl.items()}
    want = OC.draw_reference(flat["points"], flat["count"], flat["lanes_num"], hw, r.sx, r.sy, r.oy, 5, palette=r.palette)
    _same({k: v.reshape(B * T, *v.shape[2:]).cpu().numpy() for k, v in got.items()}, want, "clips")
    assert (want["label_map"] > 0).any()
    for b in range(B):
        for t in range(T):
            one = r.render({k: v[b, t] for k, v in pl.items()})
            assert tuple(one["label_map"].shape) == hw
            assert torch.equal(one["label_map"], got["label_map"][b, t]) and torch.equal(one["overlay"], got["overlay"][b, t])
