"""Camera pixel formats on the MI355X: phnet_preprocess_yuv (NV12 / YUYV surfaces in, colour conversion inside the pre-processing
launch) bit-exactly against the numpy conversion (tests/pixfmt_cases.py) followed by the pre-processing oracle
(oracle/preprocess_cpu.py) and against the RGB launch on the converted image; padding that must not matter; NV12 streams.

Bounds: out_u8 exact (integers all the way); the float tensor within 1e-6 of the oracle - the bound test_preprocess.py holds
(q/255 - mean)/std to - and torch.equal to the RGB kernel on the same 8-bit colours (one shared epilogue)."""
import functools

import numpy as np
import pytest
import torch

from oracle import preprocess_cpu as P
from tests import pixfmt_cases as C

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
T = 3


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=2)
def _surfaces(fmt, geom):
    h0, w0, _, _, _, lay = C.GEOMETRIES[geom]
    pitch, srows = lay[fmt]
    s = C.random_surfaces(fmt, T, h0, w0, pitch, srows, seed=h0 + (7 if fmt == "yuyv" else 0))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=2)
def _rgb(fmt, geom, standard, full):
    from phnet_amd.libs.dataset.openlane.preprocess import yuv_matrix
    h0, w0, _, _, _, lay = C.GEOMETRIES[geom]
    pitch, srows, _ = C.layout(fmt, h0, w0, *lay[fmt])
    rgb = C.TO_RGB[fmt](_surfaces(fmt, geom), h0, w0, pitch, srows, yuv_matrix(standard, full))
    rgb.setflags(write=False)
    return rgb


def _pre(fmt, geom, standard="bt601", full=False):
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    h0, w0, crop, oh, ow, lay = C.GEOMETRIES[geom]
    kw = {} if fmt == "rgb" else dict(pixel_format=fmt, pitch=lay[fmt][0], surface_rows=lay[fmt][1], matrix=standard, full_range=full)
    return ClipPreprocessor(oh, ow, src_h=h0, src_w=w0, crop_size=crop, mean=MEAN, std=STD, **kw)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("standard,full", C.MATRICES)
@pytest.mark.parametrize("geom", ["a", "b", "c", "d"])
@pytest.mark.parametrize("fmt", ["nv12", "yuyv"])
def test_yuv_preprocess_is_bit_exact(fmt, geom, standard, full, flip):
    _gpu()
    h0, w0, crop, oh, ow, _ = C.GEOMETRIES[geom]
    surf, rgb = _surfaces(fmt, geom), _rgb(fmt, geom, standard, full)
    for c in range(3):                                                                # the forced frames saturate both ends
        assert (rgb[:2, ..., c] == 0).any() and (rgb[:2, ..., c] == 255).any()
    want, want_u8 = P.preprocess_clip(rgb, crop, oh, ow, MEAN, STD, flip=flip)
    pre = _pre(fmt, geom, standard, full)
    assert tuple(surf.shape[1:]) == pre.frame_shape
    dev = torch.from_numpy(surf.copy()).cuda()
    got, got_u8 = pre(dev, flip=flip, return_u8=True)
    assert np.array_equal(got_u8.cpu().numpy(), want_u8)                              # the resampled 8-bit image: exact
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"{fmt} {geom} {standard} full={full} flip={flip}: max |float - oracle| = {err:.3e} (bound 1e-6)")
    assert err <= 1e-6
    via_rgb, via_rgb_u8 = _pre("rgb", geom)(torch.from_numpy(rgb.copy()).cuda(), flip=flip, return_u8=True)
    assert torch.equal(got, via_rgb) and torch.equal(got_u8, via_rgb_u8)              # one epilogue: the same bits
    assert torch.equal(pre(dev, flip=flip), got)                                      # without out_u8
    nhwc = pre(dev, flip=flip, layout="nhwc4")
    assert torch.equal(nhwc[..., :3].permute(0, 3, 1, 2), got) and float(nhwc[..., 3].abs().max()) == 0.0
    if geom == "b":
        img = rgb[:, :, ::-1] if flip else rgb
        assert np.array_equal(got_u8.cpu().numpy(), img)                              # identity resize: the converted image itself
    with pytest.raises(ValueError):
        pre(dev[:, :-1].contiguous())
    with pytest.raises(RuntimeError):
        pre(torch.from_numpy(surf.copy()))                                            # no CPU path


@pytest.mark.parametrize("fmt", ["nv12", "yuyv"])
def test_padding_and_extra_rows_never_influence_the_result(fmt):
    """Geometry a (pitch beyond the row, NV12 surface rows beyond the image) with the padding poisoned 0 / 255, then 255 / 0, then
    random: torch.equal outputs, both flips and both layouts."""
    _gpu()
    h0, w0, _, _, _, lay = C.GEOMETRIES["a"]
    pitch, srows, _ = C.layout(fmt, h0, w0, *lay[fmt])
    pad = C.padding_mask(fmt, h0, w0, pitch, srows)
    assert pad.any() and (fmt != "nv12" or (pad[h0:srows].all() and pad[srows + h0 // 2:].all()))
    base = _surfaces(fmt, "a")
    other = C.poison(base.copy(), fmt, h0, w0, pitch, srows, phase=1)
    noise = base.copy()
    noise[:, pad] = np.random.default_rng(3).integers(0, 256, (T, int(pad.sum())), dtype=np.uint8)
    assert (other != base).any() and (noise != base).any()
    assert np.array_equal(other[:, ~pad], base[:, ~pad]) and np.array_equal(noise[:, ~pad], base[:, ~pad])
    pre = _pre(fmt, "a", "bt709", False)
    for flip in (False, True):
        for layout in ("nchw", "nhwc4"):
            outs = [pre(torch.from_numpy(s.copy()).cuda(), flip=flip, layout=layout, return_u8=True) for s in (base, other, noise)]
            for o in outs[1:]:
                assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


def _model(family):
    if family == "v1":
        from oracle import phnet_cpu as O
        from phnet_amd.config import make_cfg
        from phnet_amd.libs.models.Router4OL import RouterOL
        from tests import synth
        g = O.Geometry(img_h=64, img_w=160, arch="resnet18", conf_threshold=0.3)
        model = RouterOL(make_cfg(img_h=g.img_h, img_w=g.img_w, arch=g.arch, conf_threshold=0.3), None)
        model.load_state_dict(synth.make_state(g), strict=True)
    else:
        from oracle import phnet_cpu_v2 as O2
        from phnet_amd.config import make_cfg_v2
        from phnet_amd.libs.models.Router4OLV2 import RouterOL
        from tests import synth
        g = O2.GeometryV2(img_h=64, img_w=160)
        model = RouterOL(make_cfg_v2(img_h=g.img_h, img_w=g.img_w, arch=g.arch, save_freq=1))
        model.load_state_dict(synth.make_state_v2(g), strict=True)
    return model.cuda().eval()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("family", ["v1", "v2"])
def test_nv12_stream_equals_rgb_stream(family, graph):
    """open_stream(raw=NV12 preprocessor) fed surfaces == open_stream(raw=RGB preprocessor) fed their numpy-converted RGB: the
    network input is the same bits, the launches after it are the same, so all three outputs are torch.equal on every step."""
    _gpu()
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor, yuv_matrix
    model = _model(family)
    assert model.stream_class == ("LaneStream" if family == "v1" else "LaneStreamV2")
    B, steps, h0, w0, crop, pitch, srows = 2, 4, 200, 300, 40, 320, 208
    nv12 = ClipPreprocessor(64, 160, src_h=h0, src_w=w0, crop_size=crop, pixel_format="nv12", pitch=pitch, surface_rows=srows)
    rgbp = ClipPreprocessor(64, 160, src_h=h0, src_w=w0, crop_size=crop)
    surf = C.random_surfaces("nv12", steps * B, h0, w0, pitch, srows, seed=11, extremes=False).reshape(steps, B, *nv12.frame_shape)
    rgb = C.nv12_to_rgb(surf, h0, w0, pitch, srows, yuv_matrix("bt601", False))
    surf_d, rgb_d = torch.from_numpy(surf).cuda(), torch.from_numpy(rgb).cuda()
    a = model.open_stream(streams=B, frame_hw=(64, 160), graph=graph, raw=nv12)
    b = model.open_stream(streams=B, frame_hw=(64, 160), graph=graph, raw=rgbp)
    assert tuple(a.frames.shape) == (B, *nv12.frame_shape) and tuple(b.frames.shape) == (B, h0, w0, 3)
    kept = 0
    for t in range(steps):
        got = tuple(x.clone() for x in a.step(surf_d[t]))
        want = b.step(rgb_d[t])
        for x, y, name in zip(got, want, ("kept_rows", "num", "anchors")):
            assert torch.equal(x, y), (t, name)
        kept += int(got[1].sum())
    assert kept > 0                                                                   # lanes were compared, not empty rows
    with pytest.raises(ValueError):
        a.step(rgb_d[0])                                                              # an NV12 stream takes NV12 surfaces only
