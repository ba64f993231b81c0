"""Training augmentation on the MI355X (csrc/augment.hip, csrc/lane_targets.hip rule 0b, phnet_amd/libs/dataset/openlane/augment.py)
against the restatement of tests/augment_cases.py.

Bounds.  Image: the augmented 8-bit image equals the restatement exactly (integers from the taps to the bytes; rule 1 is the same
float64 operations, not contracted, and its result is rounded to 1/32 px), and the float output equals the float32 epilogue of those
bytes bit for bit, in both layouts.  Labels: the project's rule for this kernel (tests/test_targets_gpu.py): flags, [2], [5] and the
-1e5 pattern exact, [3], [4] and the xs within 2 float32 ulps - kernel and restatement perform the same float64 operations in the same
order; every case keeps its samples 1e-3 px from the image border (asserted in tests/test_augment_cpu.py).  Launch shapes against each
other (null against identity tables, a replayed graph against eager) are compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import augment_cases as AC
from tests import target_cases as C

pytestmark = pytest.mark.gpu

ULPS = 2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _augmenter(shape):
    from phnet_amd.libs.dataset.openlane.augment import ClipAugmenter
    _, H, W = AC.SHAPES[shape]
    return ClipAugmenter(H, W, mean=AC.MEAN, std=AC.STD, device="cuda")


def _encoder():
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder
    g = C.geometry("tiny")
    return TargetEncoder(g["img_h"], g["img_w"], g["S"], g["R"], src_h=g["img_h"], src_w=g["img_w"], crop_size=0, device="cuda")      # the identity map


def _packed_labels():
    from phnet_amd.libs.dataset.openlane.targets import pack_annotations
    return tuple(t.cuda() for t in pack_annotations(AC.label_frames(), C.LIN, 16))


@pytest.mark.parametrize("shape", list(AC.SHAPES))
@pytest.mark.parametrize("name", list(AC.PARAM_SETS))
def test_image_equals_the_restatement(shape, name):
    _need_gpu()
    aug = _augmenter(shape)
    frames = torch.from_numpy(np.array(AC.frames(shape))).cuda()
    params = AC.params(shape, name).to("cuda")
    want_u8, _ = AC.expected(shape, name)
    for layout in ("nchw", "nhwc4"):
        out = torch.full((frames.shape[0], 3) + tuple(frames.shape[1:3]) if layout == "nchw" else tuple(frames.shape[:3]) + (4,), float("nan"),
                         device="cuda")
        got, got_u8 = aug(frames, params, layout=layout, out=out, return_u8=True)
        assert got.data_ptr() == out.data_ptr()
        got_u8 = got_u8.cpu().numpy()
        bad = np.argwhere(got_u8 != want_u8)
        assert len(bad) == 0, (shape, name, layout, len(bad), bad[:4].tolist(), got_u8[tuple(bad[0])], want_u8[tuple(bad[0])])
        want = AC.epilogue(want_u8, layout)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (shape, name, layout)
    plain = aug(frames, params)                                                       # without out_u8 the same floats
    assert torch.equal(_bits(plain), _bits(torch.from_numpy(AC.epilogue(want_u8, "nchw")).cuda()))


@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_identity_table_equals_the_plain_preprocessor(fmt):
    """The anchor: behind pre(frames, return_u8=True), an identity table gives pre(frames)'s floats bit for bit; and pre(..., augment=)
    is those two launches."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams, ClipAugmenter
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    T, sh, sw, crop = 3, 98, 134, 12
    pre = ClipPreprocessor(37, 53, src_h=sh, src_w=sw, crop_size=crop, device="cuda", pixel_format=fmt)
    rng = np.random.default_rng(21)
    frames = torch.from_numpy(rng.integers(0, 256, (T,) + pre.frame_shape, dtype=np.uint8)).cuda()
    aug = ClipAugmenter.for_preprocessor(pre)
    ident = AugmentParams.identity(T).to("cuda")
    for layout in ("nchw", "nhwc4"):
        want = pre(frames, layout=layout)
        _, u8 = pre(frames, layout=layout, return_u8=True)
        got, got_u8 = aug(u8, ident, layout=layout, return_u8=True)
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(got_u8, u8), (fmt, layout)
        both, both_u8 = pre(frames, layout=layout, augment=ident, return_u8=True)
        assert torch.equal(_bits(both), _bits(want)) and torch.equal(both_u8, u8), (fmt, layout)
    # and a table that does something, through the preprocessor, equals the restatement on the resized bytes
    params = AugmentParams.build([AC.PARAM_SETS["everything"][t] for t in range(T)], 37, 53)
    n = params.numpy()
    _, u8 = pre(frames, return_u8=True)
    want_u8, _ = AC.augment(u8.cpu().numpy(), n["flip2"], n["inv"], n["table"])
    got, got_u8 = pre(frames, augment=params.to("cuda"), return_u8=True)
    assert np.array_equal(got_u8.cpu().numpy(), want_u8) and not np.array_equal(want_u8, u8.cpu().numpy())
    assert np.array_equal(got.cpu().numpy().view(np.int32), AC.epilogue(want_u8).view(np.int32))


def test_labels_null_and_identity_equal_the_plain_entry():
    _need_gpu()
    from phnet_amd import hip_ops as K
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    enc = _encoder()
    pts, cnt, num = _packed_labels()
    want = enc(pts, cnt, num)
    ident = AugmentParams.identity(pts.shape[0]).to("cuda")
    assert torch.equal(_bits(enc(pts, cnt, num, augment=ident)), _bits(want))
    args = (pts, cnt, num, enc.offsets_ys, enc.max_lanes, enc.out_h, enc.out_w, enc.strip_size)
    kw = dict(crop=enc.crop, src_w=enc.src_w, scale_x=enc.scale_x, scale_y=enc.scale_y)
    for flip2, fwd in ((None, None), (ident.flip2, None), (None, ident.fwd)):
        assert torch.equal(_bits(K.lane_targets_aug(*args, flip2, fwd, **kw)), _bits(want))
    # the hand and random cases of the main geometry too: null arrays are the old entry on everything it is tested on
    g = C.geometry("main")
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder
    big = TargetEncoder(g["img_h"], g["img_w"], g["S"], g["R"], src_h=g["img_h"], src_w=g["img_w"], crop_size=0, device="cuda")
    p2, c2, n2 = (torch.from_numpy(a).cuda() for a in C.pack([c["lanes"] for c in C.cases("main")]))
    a2 = (p2, c2, n2, big.offsets_ys, big.max_lanes, big.out_h, big.out_w, big.strip_size)
    k2 = dict(crop=big.crop, src_w=big.src_w, scale_x=big.scale_x, scale_y=big.scale_y)
    assert torch.equal(_bits(K.lane_targets_aug(*a2, None, None, **k2)), _bits(big(p2, c2, n2)))
    assert torch.equal(_bits(big(p2, c2, n2, augment=AugmentParams.identity(p2.shape[0]).to("cuda"))), _bits(big(p2, c2, n2)))


@pytest.mark.parametrize("name", AC.LABEL_SETS)
def test_labels_equal_the_restatement(name):
    _need_gpu()
    enc = _encoder()
    pts, cnt, num = _packed_labels()
    want, _ = AC.expected_labels(name)
    got = enc(pts, cnt, num, augment=AC.params("tiny", name).to("cuda")).cpu().numpy()
    worst = C.assert_rows_match(got, want, ULPS, name)
    print(name, "valid rows", int(want[..., 1].sum()), "worst ulps", worst)


def test_labels_behind_the_camera_map():
    """Rule 0b behind a real rule 0: annotations at 1280 x 1920, crop 480, flipped, onto 64 x 160."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
    frames = C.source_frames(31, 3)
    enc = TargetEncoder(64, 160, 36, 4, device="cuda")
    pts, cnt, num = (t.cuda() for t in pack_annotations(frames, 4, 32))
    p = AC.params("tiny", "everything")
    n = p.numpy()
    mp = C.map_for(64, 160, 1280, 1920, 480, flip=True)
    enc_cpu = [AC.encode_frame_aug(lanes, 64, 160, 36, 4, n["flip2"][t], n["fwd"][t], mapping=mp) for t, lanes in enumerate(frames)]
    want = np.stack([lab for lab, _ in enc_cpu])
    assert all(min(abs(x), abs(x - 160.0)) >= AC.LABEL_MARGIN for _, infos in enc_cpu for i in infos for x in i["sampled"])
    got = enc(pts, cnt, num, flip=True, augment=p.to("cuda")).cpu().numpy()
    print("valid rows", int(want[..., 1].sum()), "worst ulps", C.assert_rows_match(got, want, ULPS, "camera map"))
    assert want[..., 1].sum() >= 3 and not np.array_equal(got, enc(pts, cnt, num, flip=True).cpu().numpy())


@pytest.mark.parametrize("name", ["affine_pos", "affine_neg"])
def test_image_and_labels_agree(name):
    """A 3 x 3 white blob on an annotated point of a vertical lane, warped by both halves: the intensity centroid of the kernel's image
    lies within 0.5 px of fwd applied to the point, and the kernel's label row passes through it within 0.5 px.  A transposed matrix, a
    wrong centre or a wrong rotation sign in either half moves one of them by pixels (tests/test_augment_cpu.py holds the
    restatement to the same bound)."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.targets import pack_annotations
    g = C.geometry("tiny")
    params = AC.params("tiny", name)
    fwd = params.numpy()["fwd"][0].reshape(2, 3)
    dev = params.to("cuda")
    _, u8 = _augmenter("tiny")(torch.from_numpy(AC.blob_frames()).cuda(), dev, return_u8=True)
    pts, cnt, num = (t.cuda() for t in pack_annotations([[AC.BLOB_LANE]] * 3, C.LIN, 16))
    rows = _encoder()(pts, cnt, num, augment=dev).cpu().numpy()
    cx, cy = AC.centroid(u8[0].cpu().numpy())
    wx, wy = fwd @ [AC.BLOB_XY[0], AC.BLOB_XY[1], 1.0]
    lx = AC.lane_x_at(rows[0, 0], cy, g["img_h"], g["S"])
    print(name, "centroid", (cx, cy), "fwd(point)", (wx, wy), "lane at the centroid's y", lx)
    assert np.hypot(cx - wx, cy - wy) <= AC.BLOB_BOUND
    assert rows[0, 0, 1] == 1 and rows[0, 0, 2] == 0 and abs(lx - cx) <= AC.BLOB_BOUND


def test_captured_graph_reads_the_table_at_replay():
    """pre(..., augment=, out=) and enc(..., augment=, out=) captured in ONE graph; a replay after copy_into of another table equals the
    eager result for that table."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder
    T, H, W = AC.SHAPES["tiny"]
    pre = ClipPreprocessor(H, W, src_h=100, src_w=200, crop_size=10, device="cuda")
    enc = TargetEncoder.for_preprocessor(pre, 36, 4)
    rng = np.random.default_rng(33)
    frames = torch.from_numpy(rng.integers(0, 256, (T, 100, 200, 3), dtype=np.uint8)).cuda()
    lanes = [[[(x * 200.0 / 160.0, 10.0 + y * 90.0 / 64.0) for x, y in lane] for lane in f] for f in AC.label_frames()]
    from phnet_amd.libs.dataset.openlane.targets import pack_annotations
    pts, cnt, num = (t.cuda() for t in pack_annotations(lanes, C.LIN, 16))
    tables = [AC.params("tiny", n) for n in ("affine_pos", "everything", "identity")]
    live = tables[0].to("cuda")
    clip = torch.full((T, 3, H, W), float("nan"), device="cuda")
    rows = torch.full((T, 4, 6 + 36), float("nan"), device="cuda")
    pre(frames, augment=live, out=clip); enc(pts, cnt, num, augment=live, out=rows)              # warm-up: the staging buffer exists
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pre(frames, augment=live, out=clip)
        enc(pts, cnt, num, augment=live, out=rows)
    seen = []
    for table in tables:
        table.copy_into(live)
        clip.fill_(float("nan")); rows.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        fresh = table.to("cuda")
        assert torch.equal(_bits(clip), _bits(pre(frames, augment=fresh))) and torch.equal(_bits(rows), _bits(enc(pts, cnt, num, augment=fresh)))
        seen.append((clip.clone(), rows.clone()))
    assert not torch.equal(_bits(seen[0][0]), _bits(seen[1][0])) and not torch.equal(_bits(seen[0][1]), _bits(seen[1][1]))
    assert torch.equal(_bits(seen[2][0]), _bits(pre(frames))) and torch.equal(_bits(seen[2][1]), _bits(enc(pts, cnt, num)))
