"""Line clipping in the training targets on the MI355X (csrc/lane_targets.hip rule 0c, phnet_lane_targets_clip, TargetEncoder(clip=True))
against the restatement of tests/clip_cases.py.

Tolerance: the project's rule for this kernel (tests/test_targets_gpu.py): flags, [2], [5] and the number and positions of -1e5 exact,
[3], [4] and the xs within 2 float32 ulps - kernel and restatement perform the same float64 operations in the same order, not
contracted; frag_count exact.  tests/test_lane_clip_cpu.py asserts that no predicate of the random cases is within 1e-3 px of flipping.
Launch shapes against each other (clip = 0 against phnet_lane_targets_aug, all-in frames with and without the rule, one frame per
launch, [B,T], out=, a replayed graph) are compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import augment_cases as AC
from tests import clip_cases as CC
from tests import target_cases as C

pytestmark = pytest.mark.gpu

ULPS = 2
NAMES = [g[0] for g in C.GEOMETRIES]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _encoder(name, **kw):
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder
    g = C.geometry(name)
    return TargetEncoder(g["img_h"], g["img_w"], g["S"], g["R"], src_h=g["img_h"], src_w=g["img_w"], crop_size=0, device="cuda", **kw)    # the identity map


def _packed(name):
    return tuple(torch.from_numpy(a).cuda() for a in CC.packed(name))


def _want(name, clip=True):
    exp = CC.expected(name, clip)
    return np.stack([lab for lab, _, _ in exp]), np.array([n for _, _, n in exp], np.int32)


@pytest.mark.parametrize("name", NAMES)
def test_all_cases_in_one_launch_equal_the_restatement(name):
    """The hand cases (identity rows) and the random cases (their 'basic' rows) of a geometry in ONE launch of the entry point."""
    _need_gpu()
    from phnet_amd import hip_ops as K
    g = C.geometry(name)
    enc = _encoder(name)
    pts, cnt, num = _packed(name)
    p = CC.params(name).to("cuda")
    frag = torch.full((pts.shape[0],), -7, dtype=torch.int32, device="cuda")
    got = K.lane_targets_clip(pts, cnt, num, enc.offsets_ys, g["R"], g["img_h"], g["img_w"], enc.strip_size, p.flip2, p.fwd, clip=True,
                              frag_count=frag).cpu().numpy()
    want, want_n = _want(name)
    assert got.shape == want.shape == (len(CC.cases(name)), g["R"], 6 + g["S"])
    worst = 0
    for f, c in enumerate(CC.cases(name)):
        worst = max(worst, C.assert_rows_match(got[f], want[f], ULPS, (name, c["name"])))
    assert frag.cpu().numpy().tolist() == want_n.tolist()
    print(name, "frames", len(want), "valid rows", int(want[..., 1].sum()), "worst ulps against the restatement:", worst)
    assert not np.array_equal(want, _want(name, clip=False)[0])


def test_the_long_lane_crosses_the_ballots():
    """254 points per lane, four ballots: runs that start in one group of 64 points and end in the next, and the row of the lane behind."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
    L = CC.LONG
    lanes, (want, _, want_n) = CC.long_case()
    enc = TargetEncoder(L["img_h"], L["img_w"], L["S"], L["R"], src_h=L["img_h"], src_w=L["img_w"], crop_size=0, device="cuda", clip=True)
    pts, cnt, num = (t.cuda() for t in pack_annotations([lanes, lanes[::-1]], L["lin"], L["pmax"], clip=True))
    frag = torch.zeros(2, dtype=torch.int32, device="cuda")
    got = enc(pts, cnt, num, frag_count=frag).cpu().numpy()
    print("worst ulps", C.assert_rows_match(got[0], want, ULPS, "long"))
    back = CC.encode_frame_clipped(lanes[::-1], L["img_h"], L["img_w"], L["S"], L["R"])
    C.assert_rows_match(got[1], back[0], ULPS, "long, short lane first")
    assert frag.tolist() == [want_n, back[2]] == [7, 7] and np.array_equal(got[1, 0], got[0, 6])


@pytest.mark.parametrize("name", NAMES)
def test_clip_off_is_the_aug_entry_and_all_in_frames_do_not_change(name):
    _need_gpu()
    from phnet_amd import hip_ops as K
    g = C.geometry(name)
    enc = _encoder(name)
    pts, cnt, num = _packed(name)
    p = CC.params(name).to("cuda")
    args = (pts, cnt, num, enc.offsets_ys, g["R"], g["img_h"], g["img_w"], enc.strip_size)
    aug = K.lane_targets_aug(*args, p.flip2, p.fwd)
    frag = torch.full((pts.shape[0],), -7, dtype=torch.int32, device="cuda")
    off = K.lane_targets_clip(*args, p.flip2, p.fwd, clip=False, frag_count=frag)
    assert torch.equal(_bits(off), _bits(aug)) and torch.equal(_bits(K.lane_targets_clip(*args, p.flip2, p.fwd, clip=False)), _bits(aug))
    assert frag.tolist() == _want(name, clip=False)[1].tolist() == [sum(len(lane) > 2 for lane in c["lanes"]) for c in CC.cases(name)]
    assert torch.equal(_bits(K.lane_targets_clip(*args, None, None, clip=False)), _bits(K.lane_targets(*args)))
    assert torch.equal(_bits(enc(pts, cnt, num, augment=p, clip=False)), _bits(aug)) and torch.equal(_bits(enc(pts, cnt, num, augment=p)), _bits(aug))
    on = K.lane_targets_clip(*args, p.flip2, p.fwd, clip=True)
    Wc, Hc = CC.rect(g["img_h"], g["img_w"])
    inside = [f for f, (c, row) in enumerate(zip(CC.cases(name), CC.table_rows(name)))
              if all(CC.is_in(q, Wc, Hc) for lane in c["lanes"] for q in CC.mapped_lane(lane, row, g["img_w"]))]
    assert len(inside) >= 3
    for f in inside:
        assert torch.equal(_bits(on[f]), _bits(aug[f])), CC.cases(name)[f]["name"]
    assert not torch.equal(_bits(on), _bits(aug))


def test_single_frames_and_clips_equal_the_flat_launch():
    _need_gpu()
    name = "main"
    enc = _encoder(name, clip=True)
    pts, cnt, num = _packed(name)
    p = CC.params(name)
    dev = p.to("cuda")
    n = pts.shape[0]
    frag = torch.zeros(n, dtype=torch.int32, device="cuda")
    whole = enc(pts, cnt, num, augment=dev, frag_count=frag)
    assert frag.tolist() == _want(name)[1].tolist()
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    for f in range(n):
        one_p = AugmentParams(*[x[f:f + 1].contiguous() for x in dev.tensors()])
        one_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        one = enc(pts[f:f + 1].contiguous(), cnt[f:f + 1].contiguous(), num[f:f + 1].contiguous(), augment=one_p, frag_count=one_n)
        assert torch.equal(_bits(one[0]), _bits(whole[f])) and int(one_n[0]) == int(frag[f]), CC.cases(name)[f]["name"]
    B, T = 4, n // 4
    frag_bt = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    sub = AugmentParams(*[x[:B * T].contiguous() for x in dev.tensors()])
    clips = enc(pts[:B * T].view(B, T, *pts.shape[1:]), cnt[:B * T].view(B, T, -1), num[:B * T].view(B, T), augment=sub, frag_count=frag_bt)
    assert tuple(clips.shape) == (B, T) + tuple(whole.shape[1:]) and torch.equal(_bits(clips).view(B * T, -1), _bits(whole[:B * T]).view(B * T, -1))
    assert torch.equal(frag_bt.view(-1), frag[:B * T])
    with pytest.raises(ValueError):
        enc(pts, cnt, num, augment=dev, frag_count=frag[:-1])
    with pytest.raises(ValueError):
        enc(pts, cnt, num, augment=dev, frag_count=frag.to(torch.int64))


def test_out_is_fully_overwritten_and_padding_is_never_read():
    _need_gpu()
    name = "fine"
    enc = _encoder(name, clip=True)
    dev = CC.params(name).to("cuda")
    pts, cnt, num = (a.copy() for a in CC.packed(name))
    cuda = lambda *a: tuple(torch.from_numpy(x).cuda() for x in a)                    # noqa: E731
    frag0 = torch.zeros(len(num), dtype=torch.int32, device="cuda")
    want = enc(*cuda(pts, cnt, num), augment=dev, frag_count=frag0)
    out = torch.full_like(want, float("nan"))
    got = enc(*cuda(pts, cnt, num), augment=dev, out=out)
    assert got.data_ptr() == out.data_ptr() and not bool(torch.isnan(out).any()) and torch.equal(_bits(out), _bits(want))
    rng = np.random.default_rng(19)
    junk = np.where(rng.random(pts.shape) < 0.3, np.nan, rng.standard_normal(pts.shape) * 1e4).astype(np.float32)
    junk[rng.random(pts.shape) < 0.1] = np.inf
    pad = np.arange(CC.PMAX)[None, None, :] >= cnt[:, :, None]
    pad |= (np.arange(CC.LIN)[None, :] >= num[:, None])[:, :, None]
    pts[pad] = junk[pad]
    beyond = np.arange(CC.LIN)[None, :] >= num[:, None]
    cnt[beyond] = rng.integers(-5, 400, cnt.shape)[beyond]
    assert pad.mean() > 0.5 and beyond.sum() > 20
    frag = torch.full_like(frag0, -3)
    assert torch.equal(_bits(enc(*cuda(pts, cnt, num), augment=dev, frag_count=frag)), _bits(want)) and torch.equal(frag, frag0)


def test_under_augmentation_through_the_encoder():
    """TargetEncoder(clip=True)(..., augment=AugmentParams): flip2 plus rotation, scale and translation at the ends of the 'basic' ranges,
    on the tiny geometry, against the restatement; and the same table without the rule gives other rows."""
    _need_gpu()
    name = "tiny"
    g = C.geometry(name)
    ends = [f for f, c in enumerate(CC.cases(name)) if c["name"].startswith("ends_")]
    assert [CC.cases(name)[f]["spec"] for f in ends] == list(CC.ENDS) and all(CC.table_rows(name)[f][1] != list(CC.IDENTITY) for f in ends)
    assert sum(CC.table_rows(name)[f][0] for f in ends) == 3
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    from phnet_amd.libs.dataset.openlane.targets import pack_annotations
    table = AugmentParams.build(list(CC.ENDS), g["img_h"], g["img_w"]).to("cuda")
    pts, cnt, num = (t.cuda() for t in pack_annotations([CC.cases(name)[f]["lanes"] for f in ends], CC.LIN, CC.PMAX, clip=True))
    frag = torch.zeros(len(ends), dtype=torch.int32, device="cuda")
    got = _encoder(name, clip=True)(pts, cnt, num, augment=table, frag_count=frag).cpu().numpy()
    want, want_n = _want(name)
    print("valid rows", int(want[ends][..., 1].sum()), "worst ulps", C.assert_rows_match(got, want[ends], ULPS, "ends of 'basic'"))
    assert frag.tolist() == want_n[ends].tolist() and want[ends][..., 1].sum() >= 6
    assert not np.array_equal(got, _encoder(name)(pts, cnt, num, augment=table).cpu().numpy())


def test_captured_graph_follows_the_table():
    """enc(..., augment=, out=, frag_count=) with clip=True captured in a graph equals the eager call, and a replay after copy_into of
    another table equals the eager result for that table."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    name = "tiny"
    g = C.geometry(name)
    enc = _encoder(name, clip=True)
    pts, cnt, num = _packed(name)
    n = pts.shape[0]
    first = CC.params(name)
    tables = [first, AugmentParams.build([CC.ENDS[k % 4] for k in range(n)], g["img_h"], g["img_w"]), AugmentParams.identity(n)]
    live = first.to("cuda")
    rows = torch.full((n, g["R"], 6 + g["S"]), float("nan"), device="cuda")
    frag = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    enc(pts, cnt, num, augment=live, out=rows, frag_count=frag)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enc(pts, cnt, num, augment=live, out=rows, frag_count=frag)
    seen = []
    for table in tables:
        table.copy_into(live)
        rows.fill_(float("nan")); frag.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        fresh_n = torch.zeros_like(frag)
        fresh = enc(pts, cnt, num, augment=table.to("cuda"), frag_count=fresh_n)
        assert torch.equal(_bits(rows), _bits(fresh)) and torch.equal(frag, fresh_n)
        seen.append((rows.clone(), frag.clone()))
    C.assert_rows_match(seen[0][0].cpu().numpy(), _want(name)[0], ULPS, "replay")
    assert seen[0][1].tolist() == _want(name)[1].tolist() and not torch.equal(_bits(seen[0][0]), _bits(seen[1][0]))
    assert torch.equal(_bits(seen[2][0]), _bits(enc(pts, cnt, num)))                                          # identity rows: the plain map, clipped


@pytest.mark.parametrize("name", ["affine_pos", "affine_neg"])
def test_image_and_clipped_labels_agree(name):
    """The blob tie of tests/test_augment_gpu.py with clip=True: a 3 x 3 white blob on an annotated point of a vertical lane, warped by
    both halves; the intensity centroid of the kernel's image lies within 0.5 px of fwd applied to the point and on the CLIPPED label row
    within 0.5 px."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.augment import ClipAugmenter
    from phnet_amd.libs.dataset.openlane.targets import pack_annotations
    g = C.geometry("tiny")
    T, H, W = AC.SHAPES["tiny"]
    params = AC.params("tiny", name)
    fwd = params.numpy()["fwd"][0].reshape(2, 3)
    dev = params.to("cuda")
    _, u8 = ClipAugmenter(H, W, mean=AC.MEAN, std=AC.STD, device="cuda")(torch.from_numpy(AC.blob_frames()).cuda(), dev, return_u8=True)
    pts, cnt, num = (t.cuda() for t in pack_annotations([[AC.BLOB_LANE]] * 3, C.LIN, 16, clip=True))
    frag = torch.zeros(3, dtype=torch.int32, device="cuda")
    rows = _encoder("tiny", clip=True)(pts, cnt, num, augment=dev, frag_count=frag).cpu().numpy()
    want = CC.encode_frame_clipped([AC.BLOB_LANE], H, W, g["S"], g["R"], 0, [float(v) for v in fwd.ravel()])
    C.assert_rows_match(rows[0], want[0], ULPS, name)
    cx, cy = AC.centroid(u8[0].cpu().numpy())
    wx, wy = fwd @ [AC.BLOB_XY[0], AC.BLOB_XY[1], 1.0]
    lx = AC.lane_x_at(rows[0, 0], cy, g["img_h"], g["S"])
    print(name, "centroid", (cx, cy), "fwd(point)", (wx, wy), "clipped lane at the centroid's y", lx, "fragments", frag.tolist())
    assert np.hypot(cx - wx, cy - wy) <= AC.BLOB_BOUND
    assert frag.tolist() == [want[2]] * 3 == [1] * 3 and rows[0, 0, 1] == 1 and rows[0, 0, 2] == 0 and abs(lx - cx) <= AC.BLOB_BOUND
