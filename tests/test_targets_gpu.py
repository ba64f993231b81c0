"""Training targets on the MI355X (csrc/lane_targets.hip, phnet_amd/libs/dataset/openlane/targets.py): the kernel against what the
reference's own transform_annotation gave (tests/golden/targets_tiny.json) and against the restatement of tests/target_cases.py.

Tolerance: flags, [2], [5] and the number and positions of -1e5 are exact; [3], [4] and the xs are within 2 float32 ulps.  Kernel
and restatement perform the same float64 operations in the same order, not contracted; the second ulp is margin for the device's
atan and divide sequences, nothing more.  Launch shapes against each other (one frame per launch, [B,T], out=, a replayed graph)
are compared bit for bit."""
import json

import numpy as np
import pytest
import torch

from oracle import phnet_cpu as O
from tests import synth
from tests import target_cases as C

pytestmark = pytest.mark.gpu

ULPS = 2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _encoder(name, **kw):
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder
    g = C.geometry(name)
    return TargetEncoder(g["img_h"], g["img_w"], g["S"], g["R"], src_h=g["img_h"], src_w=g["img_w"], crop_size=0, **kw)      # the identity map


def _packed(name):
    return tuple(torch.from_numpy(a).cuda() for a in C.pack([c["lanes"] for c in C.cases(name)]))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", [g[0] for g in C.GEOMETRIES])
def test_all_cases_in_one_launch_equal_reference_and_restatement(name):
    _need_gpu()
    g = C.geometry(name)
    got = _encoder(name)(*_packed(name)).cpu().numpy()
    assert got.shape == (len(C.cases(name)), g["R"], 6 + g["S"])
    golden = {r["name"]: r for r in json.load(open(C.GOLDEN))["geometries"][name]["cases"]}
    worst = [0, 0]
    for f, (c, (want, _)) in enumerate(zip(C.cases(name), C.expected(name))):
        worst[0] = max(worst[0], C.assert_rows_match(got[f], want, ULPS, (name, c["name"], "restatement")))
        if c["reference"]:
            worst[1] = max(worst[1], C.assert_rows_match(got[f], C.golden_label(golden[c["name"]], g["R"], g["S"]), ULPS, (name, c["name"], "golden")))
    assert sum(c["reference"] for c in C.cases(name)) == len(golden)
    print(name, "worst ulps against the restatement:", worst[0], "against the golden:", worst[1])


def test_single_frames_and_clips_equal_the_batched_launch():
    """The frames one launch each, and embedded as [B,T], equal the launch over all of them bit for bit."""
    _need_gpu()
    enc = _encoder("main")
    pts, cnt, num = _packed("main")
    whole = enc(pts, cnt, num)
    for f in range(pts.shape[0]):
        one = enc(pts[f:f + 1].contiguous(), cnt[f:f + 1].contiguous(), num[f:f + 1].contiguous())
        assert torch.equal(_bits(one[0]), _bits(whole[f])), C.cases("main")[f]["name"]
    B, T = 4, pts.shape[0] // 4
    clips = enc(pts[:B * T].view(B, T, *pts.shape[1:]), cnt[:B * T].view(B, T, -1), num[:B * T].view(B, T))
    assert tuple(clips.shape) == (B, T) + tuple(whole.shape[1:]) and torch.equal(_bits(clips).view(B * T, -1), _bits(whole[:B * T]).view(B * T, -1))


def test_out_is_fully_overwritten():
    _need_gpu()
    enc = _encoder("fine")
    pts, cnt, num = _packed("fine")
    want = enc(pts, cnt, num)
    out = torch.full_like(want, float("nan"))
    got = enc(pts, cnt, num, out=out)
    assert got.data_ptr() == out.data_ptr() and not bool(torch.isnan(out).any()) and torch.equal(_bits(out), _bits(want))
    with pytest.raises(ValueError):
        enc(pts, cnt, num, out=out[:-1])
    with pytest.raises(ValueError):
        enc(pts, cnt[:, :-1].contiguous(), num)


def test_garbage_in_the_padding_changes_nothing():
    """Points beyond a lane's count, and counts and points of lanes beyond lanes_num, are never used."""
    _need_gpu()
    enc = _encoder("main")
    pts, cnt, num = (a.copy() for a in C.pack([c["lanes"] for c in C.cases("main")]))
    want = enc(*(torch.from_numpy(a).cuda() for a in (pts, cnt, num)))
    rng = np.random.default_rng(9)
    junk = np.where(rng.random(pts.shape) < 0.3, np.nan, rng.standard_normal(pts.shape) * 1e4).astype(np.float32)
    junk[rng.random(pts.shape) < 0.1] = np.inf
    pad = np.arange(C.PMAX)[None, None, :] >= cnt[:, :, None]
    pad |= (np.arange(C.LIN)[None, :] >= num[:, None])[:, :, None]
    pts[pad] = junk[pad]
    beyond = np.arange(C.LIN)[None, :] >= num[:, None]
    cnt[beyond] = rng.integers(-5, 400, cnt.shape)[beyond]
    assert pad.mean() > 0.5 and beyond.sum() > 20
    got = enc(*(torch.from_numpy(a).cuda() for a in (pts, cnt, num)))
    assert torch.equal(_bits(got), _bits(want))
    full = (cnt == C.PMAX) & ~beyond                                               # a count above P is clamped to P
    cnt[full] = C.PMAX + 7
    assert full.any()
    got = enc(*(torch.from_numpy(a).cuda() for a in (pts, cnt, num)))
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("flip", [False, True])
def test_map_from_camera_coordinates(flip):
    """Annotations at 1280 x 1920, crop 480, with and without flip, against the restatement under the same rule; and
    for_preprocessor agrees with the explicit arguments."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
    frames = C.source_frames(31, 12)
    enc = TargetEncoder(320, 800, 36, 4, device="cuda")
    same = TargetEncoder.for_preprocessor(ClipPreprocessor(320, 800, device="cuda"), 36, 4)
    pts, cnt, num = (t.cuda() for t in pack_annotations(frames, 4, 32))
    got = enc(pts, cnt, num, flip=flip)
    assert torch.equal(_bits(same(pts, cnt, num, flip=flip)), _bits(got))
    mp = C.map_for(320, 800, 1280, 1920, 480, flip=flip)
    want = np.stack([C.encode_frame(lanes, 320, 800, 36, 4, mapping=mp)[0] for lanes in frames])
    worst = C.assert_rows_match(got.cpu().numpy(), want, ULPS, ("map", flip))
    print("flip", flip, "valid rows", int(want[..., 1].sum()), "worst ulps", worst)
    assert int(want[..., 1].sum()) >= 12
    if flip:
        plain = np.stack([C.encode_frame(lanes, 320, 800, 36, 4, mapping=C.map_for(320, 800, 1280, 1920, 480))[0] for lanes in frames])
        assert not np.array_equal(plain, want)


def test_captured_graph_equals_eager():
    """The call with out= captured in torch.cuda.graph and replayed on new inputs equals the eager call."""
    _need_gpu()
    enc = _encoder("main")
    pts, cnt, num = _packed("main")
    F = 8
    s_pts, s_cnt, s_num = pts[:F].clone(), cnt[:F].clone(), num[:F].clone()
    out = torch.full((F, 4, 6 + 36), float("nan"), device="cuda")
    enc(s_pts, s_cnt, s_num, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enc(s_pts, s_cnt, s_num, out=out)
    for lo in (F, 2 * F):
        s_pts.copy_(pts[lo:lo + F]); s_cnt.copy_(cnt[lo:lo + F]); s_num.copy_(num[lo:lo + F])
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        want = enc(pts[lo:lo + F].contiguous(), cnt[lo:lo + F].contiguous(), num[lo:lo + F].contiguous())
        assert torch.equal(_bits(out), _bits(want)), lo
    assert not torch.equal(_bits(out), _bits(enc(pts[:F].contiguous(), cnt[:F].contiguous(), num[:F].contiguous())))


def test_encoded_targets_train_the_tiny_model():
    """End to end: the two-lane frame of the tiny geometry, encoded on the device, goes through the tiny model's training
    forward and backward (Criterion4OL), and gives the loss the reference's own rows give.  The encoded rows are within 2 ulps
    (2.4e-7 relative) of the golden ones and the criterion is Lipschitz in its targets; 1e-5 relative leaves a factor 40."""
    _need_gpu()
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import RouterOL
    from phnet_amd.libs.utils.loss4OLV3 import Criterion4OL
    gt = C.geometry("tiny")
    g = O.Geometry(img_h=gt["img_h"], img_w=gt["img_w"], arch="resnet18")
    assert (g.num_points, g.n_strips) == (gt["S"], gt["S"] - 1)
    cfg = make_cfg(img_h=g.img_h, img_w=g.img_w, arch=g.arch)
    model = RouterOL(cfg, Criterion4OL(cfg))
    model.load_state_dict(synth.make_state(g), strict=True)
    for m in model.detNet.transformer_Dec.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    model = model.cuda().train()
    c, _, _ = C.case("tiny", "two_lanes")
    rec = next(r for r in json.load(open(C.GOLDEN))["geometries"]["tiny"]["cases"] if r["name"] == "two_lanes")
    gold = C.golden_label(rec, gt["R"], gt["S"])
    assert gold[:, 1].tolist() == [1, 1, 0, 0]
    pts, cnt, num = (torch.from_numpy(a).cuda() for a in C.pack([c["lanes"]] * 2))
    lanes = _encoder("tiny")(pts, cnt, num)
    C.assert_rows_match(lanes.cpu().numpy(), np.stack([gold, gold]), ULPS, "two_lanes")
    frames = synth.make_clip(g, 2).cuda()
    losses = []
    for tgt in (lanes, torch.from_numpy(np.stack([gold, gold])).cuda()):
        model.zero_grad(set_to_none=True)
        loss = model({"frame": frames, "lanes": tgt})
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
        losses.append(float(loss))
    print("loss from encoded targets", losses[0], "from the golden rows", losses[1])
    assert np.isfinite(losses[0]) and abs(losses[0] - losses[1]) <= 1e-5 * abs(losses[1])
