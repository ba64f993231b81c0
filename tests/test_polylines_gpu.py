"""Device-side lane polylines on the MI355X (csrc/lane_points.hip, phnet_amd/polylines.py): the kernel against
DetNetV2.predictions_to_pred on the adversarial rows and on seeded random frames, then the model surfaces of both families -
streams with polylines=True, infer_points_device on one clip and on batched clips, GraphedInference - against the host path
(`lanes` / `lanes_from_device`) on the same step outputs.

The kernel copies values and never computes one, so every comparison with the host function is EXACT: counts, slots, and points
under torch.equal after widening.  The only tolerances are the project's existing ones between two differently shaped forward
passes, which produce different kept rows to begin with: 2e-4 (V1) across batch shapes, 1e-5 graph replay against eager
(tests/test_stream_gpu.py)."""
import numpy as np
import pytest
import torch

from oracle import phnet_cpu as O
from oracle import phnet_cpu_v2 as O2
from tests import fixtures, synth
from tests import polyline_cases as C

pytestmark = pytest.mark.gpu

BATCH_TOL = 2e-4
GRAPH_TOL = 1e-5
KEYS = ("points", "count", "lanes_num", "slot")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _build_v1(g, conf_threshold=None):
    _gpu()
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import RouterOL
    cfg = make_cfg(img_h=g.img_h, img_w=g.img_w, arch=g.arch, conf_threshold=g.conf_threshold if conf_threshold is None else conf_threshold)
    model = RouterOL(cfg, None)
    model.load_state_dict(synth.make_state(g), strict=True)
    return model.cuda().eval()


def _build_v2(g):
    _gpu()
    from phnet_amd.config import make_cfg_v2
    from phnet_amd.libs.models.Router4OLV2 import RouterOL
    model = RouterOL(make_cfg_v2(img_h=g.img_h, img_w=g.img_w, arch=g.arch, save_freq=1))
    model.load_state_dict(synth.make_state_v2(g), strict=True)
    return model.cuda().eval()


def _points_close(a, b, tol, what):
    """|a - b| <= tol * (1 + |b|) element-wise: the bound the kept rows these points are copied from are held to."""
    err = (a.double() - b.double()).abs()
    print(f"{what}: max |a - b| / (1 + |b|) = {float((err / (1 + b.double().abs())).max()):.3e} (bound {tol:g})")
    assert bool((err <= tol * (1.0 + b.double().abs())).all()), (what, float(err.max()))


def _tiny_v1():
    return O.Geometry(img_h=64, img_w=160, arch="resnet18", conf_threshold=0.3)


def _equals_host(pl, kept, num, what=""):
    """Device polylines pl (dict, leading dimensions flattened here) == predictions_to_pred on kept [F,L,6+S] / num [F]: exact.
    Returns the number of lanes."""
    kept, num = kept.detach().cpu().reshape(-1, *kept.shape[-2:]), num.detach().cpu().reshape(-1)
    exp = C.expected_layout(kept, num)
    F, L = kept.shape[:2]
    got = {k: pl[k].detach().cpu().reshape(exp[k].shape) for k in KEYS}
    assert torch.equal(got["lanes_num"], torch.from_numpy(exp["lanes_num"])), (what, got["lanes_num"].tolist(), exp["lanes_num"].tolist())
    assert torch.equal(got["count"], torch.from_numpy(exp["count"])), what
    assert torch.equal(got["slot"], torch.from_numpy(exp["slot"])), what
    nan_free = torch.from_numpy(exp["points"])
    assert not bool(torch.isnan(nan_free).any())                               # a NaN x never survives
    assert torch.equal(got["points"].double(), nan_free.double()), what        # widened: the host's float64, bit for bit
    for f in range(F):                                                         # said again, explicitly: tails are zeros, metadata follows slot
        for k in range(L):
            assert not bool(got["points"][f, k, int(got["count"][f, k]):].any()), (what, f, k)
        for k, lane in enumerate(exp["lanes"][f]):
            src = int(got["slot"][f, k])
            assert 0 <= src < int(num[f])
            assert all(float(lane.metadata[key]) == float(kept[f, src, col]) for key, col in (("conf", 1), ("start_y", 2), ("start_x", 3)))
        assert bool((got["slot"][f, int(got["lanes_num"][f]):] == -1).all())
    return int(exp["lanes_num"].sum())


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("S", [C.S_MAIN, C.S_ODD])
def test_kernel_equals_the_host_function_on_the_adversarial_rows(S):
    """Every branch test_polylines_cpu.py shows the rows to hit; poisoned output buffers (NaN / -7) so that an element the kernel
    does not write shows; [F,L,6+S] and the unbatched [L,6+S] form."""
    _gpu()
    from phnet_amd import hip_ops as K
    kept, num = C.pack_frames(C.adversarial_frames(S), S, L=4)
    ys = C.head(S).prior_ys.cuda()
    F, L = kept.shape[:2]
    out = dict(points=torch.full((F, L, S, 2), float("nan"), device="cuda"), count=torch.full((F, L), -7, dtype=torch.int32, device="cuda"),
               lanes_num=torch.full((F,), -7, dtype=torch.int32, device="cuda"), slot=torch.full((F, L), -7, dtype=torch.int32, device="cuda"))
    got = K.lane_points(kept.cuda(), num.cuda(), ys, out=out)
    assert all(got[k].data_ptr() == out[k].data_ptr() for k in KEYS)
    lanes = _equals_host(got, kept, num, f"adversarial S={S}")
    assert lanes >= 16
    for f in (2, 4):
        one = K.lane_points(kept[f].cuda(), num[f].cuda(), ys)
        assert all(torch.equal(one[k], got[k][f]) for k in KEYS), f
    # the rows the host function refuses (it raises on NaN / inf in start_y or length) are no lanes, and do not disturb the others
    bad = kept[0, 0:1].repeat(4, 1).unsqueeze(0).clone()                       # four copies of a row that is a lane
    bad[0, 0, 2], bad[0, 2, 5] = float("nan"), float("inf")
    got = K.lane_points(bad.cuda(), torch.tensor([4]).cuda(), ys)
    good = K.lane_points(kept[0, 0:1].repeat(4, 1).cuda(), torch.tensor(2).cuda(), ys)
    assert got["lanes_num"].tolist() == [2] and got["slot"][0].tolist() == [1, 3, -1, -1]
    assert torch.equal(got["points"][0], good["points"]) and torch.equal(got["count"][0], good["count"])


@pytest.mark.parametrize("L,S,seed", [(4, C.S_MAIN, 11), (8, C.S_MAIN, 12), (4, C.S_ODD, 13), (8, C.S_ODD, 14)])
def test_kernel_equals_the_host_function_on_random_frames(L, S, seed):
    """4 x 600 = 2 400 seeded frames in all, num from 0 to L, in ONE launch per case; slots >= num hold garbage and are ignored.
    A second launch into the same buffers gives the same bits (every element is written, nothing accumulates)."""
    _gpu()
    from phnet_amd import hip_ops as K
    kept, num = C.random_frames(600, L, S, seed)
    ys = C.head(S).prior_ys.cuda()
    got = K.lane_points(kept.cuda(), num.cuda(), ys)
    first = {k: v.clone() for k, v in got.items()}
    lanes = _equals_host(got, kept, num, f"random L={L} S={S}")
    K.lane_points(kept.cuda(), num.cuda(), ys, out=got)
    assert all(torch.equal(first[k], got[k]) for k in KEYS)
    print(f"L = {L}, S = {S}: {lanes} lanes of {int(num.sum())} kept slots in 600 frames")
    assert 0 < lanes < int(num.sum())


def test_kernel_limits():
    """The largest sizes the header states: L = 64 (16 waves take 4 slots each), S = 256 (4 rounds of 64 offsets)."""
    _gpu()
    from phnet_amd import hip_ops as K
    for L, S in ((64, 256), (17, 129), (1, 2)):
        kept, num = C.random_frames(24, L, S, seed=L + S)
        num = num.clamp(max=L)
        got = K.lane_points(kept.cuda(), num.cuda(), C.head(S).prior_ys.cuda())
        _equals_host(got, kept, num, f"limits L={L} S={S}")


# ----------------------------------------------------------------------------------------------------------------- the models
def _fast_equals_slow(fast, slow, what):
    """Polyline lists of lanes_fast / polylines_from_device against the Lane lists of lanes / lanes_from_device: lane for lane."""
    assert len(fast) == len(slow), (what, len(fast), len(slow))
    for a, b in zip(fast, slow):
        assert a.points.dtype == np.float64 and np.array_equal(a.points, b.points), what
        assert all(float(a.metadata[k]) == float(b.metadata[k]) for k in ("conf", "start_x", "start_y")), what
    return len(fast)


@pytest.mark.parametrize("cfg", ["tiny_long", "config2"])
def test_v1_goldens_stream_and_clip(cfg):
    """The reference's eval goldens of tests/test_stream_gpu.py, one frame per step through a captured stream with polylines=True,
    and the same clip through infer_points_device: lanes_fast() == lanes() lane for lane, as many lanes per frame as the golden
    holds; kept_rows / num / anchors bit-identical to a stream opened WITHOUT polylines on the same frames."""
    if cfg == "tiny_long":
        g, T, gold = O.Geometry(img_h=64, img_w=160, arch="resnet18"), 11, fixtures.load("tiny_long_eval_r18_64x160.npz")
    else:
        g, T, gold = O.Geometry(arch="resnet34"), 5, fixtures.load("config2_r34_320x800.npz")
    model = _build_v1(g)
    frames = synth.make_clip(g, T, seed=77).cuda()
    hw = (g.img_h, g.img_w)
    s = model.open_stream(streams=1, frame_hw=hw, graph=True, polylines=True)
    plain = model.open_stream(streams=1, frame_hw=hw, graph=True)
    assert plain.polylines is None
    with pytest.raises(RuntimeError):
        plain.lanes_fast()
    total = 0
    for t in range(T):
        rows, num, anchors = s.step(frames[t:t + 1])
        for a, b, name in zip((rows, num, anchors), plain.step(frames[t:t + 1]), ("kept_rows", "num", "anchors")):
            assert torch.equal(a, b), (t, name)
        want = int((gold["eval_lane_npts"][t] > 0).sum())
        fast, slow = s.lanes_fast()[0], s.lanes(rows, num)[0]
        assert len(slow) == want and int(s.polylines["lanes_num"][0]) == want, (t, len(slow), want)
        total += _fast_equals_slow(fast, slow, f"{cfg} frame {t}")
        _equals_host(s.polylines, rows, num, f"{cfg} frame {t}")
    assert total > 0
    with torch.no_grad():
        rows, nums, anchors, pl = model.infer_points_device(frames)
        rows0, nums0, anchors0 = model.infer_device(frames)
    assert torch.equal(rows, rows0) and torch.equal(nums, nums0) and torch.equal(anchors, anchors0)
    assert tuple(pl["points"].shape) == (T, model.detNet.cfg.max_lanes, model.detNet.n_offsets, 2)
    fast, slow = model.polylines_from_device(pl, rows), model.lanes_from_device(rows, nums)["lane_lines"]
    for t in range(T):
        assert len(slow[t]) == int((gold["eval_lane_npts"][t] > 0).sum()), t
        _fast_equals_slow(fast[t], slow[t], f"{cfg} clip frame {t}")
    _equals_host(pl, rows, nums, f"{cfg} clip")


@pytest.mark.parametrize("size", ["tiny", "320x800"])
def test_v2_goldens_stream_and_clip(size):
    """The Router4OLV2 fixtures of tests/test_v2_gpu.py / test_stream_v2_gpu.py the same way.  The tiny fixture keeps
    4 4 4 4 4 3 3 4 lanes over 8 frames (W = 5): lanes after the ring has wrapped."""
    if size == "tiny":
        g, T, gold = O2.GeometryV2(img_h=64, img_w=160), 8, fixtures.load("v2_tiny_r18_64x160.npz")
    else:
        g, T, gold = O2.GeometryV2(), 6, fixtures.load("v2_r18_320x800.npz")
    model = _build_v2(g)
    W = model.save_freq_max
    frames = synth.make_clip(g, T, seed=77).cuda()
    hw = (g.img_h, g.img_w)
    s = model.open_stream(streams=1, frame_hw=hw, graph=True, polylines=True)
    plain = model.open_stream(streams=1, frame_hw=hw, graph=True)
    late = 0
    for t in range(T):
        rows, num, anchors = s.step(frames[t:t + 1])
        for a, b, name in zip((rows, num, anchors), plain.step(frames[t:t + 1]), ("kept_rows", "num", "anchors")):
            assert torch.equal(a, b), (t, name)
        want = int((gold["lane_npts"][t] > 0).sum())
        fast, slow = s.lanes_fast()[0], s.lanes(rows, num)[0]
        assert len(slow) == want and 3 <= want <= 4, (t, len(slow), want)
        n = _fast_equals_slow(fast, slow, f"v2 {size} frame {t}")
        _equals_host(s.polylines, rows, num, f"v2 {size} frame {t}")
        late += n if t >= W else 0
    assert late > 0
    rows, nums, anchors, pl = model.infer_points_device(frames)
    with torch.no_grad():
        rows0, nums0, anchors0 = model.infer_device(frames)[:3]
    assert torch.equal(rows, rows0) and torch.equal(nums, nums0) and torch.equal(anchors, anchors0)
    fast, slow = model.polylines_from_device(pl, rows), model.lanes_from_device(rows, nums)["lane_lines"]
    for t in range(T):
        assert len(slow[t]) == int((gold["lane_npts"][t] > 0).sum()), t
        _fast_equals_slow(fast[t], slow[t], f"v2 {size} clip frame {t}")
    _equals_host(pl, rows, nums, f"v2 {size} clip")


def test_graph_replay_equals_eager_and_step_does_not_synchronise():
    """V1, B = 2, 2W + 3 frames with a reset in the middle (the frames of test_one_graph_serves_every_frame), polylines=True on
    both: the replayed step - frame copy, reset, replay, now with the lane-points launch inside the graph - performs no
    synchronising device -> host copy (torch's sync debug mode in "error", checked to be honoured).  Keep decisions and the
    polylines' counts equal the eager stream's, points within the graph-replay bound of the rows they are copied from (1e-5);
    and the replayed polylines are EXACTLY the host function of the replayed rows."""
    g, B = _tiny_v1(), 2
    model = _build_v1(g, conf_threshold=0.3)
    W = model.save_freq_max
    T = 2 * W + 3
    clips = torch.stack([synth.make_clip(g, T, seed=42 + b) for b in range(B)]).cuda()
    hw = (g.img_h, g.img_w)
    eager = model.open_stream(streams=B, frame_hw=hw, graph=False, polylines=True)
    graphed = model.open_stream(streams=B, frame_hw=hw, graph=True, polylines=True)
    graph0 = graphed.graph
    only1 = torch.tensor([False, True]).cuda()
    want = []
    for t in range(T):
        if t == W + 2:
            eager.reset(only1)
        out = eager.step(clips[:, t])
        want.append(([x.clone() for x in out], {k: v.clone() for k, v in eager.polylines.items()}))
    probe = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    got = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        for t in range(T):
            if t == W + 2:
                graphed.reset(only1)
            out = graphed.step(clips[:, t])
            got.append(([x.clone() for x in out], {k: v.clone() for k, v in graphed.polylines.items()}))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert honoured, "torch.cuda.set_sync_debug_mode('error') did not flag .item()"
    assert graphed.graph is graph0 and graph0 is not None
    lanes = late = 0
    for t in range(T):
        (rows, num, anchors), pl = got[t]
        (rows_e, num_e, anchors_e), pl_e = want[t]
        assert torch.equal(num, num_e) and torch.equal(anchors, anchors_e), t
        for k in ("count", "lanes_num", "slot"):
            assert torch.equal(pl[k], pl_e[k]), (t, k)
        _points_close(pl["points"], pl_e["points"], GRAPH_TOL, f"graph vs eager frame {t}")
        n = _equals_host(pl, rows, num, f"graph frame {t}")
        _equals_host(pl_e, rows_e, num_e, f"eager frame {t}")
        lanes += n
        late += n if t >= W else 0
    assert lanes > 0 and late > 0
    fast, slow = graphed.lanes_fast(), graphed.lanes(*graphed.out[:2])
    assert sum(_fast_equals_slow(a, b, "last step") for a, b in zip(fast, slow)) > 0


def test_three_streams_with_staggered_resets_equal_their_single_streams():
    """One stream object with B = 3 and polylines=True against three B = 1 streams, resets at different frames
    (test_streams_are_independent).  Stream b's polylines are EXACTLY the kernel's output on its own rows alone (streams do not
    mix in the packing) and the host function of them; against its single stream the lane counts, point counts and slots are
    equal and the points within the 2e-4 the kept rows of the two batch shapes are allowed to differ by."""
    from phnet_amd import hip_ops as K
    g, T, B = _tiny_v1(), 11, 3
    model = _build_v1(g, conf_threshold=0.3)
    clips = torch.stack([synth.make_clip(g, T, seed=40 + b) for b in range(B)]).cuda()
    resets = {0: (), 1: (4,), 2: (3, 9)}
    hw = (g.img_h, g.img_w)
    together = model.open_stream(streams=B, frame_hw=hw, graph=True, polylines=True)
    alone = [model.open_stream(streams=1, frame_hw=hw, graph=True, polylines=True) for _ in range(B)]
    lanes = 0
    for t in range(T):
        mask = [t in resets[b] for b in range(B)]
        if any(mask):
            together.reset(mask)
            for b in range(B):
                if mask[b]:
                    alone[b].reset()
        rows, num, anchors = together.step(clips[:, t])
        lanes += _equals_host(together.polylines, rows, num, f"B=3 frame {t}")
        for b in range(B):
            own = K.lane_points(rows[b].contiguous(), num[b].contiguous(), model.detNet.prior_ys)
            assert all(torch.equal(own[k], together.polylines[k][b]) for k in KEYS), (t, b)
            r1, n1, a1 = alone[b].step(clips[b:b + 1, t])
            assert torch.equal(n1[0], num[b]) and torch.equal(a1[0], anchors[b]), (t, b)
            for k in ("count", "lanes_num", "slot"):
                assert torch.equal(alone[b].polylines[k][0], together.polylines[k][b]), (t, b, k)
            _points_close(alone[b].polylines["points"][0], together.polylines["points"][b], BATCH_TOL, f"stream {b} frame {t}")
    assert lanes > 0


def test_batched_clips_equal_clip_by_clip():
    """infer_points_device on [B,T,...] against the same call clip by clip, both families' shared code on V1: decisions and the
    polylines' counts / slots equal, points within the batch-shape bound of the rows; the batched polylines are exactly the host
    function of the batched rows, and polylines_from_device nests [B][T]."""
    g, B, T = _tiny_v1(), 3, 6
    model = _build_v1(g, conf_threshold=0.3)
    clips = torch.stack([synth.make_clip(g, T, seed=50 + b) for b in range(B)]).cuda()
    with torch.no_grad():
        rows, nums, anchors, pl = model.infer_points_device(clips)
        rows0, nums0, anchors0 = model.infer_clips_device(clips)
    assert torch.equal(rows, rows0) and torch.equal(nums, nums0) and torch.equal(anchors, anchors0)
    L, S = model.detNet.cfg.max_lanes, model.detNet.n_offsets
    assert tuple(pl["points"].shape) == (B, T, L, S, 2) and tuple(pl["lanes_num"].shape) == (B, T)
    assert _equals_host(pl, rows, nums, "batched clips") > 0
    nested = model.polylines_from_device(pl, rows)
    assert len(nested) == B and all(len(c) == T for c in nested)
    for b in range(B):
        with torch.no_grad():
            r1, n1, a1, p1 = model.infer_points_device(clips[b])
        assert torch.equal(n1, nums[b]) and torch.equal(a1, anchors[b]), b
        for k in ("count", "lanes_num", "slot"):
            assert torch.equal(p1[k], pl[k][b]), (b, k)
        _points_close(p1["points"], pl["points"][b], BATCH_TOL, f"clip {b}")
        slow = model.lanes_from_device(rows[b], nums[b])["lane_lines"]
        for t in range(T):
            _fast_equals_slow(nested[b][t], slow[t], f"clip {b} frame {t}")


def test_graphed_inference_captures_the_polylines():
    """GraphedInference(polylines=True): the same triple as without, polylines the host function of the replayed rows."""
    from phnet_amd.graphed import GraphedInference
    g, T = _tiny_v1(), 5
    model = _build_v1(g, conf_threshold=0.3)
    clip = synth.make_clip(g, T, seed=40).cuda()
    with_pl = GraphedInference(model, clip, polylines=True)
    without = GraphedInference(model, clip)
    assert without.polylines is None
    other = synth.make_clip(g, T, seed=41).cuda()
    for frames in (clip, other):
        out = with_pl(frames)
        assert len(out) == 3 and all(torch.equal(a, b) for a, b in zip(out, without(frames)))
        assert _equals_host(with_pl.polylines, out[0], out[1], "graphed clip") > 0
