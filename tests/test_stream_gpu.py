"""Streaming inference on the MI355X (phnet_amd/stream.py, csrc/stream.hip): the device-resident token ring against a torch
statement, the reference's eval goldens fed one frame per step, stream == clip, independent streams, chunked resets, one
captured graph for every frame, and raw camera frames.

Tolerances are the project's own: ACT_TOL = 1e-3 (test_model_gpu.py: activations / lane points against the reference),
2e-4 * (1 + |ref|) for kept rows across batch shapes (test_inference_batched_over_clips_equals_clip_by_clip: fp32 re-association),
1e-5 for a hipGraph replay against the eager launches (same tests).  Keep decisions (counts, anchor ids) are compared exactly."""
import collections

import numpy as np
import pytest
import torch

from oracle import phnet_cpu as O
from tests import fixtures, synth

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-3
BATCH_TOL = 2e-4
GRAPH_TOL = 1e-5


def _build(g: O.Geometry, conf_threshold=None):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import RouterOL
    # the threshold goes in through make_cfg: Cfg hands out a fresh wrapper of its nested dicts on every attribute access, so an
    # assignment to model.detNet.cfg.test_parameters.conf_threshold would not reach the decode
    cfg = make_cfg(img_h=g.img_h, img_w=g.img_w, arch=g.arch, conf_threshold=g.conf_threshold if conf_threshold is None else conf_threshold)
    model = RouterOL(cfg, None)
    model.load_state_dict(synth.make_state(g), strict=True)
    assert model.detNet.cfg.test_parameters.conf_threshold == cfg.test_parameters.conf_threshold
    return model.cuda().eval()


def _close(a, b, tol, what=""):
    """|a - b| <= tol * (1 + |b|) element-wise."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if b.numel():
        err = (a - b).abs()
        print(f"{what}: max |a - b| / (1 + |b|) = {float((err / (1 + b.abs())).max()):.3e} (bound {tol:g})")
        assert bool((err <= tol * (1.0 + b.abs())).all()), (what, float(err.max()))


def _same_frame(got, want, tol, what):
    """(kept_rows [max_lanes,6+S], num, anchors [max_lanes]) of one frame of one stream: decisions exact, rows within tol."""
    k = int(want[1])
    assert int(got[1]) == k, (what, int(got[1]), k)
    assert torch.equal(got[2][:k], want[2][:k]), (what, got[2][:k].tolist(), want[2][:k].tolist())
    _close(got[0][:k], want[0][:k], tol, what)
    return k


def _tiny(conf_threshold=0.3):
    return O.Geometry(img_h=64, img_w=160, arch="resnet18", conf_threshold=conf_threshold)


def test_ring_kernels_equal_a_deque_of_memory_tokens():
    """window / push against a Python deque per (stream, stage) of hip_ops.memory_tokens outputs, concatenated oldest first and
    zero-padded to W slots: pure data movement plus the same mean in the same order, so torch.equal.  B = 3 streams reset at
    different frames, 2W + 3 frames (the ring wraps twice), anchor lists from empty (all -1) to full (L valid)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops as K
    from phnet_amd.stream import StreamState, window_order
    S, B, W, L, N, E = 3, 3, 8, 4, 240, 128
    st = StreamState(S, B, W, L, N, E, "cuda")
    st.ring.fill_(float("nan"))                                   # validity comes from n alone: stale slots must never show
    st.ring_valid.fill_(True)
    st.reset()
    resets = {0: (), 1: (5,), 2: (3, 12)}
    fifo = [[collections.deque(maxlen=W) for _ in range(S)] for _ in range(B)]
    pushed = [0] * B
    gen = torch.Generator().manual_seed(3)

    def check(t, when):
        st.load_window()
        torch.cuda.synchronize()
        for b in range(B):
            assert bool(st.has_memory[b]) == (pushed[b] > 0), (t, when, b)
            assert len(window_order(pushed[b], W)) == len(fifo[b][0])
            for s in range(S):
                toks = [x[0] for x in fifo[b][s]] + [torch.zeros(L + 1, E, device="cuda")] * (W - len(fifo[b][s]))
                vals = [x[1] for x in fifo[b][s]] + [torch.zeros(L + 1, dtype=torch.bool, device="cuda")] * (W - len(fifo[b][s]))
                assert torch.equal(st.window[s, b], torch.cat(toks)), (t, when, b, s)
                assert torch.equal(st.window_valid[s, b], torch.cat(vals)), (t, when, b, s)

    for t in range(2 * W + 3):
        mask = torch.tensor([t in resets[b] for b in range(B)])
        if bool(mask.any()):
            st.reset(mask.cuda())
            for b in range(B):
                if mask[b]:
                    pushed[b] = 0
                    for q in fifo[b]:
                        q.clear()
        check(t, "before push")                                   # the window a frame attends to (also publishes the cursor)
        feat = torch.randn((S, B, N, E), generator=gen).cuda()
        counts = [0, L, 2] if t == 0 else torch.randint(0, L + 1, (B,), generator=gen).tolist()
        anchors = torch.full((B, L), -1, dtype=torch.int64)
        for b in range(B):
            anchors[b, :counts[b]] = torch.randperm(N, generator=gen)[:counts[b]].sort().values
        anchors = anchors.cuda()
        st.feat.copy_(feat)
        st.push(anchors)
        for b in range(B):
            for s in range(S):
                tok, val = K.memory_tokens(feat[s, b].contiguous(), anchors[b].contiguous())
                fifo[b][s].append((tok.reshape(L + 1, E), val))
            pushed[b] += 1
        check(t, "after push")
    assert st.n.cpu().tolist() == pushed


@pytest.mark.parametrize("cfg", ["tiny_long", "config2"])
def test_reference_eval_goldens_one_frame_per_step(cfg):
    """The reference's eval goldens through a B = 1 captured stream, one frame per step: kept anchors per frame exactly the golden's,
    lane polylines within ACT_TOL - the assertions of test_sync_free_eval_and_graph_replay_match_reference_goldens.  tiny_long has
    11 frames (W = 8: the ring wraps) and a memory that changes (lanes kept on some frames, none on others)."""
    if cfg == "tiny_long":
        g, T, gold = O.Geometry(img_h=64, img_w=160, arch="resnet18"), 11, fixtures.load("tiny_long_eval_r18_64x160.npz")
    else:
        g, T, gold = O.Geometry(arch="resnet34"), 5, fixtures.load("config2_r34_320x800.npz")
    model = _build(g)
    frames = synth.make_clip(g, T, seed=77).cuda()
    s = model.open_stream(streams=1, frame_hw=(g.img_h, g.img_w), graph=True)
    for t in range(T):
        rows, num, anchors = s.step(frames[t:t + 1])
        want_anchor = np.where(gold["eval_keep_inds"][t])[0][[i for i in gold["eval_keep"][t].tolist() if i >= 0]]
        n = int(num[0])
        assert anchors[0, :n].cpu().tolist() == want_anchor.tolist(), t          # kept lanes (NMS order) as anchor ids: exact
        lanes = s.lanes(rows, num)[0]
        assert len(lanes) == int((gold["eval_lane_npts"][t] > 0).sum()), t
        for j, lane in enumerate(lanes):
            k = int(gold["eval_lane_npts"][t, j])
            assert lane.points.shape == (k, 2)
            np.testing.assert_allclose(lane.points, gold["eval_lane_pts"][t, j, :k], atol=ACT_TOL)


def test_stream_equals_clip():
    """11 frames fed one per step == RouterOL.infer_device on the 11-frame clip: counts and kept anchors equal, kept rows within
    2e-4 (batch-1 trunk and batched head against the clip-shaped pass).  Seed 40 at conf_threshold = 0.3: the CPU oracle
    (oracle/phnet_cpu.py clip_forward, eval) keeps 4 lanes on every one of the 11 frames of this clip (as it does for seeds 41, 42,
    43, 5 and 77), so for the reference alone frames 8-10 keep lanes and their windows hold positive tokens of frames that were
    pushed after the ring wrapped.  Both facts are asserted below for the run itself."""
    g, T = _tiny(), 11
    model = _build(g, conf_threshold=0.3)
    W, L = model.save_freq_max, model.detNet.cfg.max_lanes
    clip = synth.make_clip(g, T, seed=40).cuda()
    with torch.no_grad():
        rows_c, nums_c, anch_c = model.infer_device(clip)
    s = model.open_stream(streams=1, frame_hw=(g.img_h, g.img_w), graph=True)
    kept_late = positives_late = 0
    for t in range(T):
        rows, num, anchors = s.step(clip[t:t + 1])
        k = _same_frame((rows[0], num[0], anchors[0]), (rows_c[t], nums_c[t], anch_c[t]), BATCH_TOL, f"frame {t}")
        if t >= W:
            kept_late += k
            positives_late += int(s.state.window_valid[:, 0].reshape(-1, W, L + 1)[:, :, :L].sum())   # the window frame t attended to
    assert kept_late > 0 and positives_late > 0, (kept_late, positives_late)


def test_streams_are_independent():
    """One LaneStream(streams=3) == three LaneStream(streams=1) on the same frames and resets (stream 1 reset before frame 4,
    stream 2 before frames 3 and 9).  At frames 3, 4 and 9 one stream has an empty memory and the others do not: the select."""
    g, T, B = _tiny(), 11, 3
    model = _build(g, conf_threshold=0.3)
    clips = torch.stack([synth.make_clip(g, T, seed=40 + b) for b in range(B)]).cuda()
    resets = {0: (), 1: (4,), 2: (3, 9)}
    hw = (g.img_h, g.img_w)
    together = model.open_stream(streams=B, frame_hw=hw, graph=False)
    alone = [model.open_stream(streams=1, frame_hw=hw, graph=False) for _ in range(B)]
    mixed = kept = 0
    for t in range(T):
        mask = [t in resets[b] for b in range(B)]
        if any(mask):
            together.reset(mask)
            for b in range(B):
                if mask[b]:
                    alone[b].reset()
        rows, num, anchors = together.step(clips[:, t])
        has = together.state.has_memory.cpu().tolist()
        assert has == [t > 0 and t not in resets[b] for b in range(B)], (t, has)
        mixed += 0 < sum(has) < B
        for b in range(B):
            r1, n1, a1 = alone[b].step(clips[b:b + 1, t])
            kept += _same_frame((rows[b], num[b], anchors[b]), (r1[0], n1[0], a1[0]), BATCH_TOL, f"stream {b} frame {t}")
    assert mixed == 3 and kept > 0


def test_reset_every_reproduces_chunked_clips():
    """reset_every = 4 over 8 frames == infer_device on frames 0-3, then on frames 4-7 (testOL.py's chunking, at 4 instead of 16)."""
    g, T = _tiny(), 8
    model = _build(g, conf_threshold=0.3)
    clip = synth.make_clip(g, T, seed=41).cuda()
    with torch.no_grad():
        want = [model.infer_device(clip[0:4]), model.infer_device(clip[4:8])]
    s = model.open_stream(streams=1, frame_hw=(g.img_h, g.img_w), graph=True, reset_every=4)
    kept = 0
    for t in range(T):
        rows, num, anchors = s.step(clip[t:t + 1])
        assert bool(s.state.has_memory[0]) == (t % 4 != 0), t
        w = want[t // 4]
        kept += _same_frame((rows[0], num[0], anchors[0]), (w[0][t % 4], w[1][t % 4], w[2][t % 4]), BATCH_TOL, f"frame {t}")
    assert kept > 0


def test_one_graph_serves_every_frame():
    """graph=True against graph=False over 2W + 3 frames with a reset in the middle: decisions equal, rows within 1e-5; the graph
    captured at construction is the one replayed at the end (a reset never recaptures), and the replayed steps - frame copy,
    reset, replay - perform no synchronising device -> host copy (torch's sync debug mode in "error"; the test first checks that
    this torch build honours the mode, and says so if it does not)."""
    g, B = _tiny(), 2
    model = _build(g, conf_threshold=0.3)
    W = model.save_freq_max
    T = 2 * W + 3
    clips = torch.stack([synth.make_clip(g, T, seed=42 + b) for b in range(B)]).cuda()
    hw = (g.img_h, g.img_w)
    eager = model.open_stream(streams=B, frame_hw=hw, graph=False)
    graphed = model.open_stream(streams=B, frame_hw=hw, graph=True)
    graph0 = graphed.graph
    only1 = torch.tensor([False, True]).cuda()
    want = []
    for t in range(T):
        if t == W + 2:
            eager.reset(only1)
        want.append(tuple(x.clone() for x in eager.step(clips[:, t])))
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
            got.append(tuple(x.clone() for x in graphed.step(clips[:, t])))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    print("sync debug mode honoured by this torch build:", honoured)
    assert honoured, "torch.cuda.set_sync_debug_mode('error') did not flag .item(): check the kernel trace for D2H copies instead"
    assert graphed.graph is graph0 and graph0 is not None
    kept = 0
    for t in range(T):
        for b in range(B):
            kept += _same_frame(tuple(x[b] for x in got[t]), tuple(x[b] for x in want[t]), GRAPH_TOL, f"stream {b} frame {t}")
    assert kept > 0


def test_raw_camera_frames_enter_the_step():
    """raw= stream on uint8 camera frames == ClipPreprocessor on the same frames, then a plain stream step on its output:
    torch.equal on all three outputs (the same launches in the same order).  The captured form of the raw step replays the eager
    one within the graph-replay bound."""
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    g, B, T = _tiny(), 2, 4
    model = _build(g, conf_threshold=0.3)
    pre = ClipPreprocessor(g.img_h, g.img_w, src_h=200, src_w=300, crop_size=40)
    gen = torch.Generator().manual_seed(11)
    cam = torch.randint(0, 256, (T, B, 200, 300, 3), generator=gen, dtype=torch.uint8).cuda()
    hw = (g.img_h, g.img_w)
    raw = model.open_stream(streams=B, frame_hw=hw, graph=False, raw=pre)
    raw_graph = model.open_stream(streams=B, frame_hw=hw, graph=True, raw=pre)
    plain = model.open_stream(streams=B, frame_hw=hw, graph=False)
    kept = 0
    for t in range(T):
        got = raw.step(cam[t])
        want = plain.step(pre(cam[t]))
        for a, b, name in zip(got, want, ("kept_rows", "num", "anchors")):
            assert torch.equal(a, b), (t, name)
        rep = raw_graph.step(cam[t])
        for b in range(B):
            kept += _same_frame(tuple(x[b] for x in rep), tuple(x[b] for x in got), GRAPH_TOL, f"raw graph stream {b} frame {t}")
    assert kept > 0
    with pytest.raises(ValueError):
        raw.step(pre(cam[0]))                                      # a raw stream takes camera frames only
