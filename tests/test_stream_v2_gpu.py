"""Streaming inference of the Router4OLV2 family on the MI355X (phnet_amd/stream.py LaneStreamV2, csrc/stream_v2.hip): the key
kernel against a torch statement, the reference's V2 fixtures fed one frame per step, stream == clip, independent streams with
save_freq = 2, clips batched through the head, chunked resets, one captured graph for every frame, raw camera frames.

Tolerances are the project's own: ACT_TOL = 1e-3 (test_model_gpu.py: lane points against the reference), 2e-3 * (1 + |ref|) for
kept rows across batch shapes (test_v2_gpu.py "stage-0 batching": other GEMM row counts -> other tile plans, fp32 re-association
through V2's cascade), 1e-5 for a hipGraph replay against the eager launches.  Keep decisions (counts, anchor ids) are compared
exactly: tests/test_stream_v2_cpu.py shows from the CPU oracle that on these clips every anchor above the confidence threshold is
>= 2.8e-4 away from the hard-routing boundary, that 3-4 lanes are kept on every frame and that both branches are taken.  Each
test asserts for its own run that lanes were kept on frames >= W (after the ring wrapped); tests of the batched / streamed head
also assert that both routing outcomes occurred among the anchors of a clip."""
import numpy as np
import pytest
import torch

from oracle import phnet_cpu_v2 as O2
from tests import fixtures, synth

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-3
BATCH_TOL = 2e-3
GRAPH_TOL = 1e-5


def _tiny():
    return O2.GeometryV2(img_h=64, img_w=160)


def _build(g: O2.GeometryV2, save_freq: int = 1):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd.config import make_cfg_v2
    from phnet_amd.libs.models.Router4OLV2 import RouterOL
    model = RouterOL(make_cfg_v2(img_h=g.img_h, img_w=g.img_w, arch=g.arch, save_freq=save_freq))
    model.load_state_dict(synth.make_state_v2(g), strict=True)
    assert model.save_freq == save_freq and model.router.cfg.save_freq == save_freq
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


class _Routes:
    """Hard-routing outcomes of the run under test, per clip / stream: add(gate_rows [S, B*N]) after every step takes the gates the
    step itself routed with (LaneStreamV2.gate_rows, or what infer_clips_device handed to hip_ops.route_lines)."""

    def __init__(self, B):
        self.B, self.to_b, self.to_a = B, [0] * B, [0] * B

    def add(self, gate_rows):
        d = gate_rows.detach().mean(dim=0).view(self.B, -1)
        for b in range(self.B):
            self.to_b[b] += int((d[b] >= 0.5).sum())
            self.to_a[b] += int((d[b] < 0.5).sum())

    def both(self):
        print("anchors routed to branch B / A per clip:", list(zip(self.to_b, self.to_a)))
        return all(x > 0 for x in self.to_b) and all(x > 0 for x in self.to_a)


def test_key_kernel_equals_a_torch_statement():
    """B = 3 streams with cursor = 0, 1, 7 and min_frames = 2: streams 0 and 1 get their own tokens (stream 1 HAS a ring entry and
    must not use it), stream 2 its window.  One add per element and data movement: torch.equal.  Also written straight into
    StreamState's buffers (tgt = feat[stage], the shared key set), and min_frames = 0 with an empty memory = own tokens."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops as K
    from phnet_amd.stream import StreamState
    B, N, W, L, E = 3, 240, 5, 4, 256
    M = W * (L + 1)
    gen = torch.Generator().manual_seed(9)
    local = torch.randn((B, N, E), generator=gen).cuda()
    pos = torch.randn((N, E), generator=gen).cuda()
    window = torch.randn((B, M, E), generator=gen).cuda()
    wvalid = (torch.rand((B, M), generator=gen) < 0.5).cuda()
    cursor = torch.tensor([0, 1, 7], dtype=torch.int32).cuda()

    def statement(min_frames, kmax):
        tgt = local + pos
        use = ((cursor >= min_frames) & (cursor > 0)).view(B, 1, 1)
        own = torch.zeros((B, kmax, E), device="cuda"); own[:, :N] = tgt
        mem = torch.zeros((B, kmax, E), device="cuda"); mem[:, :M] = window
        own_v = torch.zeros((B, kmax), dtype=torch.bool, device="cuda"); own_v[:, :N] = True
        mem_v = torch.zeros((B, kmax), dtype=torch.bool, device="cuda"); mem_v[:, :M] = wvalid
        return tgt, torch.where(use, mem, own), torch.where(use.view(B, 1), mem_v, own_v)

    for min_frames in (2, 0, 1, 8):
        tgt, keys, valid = K.stream_keys(local, pos, window, wvalid, cursor, min_frames)
        want = statement(min_frames, max(N, M))
        assert keys.shape == (B, max(N, M), E) and valid.dtype == torch.bool
        assert torch.equal(tgt, want[0]) and torch.equal(keys, want[1]) and torch.equal(valid, want[2]), min_frames
    # min_frames = 2: the three cases of the issue
    _, keys, valid = K.stream_keys(local, pos, window, wvalid, cursor, 2)
    assert torch.equal(keys[1, :N], local[1] + pos) and bool(valid[1].all())           # n = 1: own tokens, the ring entry unused
    assert torch.equal(keys[2, :M], window[2]) and torch.equal(valid[2, :M], wvalid[2]) and not bool(valid[2, M:].any())
    assert not bool(keys[2, M:].any())
    # caller-provided buffers of a stream state, stale contents overwritten
    st = StreamState(3, B, W, L, N, E, "cuda", key_sets=True)
    st.keys.fill_(float("nan")); st.keys_valid.fill_(True); st.feat.fill_(float("nan"))
    st.window[1].copy_(window); st.window_valid[1].copy_(wvalid); st.cursor.copy_(cursor)
    tgt, keys, valid = K.stream_keys(local, pos, st.window[1], st.window_valid[1], st.cursor, 2, tgt=st.feat[1], out=(st.keys, st.keys_valid))
    want = statement(2, max(N, M))
    assert tgt.data_ptr() == st.feat[1].data_ptr() and keys.data_ptr() == st.keys.data_ptr()
    assert torch.equal(st.feat[1], want[0]) and torch.equal(st.keys, want[1]) and torch.equal(st.keys_valid, want[2])
    # a window larger than the token set (Kmax = M > N)
    n2 = 16
    tgt, keys, valid = K.stream_keys(local[:, :n2].contiguous(), pos[:n2].contiguous(), window, wvalid, cursor, 2)
    assert keys.shape == (B, M, E)
    assert torch.equal(keys[0, :n2], tgt[0]) and not bool(keys[0, n2:].any()) and valid[0].tolist() == [True] * n2 + [False] * (M - n2)
    assert torch.equal(keys[2], window[2]) and torch.equal(valid[2], wvalid[2])
    with pytest.raises(ValueError):
        K.stream_keys(local, pos, window, wvalid, cursor, -1)


@pytest.mark.parametrize("size", ["tiny", "320x800"])
def test_reference_fixtures_one_frame_per_step(size):
    """The reference's V2 fixtures through a B = 1 captured stream, one frame per step: keep mask and kept indices per frame
    exactly the golden's, lane polylines within 1e-3 - the assertions test_v2_gpu.py::_end_to_end makes for the clip path.  The
    tiny fixture has 8 frames (W = 5: the ring wraps) and keeps 4 4 4 4 4 3 3 4 lanes."""
    if size == "tiny":
        g, T, gold = _tiny(), 8, fixtures.load("v2_tiny_r18_64x160.npz")
    else:
        g, T, gold = O2.GeometryV2(), 6, fixtures.load("v2_r18_320x800.npz")
    model = _build(g)
    W = model.save_freq_max
    frames = synth.make_clip(g, T, seed=77).cuda()
    s = model.open_stream(streams=1, frame_hw=(g.img_h, g.img_w), graph=True)
    kept_late = 0
    for t in range(T):
        rows, num, anchors = s.step(frames[t:t + 1])
        want_keep = [i for i in gold["keep"][t].tolist() if i >= 0]                # indices into the candidates, NMS order
        want_anchor = np.where(gold["keep_inds"][t])[0][want_keep]
        n = int(num[0])
        assert n == len(want_keep), (t, n, want_keep)
        assert anchors[0, :n].cpu().tolist() == want_anchor.tolist(), t            # keep mask + kept indices as anchor ids: exact
        lanes = s.lanes(rows, num)[0]
        assert len(lanes) == int((gold["lane_npts"][t] > 0).sum()), t
        for j, lane in enumerate(lanes):
            k = int(gold["lane_npts"][t, j])
            assert lane.points.shape == (k, 2)
            print(f"frame {t} lane {j}: max |points - golden| = {float(np.abs(lane.points - gold['lane_pts'][t, j, :k]).max()):.3e} (bound {ACT_TOL:g})")
            np.testing.assert_allclose(lane.points, gold["lane_pts"][t, j, :k], atol=ACT_TOL)
        if t >= W:
            kept_late += n
    assert kept_late > 0


@pytest.mark.parametrize("faithful", [True, False])
def test_stream_equals_clip(faithful):
    """12 frames (seed 40) fed one per step == RouterOL.infer_device on the 12-frame clip: counts and kept anchors equal, kept rows
    within 2e-3.  faithful_memory True (memory = one mean token per frame) and False (kept lanes' tokens + mean of the rest: the
    windows then hold positive tokens, asserted)."""
    g, T = _tiny(), 12
    model = _build(g)
    model.faithful_memory = faithful
    W, L = model.save_freq_max, model.router.cfg.max_lanes
    clip = synth.make_clip(g, T, seed=40).cuda()
    with torch.no_grad():
        rows_c, nums_c, anch_c, aux = model.infer_device(clip)
    s = model.open_stream(streams=1, frame_hw=(g.img_h, g.img_w), graph=True)
    routes = _Routes(1)
    kept_late = positives_late = 0
    for t in range(T):
        rows, num, anchors = s.step(clip[t:t + 1])
        routes.add(s.gate_rows)
        k = _same_frame((rows[0], num[0], anchors[0]), (rows_c[t], nums_c[t], anch_c[t]), BATCH_TOL, f"frame {t}")
        assert int(s.state.cursor[0]) == t
        if t >= W:
            kept_late += k
            positives_late += int(s.state.window_valid[:, 0].reshape(-1, W, L + 1)[:, :, :L].sum())   # the window frame t attended to
            assert int(s.state.window_valid[:, 0].sum()) >= 3 * W                                      # every slot holds its mean token
    assert kept_late > 0 and (positives_late > 0) == (not faithful), (kept_late, positives_late)
    assert routes.both()


def test_streams_are_independent_with_save_freq_two():
    """save_freq = 2.  One stream object with B = 3 (seeds 40, 41, 42) == three B = 1 streams on the same frames and resets (stream
    1 reset before frame 4, stream 2 before frames 3 and 9); both also == infer_device on the clip segments between the resets.
    Frame counts since the reset, per stream: frame 3 (3, 3, 0), frame 4 (4, 0, 1), frame 5 (5, 1, 2), frame 9 (9, 5, 0), frame 10
    (10, 6, 1).  So a stream without any ring entry (n = 0) runs beside streams deep in their memory at frames 3, 4, 9; a stream
    with a ring entry that must NOT be used yet (n = 1 < save_freq: what `n > 0` gets wrong) beside them at frames 4, 5, 10; all
    three cases at once at frame 4 - asserted for the run."""
    g, T, B = _tiny(), 12, 3
    model = _build(g, save_freq=2)
    W = model.save_freq_max
    clips = torch.stack([synth.make_clip(g, T, seed=40 + b) for b in range(B)]).cuda()
    resets = {0: (), 1: (4,), 2: (3, 9)}
    hw = (g.img_h, g.img_w)
    # the clip path on each stream's segments: the reference of what a reset means
    want_clip = []
    for b in range(B):
        cuts = [0, *resets[b], T]
        per_frame = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            with torch.no_grad():
                r, n, a, aux = model.infer_device(clips[b, lo:hi])
            per_frame += [(r[i], n[i], a[i]) for i in range(hi - lo)]
        want_clip.append(per_frame)
    together = model.open_stream(streams=B, frame_hw=hw, graph=False)
    alone = [model.open_stream(streams=1, frame_hw=hw, graph=False) for _ in range(B)]
    count = [0] * B
    routes = _Routes(B)
    mixed0 = mixed1 = mixed_all = kept = kept_late = 0
    for t in range(T):
        mask = [t in resets[b] for b in range(B)]
        if any(mask):
            together.reset(mask)
            for b in range(B):
                if mask[b]:
                    alone[b].reset()
                    count[b] = 0
        rows, num, anchors = together.step(clips[:, t])
        routes.add(together.gate_rows)
        assert together.state.cursor.cpu().tolist() == count, (t, count)
        mixed0 += (0 in count) and max(count) >= 2
        mixed1 += (1 in count) and max(count) >= 2
        mixed_all += (0 in count) and (1 in count) and max(count) >= 2
        for b in range(B):
            r1, n1, a1 = alone[b].step(clips[b:b + 1, t])
            k = _same_frame((rows[b], num[b], anchors[b]), (r1[0], n1[0], a1[0]), BATCH_TOL, f"B=3 vs B=1: stream {b} frame {t}")
            _same_frame((rows[b], num[b], anchors[b]), want_clip[b][t], BATCH_TOL, f"B=3 vs clip: stream {b} frame {t}")
            kept += k
            kept_late += k if count[b] >= W else 0
            count[b] += 1
    assert (mixed0, mixed1, mixed_all) == (3, 3, 1) and kept > 0 and kept_late > 0, (mixed0, mixed1, mixed_all, kept, kept_late)
    assert routes.both()


def test_clips_batched_through_the_head_equal_clip_by_clip(monkeypatch):
    """infer_clips_device on B = 3 clips of 12 frames (seeds 40, 41, 42) == infer_device clip by clip."""
    g, T, B = _tiny(), 12, 3
    model = _build(g)
    W = model.save_freq_max
    clips = torch.stack([synth.make_clip(g, T, seed=40 + b) for b in range(B)]).cuda()
    from phnet_amd import hip_ops as K
    routes, route_lines = _Routes(B), K.route_lines

    def spy(gates, a, b, hard):                                    # the gates the batched run itself routes with
        routes.add(gates)
        return route_lines(gates, a, b, hard)
    monkeypatch.setattr(K, "route_lines", spy)
    rows, nums, anchors = model.infer_clips_device(clips)
    monkeypatch.undo()
    assert routes.both() and sum(routes.to_a) + sum(routes.to_b) == B * T * model.router.num_priors
    assert rows.shape[:2] == (B, T) and nums.shape == (B, T) and anchors.shape[:2] == (B, T)
    kept_late = 0
    for b in range(B):
        with torch.no_grad():
            r, n, a, aux = model.infer_device(clips[b])
        for t in range(T):
            k = _same_frame((rows[b, t], nums[b, t], anchors[b, t]), (r[t], n[t], a[t]), BATCH_TOL, f"clip {b} frame {t}")
            kept_late += k if t >= W else 0
    assert kept_late > 0


def test_reset_every_reproduces_chunked_clips():
    """reset_every = 4 over 8 frames == infer_device on frames 0-3, then on frames 4-7."""
    g, T = _tiny(), 8
    model = _build(g)
    clip = synth.make_clip(g, T, seed=41).cuda()
    with torch.no_grad():
        want = [model.infer_device(clip[0:4]), model.infer_device(clip[4:8])]
    s = model.open_stream(streams=1, frame_hw=(g.img_h, g.img_w), graph=True, reset_every=4)
    routes = _Routes(1)
    kept = 0
    for t in range(T):
        rows, num, anchors = s.step(clip[t:t + 1])
        routes.add(s.gate_rows)
        assert int(s.state.cursor[0]) == t % 4, t
        w = want[t // 4]
        kept += _same_frame((rows[0], num[0], anchors[0]), (w[0][t % 4], w[1][t % 4], w[2][t % 4]), BATCH_TOL, f"frame {t}")
    assert kept > 0 and routes.both()


def test_one_graph_serves_every_frame():
    """graph=True against graph=False over 2W + 3 frames with a masked reset in the middle: decisions equal, rows within 1e-5; the
    graph captured at construction is the one replayed at the end (a reset never recaptures), and the replayed steps - frame copy,
    reset, replay - perform no synchronising device -> host copy (torch's sync debug mode in "error"; the test first checks that
    this torch build honours the mode)."""
    g, B = _tiny(), 2
    model = _build(g)
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
    kept_late = 0
    for t in range(T):
        for b in range(B):
            k = _same_frame(tuple(x[b] for x in got[t]), tuple(x[b] for x in want[t]), GRAPH_TOL, f"stream {b} frame {t}")
            kept_late += k if t >= W else 0
    assert kept_late > 0


def test_raw_camera_frames_enter_the_step():
    """raw= stream on uint8 camera frames == ClipPreprocessor on the same frames, then a plain stream step on its output:
    torch.equal on all three outputs (the same launches in the same order).  The captured form of the raw step replays the eager
    one within the graph-replay bound.  W + 2 frames, so that lanes kept after the ring wrapped are compared too."""
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    g, B = _tiny(), 2
    model = _build(g)
    W = model.save_freq_max
    T = W + 2
    pre = ClipPreprocessor(g.img_h, g.img_w, src_h=200, src_w=300, crop_size=40)
    gen = torch.Generator().manual_seed(11)
    cam = torch.randint(0, 256, (T, B, 200, 300, 3), generator=gen, dtype=torch.uint8).cuda()
    hw = (g.img_h, g.img_w)
    raw = model.open_stream(streams=B, frame_hw=hw, graph=False, raw=pre)
    raw_graph = model.open_stream(streams=B, frame_hw=hw, graph=True, raw=pre)
    plain = model.open_stream(streams=B, frame_hw=hw, graph=False)
    kept_late = 0
    for t in range(T):
        got = raw.step(cam[t])
        want = plain.step(pre(cam[t]))
        for a, b, name in zip(got, want, ("kept_rows", "num", "anchors")):
            assert torch.equal(a, b), (t, name)
        rep = raw_graph.step(cam[t])
        for b in range(B):
            k = _same_frame(tuple(x[b] for x in rep), tuple(x[b] for x in got), GRAPH_TOL, f"raw graph stream {b} frame {t}")
            kept_late += k if t >= W else 0
    assert kept_late > 0
    with pytest.raises(ValueError):
        raw.step(pre(cam[0]))                                      # a raw stream takes camera frames only
