"""Lane identities on the MI355X (csrc/lane_track.hip, phnet_amd/tracking.py): the kernel against the numpy restatement of
tests/track_cases.py - every hand case and every random sequence, outputs and all six state tensors bit for bit - and the tracker
inside the streams of both model families, in clips and on the host side.

Everything is compared exactly.  The built inputs are dyadic (track_cases.py), so no sum depends on its order; on the models'
own kept rows kernel and restatement perform the same f32 operations in the same order (ascending, not contracted)."""
import numpy as np
import pytest
import torch

from oracle import phnet_cpu as O
from oracle import phnet_cpu_v2 as O2
from tests import synth
from tests import track_cases as C

pytestmark = pytest.mark.gpu

BATCH_TOL = 2e-4                 # kept rows across batch shapes (tests/test_stream_gpu.py)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _to_device(states):
    """Per-stream numpy states -> a tracking.TrackState on the GPU."""
    from phnet_amd.tracking import TrackState
    M, S = states[0]["x"].shape
    ts = TrackState(len(states), M, S, "cuda")
    for k in C.STATE_KEYS:
        getattr(ts, k).copy_(torch.from_numpy(np.stack([st[k] for st in states])))
    return ts


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_state(ts, states, what):
    for k in C.STATE_KEYS:
        want = torch.from_numpy(np.stack([st[k] for st in states]))
        assert torch.equal(_bits(getattr(ts, k).cpu()), _bits(want)), (what, k)


def _run(kept, num, ts, max_age, resets=(), frame_by_frame=False):
    """kept [B,T,L,6+S], num [B,T] (numpy) through hip_ops.lane_track on state ts: one launch per run of frames between resets
    (or per frame) -> (track_id, hits) int32 [B,T,L] on the host."""
    from phnet_amd import hip_ops as K
    T = kept.shape[1]
    rows, n = torch.from_numpy(kept).cuda(), torch.from_numpy(num).cuda()
    cuts = sorted(set(range(T)) if frame_by_frame else {0, *resets}) + [T]
    ids, hits = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a in resets:
            ts.reset()
        if frame_by_frame:
            out = K.lane_track(rows[:, a].contiguous(), n[:, a].contiguous(), ts, float(C.THR), max_age)
            out = {k: v[:, None] for k, v in out.items()}
        else:
            out = K.lane_track(rows[:, a:b].contiguous(), n[:, a:b].contiguous(), ts, float(C.THR), max_age)
        ids.append(out["track_id"]); hits.append(out["hits"])
    return torch.cat(ids, 1).cpu(), torch.cat(hits, 1).cpu()


# ------------------------------------------------------------------------------------------------- kernel against restatement
@pytest.mark.parametrize("i", range(len(C.hand_cases())), ids=[c["name"] for c in C.hand_cases()])
def test_kernel_equals_restatement_on_hand_cases(i):
    """Outputs and the six state tensors after the sequence, torch.equal (x by its bits: a stored NaN must be the same NaN)."""
    _need_gpu()
    c = C.hand_cases()[i]
    want_ids, want_hits, _, want_state = C.hand_expected(i)
    for frame_by_frame in (False, True):
        ts = _to_device([C.new_state(c["M"], c["S"], c["next_id"])])
        ids, hits = _run(c["kept"][None], c["num"][None], ts, c["max_age"], c["resets"], frame_by_frame)
        print(c["name"], "ids", ids[0].tolist(), "hits", hits[0].tolist())
        assert torch.equal(ids[0], torch.from_numpy(want_ids)), (c["name"], ids[0].tolist(), want_ids.tolist())
        assert torch.equal(hits[0], torch.from_numpy(want_hits)), (c["name"], hits[0].tolist(), want_hits.tolist())
        _same_state(ts, [want_state], c["name"])


@pytest.mark.parametrize("S,M,max_age", C.RANDOM_CONFIGS)
def test_kernel_equals_restatement_on_random_sequences(S, M, max_age):
    """B = 3 streams, 40 frames in ONE launch == the restatement of each stream == the three streams run alone == 40 launches
    with T = 1; and garbage (NaN xs, wild extents and counters) in the free slots of the initial state changes nothing."""
    _need_gpu()
    B = C.RANDOM_STREAMS
    seqs = [C.random_sequence(S, C.random_seed(S, b)) for b in range(B)]
    kept, num = np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs])
    want = [C.random_expected(S, M, max_age, b) for b in range(B)]
    want_ids = torch.from_numpy(np.stack([w[0] for w in want]))
    want_hits = torch.from_numpy(np.stack([w[1] for w in want]))

    ts = _to_device([C.new_state(M, S) for _ in range(B)])
    ids, hits = _run(kept, num, ts, max_age)
    assert torch.equal(ids, want_ids) and torch.equal(hits, want_hits)
    _same_state(ts, [w[3] for w in want], "one launch")

    for b in range(B):                                                              # each stream alone
        one = _to_device([C.new_state(M, S)])
        i1, h1 = _run(kept[b:b + 1], num[b:b + 1], one, max_age)
        assert torch.equal(i1[0], want_ids[b]) and torch.equal(h1[0], want_hits[b]), b
        _same_state(one, [want[b][3]], f"stream {b} alone")

    ts = _to_device([C.new_state(M, S) for _ in range(B)])                         # T = 1, 40 times
    ids, hits = _run(kept, num, ts, max_age, frame_by_frame=True)
    assert torch.equal(ids, want_ids) and torch.equal(hits, want_hits)
    _same_state(ts, [w[3] for w in want], "frame by frame")

    rng = np.random.default_rng(5)                                                  # garbage in the free slots
    dirty = []
    for b in range(B):
        st = C.new_state(M, S)
        st["missed"][:] = rng.integers(-2 ** 31, 2 ** 31 - 1, M)
        st["hits"][:] = rng.integers(-2 ** 31, 2 ** 31 - 1, M)
        st["ext"][:] = rng.integers(-2 ** 31, 2 ** 31 - 1, (M, 2))
        st["x"][:] = np.where(rng.random((M, S)) < 0.5, np.nan, rng.standard_normal((M, S)) * 1e30).astype(np.float32)
        dirty.append(st)
    ts = _to_device([C.copy_state(st) for st in dirty])
    ids, hits = _run(kept, num, ts, max_age)
    assert torch.equal(ids, want_ids) and torch.equal(hits, want_hits)
    again = [C.copy_state(st) for st in dirty]
    for b in range(B):                                                              # the restatement from the same garbage
        i2, h2, _ = C.track_stream(kept[b], num[b], again[b], C.THR, max_age)
        assert np.array_equal(i2, want[b][0]) and np.array_equal(h2, want[b][1])
    _same_state(ts, again, "dirty free slots")


def test_out_buffers_and_argument_checks():
    """out= is written in place and every element of it on every call; mismatched shapes are refused before the launch."""
    _need_gpu()
    from phnet_amd import hip_ops as K
    S, M = 37, 8
    kept, num, _ = C.random_sequence(S, C.random_seed(S, 0))
    rows, n = torch.from_numpy(kept[:1]).cuda(), torch.from_numpy(num[:1]).cuda()
    ts = _to_device([C.new_state(M, S)])
    out = {k: torch.full((1, C.L_RANDOM), 77, dtype=torch.int32, device="cuda") for k in ("track_id", "hits")}
    got = K.lane_track(rows, n, ts, float(C.THR), 3, out=out)
    assert got["track_id"].data_ptr() == out["track_id"].data_ptr() and not bool((out["track_id"] == 77).any()) and not bool((out["hits"] == 77).any())
    with pytest.raises(ValueError):
        K.lane_track(rows, n[:0], ts, float(C.THR), 3)
    with pytest.raises(ValueError):
        K.lane_track(rows.repeat(2, 1, 1), n.repeat(2), ts, float(C.THR), 3)          # two streams, state of one
    with pytest.raises(RuntimeError):
        K.lane_track(rows, n, ts, 0.0, 3)                                              # PHNET_ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ the models
def _build_v1(conf_threshold=0.5):
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import RouterOL
    g = O.Geometry(img_h=64, img_w=160, arch="resnet18", conf_threshold=conf_threshold)
    model = RouterOL(make_cfg(img_h=g.img_h, img_w=g.img_w, arch=g.arch, conf_threshold=conf_threshold), None)
    model.load_state_dict(synth.make_state(g), strict=True)
    return g, model.cuda().eval()


def _build_v2():
    from phnet_amd.config import make_cfg_v2
    from phnet_amd.libs.models.Router4OLV2 import RouterOL
    g = O2.GeometryV2(img_h=64, img_w=160)
    model = RouterOL(make_cfg_v2(img_h=g.img_h, img_w=g.img_w, arch=g.arch))
    model.load_state_dict(synth.make_state_v2(g), strict=True)
    return g, model.cuda().eval()


def _restate(model, rows, nums, resets=(), max_tracks=None):
    """The restatement with the model's defaults on host copies rows [T,L,6+S] / nums [T] of ONE stream."""
    from phnet_amd.tracking import track_defaults
    M, age, thr = track_defaults(model, max_tracks)
    st = C.new_state(M, rows.shape[-1] - 6)
    ids, hits, events = C.track_stream(rows.numpy(), nums.numpy(), st, np.float32(thr), age, resets)
    return ids, hits, events


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_stream_tracks_equal_the_restatement_of_its_own_rows(family):
    """The reference's tiny eval clip of each family (synth.make_clip seed 77: tests/golden tiny_long_eval / v2_tiny), each frame
    fed twice in a row, through a captured stream with track=True, polylines=True: kept_rows / num / anchors and the polylines
    are bit-identical to a stream without tracking; stream.tracks equals the restatement on the host copy of the stream's own
    kept rows; the eager stream gives the same ids as the replayed graph; lanes_fast() carries the ids through `slot`.
    Precondition, asserted: an id lives >= 3 frames and >= 2 distinct ids appear."""
    _need_gpu()
    g, model = _build_v1() if family == "v1" else _build_v2()
    T = 11 if family == "v1" else 8
    clip = synth.make_clip(g, T, seed=77).cuda()
    hw = (g.img_h, g.img_w)
    s = model.open_stream(streams=1, frame_hw=hw, graph=True, polylines=True, track=True)
    eager = model.open_stream(streams=1, frame_hw=hw, graph=False, polylines=True, track=True)
    plain = model.open_stream(streams=1, frame_hw=hw, graph=True, polylines=True)
    assert plain.tracks is None and plain.track_state is None and s.graph is not None
    assert tuple(s.tracks["track_id"].shape) == (1, model.head.cfg.max_lanes) and s.tracks["hits"].dtype == torch.int32
    rows_all, nums_all, got_ids, got_hits = [], [], [], []
    buffers = (s.tracks["track_id"].data_ptr(), s.tracks["hits"].data_ptr())
    for t in range(2 * T):
        frame = clip[t // 2:t // 2 + 1]
        rows, num, anchors = s.step(frame)
        for a, b, name in zip((rows, num, anchors), plain.step(frame), ("kept_rows", "num", "anchors")):
            assert torch.equal(a, b), (t, name)
        for k in ("points", "count", "lanes_num", "slot"):
            assert torch.equal(_bits(s.polylines[k]), _bits(plain.polylines[k])), (t, k)
        eager.step(frame)
        assert torch.equal(eager.tracks["track_id"], s.tracks["track_id"]) and torch.equal(eager.tracks["hits"], s.tracks["hits"]), t
        ids = s.tracks["track_id"][0].cpu()
        lines, slot = s.lanes_fast()[0], s.polylines["slot"][0].cpu()
        assert len(lines) == int(s.polylines["lanes_num"][0])
        for k, line in enumerate(lines):
            assert type(line.metadata["track_id"]) is int and line.metadata["track_id"] == int(ids[slot[k]]) > 0, (t, k)
        assert all("track_id" not in line.metadata for line in plain.lanes_fast()[0])
        rows_all.append(rows[0].cpu()); nums_all.append(num[0].cpu()); got_ids.append(ids); got_hits.append(s.tracks["hits"][0].cpu())
    assert buffers == (s.tracks["track_id"].data_ptr(), s.tracks["hits"].data_ptr())          # static graph buffers
    rows_all, nums_all = torch.stack(rows_all), torch.stack(nums_all)
    want_ids, want_hits, events = _restate(model, rows_all, nums_all)
    got_ids, got_hits = torch.stack(got_ids), torch.stack(got_hits)
    print(family, "num per step", nums_all.tolist(), "\nids per step", got_ids.tolist())
    assert torch.equal(got_ids, torch.from_numpy(want_ids)) and torch.equal(got_hits, torch.from_numpy(want_hits))
    live = got_ids[got_ids > 0]
    assert int(got_hits.max()) >= 3 and len(set(live.tolist())) >= 2, (int(got_hits.max()), set(live.tolist()))
    assert sum(len(e["matches"]) for e in events) > 0 and int(s.track_state.next_id[0]) == len(set(live.tolist())) + 1


def test_reset_gives_new_ids_to_that_stream_only():
    """B = 3 streams (the clips of test_streams_are_independent), stream 0 reset before frame 4: its ids from there on are all
    new and above every id it used before; every stream equals the restatement of its own rows with its own resets."""
    _need_gpu()
    g, model = _build_v1(conf_threshold=0.3)
    B, T = 3, 8
    clips = torch.stack([synth.make_clip(g, T, seed=40 + b) for b in range(B)]).cuda()
    s = model.open_stream(streams=B, frame_hw=(g.img_h, g.img_w), graph=True, track=True)
    rows_all, nums_all, ids_all, hits_all = [], [], [], []
    for t in range(T):
        if t == 4:
            s.reset([True, False, False])
        rows, num, _ = s.step(clips[:, t])
        rows_all.append(rows.cpu()); nums_all.append(num.cpu())
        ids_all.append(s.tracks["track_id"].cpu()); hits_all.append(s.tracks["hits"].cpu())
    rows_all, nums_all = torch.stack(rows_all, 1), torch.stack(nums_all, 1)               # [B,T,..]
    ids_all, hits_all = torch.stack(ids_all, 1), torch.stack(hits_all, 1)
    print("ids", ids_all.tolist())
    for b in range(B):
        want_ids, want_hits, _ = _restate(model, rows_all[b], nums_all[b], resets=(4,) if b == 0 else ())
        assert torch.equal(ids_all[b], torch.from_numpy(want_ids)) and torch.equal(hits_all[b], torch.from_numpy(want_hits)), b
    before, after = ids_all[0, :4][ids_all[0, :4] > 0], ids_all[0, 4:][ids_all[0, 4:] > 0]
    assert before.numel() and after.numel() and int(after.min()) > int(before.max())
    assert (hits_all[0, 4][ids_all[0, 4] > 0] == 1).all()                                  # born again on the frame after the cut
    for b in (1, 2):                                                                        # the others carry on
        kept4 = ids_all[b, 4][ids_all[b, 4] > 0]
        assert kept4.numel() and set(kept4.tolist()) & set(ids_all[b, 3].tolist()), b


def test_reset_every_keeps_ids_across_the_chunk_boundary():
    """reset_every = 4 over 8 frames: the kept rows are those of the chunked clips (test_reset_every_reproduces_chunked_clips)
    and bit for bit those of the same stream without tracking; the tracks are NOT reset at frame 4 - they equal the restatement
    without a reset, and an id of frame 3 is still there on frame 4."""
    _need_gpu()
    g, model = _build_v1(conf_threshold=0.3)
    T = 8
    clip = synth.make_clip(g, T, seed=41).cuda()
    with torch.no_grad():
        want = [model.infer_device(clip[0:4]), model.infer_device(clip[4:8])]
    hw = (g.img_h, g.img_w)
    s = model.open_stream(streams=1, frame_hw=hw, graph=True, reset_every=4, track=True)
    plain = model.open_stream(streams=1, frame_hw=hw, graph=True, reset_every=4)
    rows_all, nums_all, ids_all, hits_all = [], [], [], []
    for t in range(T):
        rows, num, anchors = s.step(clip[t:t + 1])
        for a, b, name in zip((rows, num, anchors), plain.step(clip[t:t + 1]), ("kept_rows", "num", "anchors")):
            assert torch.equal(a, b), (t, name)
        assert bool(s.state.has_memory[0]) == (t % 4 != 0), t
        w = want[t // 4]
        k = int(w[1][t % 4])
        assert int(num[0]) == k and torch.equal(anchors[0, :k], w[2][t % 4][:k]), t
        err = (rows[0, :k] - w[0][t % 4][:k]).abs().double()
        assert bool((err <= BATCH_TOL * (1 + w[0][t % 4][:k].abs().double())).all()), t
        rows_all.append(rows[0].cpu()); nums_all.append(num[0].cpu())
        ids_all.append(s.tracks["track_id"][0].cpu()); hits_all.append(s.tracks["hits"][0].cpu())
    ids_all, hits_all = torch.stack(ids_all), torch.stack(hits_all)
    want_ids, want_hits, _ = _restate(model, torch.stack(rows_all), torch.stack(nums_all))
    print("ids", ids_all.tolist())
    assert torch.equal(ids_all, torch.from_numpy(want_ids)) and torch.equal(hits_all, torch.from_numpy(want_hits))
    carried = set(ids_all[3][ids_all[3] > 0].tolist()) & set(ids_all[4][ids_all[4] > 0].tolist())
    assert carried, (ids_all[3].tolist(), ids_all[4].tolist())


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_track_clips_equals_the_restatement(family):
    """model.track_clips on infer_clips_device output ([B,T,..]) and on infer_device output ([T,..]): one launch each, equal to the
    restatement clip by clip; the infer_* results themselves are untouched."""
    _need_gpu()
    g, model = _build_v1(conf_threshold=0.3) if family == "v1" else _build_v2()
    B, T = 2, 6
    clips = torch.stack([synth.make_clip(g, T, seed=40 + b) for b in range(B)]).cuda()
    with torch.no_grad():
        rows, nums = model.infer_clips_device(clips)[:2]
        rows1, nums1 = model.infer_device(clips[1])[:2]
    keep = rows.clone()
    ids, hits = model.track_clips(rows, nums)
    ids1, hits1 = model.track_clips(rows1, nums1, max_tracks=4, max_age=1)
    assert torch.equal(rows, keep) and tuple(ids.shape) == tuple(nums.shape) + (rows.shape[-2],) and ids.dtype == hits.dtype == torch.int32
    assert tuple(ids1.shape) == (T, rows.shape[-2])
    for b in range(B):
        want_ids, want_hits, _ = _restate(model, rows[b].cpu(), nums[b].cpu())
        assert torch.equal(ids[b].cpu(), torch.from_numpy(want_ids)) and torch.equal(hits[b].cpu(), torch.from_numpy(want_hits)), b
    from phnet_amd.tracking import track_defaults
    M, age, thr = track_defaults(model, 4, 1)
    st = C.new_state(M, rows1.shape[-1] - 6)
    want_ids, want_hits, _ = C.track_stream(rows1.cpu().numpy(), nums1.cpu().numpy(), st, np.float32(thr), age)
    assert torch.equal(ids1.cpu(), torch.from_numpy(want_ids)) and torch.equal(hits1.cpu(), torch.from_numpy(want_hits))
    assert int(nums.sum()) > 0 and int(hits.max()) >= 2
