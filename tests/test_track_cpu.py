"""Lane identities, the part that needs no GPU: the argument validation of phnet_lane_track (csrc/lane_track.hip), the resources
the compiler gives its kernel, the precondition of tests/test_track_gpu.py - the sequences of tests/track_cases.py really reach
every branch of the rules, by the numpy restatement alone - the invariants of the rules on those sequences, and
phnet_amd.polylines.to_host with track ids."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd import build as hip_build
from tests import polyline_cases as PC
from tests import track_cases as C

ERR_ARG = -1
MAX_TRACKS, MAX_OFFSETS, MAX_LDS_WORDS = 64, 256, 15360          # the limits include/phnet_hip.h states for phnet_lane_track


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


def test_lane_track_validates_without_a_gpu(built):
    """Each null pointer and each stated limit is PHNET_ERR_ARG before any launch (no device is touched: this runs on a machine
    without one).  Non-null pointers are made-up addresses - a call that got past the checks would try to launch."""
    lib = built
    p = 0x1000                                              # never dereferenced on the host

    def track(ptrs=(p,) * 10, b=3, t=1, l=4, s=72, m=8, thr=1.0 / 64.0, max_age=3):
        return lib.phnet_lane_track(*ptrs[:2], b, t, l, s, m, thr, max_age, *ptrs[2:], None)

    for i in range(10):
        assert track(tuple(None if j == i else p for j in range(10))) == ERR_ARG, i
    for bad in (0, -1):
        for key in ("b", "t", "l", "s", "m"):
            assert track(**{key: bad}) == ERR_ARG, (key, bad)
    assert track(s=1) == ERR_ARG and track(s=MAX_OFFSETS + 1) == ERR_ARG
    assert track(l=9, m=8) == ERR_ARG                                          # L <= M
    assert track(l=4, m=MAX_TRACKS + 1) == ERR_ARG and track(l=MAX_TRACKS + 1, m=MAX_TRACKS + 1) == ERR_ARG
    assert track(b=1 << 31) == ERR_ARG and track(b=1 << 40) == ERR_ARG         # streams are the grid's x dimension
    assert track(max_age=-1) == ERR_ARG
    for thr in (0.0, -1.0 / 64.0, float("nan"), float("inf"), float("-inf")):
        assert track(thr=thr) == ERR_ARG, thr
    # the LDS staging: (L + M) * S + 2 * L * M dwords.  L = M = 56, S = 120: 13440 + 6272 > 15360; every single limit holds
    assert (56 + 56) * 120 + 2 * 56 * 56 > MAX_LDS_WORDS and track(l=56, m=56, s=120) == ERR_ARG
    assert track(l=MAX_TRACKS, m=MAX_TRACKS, s=MAX_OFFSETS) == ERR_ARG
    from phnet_amd import hip_ops as K
    assert (K.LANE_TRACK_MAX_TRACKS, K.LANE_TRACK_MAX_OFFSETS, K.LANE_TRACK_MAX_LDS_WORDS) == (MAX_TRACKS, MAX_OFFSETS, MAX_LDS_WORDS)
    header = open(_lib.HEADER).read()
    assert "1 <= L <= M <= 64, 2 <= S <= 256, (L + M) * S + 2 * L * M <= 15360" in header
    assert "1 <= T, 1 <= B < 2^31, max_age >= 0, thr finite and > 0, all pointers non-null" in header
    names = {n: a for n, _, a in _lib.declared_functions(_lib.HEADER)}
    assert len(names["phnet_lane_track"]) == 18


def test_lane_track_kernel_compiles_without_scratch_or_spills(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/lane_track.hip: exactly one kernel, no scratch, no spilled registers."""
    src = os.path.join(hip_build.CSRC, "lane_track.hip")
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "lane_track.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len([n for n in names if "lane_track" in n]) == 1 and len(names) == 1, names
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", out.stderr)]
        assert len(vals) == 1 and not any(vals), (key, vals)
    print("VGPRs:", dict(zip(names, re.findall(r" VGPRs: (\d+)", out.stderr))),
          "occupancy:", re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr))


# ------------------------------------------------------------------------------------------------- census, by the restatement
def _hand(name):
    i = [c["name"] for c in C.hand_cases()].index(name)
    return (C.hand_cases()[i],) + C.hand_expected(i)


def test_inputs_are_dyadic():
    """xs are multiples of 1/4096 in [0, 1] (or the one NaN), r[5] an integer, r[2] * (S - 1) rounds to a small integer."""
    sets = [(c["kept"], c["S"]) for c in C.hand_cases()]
    sets += [(C.random_sequence(S, C.random_seed(S, b))[0], S) for S in (72, 37) for b in range(C.RANDOM_STREAMS)]
    assert float(C.THR) == 1.0 / 64.0
    for kept, S in sets:
        x = kept[..., 6:].astype(np.float64)
        ok = np.isnan(x) | ((x >= 0) & (x <= 1) & (x * 4096 == np.round(x * 4096)))
        assert ok.all()
        fin = np.isfinite(kept[..., 2]) & np.isfinite(kept[..., 5])
        assert (kept[..., 5][fin] == np.round(kept[..., 5][fin])).all()
        k = kept[..., 2][fin].astype(np.float64) * (S - 1)
        assert (np.abs(k - np.round(k)) < 1e-5).all() and np.round(k).min() >= 0 and np.round(k).max() <= 6


def test_hand_cases_hit_every_branch():
    """What each hand sequence is for happens in it, by the restatement alone - so equality on the GPU is not vacuous."""
    c, ids, hits, ev, st = _hand("tie_slots")
    assert ev[1]["tie_slots"] == 1 and ev[1]["matches"] == [(0, 0, 0)] and ids[1, 0] == 1 and st["missed"][1] == 1
    c, ids, hits, ev, st = _hand("tie_rows")
    assert ev[1]["tie_rows"] == 1 and ev[1]["matches"] == [(0, 0, 0)] and ids[1].tolist()[:2] == [1, 2] and ev[1]["births"] == [(1, 1, "free")]
    c, ids, hits, ev, st = _hand("strict")
    assert ev[1]["strict"] == 1 and not ev[1]["matches"] and ids[1, 0] == 2
    c, ids, hits, ev, st = _hand("disjoint")
    assert ev[1]["disjoint"] == 1 and not ev[1]["matches"] and ids[1, 0] == 2
    assert np.array_equal(c["kept"][0, 0, 6:], c["kept"][1, 0, 6:])
    c, ids, hits, ev, st = _hand("nan_x")
    assert ev[1]["nan_pair"] == 1 and ids[1, 0] == 2 and np.isnan(st["x"][1]).sum() == 1
    assert ev[2]["nan_pair"] == 1 and ev[2]["matches"] == [(0, 0, 1)] and ids[2, 0] == 1 and hits[2, 0] == 2
    c, ids, hits, ev, st = _hand("nonfinite")
    assert ev[0]["skipped"] == ["nonfinite"] * 3 and ids[0].tolist() == [-1, -1, -1, 1] and hits[0].tolist() == [0, 0, 0, 1]
    assert ev[1]["skipped"][0] == "nonfinite" and ids[1].tolist() == [-1, 1, -1, -1]
    c, ids, hits, ev, st = _hand("empty_extent")
    assert ev[0]["skipped"][:2] == ["empty", "empty"] and ids[0].tolist() == [-1, -1, 1, -1]
    assert ev[1]["skipped"][0] == "empty" and ids[1].tolist() == [-1, 1, -1, -1] and st["ext"][0].tolist() == [0, 11]
    c, ids, hits, ev, st = _hand("num_zero")
    assert (ids[1] == -1).all() and (hits[1] == 0).all() and ev[1]["skipped"] == ["num"] * 4 and ids[2, 0] == 1 and hits[2, 0] == 2
    c, ids, hits, ev, st = _hand("num_above_L")
    assert (c["num"] > c["L"]).all() and sorted(ids[0].tolist()) == [1, 2, 3, 4] and ids[1].tolist() == [2, 1, 4, 3]
    c, ids, hits, ev, st = _hand("num_negative")
    assert c["num"][1] < 0 and (ids[1] == -1).all() and ids[2, 0] == 1
    c, ids, hits, ev, st = _hand("reacquire")
    assert ev[3]["matches"] == [(0, 0, c["max_age"])] and ids[3, 0] == 1 and hits[3, 0] == 2
    c, ids, hits, ev, st = _hand("aged_out")
    assert ev[3]["aged_out"] == [0] and not ev[4]["matches"] and ids[4, 0] == 2 and hits[4, 0] == 1
    c, ids, hits, ev, st = _hand("evict")
    assert c["M"] == c["L"] and ev[2]["births"] == [(2, 0, "evict_tie")] and ev[3]["births"] == [(2, 1, "evict")]
    assert ids[3].tolist() == [4, 5, 6, -1] and not any(e["aged_out"] for e in ev)
    c, ids, hits, ev, st = _hand("wrap")
    assert ids[0].tolist()[:2] == [C.ID_MAX, 1] and ids[1].tolist()[:3] == [1, C.ID_MAX, 2] and int(st["next_id"]) == 3
    c, ids, hits, ev, st = _hand("reset")
    assert c["resets"] == (1,) and ids[:, 0].tolist() == [1, 2, 2] and hits[:, 0].tolist() == [1, 1, 2] and int(st["next_id"]) == 3


@pytest.mark.parametrize("S,M,max_age", C.RANDOM_CONFIGS)
def test_random_sequences_contain_what_they_are_for(S, M, max_age):
    """Matches, births and re-acquisitions (a match to a slot with missed > 0) in every configuration, evictions or age-outs with
    (M, max_age) = (4, 1); and the invariants: live ids within a frame are distinct, rows >= num have id -1, an id never moves to
    another ground lane (lanes are >= 500/4096 apart, jitter is +-8/4096, thr * 4096 = 64)."""
    matches = births = reacquired = evicted = aged = 0
    for b in range(C.RANDOM_STREAMS):
        kept, num, ground = C.random_sequence(S, C.random_seed(S, b))
        ids, hits, events, _ = C.random_expected(S, M, max_age, b)
        lane_of = {}
        for t in range(len(num)):
            n = int(num[t])
            assert (ids[t, n:] == -1).all() and (hits[t, n:] == 0).all() and (ids[t, :n] > 0).all() and (hits[t, :n] > 0).all()
            assert len(set(ids[t, :n].tolist())) == n
            for d in range(n):
                assert lane_of.setdefault(int(ids[t, d]), int(ground[t, d])) == int(ground[t, d]), (b, t, d)
            ev = events[t]
            matches += len(ev["matches"]); births += len(ev["births"]); aged += len(ev["aged_out"])
            reacquired += sum(m[2] > 0 for m in ev["matches"])
            evicted += sum(how != "free" for _, _, how in ev["births"])
    print(f"S = {S}, M = {M}, max_age = {max_age}: {matches} matches ({reacquired} re-acquisitions), {births} births "
          f"({evicted} by eviction), {aged} aged out")
    assert matches >= 100 and births >= 10 and reacquired >= 10
    if (M, max_age) == (4, 1):
        assert evicted + aged >= 10
    assert sorted(set(C.random_sequence(S, C.random_seed(S, 0))[1].tolist()))[0] < C.L_RANDOM       # frames with fewer than L rows


def test_random_streams_differ():
    for S in (72, 37):
        a, b = (C.random_sequence(S, C.random_seed(S, i))[0] for i in (0, 1))
        assert not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------- the host side
def _as_tensors(exp):
    return [torch.from_numpy(exp[k]) for k in ("points", "count", "lanes_num", "slot")]


def test_to_host_carries_track_ids_through_slot():
    """to_host on tensors laid out as the kernels write them: metadata["track_id"] is the id of the kept_rows slot the packed
    lane came from (frames where packing moves lanes are present), a Python int; without track_id the result is today's."""
    from phnet_amd import polylines as P
    kept, num = PC.random_frames(40, 4, PC.S_MAIN, seed=7)
    exp = PC.expected_layout(kept, num)
    ids = torch.arange(1, 40 * 4 + 1, dtype=torch.int32).view(40, 4) * 7
    plain = P.to_host(*_as_tensors(exp), kept)
    got = P.to_host(*_as_tensors(exp), kept, track_id=ids)
    moved = lanes = 0
    for f, (a, b) in enumerate(zip(got, plain)):
        assert len(a) == len(b) == int(exp["lanes_num"][f])
        for k, (x, y) in enumerate(zip(a, b)):
            src = int(exp["slot"][f, k])
            assert type(x.metadata["track_id"]) is int and x.metadata["track_id"] == int(ids[f, src])
            assert set(y.metadata) == {"start_x", "start_y", "conf"} and set(x.metadata) == set(y.metadata) | {"track_id"}
            assert np.array_equal(x.points, y.points) and all(float(x.metadata[m]) == float(y.metadata[m]) for m in y.metadata)
            moved += src != k
            lanes += 1
    assert moved > 0 and lanes > 40
    nested = P.to_host(*[t.view(2, 20, *t.shape[1:]) for t in _as_tensors(exp)], kept.view(2, 20, *kept.shape[1:]), track_id=ids.view(2, 20, 4))
    assert [[[ln.metadata["track_id"] for ln in fr] for fr in clip] for clip in nested] == \
           [[[ln.metadata["track_id"] for ln in fr] for fr in got[i:i + 20]] for i in (0, 20)]
    with pytest.raises(ValueError):
        P.to_host(*_as_tensors(exp), kept, track_id=ids.long())
    with pytest.raises(ValueError):
        P.to_host(*_as_tensors(exp), kept, track_id=ids[:, :3])


def test_surface_exists_and_refuses_to_run_without_a_gpu():
    from phnet_amd import hip_ops as K
    from phnet_amd import tracking
    from phnet_amd.libs.models import Router4OL, Router4OLV2
    from phnet_amd.stream import LaneStream
    for mod in (Router4OL, Router4OLV2):
        sig = inspect.signature(mod.RouterOL.open_stream).parameters
        assert sig["track"].default is False and all(sig[k].default is None for k in ("max_tracks", "max_age", "match_thres"))
        assert callable(mod.RouterOL.track_clips)
    sig = inspect.signature(LaneStream.__init__).parameters
    assert sig["track"].default is False and sig["polylines"].default is False
    assert inspect.signature(__import__("phnet_amd.polylines", fromlist=["to_host"]).to_host).parameters["track_id"].default is None
    st = tracking.TrackState(3, 8, 72, "cpu")
    assert [tuple(t.shape) for t in st.tensors()] == [(3, 8), (3, 8), (3, 8), (3, 8, 2), (3, 8, 72), (3,)]
    assert st.next_id.tolist() == [1, 1, 1] and st.x.dtype == torch.float32 and all(t.dtype == torch.int32 for t in st.tensors() if t is not st.x)
    st.id.fill_(5); st.next_id.fill_(9)
    st.reset(torch.tensor([True, False, True]))
    assert st.id[:, 0].tolist() == [0, 5, 0] and st.next_id.tolist() == [9, 9, 9]          # a reset frees the slots, keeps next_id
    st.reset()
    assert int(st.id.abs().sum()) == 0 and st.next_id.tolist() == [9, 9, 9]
    kept, num, _ = C.random_sequence(72, C.random_seed(72, 0))
    with pytest.raises(RuntimeError):
        K.lane_track(torch.from_numpy(kept[:3]), torch.from_numpy(num[:3]), st, float(C.THR), 3)


def test_track_defaults_follow_the_model_configuration():
    """max_tracks = 2 * max_lanes, max_age = save_freq_max, thr = float32(nms_thres / (img_w - 1)); match_thres is in pixels."""
    from types import SimpleNamespace
    from phnet_amd.config import make_cfg
    from phnet_amd.tracking import track_defaults
    cfg = make_cfg(img_w=800, nms_thres=50, max_lanes=4, save_freq_max=8)
    model = SimpleNamespace(head=SimpleNamespace(cfg=cfg, img_w=800), save_freq_max=8)
    assert track_defaults(model) == (8, 8, float(np.float32(50 / 799)))
    assert track_defaults(model, max_tracks=4, max_age=0, match_thres=12.5) == (4, 0, float(np.float32(12.5 / 799)))
    for bad in (dict(max_tracks=3), dict(max_tracks=65), dict(max_age=-1), dict(match_thres=0.0), dict(match_thres=float("nan"))):
        with pytest.raises(ValueError):
            track_defaults(model, **bad)
