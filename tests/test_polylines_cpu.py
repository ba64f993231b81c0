"""Device-side lane polylines, the part that needs no GPU: the argument validation of phnet_lane_points (csrc/lane_points.hip),
the resources the compiler gives its kernel, the precondition of tests/test_polylines_gpu.py - the adversarial rows really hit
every branch of DetNetV2.predictions_to_pred, by that host function alone - and phnet_amd.polylines.to_host on tensors laid out
the way the kernel writes them."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd import build as hip_build
from phnet_amd.evaluation.generate_lane import format_pred_lines
from tests import polyline_cases as C

ERR_ARG = -1
MAX_LANES, MAX_OFFSETS = 64, 256                 # the limits include/phnet_hip.h states for phnet_lane_points


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


def test_lane_points_validates_without_a_gpu(built):
    """Null pointers, F / L / S < 1, S = 1, S and L above the stated maxima and an F the grid cannot hold are PHNET_ERR_ARG
    before any launch (no device is touched: this runs on a machine without one).  Non-null pointers are made-up addresses - a
    call that got past the checks would try to launch."""
    lib = built
    p = 0x1000                                              # never dereferenced on the host
    ins, outs = (p,) * 3, (p,) * 4

    def points(ptrs=ins + outs, f=5, l=4, s=72):
        return lib.phnet_lane_points(*ptrs[:3], f, l, s, *ptrs[3:], None)

    for i in range(7):
        assert points(tuple(None if j == i else p for j in range(7))) == ERR_ARG, i
    for bad in (0, -1):
        for key in ("f", "l", "s"):
            assert points(**{key: bad}) == ERR_ARG, (key, bad)
    assert points(s=1) == ERR_ARG                                              # a lane needs two points
    assert points(s=MAX_OFFSETS + 1) == ERR_ARG and points(l=MAX_LANES + 1) == ERR_ARG
    assert points(f=1 << 31) == ERR_ARG and points(f=1 << 40) == ERR_ARG       # frames are the grid's x dimension
    from phnet_amd import hip_ops as K
    assert (K.LANE_POINTS_MAX_LANES, K.LANE_POINTS_MAX_OFFSETS) == (MAX_LANES, MAX_OFFSETS)
    header = open(_lib.HEADER).read()
    assert "1 <= L <= 64, 2 <= S <= 256" in header


def test_lane_points_kernel_compiles_without_scratch_or_spills(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/lane_points.hip: one kernel, no scratch, no spilled registers."""
    src = os.path.join(hip_build.CSRC, "lane_points.hip")
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "lane_points.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len([n for n in names if "lane_points" in n]) == 1 and len(names) == 1, names
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", out.stderr)]
        assert len(vals) == 1 and not any(vals), (key, vals)
    print("VGPRs:", dict(zip(names, re.findall(r" VGPRs: (\d+)", out.stderr))),
          "occupancy:", re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr))


def _facts(S, r):
    """What the host function does with one row, read off its inputs and its OUTPUT only."""
    n = S - 1
    ys = [float(v) for v in C.head(S).prior_ys.double()]
    raw = float(r[2]) * n
    start = min(max(0, int(round(raw))), n)
    length = int(round(float(r[5])))
    end_raw = start + length - 1
    lanes = C.host_lanes(S, r[None])
    idx = [ys.index(float(y)) for y in lanes[0].points[:, 1]] if lanes else []
    x = r[6:].tolist()
    inside = [0.0 <= v <= 1.0 for v in x]
    return dict(
        lane=bool(lanes), idx=idx, start=start, length=length,
        extended=bool(idx) and min(idx) < start,
        # an in-image x below the start that is NOT in the lane although the range [.., end] would reach it: the extension was cut
        cut=bool(lanes) and any(inside[i] and i not in idx and i <= end_raw for i in range(start)) and
            any(not inside[i] for i in range(start)),
        tie=(raw - math.floor(raw) == 0.5 and 0 < raw < n, int(math.floor(raw)) % 2),
        start_low=raw < -0.5, start_high=raw > n + 0.5, end_clamped=end_raw > S - 1,
        len0=length == 0, neg_slice=end_raw + 1 < 0,
        x_gt1=bool(lanes) and bool((lanes[0].points[:, 0] > 1.0).any()),
        nan=any(v != v for v in x),
        descending=idx == sorted(idx, reverse=True))


@pytest.mark.parametrize("S", [C.S_MAIN, C.S_ODD])
def test_adversarial_rows_hit_every_branch_of_the_host_function(S):
    """Precondition of the GPU comparison, by predictions_to_pred alone: the committed rows contain every case the kernel must
    get right, so equality with the host function there is not vacuous."""
    frames = C.adversarial_frames(S)
    facts = [[_facts(S, r) for r in rows] for rows in frames]
    flat = [f for rows in facts for f in rows]
    assert all(f["descending"] for f in flat)                                  # points come in descending offset index
    assert any(f["extended"] for f in flat), "no lane extended below start"
    assert any(f["cut"] for f in flat), "no extension cut by an out-of-image x"
    assert any(not f["lane"] for f in flat), "no lane dropped for <= 1 point"
    assert any(not a["lane"] and any(b["lane"] for b in rows[i + 1:]) for rows in facts for i, a in enumerate(rows)), \
        "no frame with a dropped lane before a surviving one"
    parities = {f["tie"][1] for f in flat if f["tie"][0]}
    assert parities == ({0, 1} if S == C.S_ODD else {1}), parities             # n_strips = 71 has one in-range tie: 35.5
    assert any(f["start_low"] for f in flat) and any(f["start_high"] for f in flat), "start not clamped at both ends"
    assert any(f["end_clamped"] for f in flat) and any(f["len0"] for f in flat)
    assert any(f["neg_slice"] and f["lane"] for f in flat), "no negative length that keeps a lane (negative-slice branch)"
    assert any(f["neg_slice"] and not f["lane"] for f in flat)
    assert any(f["x_gt1"] for f in flat) and any(f["nan"] and f["lane"] for f in flat)
    assert any(f["length"] > 2 ** 31 for f in flat)                            # a length no int32 holds
    print(f"S = {S}: {len(flat)} rows in {len(frames)} frames, {sum(f['lane'] for f in flat)} lanes")


def test_ties_occur_in_both_parities_over_the_two_row_sets():
    """Half-to-even matters: 35.5 -> 36 (S = 72), 4.5 -> 4, 13.5 -> 14, 22.5 -> 22, 31.5 -> 32 (S = 37), and the rows are built so
    that the lane differs if the start moves by one."""
    seen = {}
    for S in (C.S_MAIN, C.S_ODD):
        for rows in C.adversarial_frames(S):
            for r in rows:
                f = _facts(S, r)
                if f["tie"][0]:
                    seen[(S, float(r[2]) * (S - 1))] = f["start"]
    assert seen == {(72, 35.5): 36, (37, 4.5): 4, (37, 13.5): 14, (37, 22.5): 22, (37, 31.5): 32}, seen


def test_random_frames_cover_the_sizes_and_stay_mixed():
    """The seeded generator of the GPU comparison: every num from 0 to L, lanes kept and dropped, ties present."""
    for L, S in ((4, C.S_MAIN), (8, C.S_ODD)):
        kept, num = C.random_frames(120, L, S, seed=7)
        assert sorted(set(num.tolist())) == list(range(L + 1))
        exp = C.expected_layout(kept, num)
        assert 0 < int(exp["lanes_num"].sum()) < int(num.sum())
        assert any((exp["slot"][f, :exp["lanes_num"][f]] != np.arange(exp["lanes_num"][f])).any() for f in range(len(num)))   # packing matters
        prod = kept[:, :, 2].double() * (S - 1)
        assert bool(((prod - prod.floor()) == 0.5).any())


def _as_tensors(exp):
    return [torch.from_numpy(exp[k]) for k in ("points", "count", "lanes_num", "slot")]


@pytest.mark.parametrize("S", [C.S_MAIN, C.S_ODD])
def test_to_host_equals_the_lane_path(S):
    """polylines.to_host on CPU tensors laid out as the kernel writes them (built from the host function's output): the same
    points (np.array_equal, float64), the same metadata, the identical .lines.txt text, and as_lane() evaluates equal."""
    from phnet_amd import polylines as P
    kept, num = C.pack_frames(C.adversarial_frames(S), S, L=4)
    exp = C.expected_layout(kept, num)
    got = P.to_host(*_as_tensors(exp), kept)
    assert len(got) == len(exp["lanes"])
    ys = np.linspace(0.0, 1.0, 29)
    n_lanes = 0
    for fast, slow in zip(got, exp["lanes"]):
        assert len(fast) == len(slow)
        for a, b in zip(fast, slow):
            assert isinstance(a, P.Polyline) and a.points.dtype == np.float64 and np.array_equal(a.points, b.points)
            assert set(a.metadata) == set(b.metadata) == {"start_x", "start_y", "conf"}
            assert all(float(a.metadata[k]) == float(b.metadata[k]) for k in a.metadata)
            lane = a.as_lane()
            assert np.array_equal(lane.points, b.points) and np.array_equal(lane(ys.copy()), b(ys.copy()))
            assert all(float(lane.metadata[k]) == float(b.metadata[k]) for k in b.metadata)
            n_lanes += 1
        assert format_pred_lines(fast, (590, 1640)) == format_pred_lines(slow, (590, 1640))
    assert n_lanes >= 10
    assert any(format_pred_lines(slow, (590, 1640)) for slow in exp["lanes"])


def test_to_host_nests_like_the_leading_dimensions():
    """[B,T,...] in -> B lists of T lists of Polyline; one frame without leading dimensions -> its Polyline list."""
    from phnet_amd import polylines as P
    kept, num = C.random_frames(6, 4, C.S_MAIN, seed=3)
    exp = C.expected_layout(kept, num)
    flat = P.to_host(*_as_tensors(exp), kept)
    pts, cnt, ln, sl = _as_tensors(exp)
    nested = P.to_host(pts.view(2, 3, *pts.shape[1:]), cnt.view(2, 3, -1), ln.view(2, 3), sl.view(2, 3, -1), kept.view(2, 3, *kept.shape[1:]))
    assert len(nested) == 2 and all(len(clip) == 3 for clip in nested)
    for i in range(6):
        a, b = nested[i // 3][i % 3], flat[i]
        assert len(a) == len(b) == len(exp["lanes"][i]) and all(np.array_equal(x.points, y.points) for x, y in zip(a, b))
    one = P.to_host(pts[1], cnt[1], ln[1], sl[1], kept[1])
    assert len(one) == len(flat[1]) and all(np.array_equal(x.points, y.points) for x, y in zip(one, flat[1]))
    with pytest.raises(ValueError):
        P.to_host(pts, cnt, ln, sl, kept[:, :, :-1])


def test_surface_exists_and_refuses_to_run_without_a_gpu():
    """The public pieces exist; the kernel wrapper has no CPU path."""
    from phnet_amd import hip_ops as K
    from phnet_amd.graphed import GraphedInference
    from phnet_amd.libs.models import Router4OL, Router4OLV2
    from phnet_amd.stream import LaneStream
    import inspect
    for mod in (Router4OL, Router4OLV2):
        assert callable(mod.RouterOL.infer_points_device) and callable(mod.RouterOL.polylines_from_device)
        assert inspect.signature(mod.RouterOL.open_stream).parameters["polylines"].default is False
    assert Router4OLV2.RouterV2.points_device is Router4OL.DetNetV2.points_device
    assert inspect.signature(LaneStream.__init__).parameters["polylines"].default is False and callable(LaneStream.lanes_fast)
    assert inspect.signature(GraphedInference.__init__).parameters["polylines"].default is False
    kept, num = C.random_frames(2, 4, C.S_MAIN, seed=1)
    with pytest.raises(RuntimeError):
        K.lane_points(kept, num, C.head(C.S_MAIN).prior_ys)


def test_hip_ops_has_its_module_docstring():
    from phnet_amd import hip_ops as K
    assert K.__doc__ and K.__doc__.startswith("Tensor-level wrappers over the C-ABI")
