"""Line clipping in the training targets, the part that needs no GPU: the restatement of tests/clip_cases.py - each hand case reaches
the branch of rule 0c it is for, the random lanes under random 'basic' affines against an INDEPENDENT per-segment parametric clip
(Liang-Barsky on the closed rectangle, written here, sharing no code with the restatement), the guard that keeps every predicate of the
random cases away from a last-bit difference - and the argument validation of phnet_lane_targets_clip, the host side, and the
resources the compiler gives the kernel of csrc/lane_targets.hip now that it holds rule 0c."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd import build as hip_build
from tests import augment_cases as AC
from tests import clip_cases as CC
from tests import target_cases as C

ERR_ARG = -1
NAMES = [g[0] for g in C.GEOMETRIES]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


def _default(row):
    return row[0] == 1 and row[1] == 0 and (row[2:] == C.INVALID).all()


def _runs(name, case_name):
    """[[run dicts] per lane] of a hand case (identity map)."""
    g = C.geometry(name)
    c = CC.case(name, case_name)[0]
    return [CC.clip_runs(CC.mapped_lane(lane, (0, list(CC.IDENTITY)), g["img_w"]), g["img_h"], g["img_w"]) for lane in c["lanes"]]


# ---------------------------------------------------------------------------------------------------------------- the census
@pytest.mark.parametrize("name", NAMES)
def test_hand_cases_hit_every_branch(name):
    """What each hand case is for happens in it, by the restatement alone - so equality on the GPU is not vacuous."""
    g = C.geometry(name)
    H, W, S, R = g["img_h"], g["img_w"], g["S"], g["R"]
    Wc, Hc = CC.rect(H, W)
    assert (Wc, Hc) == (W - 1e-3, H - 1e-3)
    plain = lambda lanes: C.encode_frame(lanes, H, W, S, R)[0]                        # noqa: E731

    c, lab, inf, n = CC.case(name, "all_in")
    assert n == 2 and [len(r) for r in _runs(name, "all_in")] == [1, 1] and np.array_equal(lab, plain(c["lanes"]))
    c, lab, inf, n = CC.case(name, "all_out")
    assert n == 1 and _runs(name, "all_out")[0] == [] and len(c["lanes"][0]) > 2
    assert np.array_equal(lab, plain(c["lanes"][1:])) and not np.array_equal(lab, plain(c["lanes"]))       # the lane outside took row 0

    c, lab, inf, n = CC.case(name, "four_edges")
    runs = [r[0] for r in _runs(name, "four_edges")]
    assert n == 4 and all(len(r) == 1 for r in _runs(name, "four_edges")) and lab[:, 1].tolist() == [1, 1, 1, 1]
    left, right, top, bottom = runs
    assert left["E"] is None and left["X"][0] == 0.0 and 0.0 < left["X"][1] < Hc
    assert right["E"] is None and right["X"][0] == Wc and 0.0 < right["X"][1] < Hc
    assert top["E"] is None and top["X"][1] == 0.0 and 0.0 < top["X"][0] < Wc
    assert bottom["X"] is None and bottom["a"] > 0 and bottom["E"][1] == Hc and 0.0 < bottom["E"][0] < Wc and bottom["points"][0] == bottom["E"]

    c, lab, inf, n = CC.case(name, "corner_tie")
    (run,) = _runs(name, "corner_tie")[0]
    assert CC.crossing((8.0, 8.0), (-8.0, -8.0), Wc, Hc) == ((0.0, 0.0), True, (True, True))                 # both coordinates gave t
    assert run["X"] == (0.0, 0.0) and len(run["points"]) == 4 and n == 1 and lab[0, 1] == 1

    c, lab, inf, n = CC.case(name, "out_and_back")
    first, second = _runs(name, "out_and_back")
    assert len(first) == 2 and n == 3 and lab[:, 1].tolist() == [1, 1, 1, 0]
    assert first[0]["E"] is None and first[0]["X"][0] == Wc and first[1]["E"][0] == Wc and first[1]["X"] is None
    unclipped = plain(c["lanes"])
    assert unclipped[:, 1].tolist() == [1, 1, 0, 0] and np.array_equal(lab[2], unclipped[1])                 # the later lane moved down a row

    c, lab, inf, n = CC.case(name, "single_in_point")
    (run,) = _runs(name, "single_in_point")[0]
    assert (run["a"], run["b"]) == (1, 1) and run["E"] and run["X"] and len(run["points"]) == 3 and n == 1 and len(inf) == 1

    c, lab, inf, n = CC.case(name, "run_of_one_at_start")
    (run,) = _runs(name, "run_of_one_at_start")[0]
    assert (run["a"], run["b"]) == (0, 0) and run["E"] is None and run["X"] and len(run["points"]) == 2
    assert n == 1 and np.array_equal(lab, plain(c["lanes"][1:]))                                             # two points: dropped by rule 1

    c, lab, inf, n = CC.case(name, "both_out_across")
    assert _runs(name, "both_out_across") == [[]] and n == 0 and all(_default(r) for r in lab)
    assert _segment_clip(c["lanes"][0][0], c["lanes"][0][1], Wc, Hc) is not None                             # it does cross the image

    c, lab, inf, n = CC.case(name, "border_t0")
    (r0,), (r1,) = _runs(name, "border_t0")
    for run, lane, k in ((r0, c["lanes"][0], 0), (r1, c["lanes"][1], 1)):
        q, o = lane[2], lane[3]
        pt, kept, _ = CC.crossing(q, o, Wc, Hc)
        assert q[k] == 0.0 and o[k] < 0.0 and pt == q and not kept                                           # t = 0: the crossing is q
        assert (run["a"], run["b"]) == (0, 2) and run["X"] is None and len(run["points"]) == 3
    assert n == 2 and lab[:, 1].tolist() == [1, 1, 0, 0]

    c, lab, inf, n = CC.case(name, "nonfinite")
    (run,) = _runs(name, "nonfinite")[0]
    assert len(run["points"]) == len(c["lanes"][0]) and run["points"][0][0] < 0                              # not clipped: its outside point stays
    assert n == 2 and inf[0]["status"] == "nonfinite" and _default(lab[0]) and lab[1, 1] == 1

    c, lab, inf, n = CC.case(name, "more_than_R")
    (runs,) = _runs(name, "more_than_R")
    assert len(runs) == 6 == n > R and all(len(r["points"]) == 4 and r["b"] - r["a"] == 1 for r in runs) and lab[:, 1].tolist() == [1] * R


def test_the_long_lane_crosses_the_ballots():
    """Runs of the 254-point lane start in one group of 64 points and end in the next; its samples keep their distance."""
    lanes, (lab, inf, n) = CC.long_case()
    runs = CC.clip_runs(CC.mapped_lane(lanes[0], (0, list(CC.IDENTITY)), 800), 320, 800)
    assert len(lanes[0]) == CC.LONG["pmax"] == 254 and len(runs) == 6 and n == 7
    assert sum(r["a"] // 64 != r["b"] // 64 for r in runs) >= 2 and any(r["a"] >= 192 for r in runs)
    assert lab[:, 1].tolist() == [0, 1, 1, 1, 1, 1, 1, 0] and inf[0]["status"] == "no_row"                   # 6 points above the first row
    far, gap, edge = CC.guard(lanes[0], (0, list(CC.IDENTITY)), 320, 800, C.offsets(320, 36))
    assert far >= CC.MARGIN and gap >= CC.MIN_DY and edge >= C.MARGIN_X


# ------------------------------------------------------------------------------------------- against an independent clip
def _segment_clip(p, q, Wc, Hc):
    """Liang-Barsky: the parameter interval (t0, t1) of p + t (q - p), 0 <= t <= 1, inside 0 <= x <= Wc, 0 <= y <= Hc, or None."""
    t0, t1 = 0.0, 1.0
    for d, lo, hi, s in ((q[0] - p[0], 0.0, Wc, p[0]), (q[1] - p[1], 0.0, Hc, p[1])):
        if d == 0.0:
            if s < lo or s > hi:
                return None
            continue
        ta, tb = (lo - s) / d, (hi - s) / d
        if ta > tb:
            ta, tb = tb, ta
        t0, t1 = max(t0, ta), min(t1, tb)
        if t0 > t1:
            return None
    return t0, t1


def _random_lanes():
    for name in NAMES:
        g = C.geometry(name)
        ys = C.offsets(g["img_h"], g["S"])
        for c, row in zip(CC.cases(name), CC.table_rows(name)):
            if c.get("random"):
                for lane in c["lanes"]:
                    yield name, g, ys, c, row, lane


def test_random_lanes_keep_their_distance():
    """The guard, before anything is compared: every mapped point of a random lane is >= 1e-3 px from each bound of the rectangle (so
    `in` cannot flip and no crossing has t = 0), adjacent points of a surviving fragment are >= 0.25 px apart in y, and every sampled x
    is >= 1e-3 px from 0 and img_w (target_cases.MARGIN_X, the existing distance) - by the restatement."""
    lanes = affine = 0
    for name, g, ys, c, row, lane in _random_lanes():
        far, gap, edge = CC.guard(lane, row, g["img_h"], g["img_w"], ys)
        assert far >= CC.MARGIN == 1e-3 and gap >= CC.MIN_DY and edge >= C.MARGIN_X == 1e-3, (name, c["name"], far, gap, edge)
        lanes += 1
        affine += row[1] != list(CC.IDENTITY)
    assert lanes >= 100 and affine >= 70


def test_random_lanes_against_the_independent_clip():
    test_random_lanes_keep_their_distance()
    crossings = multi = dropped_short = across = 0
    worst = 0.0
    for name, g, ys, c, row, lane in _random_lanes():
        H, W = g["img_h"], g["img_w"]
        Wc, Hc = CC.rect(H, W)
        pts = CC.mapped_lane(lane, row, W)
        runs = CC.clip_runs(pts, H, W)
        assert CC.clip_lane(pts, H, W) == [r["points"] for r in runs]
        inside = [CC.is_in(p, Wc, Hc) for p in pts]
        originals = []
        for r in runs:
            assert all(CC.is_in(p, Wc, Hc) for p in r["points"]), (name, c["name"])                          # every emitted point is in
            assert all(inside[r["a"]:r["b"] + 1]) and (r["a"] == 0 or not inside[r["a"] - 1]) and (r["b"] == len(pts) - 1 or not inside[r["b"] + 1])
            originals += pts[r["a"]:r["b"] + 1]
            assert (r["E"] is not None) == (r["a"] > 0) and (r["X"] is not None) == (r["b"] < len(pts) - 1)   # the guard: none is dropped
            for cr, q, o in ((r["E"], pts[r["a"]], pts[r["a"] - 1] if r["a"] > 0 else None),
                             (r["X"], pts[r["b"]], pts[r["b"] + 1] if r["b"] < len(pts) - 1 else None)):
                if cr is None:
                    continue
                t0, t1 = _segment_clip(q, o, Wc, Hc)                                                         # q is in: t0 = 0
                want = (q[0] + t1 * (o[0] - q[0]), q[1] + t1 * (o[1] - q[1]))
                err = math.hypot(cr[0] - want[0], cr[1] - want[1])
                worst = max(worst, err)
                assert t0 == 0.0 and 0.0 < t1 < 1.0 and err <= 1e-9, (name, c["name"], err)
                assert cr[0] in (0.0, Wc) or cr[1] in (0.0, Hc)                                              # exactly on a bound
                assert min(q[0], o[0]) <= cr[0] <= max(q[0], o[0]) and min(q[1], o[1]) <= cr[1] <= max(q[1], o[1])     # on its segment
                crossings += 1
            dropped_short += len(r["points"]) <= 2
        assert originals == [p for p, k in zip(pts, inside) if k]                                            # the in-points, in order
        multi += len(runs) > 1
        across += sum(not a and not b and _segment_clip(p, q, Wc, Hc) is not None for a, b, p, q in zip(inside[:-1], inside[1:], pts[:-1], pts[1:]))
    print("crossings", crossings, "lanes with several runs", multi, "fragments of <= 2 points", dropped_short, "both-out segments across", across,
          "worst distance to the independent clip", worst)
    assert crossings >= 100 and multi >= 10 and dropped_short >= 5


@pytest.mark.parametrize("name", NAMES)
def test_a_frame_with_nothing_outside_encodes_unchanged(name):
    """The anchor: where no mapped point leaves the rectangle, clipping on and off give the same rows, and both are what
    augment_cases.encode_frame_aug (and, under the identity, target_cases.encode_frame) gives."""
    g = C.geometry(name)
    H, W, S, R = g["img_h"], g["img_w"], g["S"], g["R"]
    Wc, Hc = CC.rect(H, W)
    seen = 0
    for c, row, (lab, _, n), (lab_off, _, n_off) in zip(CC.cases(name), CC.table_rows(name), CC.expected(name), CC.expected(name, clip=False)):
        want = AC.encode_frame_aug(c["lanes"], H, W, S, R, row[0], row[1])[0]
        assert np.array_equal(lab_off, want) and n_off == sum(len(lane) > 2 for lane in c["lanes"]), c["name"]
        if all(CC.is_in(p, Wc, Hc) for lane in c["lanes"] for p in CC.mapped_lane(lane, row, W)):
            assert np.array_equal(lab, want) and n == n_off, c["name"]
            if c["spec"] == {}:
                assert np.array_equal(lab, C.encode_frame(c["lanes"], H, W, S, R)[0])
            seen += 1
        elif c.get("random") and any(len(f) > 2 for lane in c["lanes"] for f in CC.clip_lane(CC.mapped_lane(lane, row, W), H, W)):
            assert not np.array_equal(lab, want), c["name"]                                                  # and elsewhere clipping matters
    assert seen >= 3


# ------------------------------------------------------------------------------------------------------------- the entry point
def test_lane_targets_clip_validates_without_a_gpu(built):
    """Each null pointer and each stated limit is PHNET_ERR_ARG before any launch (no device is touched).  Non-null pointers are
    made-up addresses - a call that got past the checks would try to launch."""
    lib = built
    p = 0x1000                                              # never dereferenced on the host

    def targets(ptrs=(p,) * 5, f=3, lin=8, pp=64, r=4, s=36, img_h=320.0, img_w=800.0, strip=320.0 / 35, crop=0.0, src_w=800.0, sx=1.0,
                sy=1.0, flip=0, flip2=None, fwd=None, clip=1, frag=None):
        return lib.phnet_lane_targets_clip(*ptrs, f, lin, pp, r, s, img_h, img_w, strip, crop, src_w, sx, sy, flip, flip2, fwd, clip, frag, None)

    for i in range(5):
        for clip in (0, 1):
            assert targets(tuple(None if j == i else p for j in range(5)), clip=clip, frag=p) == ERR_ARG, i
    for bad in (0, -1):
        for key in ("f", "lin", "pp", "r", "s"):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    assert targets(f=1 << 31) == ERR_ARG and targets(f=1 << 40) == ERR_ARG
    assert targets(lin=65) == ERR_ARG and targets(pp=1) == ERR_ARG and targets(pp=257) == ERR_ARG and targets(pp=257, clip=0) == ERR_ARG
    assert targets(r=65) == ERR_ARG and targets(s=1) == ERR_ARG and targets(s=257) == ERR_ARG
    for key in ("img_h", "img_w", "strip", "sx", "sy"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    for key in ("crop", "src_w"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    assert targets(flip=2) == ERR_ARG and targets(flip=-1) == ERR_ARG
    for bad in (2, -1, 256):
        assert targets(clip=bad) == ERR_ARG and targets(clip=bad, frag=p, flip2=p, fwd=p) == ERR_ARG, bad
    assert targets(pp=255, clip=1) == ERR_ARG and targets(pp=256, clip=1) == ERR_ARG                        # a fragment has up to P + 2 points

    from phnet_amd import hip_ops as K
    assert K.LANE_TARGETS_MAX_POINTS_CLIP == 254 and K.LANE_TARGETS_MAX_POINTS == 256
    names = {n: a for n, _, a in _lib.declared_functions(_lib.HEADER)}
    assert len(names["phnet_lane_targets_clip"]) == len(names["phnet_lane_targets_aug"]) + 2 == 23
    assert names["phnet_lane_targets_clip"][:20] == names["phnet_lane_targets_aug"][:20]
    assert len(names["phnet_lane_targets"]) == 19 and len(names["phnet_lane_targets_aug"]) == 21            # the old entries keep their signatures
    pts, cnt, num = (torch.from_numpy(a) for a in CC.packed("tiny"))
    with pytest.raises(RuntimeError):
        K.lane_targets_clip(pts, cnt, num, torch.from_numpy(C.offsets(64, 36)), 4, 64, 160, 64 / 35)


def test_the_header_carries_the_rule():
    header = " ".join(open(_lib.HEADER).read().replace(" * ", " ").split())
    for text in ("0c. (clip = 1) rectangle: Wc = img_w - 1e-3, Hc = img_h - 1e-3",
                 "a point is in iff 0 <= x <= Wc and 0 <= y <= Hc (false for NaN)",
                 "A lane with a non-finite mapped coordinate is not clipped",
                 "every maximal run of consecutive in-points p_a .. p_b gives one fragment [E] p_a .. p_b [X]",
                 "t_c = (bound - q_c) / (o_c - q_c)", "on a tie both: a corner", "A crossing equal to q in both coordinates is dropped",
                 "A segment with BOTH ends out is never clipped",
                 "fragments of more than 2 points survive and are numbered in order of (input lane, run)",
                 "with clip = 0 this is phnet_lane_targets_aug, bit for bit", "BEFORE the R cap", "2 <= P <= 254 with clip = 1"):
        assert text in header, text


def test_encoder_with_clip_refuses_to_run_without_a_gpu():
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
    enc = TargetEncoder(64, 160, 36, 4, device="cpu", clip=True)
    assert enc.clip and not TargetEncoder(64, 160, 36, 4, device="cpu").clip                                 # the default keeps today's output
    pre = ClipPreprocessor(320, 800, src_h=1000, src_w=1600, crop_size=200, device="cpu")
    assert TargetEncoder.for_preprocessor(pre, 36, 4, clip=True).clip and not TargetEncoder.for_preprocessor(pre, 36, 4).clip
    frames = [c["lanes"] for c in CC.cases("tiny")]
    pts, cnt, num = pack_annotations(frames, CC.LIN, CC.PMAX, clip=True)
    a, b, c = CC.packed("tiny")
    assert np.array_equal(pts.numpy(), a, equal_nan=True) and np.array_equal(cnt.numpy(), b) and np.array_equal(num.numpy(), c)
    with pytest.raises(RuntimeError):
        enc(pts.clone(), cnt.clone(), num.clone())
    with pytest.raises(RuntimeError):
        enc(pts.clone(), cnt.clone(), num.clone(), clip=False, frag_count=torch.zeros(len(frames), dtype=torch.int32))
    with pytest.raises(ValueError):
        pack_annotations(frames, CC.LIN, 255, clip=True)
    assert tuple(pack_annotations(frames, CC.LIN, 254, clip=True)[0].shape) == (len(frames), CC.LIN, 254, 2)
    assert tuple(pack_annotations(frames, CC.LIN, 256)[0].shape) == (len(frames), CC.LIN, 256, 2)           # without clip: as before


def test_lane_targets_kernel_with_rule_0c_compiles_without_scratch_or_spills(tmp_path):
    """Rule 0c lives inside the one kernel of csrc/lane_targets.hip (no new kernel, no new file): that kernel still takes no scratch
    and spills no register, and the file exports the new entry."""
    src = os.path.join(hip_build.CSRC, "lane_targets.hip")
    assert "phnet_lane_targets_clip" in open(src).read() and not os.path.exists(os.path.join(hip_build.CSRC, "lane_clip.hip"))
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "lane_targets.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == 1 and "lane_targets_kernel" in names[0], names
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", out.stderr)]
        assert len(vals) == 1 and not any(vals), (key, vals)
    print("VGPRs:", re.findall(r" VGPRs: (\d+)", out.stderr), "occupancy:", re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr))
