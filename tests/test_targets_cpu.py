"""Training targets, the part that needs no GPU: the restatement of tests/target_cases.py against what the reference's own
transform_annotation gave (tests/golden/targets_tiny.json, written by tests/golden/make_goldens_targets.py), the census - each
hand case reaches the branch it is for, by the restatement alone - pack_annotations, the argument validation of
phnet_lane_targets (csrc/lane_targets.hip) and the resources the compiler gives its kernel.

Tolerance against the golden: flags, [2], [5] and the number and positions of -1e5 are exact; [3], [4] and the xs are within
1 float32 ulp - the explicit not-a-knot solve and FITPACK are two float64 evaluations of the same interpolant that agree to
well under 1e-6 px, so after the cast they can differ by one rounding at most (0 ulps are observed)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd import build as hip_build
from tests import target_cases as C

ERR_ARG = -1
ULPS_VS_GOLDEN = 1


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(C.GOLDEN))


# ------------------------------------------------------------------------------------------------------ against the reference
def test_random_lanes_keep_their_distance():
    """Precondition of every comparison: adjacent y of a random lane are >= 1 px apart and every sampled x is >= 1e-3 px from 0
    and img_w, by the restatement - no last-bit difference can move a value across the image border."""
    lanes = 0
    for name, H, W, S, R in C.GEOMETRIES:
        for c, (_, infos) in zip(C.cases(name), C.expected(name)):
            if not c.get("random"):
                continue
            for lane in c["lanes"]:
                ys = sorted(p[1] for p in lane)
                assert len(lane) > 2 and min(b - a for a, b in zip(ys[:-1], ys[1:])) >= C.MIN_DY, (name, c["name"])
            for info in infos:
                assert all(min(abs(x), abs(x - W)) >= C.MARGIN_X for x in info["sampled"]), (name, c["name"])
                lanes += 1
    assert lanes >= 40


def test_restatement_equals_the_reference(golden):
    test_random_lanes_keep_their_distance()
    rows = worst = 0
    for name, H, W, S, R in C.GEOMETRIES:
        g = golden["geometries"][name]
        assert g["head"] == dict(img_h=H, img_w=W, S=S, R=R, offsets_ys=g["head"]["offsets_ys"])
        assert np.array_equal(np.asarray(g["head"]["offsets_ys"]), C.offsets(H, S))
        pinned = [c for c in C.cases(name) if c["reference"]]
        assert [r["name"] for r in g["cases"]] == [c["name"] for c in pinned]
        for rec, c in zip(g["cases"], pinned):
            assert rec["lanes"] == [[[x, y] for x, y in lane] for lane in c["lanes"]], (name, c["name"])     # the fixture is current
            want = C.golden_label(rec, R, S)
            got = C.case(name, c["name"])[1]
            worst = max(worst, C.assert_rows_match(got, want, ULPS_VS_GOLDEN, (name, c["name"])))
            rows += int(want[:, 1].sum())
    print("valid rows compared:", rows, "worst ulps:", worst)
    assert rows >= 100
    assert np.arange(320, -1, -320 / 35)[-1] < 0                                  # the table's last entry is below 0


# ---------------------------------------------------------------------------------------------------------------- the census
def _main(name):
    c, label, infos = C.case("main", name)
    return c, label, infos


def _default(row):
    return row[0] == 1 and row[1] == 0 and (row[2:] == C.INVALID).all()


def test_hand_cases_hit_every_branch():
    """What each hand case is for happens in it, by the restatement alone - so equality on the GPU is not vacuous."""
    S, R, W = 36, 4, 800
    c, lab, inf = _main("counts_3_4_5_37")
    assert [i["n"] for i in inf] == [3, 4, 5, 37] and all(i["status"] == "valid" for i in inf) and all(i["n_ext"] > 0 for i in inf)
    c, lab, inf = _main("count_256")
    assert inf[0]["n"] == 256 == C.PMAX and inf[0]["status"] == "valid"
    c, lab, inf = _main("dup_linear_and_one_y")
    assert [len(l) for l in c["lanes"]] == [3, 3, 6] and [i["n"] for i in inf] == [2, 1, 6]
    assert [i["status"] for i in inf] == ["valid", "one_point", "valid"] and _default(lab[1]) and lab[2, 1] == 1        # row 1 is consumed
    xs = lab[0, 6:6 + inf[0]["n_in"]].astype(np.float64)
    assert np.abs(np.diff(xs, 2)).max() < 1e-4                                    # the line
    c, lab, inf = _main("two_point_lane_between")
    assert [len(l) for l in c["lanes"]] == [7, 2, 8] and len(inf) == 2 and lab[:, 1].tolist() == [1, 1, 0, 0]
    assert np.array_equal(lab[1], C.encode_frame([c["lanes"][2]], 320, W, S, R)[0][0])
    c, lab, inf = _main("five_long")
    assert len(c["lanes"]) == 5 and len(inf) == R and lab[:, 1].tolist() == [1, 1, 1, 1]
    c, lab, inf = _main("shuffled")
    assert sorted(c["lanes"][0]) == sorted(c["lanes"][1]) and c["lanes"][0] != c["lanes"][1] and np.array_equal(lab[0], lab[1]) and lab[0, 1] == 1
    c, lab, inf = _main("dup_first_wins")
    assert len(c["lanes"][0]) == 12 and inf[0]["n"] == 9 and np.array_equal(lab[0], lab[1]) and lab[0, 1] == 1
    c, lab, inf = _main("between_rows")
    assert inf[0]["status"] == "no_row" and inf[0]["n_interp"] == 0 and _default(lab[0]) and lab[1, 1] == 1
    c, lab, inf = _main("top_at_zero")
    assert min(p[1] for p in c["lanes"][0]) == 0.0 and inf[0]["n_ext"] + inf[0]["n_interp"] == S - 1 and lab[0, 6 + S - 1] == C.INVALID
    c, lab, inf = _main("bottom_exit")
    assert all(0 < i["n_out"] <= i["n_ext"] and not i["reordered"] and i["status"] == "valid" for i in inf)
    assert lab[0, 2] == np.float32(inf[0]["n_out"] / (S - 1)) and lab[0, 6] >= W and lab[1, 6] < 0
    c, lab, inf = _main("curves_out_top")
    assert all(i["reordered"] and i["n_out"] > 0 and i["status"] == "valid" for i in inf)
    assert lab[0, 6] < 0 and lab[1, 6] >= W and 0 <= lab[0, 6 + inf[0]["n_out"]] < W                          # outside values first
    c, lab, inf = _main("at_most_one_inside")
    assert [i["n_in"] for i in inf] == [1, 0] and all(i["status"] == "few_inside" for i in inf) and _default(lab[0]) and _default(lab[1])
    c, lab, inf = _main("x_zero")
    assert inf[0]["status"] == "valid" and inf[0]["n_out"] == 0 and (lab[0, 6:6 + inf[0]["n_in"]] == 0).all() and lab[0, 3] == 0
    for name in ("x_width", "x_width_cubic"):
        c, lab, inf = _main(name)
        assert inf[0]["n_in"] == 0 and inf[0]["n_out"] == 35 and all(x == W for x in inf[0]["sampled"]) and _default(lab[0])
    c, lab, inf = _main("lean_left")
    assert inf[0]["negative_thetas"] == inf[0]["n_in"] - 1 > 0 and 0.5 < lab[0, 4] < 1
    c, lab, inf = _main("vertical")
    assert len(set(inf[0]["sampled"])) == 1 and inf[0]["negative_thetas"] == 0 and abs(lab[0, 4] - 0.5) < 1e-6
    c, lab, inf = _main("no_lanes")
    assert c["lanes"] == [] and inf == [] and all(_default(r) for r in lab)
    c, lab, inf = _main("nonfinite")
    assert not c["reference"] and [i["status"] for i in inf] == ["valid", "nonfinite", "nonfinite", "valid"]
    assert lab[:, 1].tolist() == [1, 0, 0, 1] and _default(lab[1]) and _default(lab[2])


def test_map_restatement_is_the_stated_rule():
    """crop, flip and the two ratios, on a lane whose mapped points are easy to state."""
    mp = C.map_for(320, 800, 1120, 1600, 480, flip=True)                                    # both ratios are 0.5: exact
    assert mp["scale_x"] == 800.0 / 1600.0 == 0.5 and mp["scale_y"] == 320.0 / 640.0 == 0.5 and mp["crop"] == 480.0
    lane = [(1599.0 - 200.0 * k, 1120.0 - 100.0 * k) for k in range(5)]                    # flipped: x = 200 k; cropped: y = 640 - 100 k
    mapped = [(100.0 * k, 320.0 - 50.0 * k) for k in range(5)]
    a = C.encode_frame([lane], 320, 800, 36, 4, mapping=mp)[0]
    b = C.encode_frame([[(np.float32(x), np.float32(y)) for x, y in mapped]], 320, 800, 36, 4)[0]
    assert a[0, 1] == 1 and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------- the host side
def test_pack_annotations_shapes_and_errors():
    from phnet_amd.libs.dataset.openlane.targets import pack_annotations, sample_rows
    frames = [[[(1.0, 2.0), (3.0, 4.0), (5.0, 6.0)], np.array([[7.5, 8.5], [9.5, 10.5]])], [], [[]]]
    pts, cnt, num = pack_annotations(frames, 3, 4)
    assert tuple(pts.shape) == (3, 3, 4, 2) and pts.dtype == torch.float32
    assert tuple(cnt.shape) == (3, 3) and cnt.dtype == torch.int32 and tuple(num.shape) == (3,) and num.dtype == torch.int32
    assert num.tolist() == [2, 0, 1] and cnt.tolist() == [[3, 2, 0], [0, 0, 0], [0, 0, 0]]
    assert pts[0, 0, :3].tolist() == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]] and pts[0, 1, :2].tolist() == [[7.5, 8.5], [9.5, 10.5]]
    assert float(pts.abs().sum()) == sum(range(1, 7)) + 7.5 + 8.5 + 9.5 + 10.5          # everything else is zero
    with pytest.raises(ValueError):
        pack_annotations(frames, 1, 4)                                               # a frame with 2 lanes
    with pytest.raises(ValueError):
        pack_annotations(frames, 3, 2)                                               # a lane with 3 points
    for bad in ((0, 4), (65, 4), (3, 1), (3, 257)):
        with pytest.raises(ValueError):
            pack_annotations(frames, *bad)
    a, b, c = C.pack([c["lanes"] for c in C.cases("tiny")])
    p2, c2, n2 = pack_annotations([c["lanes"] for c in C.cases("tiny")], C.LIN, C.PMAX)
    assert np.array_equal(p2.numpy(), a) and np.array_equal(c2.numpy(), b) and np.array_equal(n2.numpy(), c)
    assert np.array_equal(sample_rows(320, 36), C.offsets(320, 36)) and sample_rows(384, 72).shape == (72,)
    with pytest.raises(ValueError):
        sample_rows(3, 9)                                                            # np.arange(3, -1, -3/8) has 11 entries


def test_encoder_refuses_to_run_without_a_gpu():
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
    enc = TargetEncoder(320, 800, 36, 4, device="cpu")
    assert enc.offsets_ys.dtype == torch.float64 and np.array_equal(enc.offsets_ys.numpy(), C.offsets(320, 36))
    assert (enc.scale_x, enc.scale_y, enc.strip_size) == (800.0 / 1920.0, 320.0 / 800.0, 320 / 35)
    same = TargetEncoder.for_preprocessor(ClipPreprocessor(320, 800, src_h=1000, src_w=1600, crop_size=200, device="cpu"), 36, 4)
    assert (same.src_h, same.src_w, same.crop, same.out_h, same.out_w) == (1000, 1600, 200, 320, 800)
    assert (same.scale_x, same.scale_y) == (800.0 / 1600.0, 320.0 / 800.0)
    with pytest.raises(RuntimeError):
        enc(*[t.clone() for t in pack_annotations([c["lanes"] for c in C.cases("tiny")], C.LIN, C.PMAX)])
    with pytest.raises(ValueError):
        TargetEncoder(3, 800, 9, 4, device="cpu")                                   # np.arange(3, -1, -3/8) has 11 entries
    with pytest.raises(ValueError):
        TargetEncoder(320, 800, 36, 65, device="cpu")


def test_lane_targets_validates_without_a_gpu(built):
    """Each null pointer and each stated limit is PHNET_ERR_ARG before any launch (no device is touched: this runs on a machine
    without one).  Non-null pointers are made-up addresses - a call that got past the checks would try to launch."""
    lib = built
    p = 0x1000                                              # never dereferenced on the host

    def targets(ptrs=(p,) * 5, f=3, lin=8, pp=64, r=4, s=36, img_h=320.0, img_w=800.0, strip=320.0 / 35, crop=0.0, src_w=800.0, sx=1.0,
                sy=1.0, flip=0):
        return lib.phnet_lane_targets(*ptrs, f, lin, pp, r, s, img_h, img_w, strip, crop, src_w, sx, sy, flip, None)

    for i in range(5):
        assert targets(tuple(None if j == i else p for j in range(5))) == ERR_ARG, i
    for bad in (0, -1):
        for key in ("f", "lin", "pp", "r", "s"):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    assert targets(f=1 << 31) == ERR_ARG and targets(f=1 << 40) == ERR_ARG
    assert targets(lin=65) == ERR_ARG and targets(pp=1) == ERR_ARG and targets(pp=257) == ERR_ARG
    assert targets(r=65) == ERR_ARG and targets(s=1) == ERR_ARG and targets(s=257) == ERR_ARG
    for key in ("img_h", "img_w", "strip", "sx", "sy"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    for key in ("crop", "src_w"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    assert targets(flip=2) == ERR_ARG and targets(flip=-1) == ERR_ARG
    from phnet_amd import hip_ops as K
    assert (K.LANE_TARGETS_MAX_IN_LANES, K.LANE_TARGETS_MAX_POINTS, K.LANE_TARGETS_MAX_ROWS, K.LANE_TARGETS_MAX_OFFSETS) == (64, 256, 64, 256)
    header = open(_lib.HEADER).read()
    assert "1 <= F < 2^31, 1 <= Lin <= 64, 2 <= P <= 256, 1 <= R <= 64, 2 <= S <= 256" in header
    names = {n: a for n, _, a in _lib.declared_functions(_lib.HEADER)}
    assert len(names["phnet_lane_targets"]) == 19
    pts, cnt, num = (torch.from_numpy(a) for a in C.pack([c["lanes"] for c in C.cases("tiny")]))
    with pytest.raises(RuntimeError):
        K.lane_targets(pts, cnt, num, torch.from_numpy(C.offsets(64, 36)), 4, 64, 160, 64 / 35)


def test_lane_targets_kernel_compiles_without_scratch_or_spills(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/lane_targets.hip: exactly one kernel, no scratch, no spilled registers."""
    src = os.path.join(hip_build.CSRC, "lane_targets.hip")
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "lane_targets.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len([n for n in names if "lane_targets" in n]) == 1 and len(names) == 1, names
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", out.stderr)]
        assert len(vals) == 1 and not any(vals), (key, vals)
    print("VGPRs:", dict(zip(names, re.findall(r" VGPRs: (\d+)", out.stderr))),
          "occupancy:", re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr))
