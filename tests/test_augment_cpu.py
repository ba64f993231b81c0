"""Training augmentation, the part that needs no GPU: the restatement of tests/augment_cases.py reaches every branch of the rules, the
host side (affine_matrices, AugmentParams, AugmentSampler) does what it states, both entry points are declared and refuse bad arguments
before any launch, and the compiler gives the image kernel no scratch."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd import build as hip_build
from phnet_amd.libs.dataset.openlane import augment as A
from tests import augment_cases as AC
from tests import target_cases as C

ERR_ARG = -1


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


def _mat(m):
    return np.vstack([np.asarray(m, np.float64).reshape(2, 3), [0.0, 0.0, 1.0]])


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_reaches_every_branch():
    """What each parameter set is for happens in it, by the restatement alone - so equality on the GPU is not vacuous."""
    for shape, (T, H, W) in AC.SHAPES.items():
        src = AC.frames(shape)
        px = T * H * W
        out, info = AC.expected(shape, "identity")
        assert np.array_equal(out, src) and info["one_tap"] == px and info["many_taps"] == 0 and info["guard_fill"] == 0
        for name in ("perm_201", "perm_021"):
            out, info = AC.expected(shape, name)
            perm = list(AC.PARAM_SETS[name]["perm"])
            assert np.array_equal(out, src[..., perm]) and info["perm"] == px and not np.array_equal(out, src)
        for name in ("bright_lo", "bright_hi"):
            out, info = AC.expected(shape, name)
            assert info["bright_black"] > 0 and info["bright_scaled"] > 0 and info["bright_clamped"] > 0, (shape, name, info)
            assert np.abs(out.astype(int).max(axis=3) - src.astype(int).max(axis=3)).max() <= 36          # 0.1 * 255 + 10, rounded
        lo, hi = AC.expected(shape, "bright_lo")[0], AC.expected(shape, "bright_hi")[0]
        assert (lo[src.max(axis=3) == 0] == 0).all() and (hi[src.max(axis=3) == 0] == 10).all()            # black: grey V'
        for name in ("huesat_lo", "huesat_hi"):
            out, info = AC.expected(shape, name)
            assert info["hsv_grey"] > 0 and info["hsv_black"] > 0 and info["hsv_max"] == {"r", "g", "b"}, (shape, name)
            assert info["hsv_sextants"] == set(range(6)) and info["hsv_sat_clamped"] > 0 and info["hsv_wrapped"] > 0, (shape, name, info)
            assert np.array_equal(out.max(axis=3), src.max(axis=3))                                          # V is kept
            assert (out[src.max(axis=3) == 0] == 0).all()                                                    # black stays black
        out, info = AC.expected(shape, "flip2")
        assert np.array_equal(out, src[:, :, ::-1]) and info["flipped_frames"] == T
        out, info = AC.expected(shape, "rot180")
        assert np.array_equal(out, src[:, ::-1, ::-1]) and info["one_tap"] == px
        for name in ("affine_pos", "affine_neg", "affine_basic_lo", "affine_basic_hi"):
            out, info = AC.expected(shape, name)
            assert info["many_taps"] > px // 2 and info["taps_outside"] > 0 and info["pixels_all_outside"] > 0, (shape, name, info)
        for name in ("affine_pos", "affine_neg"):                                                           # fill on two sides
            out = AC.expected(shape, name)[0]
            assert (out[:, -1, :] == 0).all() and (out[:, :, 0] == 0).all() and out[:, H // 2, W // 2].any(), (shape, name)
        out, info = AC.expected(shape, "translate_full")
        assert not out.any() and info["one_tap"] == 0 and info["many_taps"] == 0 and info["guard_fill"] + info["pixels_all_outside"] == px
        assert np.array_equal(AC.expected(shape, "drop_p0")[0], src)
        out, info = AC.expected(shape, "drop_pixel")
        dropped = (out == 0).all(axis=3) & (src != 0).any(axis=3)
        assert info["drop_elems"] == 3 * px and abs(dropped.mean() - 0.05) < 4 * np.sqrt(0.05 * 0.95 / px) + 1e-3, (shape, dropped.mean())
        assert np.array_equal(out[~dropped], src[~dropped])
        out, info = AC.expected(shape, "drop_pixel_per_channel")
        zeroed = (out == 0) & (src != 0)
        assert abs(zeroed.mean() - 0.05) < 4 * np.sqrt(0.05 * 0.95 / (3 * px)) + 1e-3 and (zeroed.sum(axis=3) == 1).any()
        assert not (zeroed.sum(axis=3) == 3).all()
        out, info = AC.expected(shape, "drop_coarse")
        gone = (out == 0).all(axis=3)[0] | (src[0] == 0).all(axis=2)
        cells = [[gone[(np.arange(H) * 3) // H == a][:, (np.arange(W) * 5) // W == b] for b in range(5)] for a in range(3)]
        state = [bool(c.all()) for r in cells for c in r]
        assert 0 < sum(state) < 15 and all(c.all() or not (c & ~((src[0] == 0).all(axis=2)[(np.arange(H) * 3) // H == a][:, (np.arange(W) * 5) // W == b])).any()
                                           for a, r in enumerate(cells) for b, c in enumerate(r))
        out, info = AC.expected(shape, "everything")
        assert info["many_taps"] > 0 and info["dropped"] > 0 and info["perm"] > 0 and info["bright_scaled"] > 0 and info["hsv_sextants"]
        if T > 1:
            assert info["flipped_frames"] == 2


def test_rot90_is_the_index_permutation():
    """A clockwise quarter turn about the centre: every tap weight is 0 or 1024, so the result is a pure rearrangement of pixels, the
    part of the source that lands outside is fill.  out[y, x] = src[cy - (x - cx), cx + (y - cy)]."""
    for shape, (T, H, W) in AC.SHAPES.items():
        src = AC.frames(shape)
        out, info = AC.expected(shape, "rot90")
        assert info["many_taps"] == 0
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        want = np.zeros_like(src)
        for y in range(H):
            for x in range(W):
                sx, sy = cx + (y - cy), cy - (x - cx)
                assert sx == int(sx) and sy == int(sy)
                if 0 <= sx < W and 0 <= sy < H:
                    want[:, y, x] = src[:, int(sy), int(sx)]
        assert np.array_equal(out, want) and want.any()
    # the convention itself: +90 degrees takes the point to the right of the centre to the point below it (clockwise, y down)
    fwd, _ = A.affine_matrices(37, 53, 90.0)
    assert np.allclose(_mat(fwd) @ [26.0 + 5.0, 18.0, 1.0], [26.0, 18.0 + 5.0, 1.0], atol=1e-12)


def test_identity_params_are_neutral():
    p = A.AugmentParams.identity(4)
    assert len(p) == 4 and p.flip2.dtype == torch.int32 and p.inv.dtype == torch.float64 and tuple(p.table.shape) == (4, A.COLS)
    n = p.numpy()
    assert not n["flip2"].any() and (n["inv"] == [1, 0, 0, 0, 1, 0]).all() and (n["fwd"] == n["inv"]).all()
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (4, 9, 13, 3), dtype=np.uint8)
    out, info = AC.augment(img, n["flip2"], n["inv"], n["table"])
    assert np.array_equal(out, img) and info["one_tap"] == img.size // 3 and info["perm"] == info["dropped"] == info["bright_scaled"] == 0
    # neutral parameters skip each op: a table that only SAYS neutral equals identity, whatever the unused columns hold
    t2 = n["table"].copy()
    t2[:, 13:] = 12345; t2[:, A.THRESH] = -1; t2[:, A.SEED_LO] = 99
    assert np.array_equal(AC.augment(img, n["flip2"], n["inv"], t2)[0], img)
    with pytest.raises(ValueError):
        A.AugmentParams.identity(3).copy_into(p)
    q = A.AugmentParams.build([dict(flip=True, value=3)] * 4, 9, 13)
    assert q.copy_into(p, non_blocking=False) is p and p.flip2.tolist() == [1] * 4 and p.table[:, A.VALUE].tolist() == [3] * 4
    assert p.to("cpu").flip2.tolist() == [1] * 4


# ------------------------------------------------------------------------------------------------------------- the host side
def test_affine_matrices_invert_each_other():
    rng = np.random.default_rng(5)
    for h, w in ((64, 160), (37, 53), (320, 800)):
        for _ in range(50):
            fwd, inv = A.affine_matrices(h, w, rng.uniform(-180, 180), rng.uniform(0.5, 2.0), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5))
            assert fwd.dtype == inv.dtype == np.float64 and fwd.shape == inv.shape == (6,)
            assert np.abs(_mat(fwd) @ _mat(inv) - np.eye(3)).max() <= 1e-12
    fwd, inv = A.affine_matrices(64, 160, 0.0, 1.0, 0.1, -0.25)                                      # translations are fractions of W, H
    assert np.array_equal(fwd, [1, 0, 16, 0, 1, -16]) and np.array_equal(inv, [1, 0, -16, 0, 1, 16])
    fwd, _ = A.affine_matrices(64, 160, 0.0, 2.0)                                                    # scale about the centre (79.5, 31.5)
    assert np.allclose(_mat(fwd) @ [79.5, 31.5, 1], [79.5, 31.5, 1]) and np.allclose(_mat(fwd) @ [80.5, 31.5, 1], [81.5, 31.5, 1])
    for bad in (dict(scale=0.0), dict(scale=-1.0), dict(rotate_deg=float("nan")), dict(translate_x=float("inf"))):
        with pytest.raises(ValueError):
            A.affine_matrices(64, 160, **bad)


def test_fwd_times_inv_is_the_identity_for_every_case():
    for shape in AC.SHAPES:
        for name in AC.PARAM_SETS:
            p = AC.params(shape, name).numpy()
            for f, i in zip(p["fwd"], p["inv"]):
                assert np.abs(_mat(f) @ _mat(i) - np.eye(3)).max() <= 1e-12, (shape, name)


def test_builder_validates():
    ok = dict(perm=(2, 1, 0), mul=1.0, add=3, value=-4, dropout=dict(mode="coarse", p=0.1, per_channel=True, seed=2 ** 64 - 1, grid=(3, 5)))
    p = A.AugmentParams.build([ok], 64, 160).numpy()
    row = AC._row(p["table"][0])
    assert row == dict(perm=[2, 1, 0], mq=256, add=3, value=-4, mode=2, per_channel=True, thresh=A.dropout_threshold(0.1), gh=3, gw=5,
                       seed=2 ** 64 - 1)
    assert (A.dropout_threshold(0.0), A.dropout_threshold(1.0), A.dropout_threshold(0.5)) == (0, 2 ** 32 - 1, 2 ** 31)
    bad = [dict(perm=(0, 0, 1)), dict(perm=(0, 1, 3)), dict(perm=(0, 1)), dict(mul=-0.1), dict(mul=300.0), dict(add=0.5), dict(add=256),
           dict(value=-256), dict(value=1.5), dict(nonsense=1), dict(scale=0.0),
           dict(dropout=dict(mode="coarse", p=0.1)), dict(dropout=dict(mode="coarse", p=0.1, grid=(0, 5))),
           dict(dropout=dict(mode="coarse", p=0.1, grid=(3, 40000))), dict(dropout=dict(mode="blur", p=0.1)),
           dict(dropout=dict(mode="pixel", p=1.5)), dict(dropout=dict(mode="pixel", p=0.1, seed=-1)),
           dict(dropout=dict(mode="pixel", p=0.1, seed=2 ** 64)), dict(dropout=dict(mode="pixel", p=0.1, colour=3))]
    for d in bad:
        with pytest.raises(ValueError):
            A.AugmentParams.build([d], 64, 160)
    z = torch.zeros
    for args in ((z(3, dtype=torch.int64), z(3, 6, dtype=torch.float64), z(3, 6, dtype=torch.float64), z(3, 16, dtype=torch.int32)),
                 (z(3, dtype=torch.int32), z(3, 6), z(3, 6, dtype=torch.float64), z(3, 16, dtype=torch.int32)),
                 (z(3, dtype=torch.int32), z(2, 6, dtype=torch.float64), z(3, 6, dtype=torch.float64), z(3, 16, dtype=torch.int32)),
                 (z(3, dtype=torch.int32), z(3, 6, dtype=torch.float64), z(3, 6, dtype=torch.float64), z(3, 12, dtype=torch.int32))):
        with pytest.raises(ValueError):
            A.AugmentParams(*args)
    with pytest.raises(ValueError):
        A.AugmentSampler("heavy", 64, 160, 0)
    with pytest.raises(ValueError):
        A.AugmentSampler("basic", 64, 160, 0, per="video")
    with pytest.raises(ValueError):
        A.ClipAugmenter(64, 160, std=(0.2, 0.0, 0.2), device="cpu")
    with pytest.raises(ValueError):
        A.ClipAugmenter(64, 40000, device="cpu")


def test_python_side_refuses_wrong_shapes_and_the_cpu():
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
    aug = A.ClipAugmenter.for_preprocessor(ClipPreprocessor(64, 160, src_h=100, src_w=200, crop_size=10, device="cpu"))
    assert (aug.out_h, aug.out_w, aug.device) == (64, 160, torch.device("cpu"))
    assert [round(v, 6) for v in aug._mean] == [0.485, 0.456, 0.406] and [round(v, 6) for v in aug._std] == [0.229, 0.224, 0.225]
    frames = torch.zeros((3, 64, 160, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        aug(frames[:, :32], A.AugmentParams.identity(3))
    with pytest.raises(ValueError):
        aug(frames, A.AugmentParams.identity(2))
    with pytest.raises(RuntimeError):
        aug(frames, A.AugmentParams.identity(3))                                     # no CPU path
    enc = TargetEncoder(64, 160, 36, 4, src_h=64, src_w=160, crop_size=0, device="cpu")
    packed = [t.clone() for t in pack_annotations(AC.label_frames(), C.LIN, 16)]
    with pytest.raises(RuntimeError):
        enc(*packed, augment=A.AugmentParams.identity(3))


# ---------------------------------------------------------------------------------------------------------------- the sampler
def test_sampler_is_deterministic_per_seed():
    a = A.AugmentSampler("complex", 320, 800, seed=7).sample(64).numpy()
    b = A.AugmentSampler("complex", 320, 800, seed=7).sample(64).numpy()
    c = A.AugmentSampler("complex", 320, 800, seed=8).sample(64).numpy()
    assert all(np.array_equal(a[k], b[k]) for k in a) and any(not np.array_equal(a[k], c[k]) for k in a)


def test_per_clip_repeats_one_draw_and_per_frame_does_not():
    T = 16
    clip = A.AugmentSampler("basic", 320, 800, seed=3, per="clip")
    for _ in range(4):
        p = clip.sample(T).numpy()
        assert all((p[k] == p[k][:1]).all() for k in p)
    assert any(not np.array_equal(clip.sample(T).numpy()["fwd"], clip.sample(T).numpy()["fwd"]) for _ in range(4))      # clips differ
    frame = A.AugmentSampler("basic", 320, 800, seed=3).sample(T).numpy()
    assert A.AugmentSampler("basic", 320, 800, seed=3).per == "frame"
    assert len({tuple(r) for r in frame["fwd"]}) > T // 2 and 0 < frame["flip2"].sum() < T


@pytest.mark.parametrize("mode", ["basic", "complex"])
def test_sampler_rates_and_ranges(mode):
    """20 000 draws: each op is on at its probability of transforms.py:190-249 within 4 standard errors, every parameter in its range."""
    N = 20000
    s = A.AugmentSampler(mode, 320, 800, seed=2024)
    draws = [s.draw() for _ in range(N)]
    r = A.RECIPES[mode]
    want = {"basic": dict(flip=0.5, affine=0.7), "complex": dict(flip=0.1, shuffle=0.1, brightness=0.1, hue_sat=0.1, dropout=0.1, affine=0.1)}[mode]
    for op in ("flip", "shuffle", "brightness", "hue_sat", "dropout", "affine"):
        rate, p = sum(op in d["ops"] for d in draws) / N, want.get(op, 0.0)
        assert r[op] == p and abs(rate - p) <= 4 * np.sqrt(p * (1 - p) / N), (op, rate, p)
    rot, (s_lo, s_hi) = {"basic": 10.0, "complex": 5.0}[mode], {"basic": (0.8, 1.2), "complex": (0.9, 1.1)}[mode]
    seen = set()
    for d in draws:
        assert set(d) - {"ops"} <= {"flip", "perm", "mul", "add", "value", "dropout", "rotate", "scale", "translate"}
        if "perm" in d:
            assert sorted(d["perm"]) == [0, 1, 2]
        if "mul" in d:
            assert 0.9 <= d["mul"] <= 1.1 and -10 <= d["add"] <= 10 and isinstance(d["add"], int)
            seen.add(("add", d["add"]))
        if "value" in d:
            assert -10 <= d["value"] <= 10 and isinstance(d["value"], int)
            seen.add(("value", d["value"]))
        if "dropout" in d:
            dr = d["dropout"]
            assert 0.0 <= dr["p"] <= 0.05 and 0 <= dr["seed"] < 2 ** 64 and dr["mode"] in ("pixel", "coarse")
            seen.add((dr["mode"], dr["per_channel"]))
            if dr["mode"] == "coarse":
                assert 3 <= dr["grid"][0] <= 80 and 16 <= dr["grid"][1] <= 200           # 2 % .. 25 % of 320 x 800, at least 3
        if "rotate" in d:
            assert -rot <= d["rotate"] <= rot and s_lo <= d["scale"] <= s_hi and all(-0.1 <= v <= 0.1 for v in d["translate"])
    if mode == "complex":
        assert {("add", -10), ("add", 10), ("value", -10), ("value", 10)} <= seen                          # both ends are reachable
        assert {("pixel", True), ("pixel", False), ("coarse", True), ("coarse", False)} <= seen
        kinds = [d["dropout"] for d in draws if "dropout" in d]
        pix = [k for k in kinds if k["mode"] == "pixel"]
        n = len(kinds)
        assert abs(len(pix) / n - 0.5) <= 4 * np.sqrt(0.25 / n)                                            # OneOf
        assert abs(np.mean([k["per_channel"] for k in pix]) - 0.5) <= 4 * np.sqrt(0.25 / len(pix))
        assert abs(np.mean([k["per_channel"] for k in kinds if k["mode"] == "coarse"]) - 0.2) <= 4 * np.sqrt(0.16 / (n - len(pix)))
    A.AugmentParams.build([{k: v for k, v in d.items() if k != "ops"} for d in draws[:500]], 320, 800)      # every draw is a valid frame


# --------------------------------------------------------------------------------------------------------------- the labels
def test_label_cases_keep_their_distance_and_reach_their_branches():
    """Precondition of the GPU comparison: under every label set each warped sample is >= 1e-3 px from 0 and img_w and adjacent warped
    points are >= 0.25 px apart in y, by the restatement - no last-bit difference can move a value across the image border."""
    g = C.geometry("tiny")
    lanes = [lane for frame in AC.label_frames() for lane in frame]
    assert len(lanes) == 9 and all(float(v) * 64 == int(float(v) * 64) for lane in lanes for p in lane for v in p)
    for lane in lanes:
        far, gap = AC.label_margins(lane, g["img_h"], g["img_w"], g["S"])
        assert far >= AC.LABEL_MARGIN and gap >= AC.LABEL_MIN_DY
    plain, _ = AC.expected_labels("identity")
    want = np.stack([C.encode_frame(f, g["img_h"], g["img_w"], g["S"], g["R"])[0] for f in AC.label_frames()])
    assert np.array_equal(plain, want) and plain[..., 1].sum() == 9                                         # rule 0b with the identity is nothing
    for name in AC.LABEL_SETS[1:]:
        lab, infos = AC.expected_labels(name)
        assert not np.array_equal(lab, plain), name
        if name == "translate_full":
            assert sum(i["status"] == "few_inside" for f in infos for i in f) >= 8 and lab[..., 1].sum() <= 1      # (nearly) all left the image
        else:
            assert lab[..., 1].sum() >= 6, (name, lab[..., 1].sum())
    assert any(i["n_out"] > 0 for n in ("affine_pos", "affine_basic_hi", "everything") for f in AC.expected_labels(n)[1] for i in f)
    # flip2 alone mirrors every x about (img_w - 1) / 2: the mirrored lanes through the plain restatement give the same rows
    mirrored = [[[(g["img_w"] - 1.0 - x, y) for x, y in lane] for lane in f] for f in AC.label_frames()]
    want = np.stack([C.encode_frame(f, g["img_h"], g["img_w"], g["S"], g["R"])[0] for f in mirrored])
    assert np.array_equal(AC.expected_labels("flip2")[0], want)
    # a half turn: (x, y) -> (W - 1 - x, H - 1 - y), up to the rounding of cos / sin
    turned = [[[(g["img_w"] - 1.0 - x, g["img_h"] - 1.0 - y) for x, y in lane] for lane in f] for f in AC.label_frames()]
    want = np.stack([C.encode_frame(f, g["img_h"], g["img_w"], g["S"], g["R"])[0] for f in turned])
    got = AC.expected_labels("rot180")[0]
    assert np.array_equal(got == C.INVALID, want == C.INVALID) and np.abs(got - want)[got != C.INVALID].max() < 1e-3


def test_blob_and_lane_agree_in_the_restatement():
    """The margin of the GPU test comes from here: the restatement's own centroid of the warped blob lies within 0.5 px of fwd applied
    to the annotated point, and the restatement's warped lane passes the centroid within 0.5 px."""
    g = C.geometry("tiny")
    for name in ("affine_pos", "affine_neg"):
        p = AC.params("tiny", name).numpy()
        out, _ = AC.augment(AC.blob_frames(), p["flip2"], p["inv"], p["table"])
        lab, _ = AC.encode_frame_aug([AC.BLOB_LANE], g["img_h"], g["img_w"], g["S"], g["R"], p["flip2"][0], p["fwd"][0])
        cx, cy = AC.centroid(out[0])
        wx, wy, _ = _mat(p["fwd"][0]) @ [AC.BLOB_XY[0], AC.BLOB_XY[1], 1.0]
        print(name, "centroid", (cx, cy), "fwd(point)", (wx, wy), "lane at centroid y", AC.lane_x_at(lab[0], cy, g["img_h"], g["S"]))
        assert np.hypot(cx - wx, cy - wy) <= AC.BLOB_BOUND
        assert lab[0, 1] == 1 and lab[0, 2] == 0 and abs(AC.lane_x_at(lab[0], cy, g["img_h"], g["S"]) - cx) <= AC.BLOB_BOUND
        # a transposed matrix or a wrong rotation sign would be far off: the other set's point is several pixels away
        other = AC.params("tiny", "affine_neg" if name == "affine_pos" else "affine_pos").numpy()
        ox, oy, _ = _mat(other["fwd"][0]) @ [AC.BLOB_XY[0], AC.BLOB_XY[1], 1.0]
        assert np.hypot(cx - ox, cy - oy) > 4 * AC.BLOB_BOUND


# ------------------------------------------------------------------------------------------------------------ the entry points
def test_both_symbols_are_declared_and_exported(built):
    names = {n: a for n, _, a in _lib.declared_functions(_lib.HEADER)}
    assert len(names["phnet_augment_u8"]) == 13 and len(names["phnet_lane_targets_aug"]) == 21 and len(names["phnet_lane_targets"]) == 19
    assert hasattr(built, "phnet_augment_u8") and hasattr(built, "phnet_lane_targets_aug")
    header = open(_lib.HEADER).read()
    for rule in ("U = floor(u * 32 + 0.5)", "0b. flip2[f] != 0", "(sum over the taps of weight * tap + 512) >> 10"):
        assert rule in header, rule


def test_augment_validates_without_a_gpu(built):
    """Each null pointer and each stated limit is PHNET_ERR_ARG before any launch (no device is touched: this runs on a machine
    without one).  Non-null device pointers are made-up addresses - a call that got past the checks would try to launch."""
    import ctypes
    lib = built
    p = 0x1000
    mean, std, zero = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2), (ctypes.c_float * 3)(0.2, 0.0, 0.2)
    host = lambda a: ctypes.cast(a, ctypes.c_void_p)                                  # noqa: E731

    def aug(ptrs=(p, p, None, p, p, p), T=3, H=64, W=160, layout=0, mean=host(mean), std=host(std)):
        return lib.phnet_augment_u8(*ptrs, T, H, W, layout, mean, std, None)

    for i in (0, 1, 3, 4, 5):
        assert aug(tuple(None if j == i else (p if j != 2 else None) for j in range(6))) == ERR_ARG, i
    assert aug(mean=None) == ERR_ARG and aug(std=None) == ERR_ARG and aug(std=host(zero)) == ERR_ARG
    assert aug(layout=2) == ERR_ARG and aug(layout=-1) == ERR_ARG
    assert aug(T=-1) == ERR_ARG and aug(H=0) == ERR_ARG and aug(W=0) == ERR_ARG and aug(H=32769) == ERR_ARG and aug(W=32769) == ERR_ARG
    assert aug(H=32768, W=32768) == ERR_ARG                                          # H W 4 >= 2^31
    assert aug(T=2 ** 31 - 1, H=1024, W=1024) == ERR_ARG                              # T ceil(H W / 256) >= 2^31
    assert aug(T=0) == 0 and aug((None,) * 6, T=0) == 0                               # a no-op, before the pointers are looked at


def test_lane_targets_aug_validates_without_a_gpu(built):
    lib = built
    p = 0x1000

    def targets(ptrs=(p,) * 5, f=3, lin=8, pp=64, r=4, s=36, img_h=320.0, img_w=800.0, strip=320.0 / 35, crop=0.0, src_w=800.0, sx=1.0,
                sy=1.0, flip=0, aug=(p, p)):
        return lib.phnet_lane_targets_aug(*ptrs, f, lin, pp, r, s, img_h, img_w, strip, crop, src_w, sx, sy, flip, *aug, None)

    for aug in ((p, p), (None, p), (p, None), (None, None)):                          # the two new arrays are optional; the rest is not
        for i in range(5):
            assert targets(tuple(None if j == i else p for j in range(5)), aug=aug) == ERR_ARG, (i, aug)
    for bad in (0, -1):
        for key in ("f", "lin", "pp", "r", "s"):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    assert targets(f=1 << 31) == ERR_ARG and targets(lin=65) == ERR_ARG and targets(pp=1) == ERR_ARG and targets(pp=257) == ERR_ARG
    assert targets(r=65) == ERR_ARG and targets(s=1) == ERR_ARG and targets(s=257) == ERR_ARG
    for key in ("img_h", "img_w", "strip", "sx", "sy"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    for key in ("crop", "src_w"):
        for bad in (float("nan"), float("inf")):
            assert targets(**{key: bad}) == ERR_ARG, (key, bad)
    assert targets(flip=2) == ERR_ARG and targets(flip=-1) == ERR_ARG


def test_augment_kernels_compile_without_scratch_or_spills(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/augment.hip: the two layouts of one kernel, no scratch, no spilled registers."""
    src = os.path.join(hip_build.CSRC, "augment.hip")
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "augment.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == 2 and all("augment_kernel" in n for n in names), names
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", out.stderr)]
        assert len(vals) == 2 and not any(vals), (key, vals)
    print("VGPRs:", re.findall(r" VGPRs: (\d+)", out.stderr), "occupancy:", re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr))
