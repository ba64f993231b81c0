"""Pins the CPU oracle (oracle/phnet_cpu.py) to fixtures produced by the reference's own Python
(tests/golden/make_goldens.py).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import lane_nms as ONMS
from oracle import phnet_cpu as O
from tests import fixtures, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _lines_close(a, b, what=""):
    """Oracle vs reference lane tensors [...,6+S].  Both are fp32 PyTorch-CPU programs, so they agree to ~1e-6 where
    the arithmetic is well conditioned - but the reduction order of PyTorch's CPU kernels depends on the thread count
    of the machine, and the refinement cascade (re-sampling at predicted positions, 1/tan near its poles) amplifies
    that last-bit noise.  Criterion: >= 99 % of the entries within 1e-4 (relative to the row's scale for the x
    columns), none beyond 5e-3."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    head = np.abs(a[..., :6] - b[..., :6]) / (1.0 + np.abs(b[..., :6]))
    xs = np.abs(a[..., 6:] - b[..., 6:]) / (1.0 + np.abs(b[..., 6:]).max(axis=-1, keepdims=True))
    err = np.concatenate([head, xs], axis=-1)
    assert (err <= 1e-4).mean() >= 0.99 and err.max() <= 5e-3, (what, float((err <= 1e-4).mean()), float(err.max()))


def _load(name):
    return fixtures.load(name)


def _train(g, T, counts=None):
    sd = synth.make_state(g)
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k and k.split(".")[-1] not in (
                "prior_feat_ys", "prior_ys", "priors", "priors_on_featmap"):
            v.requires_grad_(True)
    col = {}
    loss = O.clip_forward(sd, synth.make_clip(g, T), synth.make_targets(g, T, counts=counts), g, training=True,
                          track_running_stats=True, collect=col)
    loss.backward()
    return sd, loss, col


def _check_train(gold, sd, loss, col, g, names, full):
    assert abs(loss.item() - gold["train_loss"]) <= 5e-4 * abs(gold["train_loss"])
    T = len(col["frames"])
    for t in range(T):
        fo = col["frames"][t]
        gate = torch.stack([x[0, :, 0] for x in fo.gates]).detach().numpy()
        gerr = np.abs(gate - gold["train_gate"][t])
        assert (gerr <= 1e-4).mean() >= 0.99 and gerr.max() <= 5e-3, (t, float(gerr.max()))
        for s in range(3):
            m = col["positives"][t][s].numpy()
            assert m.tolist() == [i for i in gold["train_matched"][t, s].tolist() if i >= 0]
        if "train_fir" in gold:
            fir = torch.stack([x[0] for x in fo.predictions_fir]).detach().numpy()
            sec = torch.stack([x[0] for x in fo.predictions_sec]).detach().numpy()
            _lines_close(fir, gold["train_fir"][t], f"fir t={t}")
            _lines_close(sec, gold["train_sec"][t], f"sec t={t}")
    if full:
        for j in range(3):
            np.testing.assert_allclose(col["fpn"][j].detach().numpy(), gold[f"train_fpn{j}"], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(sd["backbone.backbone.model.bn1.running_mean"].numpy(), gold["train_bn1_running_mean"], atol=1e-6)
    np.testing.assert_allclose(sd["backbone.backbone.model.bn1.running_var"].numpy(), gold["train_bn1_running_var"], rtol=1e-5)
    for i, k in enumerate(names):
        gr = sd[k].grad
        assert gr is not None, k
        ref = gold["train_grad_norm"][i]
        assert abs(float(gr.double().norm()) - ref) <= 3e-3 * ref + 1e-6, (k, float(gr.double().norm()), ref)
        head = gr.flatten()[:4].double().numpy()
        np.testing.assert_allclose(head, gold["train_grad_head"][i][:len(head)], rtol=2e-2, atol=2e-2 * ref / max(1.0, gr.numel() ** 0.5) + 1e-7)


def _check_eval(gold, g, T):
    sd = synth.make_state(g)
    with torch.no_grad():
        dec = O.clip_forward(sd, synth.make_clip(g, T, seed=77), None, g, training=False, nms_fn=ONMS.lane_nms)
    for t, d in enumerate(dec):
        _lines_close(d["lines"].numpy(), gold["eval_lines"][t], f"eval lines t={t}")
        assert (d["keep_inds"].numpy() == gold["eval_keep_inds"][t]).all()
        assert d["keep"].tolist() == [i for i in gold["eval_keep"][t].tolist() if i >= 0]
        assert len(d["lanes"]) == int((gold["eval_lane_npts"][t] > 0).sum())
        for j, (pts, sx, sy, conf) in enumerate(d["lanes"]):
            n = int(gold["eval_lane_npts"][t, j])
            assert pts.shape == (n, 2)
            np.testing.assert_allclose(pts, gold["eval_lane_pts"][t, j, :n], atol=1e-3)
            np.testing.assert_allclose([sx, sy, conf], gold["eval_lane_meta"][t, j], atol=1e-3)


def test_state_spec_matches_reference_state_dict():
    keys = json.load(open(os.path.join(GOLD, "state_keys.json")))
    for arch in ("resnet18", "resnet34"):
        spec = synth.state_spec(O.Geometry(arch=arch))
        assert list(spec) == list(keys[arch])
        assert all(list(spec[k]) == keys[arch][k] for k in spec)


def test_tiny_train_matches_reference():
    g = O.Geometry(img_h=64, img_w=160, arch="resnet18")
    gold = _load("tiny_r18_64x160.npz")
    names = json.load(open(os.path.join(GOLD, "grad_names_resnet18.json")))
    sd, loss, col = _train(g, 3)
    _check_train(gold, sd, loss, col, g, names, full=True)


def test_tiny_ragged_targets_match_reference():
    """Frames with 0 / 4 / 1 / 2 valid lanes (make_goldens.py --only-ragged): the empty-target branch of the criterion
    (loss4OLV3.py:45-48: classification term only), a full 4-lane assignment, memory tokens without positives."""
    g = O.Geometry(img_h=64, img_w=160, arch="resnet18")
    gold = _load("tiny_ragged_r18_64x160.npz")
    names = json.load(open(os.path.join(GOLD, "grad_names_resnet18.json")))
    counts = (0, 4, 1, 2)
    sd, loss, col = _train(g, len(counts), counts=counts)
    assert [len([i for i in gold["train_matched"][t, 0] if i >= 0]) for t in range(4)] == list(counts)
    _check_train(gold, sd, loss, col, g, names, full=False)
    np.testing.assert_allclose(col["frame_loss"], gold["train_frame_loss"], rtol=1e-3)     # frame 0: classification term only


def test_tiny_eleven_frame_eval_matches_reference():
    """Three frames past the memory depth (save_freq_max = 8): the FIFO of saveMemory4Test drops its oldest entries
    (make_goldens.py --only-long, produced by the reference)."""
    _check_eval(_load("tiny_long_eval_r18_64x160.npz"), O.Geometry(img_h=64, img_w=160, arch="resnet18"), 11)


def test_tiny_eval_matches_reference():
    _check_eval(_load("tiny_r18_64x160.npz"), O.Geometry(img_h=64, img_w=160, arch="resnet18"), 4)


def test_config1_single_frame_r18():
    g = O.Geometry(arch="resnet18")
    gold = _load("config1_r18_320x800.npz")
    sd = synth.make_state(g)
    with torch.no_grad():
        feats = O.fpn_neck(sd, O.resnet_trunk(sd, synth.make_clip(g, 1), g, training=False))
    for j, f in enumerate(feats):
        np.testing.assert_allclose(f[..., ::4, ::5].numpy(), gold[f"fpn{j}_strided"], atol=5e-5, rtol=1e-5)
        np.testing.assert_allclose(f.double().sum(dim=(2, 3)).numpy(), gold[f"fpn{j}_chansum"], rtol=1e-4, atol=1e-2)
    _check_eval(gold, g, 1)


def test_config2_clip_r34_train_and_eval():
    g = O.Geometry(arch="resnet34")
    gold = _load("config2_r34_320x800.npz")
    names = json.load(open(os.path.join(GOLD, "grad_names_resnet34.json")))
    sd, loss, col = _train(g, 5)
    _check_train(gold, sd, loss, col, g, names, full=False)
    _check_eval(gold, g, 5)


def test_config4_geometry_ten_frame_clip_eval():
    """BASELINE.json configs[3] geometry (10 frames 3x384x960; ResNet-34 because the reference has no DLA-34): feature maps
    12x30 .. 48x120, eval clip longer than the memory depth, against the reference's own output
    (make_goldens.py --only-config4)."""
    _check_eval(_load("config4_r34_384x960.npz"), O.Geometry(img_h=384, img_w=960, arch="resnet34"), 10)


@pytest.mark.skipif(os.environ.get("PHNET_SLOW_TESTS") != "1", reason="5 minutes of CPU: set PHNET_SLOW_TESTS=1 (passes; the GPU "
                    "suite holds the HIP path to the same fixture on every run)")
def test_config4_geometry_ten_frame_clip_train():
    """The same geometry, TRAINING clip longer than the memory depth (FIFO of saveMemory, Router4OL.py:563-584)."""
    g = O.Geometry(img_h=384, img_w=960, arch="resnet34")
    gold = _load("config4_r34_384x960.npz")
    names = json.load(open(os.path.join(GOLD, "grad_names_resnet34.json")))
    sd, loss, col = _train(g, 10)
    _check_train(gold, sd, loss, col, g, names, full=False)
    np.testing.assert_allclose(col["frame_loss"], gold["train_frame_loss"], rtol=1e-3)


@pytest.mark.skipif(os.environ.get("PHNET_SLOW_TESTS") != "1", reason="1.5 minutes of CPU: set PHNET_SLOW_TESTS=1 (passes; the GPU "
                    "suite holds the HIP path to the same fixture on every run)")
@pytest.mark.parametrize("tag,fixture,T,seeds", [("pair", "tiny_pair_syncbn_r18_64x160.npz", 3, (3407, 3408)),
                                                ("quad", "tiny_quad_syncbn_r18_64x160.npz", 2, (3407, 3408, 3409, 3410))])
def test_tiny_pair_of_clips_with_joint_batchnorm_statistics(tag, fixture, T, seeds):
    """Two clips = two data-parallel ranks with SyncBatchNorm (make_goldens.py --only-pair: the reference's trunk run once over
    the frames of both clips, its head and criterion per clip, summed loss); quad: four clips = 2 ranks x 2 clips per rank
    (BASELINE.json configs[2] as one workload, make_goldens.py --only-quad)."""
    g = O.Geometry(img_h=64, img_w=160, arch="resnet18")
    gold = {k.replace(tag + "_", "pair_", 1): v for k, v in _load(fixture).items()}
    names = json.load(open(os.path.join(GOLD, "grad_names_resnet18.json")))
    sd = synth.make_state(g)
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k and k.split(".")[-1] not in (
                "prior_feat_ys", "prior_ys", "priors", "priors_on_featmap"):
            v.requires_grad_(True)
    clips = [synth.make_clip(g, T, seed=s) for s in seeds]
    feats = O.fpn_neck(sd, O.resnet_trunk(sd, torch.cat(clips), g, True, True))
    total, cols = 0.0, []
    for b, fr in enumerate(clips):
        col = {}
        total = total + O.clip_forward(sd, fr, synth.make_targets(g, T), g, training=True, collect=col,
                                       feats=[f[b * T:(b + 1) * T] for f in feats])
        cols.append(col)
    total.backward()
    assert abs(total.item() - gold["pair_loss"]) <= 5e-4 * abs(gold["pair_loss"])
    for b in range(len(seeds)):
        np.testing.assert_allclose(cols[b]["frame_loss"], gold["pair_frame_loss"][b], rtol=1e-3)
        for t in range(T):
            for s_ in range(3):
                assert cols[b]["positives"][t][s_].tolist() == [i for i in gold["pair_matched"][b, t, s_].tolist() if i >= 0]
    np.testing.assert_allclose(sd["backbone.backbone.model.bn1.running_mean"].numpy(), gold["pair_bn1_running_mean"], atol=1e-6)
    np.testing.assert_allclose(sd["backbone.backbone.model.bn1.running_var"].numpy(), gold["pair_bn1_running_var"], rtol=1e-5)
    for i, k in enumerate(names):
        ref = gold["pair_grad_norm"][i]
        got = float(sd[k].grad.double().norm())
        assert abs(got - ref) <= 3e-3 * ref + 1e-6, (k, got, ref)
