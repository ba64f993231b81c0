"""The lane head's autograd nodes (phnet_amd/functional.py) and modules on a real MI355X against fp64 autograd of the statements
in tests/head_cases.py - every forward output and every gradient of a case, all entries, by the rule of the encoder tests:

    e_hip <= 4 * max(e32, median e32 over the case's tensors)       for ||g - g64|| / ||g64|| and for max|g - g64| / max|g64|

with e32 the error of plain torch fp32 on the CPU through the same statement and the same ReLU masks.  Observable ReLU masks are
recorded by wrapping the `functional` entry points and held to the mask conditions; hidden ones rely on the seed condition
(head_cases.py).  Every node runs through its public wrapper under three kinds of destination: plain leaves (autograd returns the
gradients), nn.Parameters in a GradArena whose .grad holds a known pattern g0 (expected g0 + gradient), and grad_sink tensors used
twice before one backward (expected twice the gradient).  Which way out a backward took is read from wrapped hip_ops calls.

Measured on an MI355X, median / max over the case's tensors (forward outputs and gradients), the worst of the destination kinds run;
"torch fp32" is e32, the CPU floor.  No device ReLU unit was off fp64's own mask in any case (last column), every hidden-ReLU case
meets its seed condition.

    case                                           destinations     relative L2: device, torch fp32      entry-wise: device, torch fp32       units off
    linear fused_relu_M37                          leaf,arena,sink  9.7e-8 / 1.3e-7   8.5e-8 / 1.3e-7   1.3e-7 / 2.6e-7   1.2e-7 / 2.2e-7   0
    linear fused_M240_nobias                       leaf,arena,sink  2.0e-7 / 3.3e-7   2.0e-7 / 2.0e-7   3.7e-7 / 7.2e-7   3.6e-7 / 4.4e-7   0
    linear padded_N2                               leaf,arena       9.3e-8 / 3.0e-7   6.4e-8 / 2.6e-7   8.1e-8 / 3.3e-7   8.2e-8 / 3.3e-7   0
    linear padded_N42_relu                         leaf,arena       9.3e-8 / 1.4e-7   8.9e-8 / 1.1e-7   1.3e-7 / 2.5e-7   1.3e-7 / 1.7e-7   0
    linear rows_packed_128                         leaf,arena       1.8e-7 / 2.9e-7   1.6e-7 / 2.4e-7   3.0e-7 / 7.2e-7   2.6e-7 / 6.8e-7   0
    linear unfused_M300                            leaf,arena,sink  1.1e-7 / 1.3e-7   1.1e-7 / 1.7e-7   2.1e-7 / 2.9e-7   2.5e-7 / 2.7e-7   0
    linear x_without_grad                          leaf,arena       1.1e-7 / 1.2e-7   1.1e-7 / 1.3e-7   2.4e-7 / 2.8e-7   1.7e-7 / 2.1e-7   0
    linear x_3d_view                               leaf,arena       8.7e-8 / 1.3e-7   8.9e-8 / 1.2e-7   1.6e-7 / 2.9e-7   2.0e-7 / 3.1e-7   0
    linear w_arena_b_plain                         arena            8.5e-8 / 1.2e-7   8.4e-8 / 1.4e-7   1.3e-7 / 2.8e-7   1.2e-7 / 2.9e-7   0
    linear gate_mlp_K2304_N576                     leaf,arena       8.4e-8 / 3.0e-7   8.3e-8 / 2.3e-7   2.4e-7 / 6.0e-7   2.1e-7 / 4.2e-7   0
    linear w_frozen_bias_only                      leaf,arena       1.1e-7 / 1.3e-7   1.2e-7 / 1.5e-7   1.5e-7 / 2.6e-7   2.6e-7 / 3.0e-7   0
    layer_norm L64                                 leaf,arena,sink  5.2e-8 / 7.2e-8   7.3e-8 / 8.1e-8   7.3e-8 / 1.1e-7   1.3e-7 / 1.8e-7   0
    layer_norm L128_relu                           leaf,arena,sink  4.9e-8 / 9.1e-8   7.2e-8 / 8.2e-8   8.5e-8 / 1.3e-7   8.8e-8 / 1.3e-7   0
    layer_norm L1000_relu_res                      leaf,arena,sink  5.2e-8 / 7.5e-8   5.5e-8 / 7.9e-8   8.6e-8 / 1.3e-7   1.2e-7 / 1.6e-7   0
    layer_norm L2304_res                           leaf,arena,sink  5.2e-8 / 8.9e-8   5.5e-8 / 8.5e-8   1.1e-7 / 1.7e-7   1.2e-7 / 1.6e-7   0
    layer_norm CP_64x36_relu_res                   leaf,arena,sink  4.2e-8 / 6.0e-8   4.9e-8 / 7.6e-8   6.5e-8 / 1.0e-7   9.7e-8 / 2.0e-7   0
    dyn N3_36x64x128                               leaf,arena,sink  1.3e-7 / 2.2e-7   1.3e-7 / 2.2e-7   2.1e-7 / 4.2e-7   2.0e-7 / 3.2e-7   0
    dyn N241_36x128x64_x_without_grad              leaf,arena,sink  1.4e-7 / 2.4e-7   1.5e-7 / 4.9e-7   2.8e-7 / 3.8e-7   3.9e-7 / 4.4e-7   0
    dyn N3_5x64x32_x_without_grad                  leaf,arena,sink  1.1e-7 / 1.5e-7   1.0e-7 / 1.4e-7   1.3e-7 / 1.8e-7   8.8e-8 / 2.1e-7   0
    dyn N241_5x64x32                               leaf,arena,sink  1.3e-7 / 2.1e-7   1.4e-7 / 3.3e-7   1.9e-7 / 3.1e-7   2.3e-7 / 4.1e-7   0
    dwconv N7_16x24                                leaf,arena,sink  5.7e-8 / 1.0e-7   5.7e-8 / 4.6e-7   9.7e-8 / 1.5e-7   1.0e-7 / 9.2e-7   0
    dwconv N5_64x36_x_without_grad                 leaf,arena,sink  1.1e-7 / 1.8e-7   8.6e-7 / 1.4e-6   1.4e-7 / 1.5e-7   1.3e-6 / 1.6e-6   0
    gate_tail N37_K576                             leaf,arena,sink  6.7e-8 / 1.2e-7   6.3e-8 / 1.6e-7   7.6e-8 / 1.5e-7   1.3e-7 / 2.5e-7   0
    gate_tail N240_K96_h_without_grad              leaf,arena,sink  1.3e-7 / 4.1e-7   6.7e-8 / 2.1e-7   9.6e-8 / 4.1e-7   8.3e-8 / 2.1e-7   0
    gate_stack anchors_none_3                      leaf,arena,sink  2.2e-7 / 5.4e-7   2.1e-7 / 6.3e-7   2.2e-7 / 5.4e-7   2.7e-7 / 7.3e-7   0
    gate_stack anchors_3_planes_6                  leaf,arena,sink  2.0e-7 / 5.1e-7   2.3e-7 / 5.1e-7   2.0e-7 / 4.9e-7   2.4e-7 / 6.7e-7   0
    towers c64_one_use                             leaf,arena       1.4e-7 / 2.0e-7   1.6e-7 / 2.1e-7   1.6e-7 / 4.0e-7   1.7e-7 / 2.6e-7   0
    towers c128_two_uses                           leaf,arena       2.0e-7 / 3.0e-7   2.0e-7 / 2.9e-7   2.6e-7 / 5.0e-7   1.9e-7 / 4.7e-7   0
    towers c64_two_uses_side_gradient              leaf,arena       1.7e-7 / 2.3e-7   1.4e-7 / 2.0e-7   1.6e-7 / 3.5e-7   1.6e-7 / 3.1e-7   0
    roi_pool 2x5_B1_both                           leaf             7.4e-8 / 1.5e-7   1.5e-7 / 1.8e-7   1.2e-7 / 2.1e-7   2.4e-7 / 2.8e-7   0
    roi_pool 10x25_B2_map_only                     leaf             2.3e-7 / 7.5e-7   7.4e-7 / 7.5e-7   5.0e-7 / 1.3e-6   8.3e-7 / 1.3e-6   0
    roi_pool 10x25_B1_xs_only                      leaf             1.8e-7 / 7.2e-7   3.0e-7 / 7.2e-7   2.7e-7 / 1.3e-6   5.5e-7 / 1.3e-6   0
    roi_pool 2x5_B2_both                           leaf             8.5e-8 / 1.7e-7   1.5e-7 / 1.7e-7   1.1e-7 / 3.0e-7   1.8e-7 / 2.4e-7   0
    roi_pool 10x25_B1_droi_none                    leaf             7.1e-7 / 7.1e-7   7.1e-7 / 7.1e-7   1.3e-6 / 1.3e-6   1.3e-6 / 1.3e-6   0
    lane_update preds_only                         leaf             7.1e-8 / 2.9e-7   7.3e-8 / 2.9e-7   1.3e-7 / 4.4e-7   1.5e-7 / 4.5e-7   0
    lane_update lines_only_priors_grad             leaf             9.0e-8 / 2.2e-7   9.2e-8 / 3.2e-7   2.2e-7 / 3.0e-7   2.3e-7 / 4.0e-7   0
    lane_update both_priors_grad                   leaf             9.0e-8 / 6.0e-7   9.0e-8 / 6.0e-7   3.5e-7 / 1.3e-6   3.5e-7 / 1.3e-6   0
    lane_update both                               leaf             5.5e-8 / 7.3e-8   6.7e-8 / 2.4e-7   3.5e-8 / 1.3e-7   1.3e-7 / 2.7e-7   0
    lane_update neither                            leaf             2.6e-8 / 1.1e-7   3.0e-8 / 1.1e-7   3.4e-8 / 1.9e-7   3.9e-8 / 1.9e-7   0
    dropout_add dropout_add_p0.0                   leaf             0 / 2.8e-8        0 / 2.8e-8        0 / 4.3e-8        0 / 4.3e-8        0
    dropout_add dropout_add_p0.3                   leaf             3.6e-8 / 3.8e-8   3.6e-8 / 3.8e-8   6.8e-8 / 6.9e-8   6.8e-8 / 6.9e-8   0
    dropout_add_ln dropout_add_ln_p0.0             leaf,arena       4.5e-8 / 7.9e-8   5.2e-8 / 9.9e-8   7.4e-8 / 1.1e-7   9.0e-8 / 1.4e-7   0
    dropout_add_ln dropout_add_ln_p0.3             leaf,arena       4.9e-8 / 8.5e-8   5.7e-8 / 9.5e-8   8.2e-8 / 1.0e-7   1.2e-7 / 1.4e-7   0
    gelu_dropout gelu_dropout_p0.0                 leaf             3.9e-8 / 4.7e-8   5.4e-8 / 1.0e-7   6.2e-8 / 9.4e-8   1.6e-7 / 1.9e-7   0
    gelu_dropout gelu_dropout_p0.3                 leaf             5.0e-8 / 6.1e-8   7.4e-8 / 1.1e-7   6.9e-8 / 1.1e-7   1.2e-7 / 2.1e-7   0
    dropout_add_ln dropout_add_ln_p0.0_dh_none     leaf,arena       0 / 4.8e-8        0 / 4.8e-8        0 / 9.4e-8        0 / 9.4e-8        0
    dropout_add_ln dropout_add_ln_p0.3_dh_none     leaf,arena       0 / 5.4e-8        0 / 5.6e-8        0 / 1.2e-7        0 / 1.2e-7        0
    dropout_add_ln dropout_add_ln_p0.0_dt_none     leaf,arena       5.9e-8 / 7.0e-8   5.9e-8 / 8.9e-8   9.9e-8 / 1.2e-7   9.1e-8 / 1.4e-7   0
    dropout_add_ln dropout_add_ln_p0.3_dt_none     leaf,arena       5.4e-8 / 8.9e-8   6.7e-8 / 1.1e-7   7.8e-8 / 1.3e-7   9.1e-8 / 1.6e-7   0
    dropout_add_ln dropout_add_ln_p0.0_both_none   leaf,arena       2.8e-8 / 4.8e-8   2.8e-8 / 4.9e-8   4.9e-8 / 7.3e-8   4.9e-8 / 1.1e-7   0
    attention packed_E128_B1_L7                    leaf             8.1e-8 / 1.4e-7   8.7e-8 / 1.1e-7   1.4e-7 / 1.9e-7   1.3e-7 / 1.4e-7   0
    attention packed_E256_B3_L37                   forward only     1.2e-7 / 1.2e-7   2.0e-7 / 2.0e-7   2.3e-7 / 2.3e-7   2.8e-7 / 2.8e-7   0
    attention cross_E128_B3_37x11_masked           leaf             1.3e-7 / 2.4e-7   1.2e-7 / 1.3e-7   1.3e-7 / 4.9e-7   1.5e-7 / 1.8e-7   0
    attention cross_E256_B1_7x3_masked             forward only     6.7e-8 / 6.7e-8   6.6e-8 / 6.6e-8   1.2e-7 / 1.2e-7   1.0e-7 / 1.0e-7   0
    attention cross_E128_B1_37x11                  leaf             1.6e-7 / 2.0e-7   1.4e-7 / 1.5e-7   1.9e-7 / 3.2e-7   2.1e-7 / 2.4e-7   0
    attention cross_E128_B1_7x3_masked             leaf             1.3e-7 / 1.9e-7   9.9e-8 / 1.4e-7   1.5e-7 / 2.8e-7   1.3e-7 / 1.5e-7   0
    decoder L37_M11_masked_B1                      plain,arena      4.0e-7 / 8.5e-7   4.0e-7 / 8.3e-7   4.3e-7 / 1.2e-6   3.7e-7 / 9.6e-7   0
    decoder L20_M7_B3                              plain,arena      4.8e-7 / 7.8e-7   4.8e-7 / 8.1e-7   5.0e-7 / 1.1e-6   4.9e-7 / 8.5e-7   0
    router B1                                      plain,arena      1.1e-6 / 1.7e-6   1.3e-6 / 6.3e-6   1.1e-6 / 2.2e-6   1.2e-6 / 6.3e-6   0
    router B2                                      plain,arena      4.6e-7 / 1.3e-6   3.3e-7 / 1.4e-6   4.5e-7 / 1.2e-6   3.4e-7 / 1.7e-6   0
    dynconv B1_24_anchors                          plain,arena      7.2e-7 / 1.3e-6   6.6e-7 / 7.6e-7   6.7e-7 / 1.1e-6   6.5e-7 / 1.0e-6   0
    dynconv B2_24_anchors                          plain,arena      6.9e-7 / 1.6e-6   6.1e-7 / 7.5e-7   6.9e-7 / 1.1e-6   5.4e-7 / 1.1e-6   0
    branch fir                                     plain,arena      1.8e-7 / 7.8e-7   1.6e-7 / 5.3e-7   4.4e-7 / 9.4e-7   2.5e-7 / 8.0e-7   0
    branch sec                                     plain,arena      2.1e-7 / 5.0e-7   2.0e-7 / 7.7e-7   4.3e-7 / 8.3e-7   3.7e-7 / 1.7e-6   0

The one tensor outside the rule: d b of gate_tail at N = 240 (4.1e-7 against 2.7e-7), one number summed in another order than torch
- granted the kernel's own 1e-5 (tests/head_cases.py _gate_tail).  Zero gradients (the depth-wise conv biases in front of a
LayerNorm) are held to the kernel tests' noise rule.  Head width 32 has a forward kernel only: those attention cases hold the
forward and assert that a backward is refused.  The decoder's in_proj weights and biases are judged per q / k / v row block; the k
block of a bias (true gradient zero) as a difference in units of the whole bias gradient.  The cases without any cotangent
(lane_update neither, roi_pool droi_none, dropout_add_ln both_none) still enter the node's backward, on undefined gradients: their
rows hold the forward only, and the tests assert that nothing was launched and no destination was touched.

What the bound sees (test_the_bound_fails_when_it_should, one hip_ops call wrapped): the linear_bwd weight destination times
1 + 1e-3 -> d w off by 1.0e-3 against a bound of 3.4e-7 (the smallest factor still seen: 1 + 4e-7); colsum skipped -> d b off by
1.0 against 5.0e-7 (seen down to a 5e-7 share of the bias gradient missing); d k of one of eight heads zeroed -> d kv off by 0.16
against 5.3e-7 (seen down to that head's d k scaled by 1 - 4e-6); the sink added twice -> d w, d b off by 1.0 against 3.4e-7 (seen down
to a 4e-7 share added again).

Run with -m gpu.
"""
import inspect
from collections import OrderedDict

import pytest
import torch

from tests import head_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops
    assert hip_ops.mma_mode() == 3 and hip_ops.CONV3P, "the suite runs in the default arithmetic"
    return hip_ops


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    """The cached fp64 / fp32 runs (the dynamic head's hold ~1 GB) go when the module is done."""
    yield
    H.release()


@pytest.fixture
def dropout_stream():
    """DropoutStream as the test found it: counters, slots and site numbering are put back, so later tests draw the masks they
    would have drawn without this module."""
    from phnet_amd import functional as PF
    S = PF.DropoutStream
    S._ring(torch.device("cuda", torch.cuda.current_device()))
    saved = ({k: v.clone() for k, v in S._state.items()}, dict(S._slot), S._calls)
    yield S
    for k, v in saved[0].items():
        S._state[k].copy_(v)
    S._slot.clear()
    S._slot.update(saved[1])
    S._calls = saved[2]


def dev(v):
    return v.float().cuda() if v.is_floating_point() else v.cuda()


# ------------------------------------------------------------------------------------------------ recording
class MaskRecorder:
    """Wraps the `functional` entry points whose output is a ReLU; keeps y > 0 of every such call, in call order."""

    def __init__(self, monkeypatch):
        from phnet_amd import functional as PF
        self.masks = []
        lin, ln, dyn = PF.linear, PF.layer_norm, PF.dyn_bmm_ln_relu

        def keep(y):
            self.masks.append((y.detach() > 0).cpu())
            return y

        def linear(x, w, b=None, relu=False, rows=None):
            y = lin(x, w, b, relu, rows)
            return keep(y) if relu else y

        def layer_norm(x, w, b, res=None, relu=False, eps=1e-5):
            y = ln(x, w, b, res, relu, eps)
            return keep(y) if relu else y

        monkeypatch.setattr(PF, "linear", linear)
        monkeypatch.setattr(PF, "layer_norm", layer_norm)
        monkeypatch.setattr(PF, "dyn_bmm_ln_relu", lambda *a, **kw: keep(dyn(*a, **kw)))


class Spy:
    """Wraps hip_ops calls; keeps (name, bound arguments) of every call."""

    def __init__(self, monkeypatch, K, names):
        self.calls = []
        for name in names:
            self._wrap(monkeypatch, K, name)

    def _wrap(self, monkeypatch, K, name):
        orig = getattr(K, name)
        sig = inspect.signature(orig)

        def wrapper(*a, **kw):
            self.calls.append((name, sig.bind(*a, **kw).arguments))
            return orig(*a, **kw)
        monkeypatch.setattr(K, name, wrapper)

    def count(self, name):
        return sum(n == name for n, _ in self.calls)

    def args(self, name):
        return [a for n, a in self.calls if n == name]


# ------------------------------------------------------------------------------------------------ the nodes on the device
def entries(monkeypatch, node) -> list:
    """Wraps `node.backward` (an autograd Function of phnet_amd.functional); the returned list gets the cotangents of every call."""
    orig, seen = node.backward, []

    def backward(ctx, *gs):
        seen.append(gs)
        return orig(ctx, *gs)
    monkeypatch.setattr(node, "backward", staticmethod(backward))
    return seen


class _DropGrad(torch.autograd.Function):
    """Identity whose backward hands `None` on: how a node meets an undefined cotangent."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return None


def _d_linear(PF, t, o):
    if o.get("rows"):
        e = o["rows"]
        return OrderedDict(q=PF.linear(t["x"], t["w"], t["b"], rows=(0, e)), kv=PF.linear(t["x2"], t["w"], t["b"], rows=(e, 3 * e)))
    return OrderedDict(y=PF.linear(t["x"], t["w"], t.get("b"), relu=o["relu"]))


def _d_towers(PF, t, o):
    params = [t[k] for k in H.tower_param_names()]
    w1, b1, w2, b2, wh, bh = PF.assemble_towers(o["c"], H.TOWER_OUT, None, params)
    n_out = sum(H.TOWER_OUT)
    assert wh.shape[0] == 44 and not bool(wh[n_out:].any()) and not bool(bh[n_out:].any())
    outs = OrderedDict()
    for i in range(t["x"].shape[0]):
        h = PF.linear(PF.linear(t["x"][i], w1, b1, relu=True), w2, b2, relu=True)
        outs[f"y{i}"] = PF.linear(h, wh, bh)[:, :n_out]
    if o.get("side"):
        outs["b1"] = b1 * 1.0
    return outs


def _d_roi_pool(PF, t, o):
    roi, roi_cp = PF.roi_pool(t["fmap"], t["xs"], H.O.prior_feat_ys(H.GEOM).cuda())
    assert not roi_cp.requires_grad and torch.equal(roi_cp, roi.detach().permute(0, 1, 3, 2))
    return OrderedDict(roi=roi)


def _d_lane_update(PF, t, o):
    preds, lines = PF.lane_update(t["priors"], t["head"], H.O.prior_ys(H.GEOM).cuda(), H.GEOM.img_w, H.GEOM.img_h)
    return OrderedDict(preds=preds, lines=lines)


def _d_attention(PF, t, o):
    if o["packed"]:
        return OrderedDict(y=PF.attention_packed(t["qkv"], o["heads"], 0.0, o["batch"]))
    return OrderedDict(y=PF.attention_cross(t["q"], t["kv"], o["heads"], 0.0, t.get("valid"), o["batch"]))


def _d_dropout_add_ln(PF, t, o):
    tt, h = PF.dropout_add_ln(t["res"], t["x"], t["w"], t["b"], o["p"], H.EPS)
    return OrderedDict(t=tt, h=h)


DEVICE = {
    "linear": _d_linear,
    "layer_norm": lambda PF, t, o: OrderedDict(y=PF.layer_norm(t["x"], t["w"], t["b"], t.get("res"), o["relu"], H.EPS)),
    "dyn": lambda PF, t, o: OrderedDict(y=PF.dyn_bmm_ln_relu(t["x"], t["w"], t["gamma"], t["beta"], H.EPS)),
    "dwconv": lambda PF, t, o: OrderedDict(y=PF.dwconv3x3(t["x"], t["w"], t["b"])),
    "gate_tail": lambda PF, t, o: OrderedDict(y=PF.gate_tail(t["h"], t["w"], t["b"]).view(-1)),
    "gate_stack": lambda PF, t, o: OrderedDict(y=PF.gate_stack(t["x"], [t[k] for k in H.gate_param_names()], H.EPS, o["anchors"])),
    "roi_pool": _d_roi_pool,
    "lane_update": _d_lane_update,
    "dropout_add": lambda PF, t, o: OrderedDict(y=PF.dropout_add(t["res"], t["x"], o["p"])),
    "dropout_add_ln": _d_dropout_add_ln,
    "gelu_dropout": lambda PF, t, o: OrderedDict(y=PF.gelu_dropout(t["x"], o["p"])),
    "attention": _d_attention,
    "towers": _d_towers,
}


class DeviceRun:
    """One piece through its public wrapper under one kind of destination.  outs / grads: CPU tensors; g0: what the arena held;
    times: how often the graph fed the destinations; none: leaves that autograd handed no gradient at all (compared as zeros)."""

    def __init__(self, piece, mode, masks: MaskRecorder = None):
        from phnet_amd import functional as PF
        from phnet_amd.arena import GradArena, grad_sink
        o = piece.opts
        t, leaves = {}, {}
        for k, v in piece.tensors.items():
            d = dev(v)
            if k in piece.diff:
                if k == "x" and o.get("x_view"):                                  # x as a non-contiguous 3-D view of a [K,A,B] leaf
                    leaves[k] = d.permute(2, 0, 1).contiguous().requires_grad_(True)
                    d = leaves[k].permute(1, 2, 0)
                    assert not d.is_contiguous()
                elif k in piece.params and mode == "arena" and k not in o.get("plain", ()):
                    d = leaves[k] = torch.nn.Parameter(d)
                else:
                    leaves[k] = d.requires_grad_(True)
            t[k] = d
        in_arena = [k for k in piece.params if isinstance(leaves[k], torch.nn.Parameter)]
        self.g0, self.times = {}, 2.0 if mode == "sink" else 1.0
        arena = GradArena([leaves[k] for k in in_arena]) if in_arena else None
        try:
            for k in in_arena:
                self.g0[k] = H.g0_pattern(leaves[k].shape)
                leaves[k].grad.copy_(self.g0[k])
            if mode == "sink":
                for k in piece.params:
                    t[k] = grad_sink(leaves[k])
                    assert t[k]._phnet_sink is not None and not bool(t[k]._phnet_sink.any())
            runs = [DEVICE[piece.kind](PF, t, o) for _ in range(2 if mode == "sink" else 1)]
            n_masks = 0 if masks is None else len(masks.masks) // len(runs)
            if len(runs) == 2:
                assert all(torch.equal(a, b) for a, b in zip(runs[0].values(), runs[1].values()))
                assert all(torch.equal(a, b) for a, b in zip(masks.masks[:n_masks], masks.masks[n_masks:]))
            self.masks = (masks.masks[:n_masks] or None) if masks is not None else None
            self.outs = OrderedDict((k, v.detach().cpu()) for k, v in runs[0].items())
            cots = H.cotangents(piece, {k: v.shape for k, v in self.outs.items()})
            used = [k for k in self.outs if piece.cot_on is None or k in piece.cot_on]
            drop_grad = piece.cot_on == () and bool(leaves)                       # no cotangent at all: the node's backward still runs,
            if drop_grad:                                                        # on undefined gradients for every output
                torch.autograd.backward([_DropGrad.apply(r[k]) for r in runs for k in self.outs],
                                        [dev(cots[k]) for r in runs for k in self.outs])
            elif used and leaves:
                torch.autograd.backward([r[k] for r in runs for k in used], [dev(cots[k]) for r in runs for k in used])
            torch.cuda.synchronize()
            if arena is not None:
                lo, hi = arena.flat.data_ptr(), arena.flat.data_ptr() + arena.flat.numel() * 4
                assert all(lo <= leaves[k].grad.data_ptr() < hi for k in in_arena), "a gradient left the arena"
            self.grads, self.none = {}, []
            for k, leaf in leaves.items():
                g = leaf.grad
                if not used or drop_grad:
                    assert g is None or (k in self.g0 and torch.equal(g.cpu(), self.g0[k])), (k, "touched without a cotangent")
                    continue
                if g is None:                                                    # autograd got `None` for this leaf: a zero gradient
                    self.none.append(k)
                    g = torch.zeros_like(leaf)
                self.grads[k] = (g.permute(1, 2, 0) if (k == "x" and o.get("x_view")) else g).detach().cpu().clone()
        finally:
            if arena is not None:
                arena.release()


def held(piece, run: DeviceRun, what: str) -> H.Report:
    rep = H.compare(piece, run.outs, run.grads, run.masks, g0=run.g0, times=run.times)
    print("\n" + rep.line(f"{piece.kind} {piece.name} [{what}]"))
    assert not rep.bad, (piece.name, what, rep.bad)
    return rep


# ------------------------------------------------------------------------------------------------ Part 1: _Linear, every way out
LINEAR_RUNS = [(p, m) for p in H.LINEAR for m in ("leaf", "arena", "sink") if m in p.opts["ways"]]


@pytest.mark.parametrize("piece,mode", LINEAR_RUNS, ids=[f"{p.name}-{m}" for p, m in LINEAR_RUNS])
def test_linear_every_way_out(K, monkeypatch, piece, mode):
    """_Linear.backward: the one-launch linear_bwd (with / without the ReLU mask), dgrad + wgrad into the arena, dgrad + wgrad
    returned to autograd, the separate colsum for the bias (into the arena and returned), zero-padded widths (which leave the arena
    path and are still right with arena-backed parameters), both row blocks of a packed weight in one graph."""
    o, way = piece.opts, piece.opts["ways"][mode]
    spy = Spy(monkeypatch, K, ("linear_bwd", "linear_wgrad", "colsum", "linear_dgrad"))
    run = DeviceRun(piece, mode, MaskRecorder(monkeypatch))
    uses = (2 if o.get("rows") else 1) * (2 if mode == "sink" else 1)
    # the class the case claims
    if o.get("rows"):
        e = o["rows"]
        assert K.linear_bwd_fusable(37, e, e) and K.linear_bwd_fusable(11, e, 2 * e)
    else:
        n4 = o["n"] + (-o["n"]) % 4
        assert K.linear_bwd_fusable(o["m"], o["k"], n4) == (o["m"] <= 256), (o["m"], o["k"], n4)
    counts = {n: spy.count(n) for n in ("linear_bwd", "linear_wgrad", "colsum")}
    if way == "fused":
        assert counts == dict(linear_bwd=uses, linear_wgrad=0, colsum=0) and spy.count("linear_dgrad") == 0, counts
        assert all(a["accumulate"] and (a["relu_y"] is not None) == o["relu"] and (a["dbias"] is not None) == ("b" in piece.params)
                   for a in spy.args("linear_bwd"))
    elif way in ("wgrad_arena", "wgrad_returned"):
        assert counts == dict(linear_bwd=0, linear_wgrad=uses, colsum=0), counts
        for a in spy.args("linear_wgrad"):                                       # the bias gradient comes out of the same launch
            assert (a.get("dw") is not None) == (way == "wgrad_arena") and bool(a.get("accumulate")) == (way == "wgrad_arena")
            assert (a.get("dbias") is not None) == ("b" in piece.params)
        assert spy.count("linear_dgrad") == (uses if "x" in piece.inputs else 0)
    else:
        assert counts == dict(linear_bwd=0, linear_wgrad=0, colsum=uses), counts
        assert all((a.get("out") is not None) == (way == "colsum_arena") for a in spy.args("colsum"))
    if o.get("plain"):
        assert set(run.g0) == {"w"}
    held(piece, run, f"{mode}: {way}")


# ------------------------------------------------------------------------------------------------ Part 1: the other nodes
# kind -> (the hip_ops backward whose `accumulate` flag says "into direct_grad(p)" / "returned to autograd", its need-dx argument)
SWITCH = {"layer_norm": ("layernorm_bwd", None), "dyn": ("dyn_bmm_ln_relu_bwd", "need_dx"), "dwconv": ("dwconv3x3_wgrad", None),
          "gate_tail": ("gate_tail_bwd", "need_dh"), "gate_stack": ("gate_stack_bwd", None), "dropout_add_ln": ("dropout_add_ln_bwd", None),
          "towers": ("scatter_tower_grads", None)}
NODE_RUNS = ([(p, m) for p in H.LAYER_NORM + H.DYN + H.DWCONV + H.GATE_TAIL + H.gate_stack_pieces() for m in ("leaf", "arena", "sink")]
             + [(p, m) for p in H.TOWERS for m in ("leaf", "arena")])


@pytest.mark.parametrize("piece,mode", NODE_RUNS, ids=[f"{p.kind}-{p.name}-{m}" for p, m in NODE_RUNS])
def test_node_direct_and_returned_destinations(K, monkeypatch, piece, mode):
    """_LayerNorm, _DynBmmLnRelu, _DwConv, _GateTail, _GateStack, _AssembleTowers: parameter gradients accumulated into
    direct_grad(p) (arena, sink) or returned to autograd (plain leaves) - the wrapped backward call says which - and dx skipped
    where the input needs none."""
    name, need = SWITCH[piece.kind]
    spy = Spy(monkeypatch, K, (name,))
    run = DeviceRun(piece, mode, MaskRecorder(monkeypatch))
    calls = spy.args(name)
    assert len(calls) == (2 if mode == "sink" else 1), (name, len(calls))        # a sink used twice: one backward per use
    assert all(bool(c.get("accumulate", False)) == (mode != "leaf") for c in calls)
    if need is not None:
        assert all(bool(c.get(need, True)) == ("x" in piece.inputs or "h" in piece.inputs) for c in calls)
    if piece.kind == "gate_tail":
        assert 0.2 < float((run.outs["y"] == 0.5).float().mean()) < 0.8           # closed ReLUs are part of the case
    held(piece, run, mode)


# ------------------------------------------------------------------------------------------------ ROI pooling, prior update
@pytest.mark.parametrize("piece", H.ROI_POOL, ids=H.ids(H.ROI_POOL))
def test_roi_pool(K, monkeypatch, piece):
    """_RoiPool: gradient to the map only / to xs only / to both, B in {1, 2}, samples outside the map, and an undefined `droi`."""
    spy = Spy(monkeypatch, K, ("roi_pool_bwd",))
    from phnet_amd import functional as PF
    none = piece.cot_on == ()
    seen = entries(monkeypatch, PF._RoiPool)
    run = DeviceRun(piece, "leaf")
    assert float((piece.tensors["xs"] < 0).double().mean()) > 0.05 and float((piece.tensors["xs"] > 1).double().mean()) > 0.05
    assert len(seen) == 1
    if none:                                                                     # the backward ran, on droi = None, and launched nothing
        assert seen[0][0] is None and spy.count("roi_pool_bwd") == 0 and run.grads == {}
    else:
        (a,) = spy.args("roi_pool_bwd")
        assert (a["dmap"] is not None) == ("fmap" in piece.inputs) and bool(a["need_dxs"]) == ("xs" in piece.inputs)
    held(piece, run, "leaf")


@pytest.mark.parametrize("piece", H.LANE_UPDATE, ids=H.ids(H.LANE_UPDATE))
def test_lane_update(K, monkeypatch, piece):
    """_LaneUpdate: a cotangent on preds only, on lines only, on both and on neither; priors with and without grad."""
    from phnet_amd import functional as PF
    spy = Spy(monkeypatch, K, ("lane_update_bwd",))
    seen = entries(monkeypatch, PF._LaneUpdate)
    run = DeviceRun(piece, "leaf")
    assert len(seen) == 1
    if not piece.cot_on:                                                         # the backward ran on (None, None): no launch, no gradient
        assert seen[0] == (None, None) and spy.count("lane_update_bwd") == 0 and run.grads == {}
    else:
        (a,) = spy.args("lane_update_bwd")
        assert (a["dpreds"] is not None) == ("preds" in piece.cot_on) and (a["dlines"] is not None) == ("lines" in piece.cot_on)
        assert bool(a["need_dpriors"]) == piece.opts["pri_grad"]
        assert not bool(run.grads["head"][..., 6 + H.GEOM.num_points:].any())     # the head's padding columns get no gradient
    held(piece, run, "leaf")


# ------------------------------------------------------------------------------------------------ dropout nodes
DROPOUT_RUNS = [(p, m) for p in H.DROPOUT + H.DROPOUT_LN_WAYS for m in (("leaf", "arena") if p.params else ("leaf",))]


@pytest.mark.parametrize("piece,mode", DROPOUT_RUNS, ids=[f"{p.name}-{m}" for p, m in DROPOUT_RUNS])
def test_dropout_nodes(K, monkeypatch, dropout_stream, piece, mode):
    """_DropoutAdd, _DropoutAddLN, _GeluDropout at p = 0 and at p = 0.3 inside DropoutStream.begin_step: the mask is recovered from
    the forward (t - res != 0, y != 0), the reference applies it with 1 / (1 - p), so a backward that drew another mask fails.
    _DropoutAddLN also with `dh is None` (plain dropout backward, no LayerNorm launch), `dt is None` and neither cotangent."""
    p = piece.opts["p"]
    if p > 0:
        dropout_stream.begin_step(torch.device("cuda", torch.cuda.current_device()))
    from phnet_amd import functional as PF
    spy = Spy(monkeypatch, K, ("dropout_add_ln_bwd", "dropout_add", "gelu_dropout_bwd"))
    seen = entries(monkeypatch, PF._DropoutAddLN)
    run = DeviceRun(piece, mode)
    first = next(iter(run.outs.values()))
    res = piece.tensors["res"].float() if "res" in piece.tensors else None
    keep = H.recovered_keep(first, res)
    if p == 0:
        assert bool(keep.all()) or piece.kind == "gelu_dropout"
        keep = torch.ones_like(keep)
    else:
        assert abs(float(keep.mean()) - (1 - p)) < 0.03, float(keep.mean())
    piece = piece.with_tensors(keep=keep)
    if piece.kind == "dropout_add_ln":
        cot = piece.cot_on
        calls = spy.args("dropout_add_ln_bwd")
        if cot is None or "h" in cot:                                            # the LayerNorm backward, into the arena or returned
            assert len(calls) == 1 and bool(calls[0].get("accumulate", False)) == (mode == "arena")
            assert (calls[0]["dt"] is not None) == (cot is None)
        else:                                                                    # dh is None: no LayerNorm launch; parameters untouched
            assert calls == [] and spy.count("dropout_add") == (1 if (p > 0 and cot) else 0)
            assert mode == "arena" or not cot or set(run.none) == {"w", "b"}
        assert len(seen) == 1 and tuple(g is not None for g in seen[0]) == (cot is None or "t" in cot, cot is None or "h" in cot)
        if cot == ():                                                            # (None, None): nothing launched, no leaf touched, g0 kept
            assert spy.calls == [] and run.grads == {}
    held(piece, run, mode)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("piece", H.ATTENTION, ids=H.ids(H.ATTENTION))
def test_attention(K, monkeypatch, piece):
    """_Attention: packed and cross layouts, head width 16 and 32, a key mask with a clip that has a single valid key, batch 1 and
    3, p = 0.  Gradients arrive in packed buffers of the inputs' layout."""
    spy = Spy(monkeypatch, K, ("attention_bwd",))
    if not piece.inputs:                                                         # head width 32: forward only - a backward is an error
        from phnet_amd import functional as PF
        t = {k: dev(v) for k, v in piece.tensors.items()}
        first = "qkv" if piece.opts["packed"] else "q"
        t[first].requires_grad_(True)
        y = DEVICE["attention"](PF, t, piece.opts)["y"]
        with pytest.raises(RuntimeError, match="phnet_attention_bwd failed"):
            y.backward(torch.ones_like(y))
        assert t[first].grad is None
        run = DeviceRun(piece, "leaf")
        assert spy.count("attention_bwd") == 1 and run.grads == {}
        held(piece, run, "forward only")
        return
    run = DeviceRun(piece, "leaf")
    (a,) = spy.args("attention_bwd")
    assert a["batch"] == piece.opts["batch"] and a["heads"] == piece.opts["heads"]
    assert (a["key_valid"] is not None) == ("valid" in piece.tensors)
    if "valid" in piece.tensors:
        v = piece.tensors["valid"].view(piece.opts["batch"], -1)
        assert (int(v[0].sum()) == 1) == (piece.opts["batch"] > 1) and not bool(v.all()) and bool(v.any(dim=1).all())
        assert not bool(run.grads["kv"][~piece.tensors["valid"]].any())          # a masked key gets no gradient
    held(piece, run, "leaf")


# ------------------------------------------------------------------------------------------------ Part 2: the decoder
def build_decoder(piece):
    from phnet_amd.libs.models.utils.transformer import TransformerDecoder, TransformerDecoderLayer
    o = piece.opts
    layer = TransformerDecoderLayer(o["e"], o["heads"], o["ff"], dropout=0.0, activation="gelu", normalize_before=True)
    dec = TransformerDecoder(layer, o["layers"], torch.nn.LayerNorm(o["e"]))
    assert sorted(k for k, _ in dec.named_parameters()) == sorted(H.decoder_param_names(o["layers"]))
    with torch.no_grad():
        for k, p in dec.named_parameters():
            p.copy_(piece.tensors[k])
    return dec.cuda().train()


def module_run(piece, module, forward, arena_mode: bool, names):
    """forward(leaves) -> {name: output} on a module whose parameters `names` (a subset may stay unused) are compared; leaves =
    the piece's differentiable inputs on the device.  Returns (outs, grads, g0)."""
    from phnet_amd.arena import GradArena
    leaves = {k: dev(piece.tensors[k]).requires_grad_(True) for k in piece.inputs}
    params = dict(module.named_parameters())
    arena, g0 = (GradArena(module.parameters()), {}) if arena_mode else (None, {})
    try:
        if arena_mode:
            for k, p in params.items():
                g0[k] = H.g0_pattern(p.shape)
                p.grad.copy_(g0[k])
        outs = forward(leaves)
        cots = H.cotangents(piece, {k: v.shape for k, v in outs.items()})
        torch.autograd.backward(list(outs.values()), [dev(cots[k]) for k in outs])
        torch.cuda.synchronize()
        grads = {k: leaves[k].grad.detach().cpu() for k in leaves}
        for k, p in params.items():
            if k in names:
                assert p.grad is not None, k
                grads[k] = p.grad.detach().cpu().clone()
            else:                                                                # a parameter the piece does not use stays as it was
                assert p.grad is None or torch.equal(p.grad.cpu(), g0[k]), k
        if arena_mode:
            lo, hi = arena.flat.data_ptr(), arena.flat.data_ptr() + arena.flat.numel() * 4
            assert all(lo <= p.grad.data_ptr() < hi for p in params.values()), "a gradient left the arena"
        return OrderedDict((k, v.detach().cpu()) for k, v in outs.items()), grads, {k: v for k, v in g0.items() if k in names}
    finally:
        if arena is not None:
            arena.release()


@pytest.mark.parametrize("arena", [False, True], ids=["plain", "arena"])
@pytest.mark.parametrize("piece", H.DECODER, ids=H.ids(H.DECODER))
def test_decoder_training_path(K, monkeypatch, piece, arena):
    """TransformerDecoder (2 pre-norm GELU layers, d_model 128, 8 heads, ff 256, final LayerNorm) in train mode at dropout 0 under
    autograd - the unfused path: every parameter gradient (the q / k / v row blocks of both in_proj_weights one tensor each), d tgt
    and d memory."""
    dec = build_decoder(piece)
    spy = Spy(monkeypatch, K, ("rowchain_fwd", "linear_bwd", "linear_wgrad", "attention_bwd", "dropout_add_ln_bwd"))
    valid = dev(piece.tensors["valid"]) if "valid" in piece.tensors else None
    batch = piece.opts["batch"]

    def forward(leaves):
        assert torch.is_grad_enabled() and not dec._can_fuse(leaves["tgt"], leaves["memory"])
        return OrderedDict(y=dec(leaves["tgt"], leaves["memory"], valid, batch=batch))

    outs, grads, g0 = module_run(piece, dec, forward, arena, set(piece.params))
    assert spy.count("rowchain_fwd") == 0 and spy.count("attention_bwd") == 4 and spy.count("dropout_add_ln_bwd") == 6
    # 7 Linear nodes per layer (q|k|v, out; q rows, k|v rows, out; 2 feed-forward): one fused launch each with arena destinations
    assert (spy.count("linear_bwd"), spy.count("linear_wgrad")) == ((14, 0) if arena else (0, 14))
    rep = H.compare(piece, outs, grads, None, g0=g0)
    print("\n" + rep.line(f"decoder {piece.name} [{'arena' if arena else 'plain'}]"))
    assert len([k for k in rep.e_l2 if k.startswith("grad:")]) == 2 * 26 + 2 + 2
    assert not rep.bad, rep.bad


# ------------------------------------------------------------------------------------------------ Part 2: the routing gate
@pytest.mark.parametrize("arena", [False, True], ids=["plain", "arena"])
@pytest.mark.parametrize("piece", H.router_pieces(), ids=H.ids(H.router_pieces()))
def test_router_module(K, monkeypatch, piece, arena):
    """AdaptiveRouter4Lane(num_priors=5, features_channels=16, num_points=24) at stage 1 over B in {1, 2} frames: gate stack,
    Linear + ReLU, gate tail.  All its ReLUs are covered by the seed condition; the input gets no gradient; the parameters of the
    other stages stay untouched."""
    from phnet_amd.libs.models.Router import AdaptiveRouter4Lane
    o = piece.opts
    gate = AdaptiveRouter4Lane(num_priors=o["n"], features_channels=o["c"], num_points=o["p"], stages=3)
    with torch.no_grad():
        for k, p in gate.named_parameters():
            if k in piece.tensors:
                p.copy_(piece.tensors[k])
    gate = gate.cuda().train()
    spy = Spy(monkeypatch, K, ("gate_stack_bwd", "gate_tail_bwd", "linear_bwd", "linear_wgrad"))
    x = dev(piece.tensors["x"])
    outs, grads, g0 = module_run(piece, gate, lambda leaves: OrderedDict(y=gate(x, o["stage"])), arena, set(piece.params))
    assert not x.requires_grad and x.grad is None
    assert all(bool(c["accumulate"]) == arena for c in spy.args("gate_stack_bwd")) and spy.count("gate_stack_bwd") == 1
    assert [bool(c.get("accumulate", False)) for c in spy.args("gate_tail_bwd")] == [arena]
    assert (spy.count("linear_bwd"), spy.count("linear_wgrad")) == ((1, 0) if arena else (0, 1))
    closed = float((outs["y"] == 0.5).float().mean())
    assert 0.0 < closed < 1.0
    rep = H.compare(piece, outs, grads, None, g0=g0)
    print("\n" + rep.line(f"router {piece.name} [{'arena' if arena else 'plain'}]"))
    assert not rep.bad, rep.bad


# ------------------------------------------------------------------------------------------------ sensitivity
def _scaled_weight_destination(K):
    orig = K.linear_bwd

    def linear_bwd(dy, x, w, dw, dbias, accumulate, relu_y=None):
        dx = orig(dy, x, w, dw, dbias, accumulate, relu_y)
        dw.mul_(1.0 + 1e-3)
        return dx
    return "linear_bwd", linear_bwd


def _colsum_skipped(K):
    return "colsum", lambda a, out=None, accumulate=False: out


def _one_head_dk_zeroed(K):
    orig = K.attention_bwd

    def attention_bwd(q, k, v, o, dout, lse, heads, dq, dk, dv, *a, **kw):
        orig(q, k, v, o, dout, lse, heads, dq, dk, dv, *a, **kw)
        dk[:, :q.shape[1] // heads].zero_()
    return "attention_bwd", attention_bwd


def _sink_added_twice(K):
    orig = K.linear_bwd

    def linear_bwd(*a, **kw):
        orig(*a, **kw)
        return orig(*a, **kw)
    return "linear_bwd", linear_bwd


SENSITIVITY = OrderedDict([
    ("linear_bwd_weight_destination_times_1.001", (H.LINEAR[0], "arena", _scaled_weight_destination, {"grad:w"})),
    ("colsum_skipped", (H.LINEAR[10], "arena", _colsum_skipped, {"grad:b"})),
    ("attention_dk_of_one_head_zeroed", (H.ATTENTION[2], "leaf", _one_head_dk_zeroed, {"grad:kv"})),
    ("sink_added_twice", (H.LINEAR[0], "sink", _sink_added_twice, {"grad:w", "grad:b"})),
])


@pytest.mark.parametrize("what", list(SENSITIVITY))
def test_the_bound_fails_when_it_should(K, monkeypatch, what):
    """One hip_ops call wrapped: the comparison reports violations on exactly the perturbed tensors (and reports none without the
    wrapper: the other tests).  Printed: the error the perturbation causes against the bound, i.e. how much smaller it could be."""
    piece, mode, wrap, expect = SENSITIVITY[what]
    monkeypatch.setattr(K, *wrap(K))
    run = DeviceRun(piece, mode, MaskRecorder(monkeypatch))
    rep = H.compare(piece, run.outs, run.grads, run.masks, g0=run.g0, times=run.times)
    seen = {k for k, *_ in rep.bad}
    print(f"\n{what}: " + "; ".join(f"{k} {m} {e:.1e} against a bound of {b:.1e}" for k, m, e, b in rep.bad))
    assert seen == expect, rep.bad


# ------------------------------------------------------------------------------------------------ Part 2: the dynamic head
@pytest.mark.parametrize("arena", [False, True], ids=["plain", "arena"])
@pytest.mark.parametrize("b", [1, 2], ids=["B1", "B2"])
def test_dynamic_conv_module(K, monkeypatch, b, arena):
    """DynamicConv(feat_size=36, inplanes=64) on 24 anchors, B in {1, 2}: begin_clip(SinkPool()), two calls inside the clip
    before one backward (the second call hits the fold cache, the sinks of the folded weights gather both uses), against
    oracle.dynamic_head unfolded with its detach in place, through the device's masks of both ReLUs.  A second begin_clip hands
    out fresh sinks."""
    from phnet_amd.arena import SinkPool
    from phnet_amd.libs.models.utils.dynamic_head import DynamicConv
    piece = H.dynconv_piece(b)
    m = DynamicConv(feat_size=piece.opts["p"], inplanes=piece.opts["c"])
    assert sorted(k for k, _ in m.named_parameters()) == sorted(H.DYNCONV_KEYS)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(piece.tensors[k])
    m = m.cuda().train()
    rec = MaskRecorder(monkeypatch)
    spy = Spy(monkeypatch, K, ("dyn_bmm_ln_relu_bwd", "layernorm_bwd"))
    seen = {}

    def forward(leaves):
        m.begin_clip(SinkPool())
        outs = OrderedDict()
        for i in range(piece.opts["uses"]):
            outs[f"y{i}"] = m(leaves[f"pro{i}"], leaves[f"roi{i}"])
            if i == 0:
                seen["folded"] = dict(m._folded)
        assert set(m._folded) == {"dynamic_layer_1", "out_layer"}
        assert all(m._folded[k][j] is seen["folded"][k][j] for k in m._folded for j in (0, 1)), "the second call folded again"
        seen["sinks"] = [t._phnet_sink for pair in m._folded.values() for t in pair]
        assert all(not bool(s.any()) for s in seen["sinks"])
        return outs

    outs, grads, g0 = module_run(piece, m, forward, arena, set(piece.params))
    assert all(bool(s.any()) for s in seen["sinks"])                              # the folded weights' gradients went through the sinks
    assert [bool(c.get("accumulate", False)) for c in spy.args("dyn_bmm_ln_relu_bwd")] == [arena] * 4
    assert [bool(c.get("accumulate", False)) for c in spy.args("layernorm_bwd")] == [arena] * 2
    masks = list(rec.masks)
    assert len(masks) == 4
    m.begin_clip(SinkPool())                                                     # the next clip: fresh, zero sinks
    m(dev(piece.tensors["pro0"]), dev(piece.tensors["roi0"]))
    fresh = [t._phnet_sink for pair in m._folded.values() for t in pair]
    assert all(not bool(f.any()) and f.data_ptr() != s.data_ptr() for f, s in zip(fresh, seen["sinks"]))
    rep = H.compare(piece, outs, grads, masks, g0=g0)
    print("\n" + rep.line(f"dynconv {piece.name} [{'arena' if arena else 'plain'}]"))
    assert not rep.bad, rep.bad


# ------------------------------------------------------------------------------------------------ Part 2: a branch of the head
@pytest.fixture(scope="module")
def detnet(K):
    """DetNetV2 of a model built at the tiny geometry with synth.make_state."""
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import DetNetV2
    g = H.TINY
    det = DetNetV2(cfg=make_cfg(img_h=g.img_h, img_w=g.img_w, arch=g.arch))
    det.load_state_dict(OrderedDict((k[len("detNet."):], v) for k, v in H.tiny_state().items() if k.startswith("detNet.")), strict=True)
    return det.cuda().train()


@pytest.mark.parametrize("arena", [False, True], ids=["plain", "arena"])
@pytest.mark.parametrize("sec", [False, True], ids=["fir", "sec"])
def test_branch_under_autograd(K, monkeypatch, detnet, sec, arena):
    """DetNetV2._branch (assembled towers -> three PF.linear -> lane_update) for `sec` False and True (C = 64 and 128), called
    twice per clip before one backward, through the device's tower masks; x columns judged against the row scale."""
    from phnet_amd.arena import SinkPool
    piece = H.branch_piece(sec)
    for p in detnet.parameters():
        p.grad = None
    rec = MaskRecorder(monkeypatch)
    spy = Spy(monkeypatch, K, ("tower_chain_fwd", "assemble_towers", "scatter_tower_grads", "linear_bwd"))
    priors = dev(piece.tensors["priors"])
    keys = dict(zip(H.branch_tower_keys(sec), H.tower_param_names()))

    def forward(leaves):
        detnet._branch_cache, detnet._sink_pool = None, SinkPool()
        outs = OrderedDict()
        for i in range(leaves["feat"].shape[0]):
            outs[f"preds{i}"], outs[f"lines{i}"] = detnet._branch(leaves["feat"][i][None], priors, sec)
        return outs

    try:
        outs, grads, g0 = module_run(piece, detnet, forward, arena, set(keys))
    finally:
        detnet._branch_cache = detnet._sink_pool = None
    assert spy.count("tower_chain_fwd") == 0 and spy.count("assemble_towers") == 1           # assembled once per clip
    assert [bool(c["accumulate"]) for c in spy.args("scatter_tower_grads")] == [arena]
    assert spy.count("linear_bwd") == 6                                          # three layers, two uses: into the assembled sinks
    grads = {keys.get(k, k): v for k, v in grads.items()}
    g0 = {keys[k]: v for k, v in g0.items()}
    rep = H.compare(piece, outs, grads, [m[0] for m in rec.masks], g0=g0)          # [1,N,3C] on the device, [N,3C] in the statement
    print("\n" + rep.line(f"branch {piece.name} [{'arena' if arena else 'plain'}]"))
    assert not rep.bad, rep.bad
