"""The hand-written encoder schedule (phnet_amd/trunk.py: 20 / 36 conv-BN records, BN-backward -> dgrad -> wgrad, the residual
gradient through the data-gradient addend, the neck's sums, the stem's un-padding, arena destinations) on a real MI355X against
fp64 autograd of tests/encoder_cases.py - every parameter, all entries.

The fp64 reference differentiates through the ReLU masks and max-pool winners read from the DEVICE tape (why: encoder_cases.py),
after those masks passed the mask conditions: a device unit may differ from fp64's own choice only where the fp64
pre-activation is within 1e-4 of its tensor's RMS of zero, in at most 32 units; a device pool winner holds the fp64 window
maximum to 1e-4 RMS.  The bound is not a constant: for every parameter p, with e32(p) the error of plain torch fp32 on the CPU
(the reference's own arithmetic at fp32, forced through ITS masks),

    e_hip(p) <= 4 * max(e32(p), median e32)            for ||g - g64|| / ||g64|| and for max|g - g64| / max|g64|

(4: split-K partials, BN sums from per-slab partials and the three-term bf16 split's dropped terms <= 2^-24 order the sums
differently from the CPU; the per-kernel tests grant the kernels 2e-5 where torch fp32 sits near 5e-6 - the same ratio).
The forward (P3-P5) and the BatchNorm running statistics are held by the same rule.

Each case runs in three arithmetics: "packed" (default bf16x3: conv3p forward and data gradient with addend), "generic"
(hip_ops.CONV3P off: conv2d_fwd(stats=True) / conv2d_dgrad in bf16x3) and "f32" (f32-input MFMA, no packed path).

Measured on an MI355X, parameter gradients, median / max over the 72 / 120 parameters; "torch fp32" is e32, the CPU stand-in:

    case            arithmetic   relative L2          entry-wise           P3-P5 L2   running stats   units off fp64's mask
    r18_64x160_T2   torch fp32   2.7e-6 / 5.4e-6      2.6e-6 / 8.8e-6      3.5e-6     6.1e-7          2 (|pre|/rms 1.7e-7)
                    packed       2.7e-6 / 5.8e-6      2.8e-6 / 6.5e-6      3.6e-6     6.3e-7          1 (1.3e-7)
                    generic      2.9e-6 / 6.2e-6      2.9e-6 / 7.6e-6      4.1e-6     6.8e-7          1 (1.3e-7)
                    f32          3.1e-6 / 6.1e-6      3.1e-6 / 1.1e-5      4.1e-6     6.8e-7          1 (1.3e-7)
                    arena, 2x    2.7e-6 / 5.8e-6
    r34_64x160_T3   torch fp32   5.5e-6 / 1.2e-5      5.6e-6 / 1.7e-5      9.1e-6     1.2e-6          2 (4.2e-6)
                    packed       5.6e-6 / 1.2e-5      5.3e-6 / 1.4e-5      8.6e-6     1.2e-6          1 (4.2e-6)
                    generic      5.9e-6 / 1.3e-5      5.5e-6 / 1.9e-5      9.3e-6     1.3e-6          1 (4.2e-6)
                    f32          6.8e-6 / 1.5e-5      7.0e-6 / 2.2e-5      1.1e-5     1.5e-6          1 (1.3e-6)
                    arena, 2x    5.6e-6 / 1.2e-5
    r18_80x176_T1   torch fp32   2.8e-6 / 4.8e-6      2.9e-6 / 6.3e-6      3.3e-6     6.4e-7          0
                    packed       2.8e-6 / 5.1e-6      2.9e-6 / 6.7e-6      3.2e-6     6.3e-7          0
                    generic      3.1e-6 / 5.3e-6      3.1e-6 / 8.3e-6      3.7e-6     7.1e-7          0
                    f32          3.4e-6 / 5.9e-6      3.4e-6 / 7.6e-6      3.8e-6     7.4e-7          0
                    arena, 2x    2.8e-6 / 5.1e-6

Every pool winner was fp64's own.  Eval mode (folded BatchNorm): P3-P5 8e-7 .. 1.1e-6
where torch fp32 gives 6e-7 .. 8e-7.  What the bound sees, measured by wrapping one hip_ops call of the r34 case: a residual
addend scaled by 0.999 on one block (conv1.weight 6.3e-4 against a bound of 2.2e-5), the addend dropped or the residual
gradient taken before the ReLU mask on one block (0.6), one BatchNorm's data gradient scaled by 1 + 1e-4 (6.3e-5).

Run with -m gpu.
"""
import functools

import pytest
import torch

from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

VARIANTS = ("packed", "generic", "f32")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops
    assert hip_ops.mma_mode() == 3 and hip_ops.CONV3P, "the suite runs in the default arithmetic"
    return hip_ops


def build_encoder(case):
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import Encoder
    enc = Encoder(make_cfg(img_h=case.img_h, img_w=case.img_w, arch=case.arch))
    enc.load_state_dict(E.encoder_state(case.arch), strict=True)
    return enc.cuda().train()


def nhwc_dev(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def nchw_cpu(t):
    return t.detach().permute(0, 3, 1, 2).contiguous().cpu()


def buffers_of(enc):
    return {k: v.detach().cpu().clone() for k, v in enc.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}


def staged_forward(enc, case):
    """One staged forward: (leaves, NCHW outputs on the host, ReLU masks, pool winners, [(record is 3x3 / stride 1, took the packed
    kernel)]) - the masks are read from the tape BEFORE the backward consumes it."""
    from phnet_amd import trunk
    enc.staged = True
    leaves = enc(E.frames(case).cuda())
    ctx, _ = enc._staged
    masks = E.masks_from_tape(ctx.tape)
    winners = E.winners_from_argmax(ctx.argmax, ctx.stem_shape[1:3])
    packed = [(trunk._is3x3s1(r.conv), r.packed is not None) for r in ctx.tape]
    return leaves, [nchw_cpu(l) for l in leaves], masks, winners, packed


class DeviceRun:
    """Staged forward + backward of a fresh encoder on the fixed cotangents."""

    def __init__(self, case):
        enc = build_encoder(case)
        leaves, self.outs, self.masks, self.winners, self.packed = staged_forward(enc, case)
        for l, c in zip(leaves, E.cotangents(case)):
            l.grad = nhwc_dev(c)
        self.fired = []
        enc.finish_backward(self.fired.append)
        torch.cuda.synchronize()
        assert enc._staged is None
        self.grads = {k: p.grad.detach().cpu() for k, p in enc.named_parameters()}
        self.buffers = buffers_of(enc)


@functools.lru_cache(maxsize=None)
def default_run(case) -> DeviceRun:
    """The default-arithmetic run, shared by the tests that compare another way in with it."""
    from phnet_amd import hip_ops
    assert hip_ops.mma_mode() == 3 and hip_ops.CONV3P
    return DeviceRun(case)


def held(errs, floors, what):
    """errs / floors: {name: error}.  e <= 4 * max(e32, median e32) for every entry."""
    b = E.bounds(floors)
    bad = {k: (v, b[k]) for k, v in errs.items() if not v <= b[k]}
    assert not bad, (what, bad)


def check_against_fp64(case, run: DeviceRun, label: str):
    """Mask conditions, forward, running statistics and every parameter gradient of `run` against the fp64 reference forced
    through the run's own masks, each by the 4x-of-the-fp32-floor rule."""
    floor = E.stand_in(case)
    ref = E.forced_reference(case, run.masks, run.winners)
    report = E.mask_report(ref.hooks, run.masks, run.winners)
    grads, ref_grads = run.grads, ref.grads
    e_l2 = {k: E.rel_l2(grads[k], g) for k, g in ref_grads.items()}
    e_max = {k: E.rel_max(grads[k], g) for k, g in ref_grads.items()}
    e_fwd = {i: E.rel_l2(a, b) for i, (a, b) in enumerate(zip(run.outs, ref.outs))}
    e_stats = {k: E.rel_l2(run.buffers[k], v) for k, v in ref.buffers.items() if v.is_floating_point()}
    print(f"\n{case.name} {label}: gradients relative L2 median / max {E.summary(e_l2)} (fp32 floor {E.summary(floor.e_l2)}), "
          f"entry-wise {E.summary(e_max)} (floor {E.summary(floor.e_max)}); forward {max(e_fwd.values()):.1e} "
          f"(floor {max(floor.e_fwd):.1e}); running statistics {max(e_stats.values()):.1e} (floor {max(floor.e_stats.values()):.1e}); "
          f"units off fp64's mask {report[0]} (|pre| / rms <= {report[1]:.1e}), pool gap {report[2]:.1e}")
    E.check_masks(report, f"{case.name} {label}")
    held(e_fwd, dict(enumerate(floor.e_fwd)), "forward")
    held(e_stats, floor.e_stats, "running statistics")
    for k, v in ref.buffers.items():
        if k.endswith("num_batches_tracked"):
            assert int(run.buffers[k]) == int(v) == 1, k
    bad = E.grad_violations(grads, ref_grads, floor.e_l2, floor.e_max)
    assert not bad, (case.name, label, bad)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_staged_backward_against_fp64(K, monkeypatch, case, variant):
    from phnet_amd import trunk
    if variant == "packed":
        run = default_run(case)
    else:
        try:
            if variant == "generic":
                monkeypatch.setattr(K, "CONV3P", False)
            else:
                K.set_mma_mode("f32")
            assert not trunk.packed_path()
            run = DeviceRun(case)
        finally:
            K.set_mma_mode(K.DEFAULT_MMA)
    # which kernels ran: the packed variant took the packed kernel for every 3x3 / stride-1 conv of layer1-layer4, the others for none
    n3 = sum(is3 for is3, _ in run.packed)
    blocks = sum(E.O.BLOCKS_PER_LAYER[case.arch])
    assert n3 == 2 * blocks - 3 and len(run.packed) == 2 * blocks + 4            # (three stride-2 conv1, three downsamples, the stem)
    assert [p for _, p in run.packed] == [is3 and variant == "packed" for is3, _ in run.packed]
    assert tuple(run.fired) == trunk.PARTS
    check_against_fp64(case, run, variant)


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_autograd_function_equals_staged(K, case):
    """EncoderFunction (what RouterOL.forward uses) runs the same schedule: same outputs, same gradients, bit for bit."""
    run = default_run(case)
    enc = build_encoder(case)
    frames = E.frames(case).cuda().requires_grad_(True)
    outs = enc(frames)
    assert enc._staged is None and all(o.requires_grad for o in outs)
    torch.autograd.backward(outs, [nhwc_dev(c) for c in E.cotangents(case)])
    torch.cuda.synchronize()
    assert frames.grad is None
    for o, s in zip(outs, run.outs):
        assert torch.equal(nchw_cpu(o), s)
    for k, p in enc.named_parameters():
        assert p.grad is not None and torch.equal(p.grad.cpu(), run.grads[k]), k
    assert all(torch.equal(v, run.buffers[k]) for k, v in buffers_of(enc).items())


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_train_mode_forward_without_grad(K, case):
    """Under no_grad in train mode: the training arithmetic without a tape - same outputs, running statistics moved once."""
    run = default_run(case)
    enc = build_encoder(case)
    with torch.no_grad():
        outs = enc(E.frames(case).cuda())
    torch.cuda.synchronize()
    assert not any(o.requires_grad for o in outs)
    for o, s in zip(outs, run.outs):
        assert torch.equal(nchw_cpu(o), s)
    got = buffers_of(enc)
    assert set(got) == set(run.buffers)
    for k, v in got.items():
        assert torch.equal(v, run.buffers[k]), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_arena_accumulates_two_passes(K, case):
    """Arena destinations (bn_back's param_accumulate, conv_wgrad_into(accumulate=True), the stem's add_): two staged passes
    without zeroing in between hold the sum of the two single-pass gradients - against the fp64 sum, by the same rule."""
    from phnet_amd.arena import GradArena
    run = default_run(case)
    enc = build_encoder(case)
    arena = GradArena(enc.parameters())
    try:
        lo, hi = arena.flat.data_ptr(), arena.flat.data_ptr() + arena.flat.numel() * 4
        for _ in range(2):
            leaves, outs, masks, winners, _ = staged_forward(enc, case)
            # the forward repeats bit for bit, so both passes differentiate through the masks of the shared run
            assert all(torch.equal(a, b) for a, b in zip(masks, run.masks)) and torch.equal(winners, run.winners)
            assert all(torch.equal(a, b) for a, b in zip(outs, run.outs))
            for l, c in zip(leaves, E.cotangents(case)):
                l.grad = nhwc_dev(c)
            enc.finish_backward()
        torch.cuda.synchronize()
        for k, p in enc.named_parameters():
            assert lo <= p.grad.data_ptr() < hi, k
        grads = {k: p.grad.detach().cpu() for k, p in enc.named_parameters()}
    finally:
        arena.release()
    floor = E.stand_in(case)
    ref = E.forced_reference(case, run.masks, run.winners)
    ref_sum = {k: 2.0 * g for k, g in ref.grads.items()}
    e_l2 = {k: E.rel_l2(grads[k], g) for k, g in ref_sum.items()}
    print(f"\n{case.name} arena, two passes: relative L2 median / max {E.summary(e_l2)} (fp32 floor {E.summary(floor.e_l2)})")
    bad = E.grad_violations(grads, ref_sum, floor.e_l2, floor.e_max)
    assert not bad, (case.name, bad)


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_eval_forward_against_fp64(K, case):
    """Eval mode: BatchNorm folded into the weights, one launch per block.  P3-P5 against the fp64 eval forward; a second call
    after one running_var changed in place sees the new statistic (the fold cache's key)."""
    enc = build_encoder(case).eval()
    frames = E.frames(case).cuda()
    key = E.TRUNK + "layer2.0.bn2.running_var"

    def compare(outs, what, var_key=None, scale=1.0):
        ref = E.eval_forward(case, torch.float64, var_key, scale)
        floor = [E.rel_l2(a, b) for a, b in zip(E.eval_forward(case, torch.float32, var_key, scale), ref)]
        errs = {i: E.rel_l2(nchw_cpu(o), r) for i, (o, r) in enumerate(zip(outs, ref))}
        print(f"\n{case.name} eval {what}: P3-P5 relative L2 {[f'{e:.1e}' for e in errs.values()]} (fp32 floor {[f'{e:.1e}' for e in floor]})")
        held(errs, dict(enumerate(floor)), f"eval forward {what}")
        return ref

    with torch.no_grad():
        outs = enc(frames)
        ref0 = compare(outs, "first call")
        before = buffers_of(enc)
        enc.backbone.model.layer2[0].bn2.running_var.mul_(4.0)
        outs2 = enc(frames)
        ref1 = compare(outs2, "after running_var * 4", key, 4.0)
    assert min(E.rel_l2(a, b) for a, b in zip(ref1, ref0)) > 1e-2             # the changed statistic is visible at every level
    after = buffers_of(enc)
    assert all(torch.equal(after[k], v) for k, v in before.items() if k != key)  # eval moves no statistic
