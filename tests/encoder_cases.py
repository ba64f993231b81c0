"""The encoder (ResNet trunk + FPN neck) as a plain torch statement with two hooks, for holding the hand-written schedule
of phnet_amd/trunk.py to fp64 autograd.  CPU only: nothing here touches the GPU; tests/test_encoder_backward_cpu.py proves
this harness on the CPU, tests/test_encoder_backward_gpu.py uses it against the device.

Why the hooks.  A train-mode encoder back-propagated in fp32 and in fp64 differs by 1e-3 .. 2e-2 per parameter whenever ONE
ReLU unit in a million sits close enough to zero to take the other branch in fp32 (train-mode BatchNorm over 10-40 samples
per channel in layer4 spreads the flipped unit over everything upstream), and whether a case has such a unit is a matter of
rounding.  Once the fp64 reference differentiates through the SAME ReLU masks and max-pool winners as the implementation
under test, fp32 arithmetic sits at 5e-6 (ResNet-18) / 1.4e-5 (ResNet-34) relative L2 per parameter.  So:

  * `Hooks.relu` runs free (own mask, recorded) or as "ReLU with a given backward mask": forward clamp(min=0), backward g * mask;
  * `Hooks.pool` (3x3 / stride 2 / pad 1) runs free (own winners, recorded) or back-propagates to given winner positions;
  * the fp64 pre-activation of every ReLU and the fp64 input of the pool are recorded, and `mask_report` / `check_masks` hold
    the forced masks to conditions that keep the forcing from hiding a forward bug: a forced unit may differ from the fp64
    run's own choice only where fp64 itself is within 1e-4 of the tensor's RMS of the decision boundary.

`run_encoder` mirrors libs/models/resnet.py:79-95, 293-307 and libs/models/fpn.py:109-163 (the statement of
oracle/phnet_cpu.py resnet_trunk / fpn_neck with the two hooks in place of F.relu / F.max_pool2d) over a state dict in the
dtype of its tensors; ReLUs are numbered in execution order (stem, then conv1 / block output of every basic block), which is
the order of the `relu=True` records on the device tape.
"""
import functools
import hashlib
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import phnet_cpu as O
from tests import synth

TRUNK = "backbone.model."                 # keys as seen from the Encoder module (the state dict's "backbone." prefix stripped)
NECK = "neck."
BN_MOMENTUM, BN_EPS = 0.1, 1e-5           # nn.BatchNorm2d defaults (resnet.py builds its norm layers with them)

# mask conditions (conditions, not tolerances; measured for torch fp32: <= 4.2e-6, <= 2 units, ties only)
MASK_NEAR = 1e-4                          # |fp64 pre-activation| / RMS of its tensor wherever a forced mask differs from fp64's own
MASK_MAX_UNITS = 32                       # such units per case
POOL_NEAR = 1e-4                          # (fp64 window maximum - fp64 value at the forced winner) / RMS of the pool's input
MARGIN = 4.0                              # error of the code under test <= MARGIN * max(e32(p), median e32)


@dataclass(frozen=True)
class Case:
    name: str
    arch: str
    img_h: int
    img_w: int
    T: int
    seed: int

    @property
    def geometry(self) -> O.Geometry:
        return O.Geometry(img_h=self.img_h, img_w=self.img_w, arch=self.arch)


CASES = (
    Case("r18_64x160_T2", "resnet18", 64, 160, 2, 3),
    Case("r34_64x160_T3", "resnet34", 64, 160, 3, 5),
    # odd maps 20x44 -> 10x22 -> 5x11 -> 3x6 and a non-integer nearest up-sampling 3x6 -> 5x11
    Case("r18_80x176_T1", "resnet18", 80, 176, 1, 3),
)
CASE_IDS = [c.name for c in CASES]


def _half(n: int, times: int) -> int:
    for _ in range(times):
        n = (n - 1) // 2 + 1
    return n


def level_shapes(case: Case):
    """NCHW shapes of P3, P4, P5."""
    return [(case.T, 64, _half(case.img_h, k), _half(case.img_w, k)) for k in (3, 4, 5)]


@functools.lru_cache(maxsize=None)
def encoder_state(arch: str) -> "OrderedDict[str, torch.Tensor]":
    """The encoder's part of synth.make_state, keyed as Encoder.state_dict() (fp32; shared between tests: never written to)."""
    sd = synth.make_state(O.Geometry(arch=arch))
    return OrderedDict((k[len("backbone."):], v) for k, v in sd.items() if k.startswith("backbone."))


@functools.lru_cache(maxsize=None)
def frames(case: Case) -> torch.Tensor:
    return synth.make_clip(case.geometry, case.T, seed=case.seed)


@functools.lru_cache(maxsize=None)
def cotangents(case: Case):
    """One fixed cotangent per output level (NCHW, fp64 holding fp32-representable values: every arithmetic sees the same numbers)."""
    gen = torch.Generator().manual_seed(20240 + case.seed)
    return tuple(torch.randn(s, dtype=torch.float64, generator=gen).float().double() for s in level_shapes(case))


def leaf_state(arch: str, dtype) -> Dict[str, torch.Tensor]:
    """A fresh copy of the state in `dtype`: every floating-point parameter a leaf, running statistics as plain buffers."""
    out = {}
    for k, v in encoder_state(arch).items():
        if not v.is_floating_point():
            out[k] = v.clone()
        elif k.endswith("running_mean") or k.endswith("running_var"):
            out[k] = v.to(dtype).clone()
        else:
            out[k] = v.to(dtype).clone().requires_grad_(True)
    return out


def param_names(sd) -> List[str]:
    return [k for k, v in sd.items() if v.is_floating_point() and v.requires_grad]


# ------------------------------------------------------------------------------------------------ the two hooks
class _MaskedReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return x.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask.to(g.dtype), None


class _RoutedPool(torch.autograd.Function):
    """Forward: the 3x3 / s2 / p1 window maximum.  Backward: every output's gradient goes to the given input position."""

    @staticmethod
    def forward(ctx, x, winners):
        ctx.save_for_backward(winners)
        ctx.in_shape = x.shape
        return F.max_pool2d(x, kernel_size=3, stride=2, padding=1)

    @staticmethod
    def backward(ctx, g):
        (winners,) = ctx.saved_tensors
        n, c, h, w = ctx.in_shape
        gx = g.new_zeros(n, c, h * w)
        gx.scatter_add_(2, winners.flatten(2), g.reshape(n, c, -1))
        return gx.view(n, c, h, w), None


class Hooks:
    """relu_masks: one bool NCHW tensor per ReLU in execution order, or None = free.  pool_winners: int64 [N,C,Ho,Wo] of
    positions iy * W + ix in the pool's input plane (the layout of F.max_pool2d(return_indices=True)), or None = free.
    After a run: `pre` (detached pre-activations), `masks` (the run's own pre > 0), `pool_in`, `winners` (the run's own)."""

    def __init__(self, relu_masks: Optional[Sequence[torch.Tensor]] = None, pool_winners: Optional[torch.Tensor] = None):
        self.given_masks, self.given_winners = relu_masks, pool_winners
        self.pre: List[torch.Tensor] = []
        self.masks: List[torch.Tensor] = []
        self.pool_in = None
        self.winners = None

    def relu(self, x):
        i = len(self.pre)
        self.pre.append(x.detach())
        self.masks.append(x.detach() > 0)
        if self.given_masks is None:
            return F.relu(x)
        assert self.given_masks[i].shape == x.shape, (i, self.given_masks[i].shape, x.shape)
        return _MaskedReLU.apply(x, self.given_masks[i])

    def pool(self, x):
        self.pool_in = x.detach()
        if self.given_winners is None:
            y, self.winners = F.max_pool2d(x, kernel_size=3, stride=2, padding=1, return_indices=True)
            return y
        with torch.no_grad():
            self.winners = F.max_pool2d(x, kernel_size=3, stride=2, padding=1, return_indices=True)[1]
        assert self.given_winners.shape == self.winners.shape
        return _RoutedPool.apply(x, self.given_winners)


# ------------------------------------------------------------------------------------------------ the network
class Run:
    """outs: (P3, P4, P5) NCHW; sd: the state the run used (running statistics moved when it trained); hooks: what it recorded."""

    def __init__(self, outs, sd, hooks):
        self.outs, self.sd, self.hooks = outs, sd, hooks

    def grads(self, cots) -> Dict[str, torch.Tensor]:
        names = param_names(self.sd)
        gs = torch.autograd.grad(self.outs, [self.sd[k] for k in names], [c.to(o.dtype) for c, o in zip(cots, self.outs)])
        return dict(zip(names, gs))


def run_encoder(sd: Dict[str, torch.Tensor], x: torch.Tensor, arch: str, training: bool, hooks: Optional[Hooks] = None) -> Run:
    """resnet.py:293-307 (stem, max-pool, four stages of resnet.py:79-95 basic blocks) + fpn.py:109-163 (layer1 dropped, 1x1
    laterals, nearest top-down add, 3x3 outputs).  Training: batch statistics, running statistics of `sd` tracked in place."""
    hooks = hooks or Hooks()

    def bn(key, t):
        y = F.batch_norm(t, sd[key + ".running_mean"], sd[key + ".running_var"], sd[key + ".weight"], sd[key + ".bias"],
                         training, BN_MOMENTUM, BN_EPS)
        if training:
            sd[key + ".num_batches_tracked"] += 1
        return y

    p = TRUNK
    x = F.conv2d(x, sd[p + "conv1.weight"], None, stride=2, padding=3)
    x = hooks.pool(hooks.relu(bn(p + "bn1", x)))
    stages = []
    for li, nblocks in enumerate(O.BLOCKS_PER_LAYER[arch]):
        for bi in range(nblocks):
            q = f"{p}layer{li + 1}.{bi}."
            stride = 2 if (li > 0 and bi == 0) else 1
            y = F.conv2d(x, sd[q + "conv1.weight"], None, stride=stride, padding=1)
            y = hooks.relu(bn(q + "bn1", y))
            y = bn(q + "bn2", F.conv2d(y, sd[q + "conv2.weight"], None, stride=1, padding=1))
            if (q + "downsample.0.weight") in sd:
                idn = bn(q + "downsample.1", F.conv2d(x, sd[q + "downsample.0.weight"], None, stride=stride))
            else:
                idn = x
            x = hooks.relu(y + idn)
        stages.append(x)
    feats = stages[-3:]
    lat = [F.conv2d(f, sd[f"{NECK}lateral_convs.{i}.conv.weight"], sd[f"{NECK}lateral_convs.{i}.conv.bias"]) for i, f in enumerate(feats)]
    for i in (2, 1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
    outs = tuple(F.conv2d(lat[i], sd[f"{NECK}fpn_convs.{i}.conv.weight"], sd[f"{NECK}fpn_convs.{i}.conv.bias"], padding=1)
                 for i in range(3))
    return Run(outs, sd, hooks)


def run_case(case: Case, dtype, training: bool = True, relu_masks=None, pool_winners=None, sd=None) -> Run:
    sd = leaf_state(case.arch, dtype) if sd is None else sd
    return run_encoder(sd, frames(case).to(dtype), case.arch, training, Hooks(relu_masks, pool_winners))


# ------------------------------------------------------------------------------------------------ cached references
class Reference:
    """A finished fp64 run: forward values, moved statistics, what the hooks recorded and the parameter gradients."""

    def __init__(self, run: Run, case: Case):
        self.outs = [o.detach() for o in run.outs]
        self.buffers = {k: v for k, v in run.sd.items() if not (v.is_floating_point() and v.requires_grad)}
        self.hooks = run.hooks
        self.grads = run.grads(cotangents(case))


def _digest(masks, winners) -> str:
    h = hashlib.sha1()
    for m in masks:
        h.update(m.contiguous().numpy().tobytes())
    h.update(winners.contiguous().numpy().tobytes())
    return h.hexdigest()


_FORCED: Dict[tuple, Reference] = {}


def forced_reference(case: Case, masks, winners) -> Reference:
    """fp64 forward / backward through the given ReLU masks and pool winners (computed once per distinct set of masks: the
    arithmetics under test mostly agree on them).  The result is shared: leave it unchanged."""
    key = (case.name, _digest(masks, winners))
    if key not in _FORCED:
        _FORCED[key] = Reference(run_case(case, torch.float64, relu_masks=masks, pool_winners=winners), case)
    return _FORCED[key]


@functools.lru_cache(maxsize=None)
def free_reference(case: Case) -> Reference:
    """Plain fp64 autograd: F.relu and F.max_pool2d with their own masks."""
    return Reference(run_case(case, torch.float64), case)


class StandIn:
    """Plain torch fp32 on the CPU, run free - the reference's own arithmetic at the precision of the code under test (never
    the code under test itself) - and its errors against the fp64 reference forced through ITS masks: the fp32 floor e32."""

    def __init__(self, case: Case):
        run = run_case(case, torch.float32)
        self.masks, self.winners = run.hooks.masks, run.hooks.winners
        self.outs = [o.detach() for o in run.outs]
        self.buffers = {k: v for k, v in run.sd.items() if not (v.is_floating_point() and v.requires_grad)}
        self.grads = run.grads(cotangents(case))
        self.ref = forced_reference(case, self.masks, self.winners)
        self.e_l2 = {k: rel_l2(g, self.ref.grads[k]) for k, g in self.grads.items()}
        self.e_max = {k: rel_max(g, self.ref.grads[k]) for k, g in self.grads.items()}
        self.e_fwd = [rel_l2(a, b) for a, b in zip(self.outs, self.ref.outs)]
        self.e_stats = {k: rel_l2(v, self.ref.buffers[k]) for k, v in self.buffers.items() if v.is_floating_point()}


@functools.lru_cache(maxsize=None)
def stand_in(case: Case) -> StandIn:
    return StandIn(case)


@functools.lru_cache(maxsize=None)
def eval_forward(case: Case, dtype, var_key: Optional[str] = None, var_scale: float = 1.0):
    """Eval-mode (running statistics) P3-P5 in `dtype`; var_key: one running_var multiplied by var_scale first."""
    sd = leaf_state(case.arch, dtype)
    if var_key is not None:
        sd[var_key] = sd[var_key] * var_scale
    with torch.no_grad():
        return [o.detach() for o in run_case(case, dtype, training=False, sd=sd).outs]


# ------------------------------------------------------------------------------------------------ error measures and bounds
def rel_l2(g: torch.Tensor, ref: torch.Tensor) -> float:
    """||g - ref|| / ||ref||"""
    return float((g.double() - ref).norm() / ref.norm())


def rel_max(g: torch.Tensor, ref: torch.Tensor) -> float:
    """max|g - ref| / max|ref|"""
    return float((g.double() - ref).abs().max() / ref.abs().max())


def median(values) -> float:
    return float(torch.tensor(list(values), dtype=torch.float64).median())


def bounds(e32: Dict[str, float]) -> Dict[str, float]:
    """MARGIN * max(e32(p), median e32): what the code under test may show where plain torch fp32 shows e32."""
    med = median(e32.values())
    return {k: MARGIN * max(v, med) for k, v in e32.items()}


def summary(errs: Dict[str, float]) -> str:
    return f"{median(errs.values()):.1e} / {max(errs.values()):.1e}"


def grad_violations(grads, ref_grads, floor_l2, floor_max):
    """[(parameter, measure, error, bound)] over every parameter, all entries, both measures."""
    assert set(grads) == set(ref_grads), set(grads) ^ set(ref_grads)
    b_l2, b_max = bounds(floor_l2), bounds(floor_max)
    bad = []
    for k, ref in ref_grads.items():
        assert grads[k].shape == ref.shape, (k, grads[k].shape, ref.shape)
        assert bool(torch.isfinite(grads[k]).all()), k
        e2, em = rel_l2(grads[k], ref), rel_max(grads[k], ref)
        if not e2 <= b_l2[k]:
            bad.append((k, "l2", e2, b_l2[k]))
        if not em <= b_max[k]:
            bad.append((k, "max", em, b_max[k]))
    return bad


# ------------------------------------------------------------------------------------------------ mask conditions
def mask_report(hooks: Hooks, masks, winners):
    """(units whose forced mask differs from the fp64 run's own, the largest |fp64 pre-activation| / RMS among them,
    the largest (fp64 window maximum - fp64 value at the forced winner) / RMS of the pool's input)."""
    assert len(masks) == len(hooks.pre), (len(masks), len(hooks.pre))
    units, worst = 0, 0.0
    for pre, own, m in zip(hooks.pre, hooks.masks, masks):
        assert m.shape == own.shape and m.dtype == torch.bool, (m.shape, own.shape, m.dtype)
        diff = own != m
        k = int(diff.sum())
        if k:
            units += k
            worst = max(worst, float(pre[diff].abs().max() / pre.pow(2).mean().sqrt()))
    x = hooks.pool_in
    n, c, h, w = x.shape
    assert winners.dtype == torch.int64 and int(winners.min()) >= 0 and int(winners.max()) < h * w
    # a winner lies inside its own 3x3 window
    oy = torch.arange(winners.shape[2]).view(-1, 1)
    ox = torch.arange(winners.shape[3]).view(1, -1)
    dy, dx = winners // w - (2 * oy - 1), winners % w - (2 * ox - 1)
    assert bool(((dy >= 0) & (dy <= 2) & (dx >= 0) & (dx <= 2)).all()), "pool winner outside its window"
    top = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    got = x.flatten(2).gather(2, winners.flatten(2)).view_as(top)
    gap = float((top - got).max() / x.pow(2).mean().sqrt())
    return units, worst, gap


def check_masks(report, what=""):
    units, worst, gap = report
    assert worst <= MASK_NEAR, (what, "a forced ReLU unit is not near zero in fp64", report)
    assert units <= MASK_MAX_UNITS, (what, "too many ReLU units differ from fp64", report)
    assert gap <= POOL_NEAR, (what, "a forced pool winner is not a maximum in fp64", report)


# ------------------------------------------------------------------------------------------------ from the device tape
def masks_from_tape(records) -> List[torch.Tensor]:
    """`relu=True` conv/BN records hold y = relu(...) in NHWC: y > 0 is the mask the backward kernels apply."""
    return [(r.y > 0).permute(0, 3, 1, 2).contiguous().cpu() for r in records if r.relu]


def winners_from_argmax(argmax: torch.Tensor, in_hw) -> torch.Tensor:
    """uint8 NHWC window slots r * 3 + q of phnet_maxpool3x3s2_fwd (input pixel (2 oy - 1 + r, 2 ox - 1 + q)) ->
    int64 NCHW positions iy * W + ix in the pool's input plane."""
    h, w = in_hw
    a = argmax.permute(0, 3, 1, 2).contiguous().cpu().long()
    assert int(a.max()) <= 8
    oy = torch.arange(a.shape[2]).view(-1, 1)
    ox = torch.arange(a.shape[3]).view(1, -1)
    iy, ix = 2 * oy - 1 + a // 3, 2 * ox - 1 + a % 3
    assert bool(((iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)).all()), "pool winner in the padding"
    return iy * w + ix


def nearest_source_index(out_size: int, in_size: int) -> torch.Tensor:
    """The source index rule of the top-down path's nearest up-sampling (csrc/norm.hip upsample_add_kernel)."""
    return torch.clamp((torch.arange(out_size) * in_size) // out_size, max=in_size - 1)
