"""Tensor-level wrappers over the C-ABI (include/phnet_hip.h): shape checks, output allocation, stream plumbing.

PyTorch is used here only for device memory and the current HIP stream.  No op in this file has a
fallback: a non-CUDA tensor or a missing library raises.
"""
import contextlib
import ctypes
import os
from typing import Optional, Tuple

import torch

from ._lib import check, lib

_WS = {}

# Optional kernel timer (bench.py): when TIMER is a list, every conv/linear GEMM launch is bracketed by two events on
# the launch stream and recorded as (kernel symbol, algorithmic FLOPs, start event, end event).
TIMER = None


def _kernel(query, *shape_args, has_splits=True):
    """(kernel symbol, split factor) of the launch entry with the same shape arguments, from the library's host-only
    phnet_*_kernel queries: the decision function that launches the kernel also names it."""
    name, splits = ctypes.create_string_buffer(96), ctypes.c_int32(0)
    check(query(*shape_args, name, len(name), *([ctypes.byref(splits)] if has_splits else [])), "kernel query")
    return name.value.decode(), splits.value


def _timed_launch(sym_fn, flops, launch, shape=None, nbytes=None):
    """Runs `launch()`.  With the timer on, also records (symbol, split-K factor, FLOPs, start event, end event, launch):
    bench.py re-launches the recorded closures in isolation inside small hipGraphs to get device-side durations that
    are free of host launch gaps (the event pair around a live eager launch includes them for microsecond kernels)."""
    if TIMER is None:
        return launch()
    sym, splits = sym_fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = launch()
    e1.record()
    TIMER.append((sym, splits, flops, e0, e1, launch, shape, nbytes))     # shape: ("fwd" | "dgrad" | "wgrad" | "linbwd", GEMM rows, cols, depth) for tests/tools/gemm_shapes.py; nbytes: algorithmic HBM bytes
    return out


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype=torch.float32, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA(HIP) tensor; phnet_amd has no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


_WS_RETIRED = []


def workspace_buffers() -> dict:
    """{(device index, slot): tensor} of the live scratch buffers (a copy: tests watch them for growth)."""
    return dict(_WS)


def workspace(nbytes: int, device, slot: int = 0) -> torch.Tensor:
    """Grow-only scratch buffer per (device, slot).  Kernels on one stream serialise, so sharing is safe.
    A buffer that is outgrown is RETIRED, never freed: a captured hipGraph may hold its address (split-K partials,
    BatchNorm partials, LayerNorm scratch), and handing that memory back to the caching allocator would let a later replay
    scribble over tensors that reuse it.  (A few MB per growth step, a handful of steps per process.)"""
    key = (torch.device(device).index, slot)
    cur = _WS.get(key)
    if cur is None or cur.numel() < nbytes:
        if cur is not None:
            _WS_RETIRED.append(cur)
        cur = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = cur
    return cur


# ------------------------------------------------------------------------------------------------ NMS
def lane_nms(rows: torch.Tensor, scores: torch.Tensor, thresh: float, top_k: int,
             counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """rows [K,5+S] or [F,K,5+S]; returns (keep, num_to_keep, parent) shaped like the reference's outputs."""
    _req(rows, name="rows"); _req(scores, name="scores")
    batched = rows.dim() == 3
    f = rows.shape[0] if batched else 1
    k, prop = rows.shape[-2], rows.shape[-1]
    if scores.numel() != f * k:
        raise RuntimeError("scores must have one entry per row")
    if counts is not None:
        _req(counts, torch.int32, "counts")
    keep = torch.empty((f, k), dtype=torch.int64, device=rows.device)
    parent = torch.empty((f, k), dtype=torch.int64, device=rows.device)
    num = torch.empty((f,), dtype=torch.int64, device=rows.device)
    check(lib().phnet_lane_nms(_ptr(rows), _ptr(scores), _ptr(counts), f, k, prop - 5, float(thresh), int(top_k),
                               _ptr(keep), _ptr(num), _ptr(parent), _stream()), "phnet_lane_nms")
    if batched:
        return keep, num, parent
    return keep[0], num[0], parent[0]


# ------------------------------------------------------------------------------------------------ ROI pooling
def roi_pool_fwd(fmap: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, with_cp: bool = False):
    """fmap [B,h,w,64] NHWC, xs [B,N,P], ys [P] -> [B,N,P,64] (and the [B,N,64,P] copy for the gate)."""
    _req(fmap, name="fmap"); _req(xs, name="xs"); _req(ys, name="ys")
    b, h, w, c = fmap.shape
    _, n, p = xs.shape
    out = torch.empty((b, n, p, c), dtype=torch.float32, device=fmap.device)
    out_cp = torch.empty((b, n, c, p), dtype=torch.float32, device=fmap.device) if with_cp else None
    check(lib().phnet_roi_pool_fwd(_ptr(fmap), _ptr(xs), _ptr(ys), _ptr(out), _ptr(out_cp), b, n, p, h, w, c, _stream()),
          "phnet_roi_pool_fwd")
    return (out, out_cp) if with_cp else out


def roi_pool_bwd(dout, fmap, xs, ys, dmap: Optional[torch.Tensor], need_dxs: bool):
    _req(dout, name="dout")
    b, h, w, c = fmap.shape
    _, n, p = xs.shape
    dxs = torch.empty_like(xs) if need_dxs else None
    check(lib().phnet_roi_pool_bwd(_ptr(dout), _ptr(fmap), _ptr(xs), _ptr(ys), _ptr(dmap), _ptr(dxs),
                                   b, n, p, h, w, c, _stream()), "phnet_roi_pool_bwd")
    return dxs


# ------------------------------------------------------------------------------------------------ conv / linear
def conv_out_hw(hi, wi, r, s, stride, pad):
    return (hi + 2 * pad - r) // stride + 1, (wi + 2 * pad - s) // stride + 1


def splitk_workspace_bytes(m: int, cols: int) -> int:
    """Split-K scratch every forward / data-gradient launch with an [m, cols] output is handed: room for 8 slabs of partial sums.
    The plan (csrc/conv.hip plan_conv) sees the size THIS shape asks for, not whatever the shared buffer has grown to - the same
    shape always runs the same plan, whatever ran before it in the process."""
    return 8 * m * cols * 4 if m * cols < (1 << 23) else 0


def conv2d_fwd(x, w, bias, stride: int, pad: int, relu: bool = False, out: Optional[torch.Tensor] = None,
               addend: Optional[torch.Tensor] = None, stats: bool = False):
    """x NHWC [N,Hi,Wi,Ci]; w OHWI [Co,R,S,Ci]; -> NHWC [N,Ho,Wo,Co].
    addend (shaped like the output): y = relu?(conv + bias + addend) in the kernel's epilogue.
    stats=True: also returns (partial, nblk) - per-channel (sum | sum of squares) partials of y written by the epilogue, for
    bn_fwd(..., partials=...): no separate statistics pass over y."""
    _req(x, name="x"); _req(w, name="w")
    n, hi, wi, ci = x.shape
    co, r, s, ci2 = w.shape
    assert ci == ci2, (x.shape, w.shape)
    ho, wo = conv_out_hw(hi, wi, r, s, stride, pad)
    if out is None:
        out = torch.empty((n, ho, wo, co), dtype=torch.float32, device=x.device)
    m, k = n * ho * wo, r * s * ci
    need = splitk_workspace_bytes(m, co)
    ws = workspace(need, x.device) if need else None
    part, nblk = None, 0
    if stats:
        nblk = int(lib().phnet_conv2d_stats_blocks(m, co, k, need))
        part = workspace(nblk * 2 * co * 4, x.device, 1)
    if addend is not None:
        _req(addend, name="addend")
        assert addend.shape == out.shape
    if addend is not None or stats:
        launch = lambda: check(lib().phnet_conv2d_fwd_fused(_ptr(x), _ptr(w), _ptr(bias), _ptr(addend), _ptr(out), _ptr(part), n, hi, wi,
                                                            ci, co, r, s, stride, pad, int(relu), _ptr(ws), need, _stream()),
                               "phnet_conv2d_fwd_fused")
    else:
        launch = lambda: check(lib().phnet_conv2d_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), n, hi, wi, ci, co, r, s, stride,
                                                      pad, int(relu), _ptr(ws), need, _stream()), "phnet_conv2d_fwd")
    _timed_launch(lambda: _kernel(lib().phnet_conv2d_kernel, 0, n, hi, wi, ci, co, r, s, stride, pad, need), 2.0 * m * co * k, launch,
                  shape=("fwd", m, co, k, r), nbytes=4.0 * (n * hi * wi * ci + m * co + co * k))
    return (out, (part, nblk)) if stats else out


def _forward_only(what: str) -> None:
    """The bf16 inference arithmetic has no backward: the library returns PHNET_ERR_ARG there, the wrappers say why."""
    if mma_mode() == MMA_MODES["bf16"]:
        raise RuntimeError(f'{what}: GEMM arithmetic mode "bf16" (phnet_tune_mma(4)) is forward-only; run the backward in the '
                           f'default "bf16x3" arithmetic')


def conv3p_applies(m: int, ca: int, nn: int) -> bool:
    return bool(lib().phnet_conv3p_applies(int(m), int(ca), int(nn)))


def conv3p_planes() -> int:
    """bf16 planes of the packed image phnet_conv3p_fwd takes in the current arithmetic: 1 in "bf16" (every weight rounded once), else 3."""
    return 1 if mma_mode() == MMA_MODES["bf16"] else 3


def conv3p_packed_bytes(co: int, ci: int, planes: int = 3) -> int:
    assert planes in (1, 3), planes
    return int(lib().phnet_conv3p_packed_bytes_bf16(co, ci) if planes == 1 else lib().phnet_conv3p_packed_bytes(co, ci))


def conv3p_pack(w: torch.Tensor, dgrad: bool, out: Optional[torch.Tensor] = None, planes: Optional[int] = None) -> torch.Tensor:
    """w OHWI [Co,3,3,Ci] f32 -> the packed operand of conv3p (bf16 planes in MFMA fragment order, csrc/conv3p.hip): three planes
    (the exact split), or ONE (planes=1: the image of the "bf16" arithmetic, a third of the bytes, forward packing only).
    planes=None: what the current arithmetic's conv3p takes."""
    _req(w, name="w")
    co, r, s_, ci = w.shape
    assert r == 3 and s_ == 3, w.shape
    planes = conv3p_planes() if planes is None else planes
    if planes == 1 and dgrad:
        raise RuntimeError('conv3p_pack: the one-plane image of arithmetic mode "bf16" has no data-gradient packing (forward-only)')
    nbytes = conv3p_packed_bytes(co, ci, planes)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    assert out.numel() >= nbytes and out.is_contiguous()
    if planes == 1:
        check(lib().phnet_conv3p_pack_bf16(_ptr(w), _ptr(out), co, ci, _stream()), "phnet_conv3p_pack_bf16")
    else:
        check(lib().phnet_conv3p_pack(_ptr(w), _ptr(out), co, ci, int(dgrad), _stream()), "phnet_conv3p_pack")
    return out


class Conv3pPackPlan:
    """The packed images (forward + data gradient) of a list of 3x3 weights in ONE buffer, refreshed by ONE launch
    (phnet_conv3p_pack_jobs): what a training step runs once before its first convolution.  The job table holds raw pointers:
    it is rebuilt when a weight has moved (`matches`)."""

    def __init__(self, weights, with_dgrad: bool = True, planes: int = 3):
        """weights: contiguous OHWI tensors [Co,3,3,Ci].  planes=1: one-plane images of the "bf16" arithmetic (forward only)."""
        dev = weights[0].device
        if planes == 1 and with_dgrad:
            raise RuntimeError('Conv3pPackPlan: the one-plane images of arithmetic mode "bf16" are forward-only (with_dgrad=False)')
        self.planes = planes
        self.ptrs = tuple(int(w.data_ptr()) for w in weights)
        sizes = [conv3p_packed_bytes(w.shape[0], w.shape[3], planes) for w in weights]
        kinds = (False, True) if with_dgrad else (False,)
        self.buf = torch.empty(sum(sizes) * len(kinds), dtype=torch.uint8, device=dev)
        self.images, rows, off, first = [], [], 0, 0
        for w, nbytes in zip(weights, sizes):
            _req(w, name="w")
            co, _, _, ci = w.shape
            per = {}
            for dg in kinds:
                ca, nn = (co, ci) if dg else (ci, co)
                assert ca % 16 == 0 and nn % 32 == 0, w.shape
                img = self.buf[off:off + nbytes]
                rows.append([int(w.data_ptr()), int(img.data_ptr()), co | (ci << 32), int(dg), first])
                first += 9 * (ca // 16) * (nn // 32) * 64
                off += nbytes
                per[dg] = img
            self.images.append(per)
        self.total = first
        self.jobs = torch.tensor(rows, dtype=torch.int64).to(dev)

    def matches(self, weights) -> bool:
        return self.ptrs == tuple(int(w.data_ptr()) for w in weights)

    def refresh(self):
        if self.planes == 1:
            check(lib().phnet_conv3p_pack_jobs_bf16(_ptr(self.jobs), self.jobs.shape[0], self.total, _stream()), "phnet_conv3p_pack_jobs_bf16")
            return
        check(lib().phnet_conv3p_pack_jobs(_ptr(self.jobs), self.jobs.shape[0], self.total, _stream()), "phnet_conv3p_pack_jobs")


def conv3p(x: torch.Tensor, packed: torch.Tensor, nn: int, dgrad: bool = False, bias=None, addend=None, relu: bool = False,
           stats: bool = False):
    """3x3 / stride 1 / pad 1 convolution (dgrad=False) or its data gradient (dgrad=True: x = dy) on packed weights.
    x NHWC [N,H,W,Ca] -> NHWC [N,H,W,nn]; stats as conv2d_fwd.  In the "bf16" arithmetic `packed` is the one-plane image
    (conv3p_pack(..., planes=1)) and there is no data gradient."""
    _req(x, name="x")
    if dgrad:
        _forward_only("conv3p(dgrad=True)")
    n, h, w_, ca = x.shape
    planes = conv3p_planes()
    assert packed.numel() >= 9 * ca * nn * 2 * planes, (packed.numel(), ca, nn, planes)
    out = torch.empty((n, h, w_, nn), dtype=torch.float32, device=x.device)
    m = n * h * w_
    need = splitk_workspace_bytes(m, nn)
    ws = workspace(need, x.device) if need else None
    part, nblk = None, 0
    if stats:
        nblk = int(lib().phnet_conv3p_stats_blocks(m, ca, nn, need))
        part = workspace(nblk * 2 * nn * 4, x.device, 1)
    if addend is not None:
        _req(addend, name="addend")
        assert addend.shape == out.shape
    _timed_launch(lambda: _kernel(lib().phnet_conv3p_kernel, m, ca, nn, need),
                  2.0 * m * nn * 9 * ca,
                  lambda: check(lib().phnet_conv3p_fwd(_ptr(x), _ptr(packed), _ptr(bias), _ptr(addend), _ptr(out), _ptr(part), n, h, w_, ca, nn,
                                                       int(relu), _ptr(ws), need, _stream()), "phnet_conv3p_fwd"),
                  shape=("dgrad" if dgrad else "fwd", m, nn, 9 * ca, 3),
                  nbytes=4.0 * m * (ca + nn) + 2.0 * planes * 9 * ca * nn + (4.0 * m * nn if addend is not None else 0.0))
    return (out, (part, nblk)) if stats else out


def conv2d_dgrad(dy, w, in_hw: Tuple[int, int], stride: int, pad: int, addend: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None):
    _req(dy, name="dy"); _req(w, name="w")
    _forward_only("conv2d_dgrad")
    n = dy.shape[0]
    co, r, s, ci = w.shape
    hi, wi = in_hw
    dx = torch.empty((n, hi, wi, ci), dtype=torch.float32, device=dy.device) if out is None else _req(out, name="out")
    assert dx.shape == (n, hi, wi, ci)
    m, k = n * hi * wi, r * s * co
    need = splitk_workspace_bytes(m, ci)
    ws = workspace(need, dy.device) if need else None
    _timed_launch(lambda: _kernel(lib().phnet_conv2d_kernel, 1, n, hi, wi, ci, co, r, s, stride, pad, need), 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * co * r * s * ci,
                  lambda: check(lib().phnet_conv2d_dgrad(_ptr(dy), _ptr(w), _ptr(addend), _ptr(dx), n, hi, wi, ci, co, r, s, stride,
                                                         pad, _ptr(ws), need, _stream()), "phnet_conv2d_dgrad"),
                  shape=("dgrad", m, ci, k, r), nbytes=4.0 * (dy.numel() + m * ci + co * r * s * ci))
    return dx


CONV3P = os.environ.get("PHNET_CONV3P", "1") != "0"           # packed-weight 3x3 kernel for the trunk / FPN forward and data gradient (trunk.packed_path); bench A/B switch


def conv2d_wgrad(dy, x, w_shape, stride: int, pad: int, dw: Optional[torch.Tensor] = None, accumulate: bool = False,
                 dbias: Optional[torch.Tensor] = None):
    """dW (and, when `dbias` is given, the bias gradient = column sums of dy) in one launch (+ reduce when split).
    `accumulate` applies to both destinations."""
    _req(dy, name="dy"); _req(x, name="x")
    _forward_only("conv2d_wgrad")
    n, hi, wi, ci = x.shape
    co, r, s, _ = w_shape
    if dw is None:
        dw = torch.empty((co, r, s, ci), dtype=torch.float32, device=x.device)
        assert not accumulate
    need = lib().phnet_conv2d_wgrad_workspace(n, hi, wi, ci, co, r, s, stride, pad)
    ws = workspace(need, x.device) if need else None
    ho, wo = conv_out_hw(hi, wi, r, s, stride, pad)
    _timed_launch(lambda: _kernel(lib().phnet_conv2d_wgrad_kernel, n, hi, wi, ci, co, r, s, stride, pad, int(dbias is not None), need),
                  2.0 * n * ho * wo * co * r * s * ci,
                  lambda: check(lib().phnet_conv2d_wgrad(_ptr(dy), _ptr(x), _ptr(dw), _ptr(dbias), n, hi, wi, ci, co, r, s, stride,
                                                         pad, int(accumulate), _ptr(ws), need, _stream()), "phnet_conv2d_wgrad"),
                  shape=("wgrad", co, r * s * ci, n * ho * wo, r), nbytes=4.0 * (dy.numel() + x.numel() + co * r * s * ci))
    return dw


def linear_fwd(x2d, w, bias, relu: bool = False):
    """x [M,K], w [N,K] -> [M,N] (= conv 1x1 on an [M,1,1,K] image)."""
    m, k = x2d.shape
    return conv2d_fwd(x2d.view(m, 1, 1, k), w.view(w.shape[0], 1, 1, k), bias, 1, 0, relu).view(m, w.shape[0])


def linear_dgrad(dy2d, w):
    m, n = dy2d.shape
    k = w.shape[1]
    return conv2d_dgrad(dy2d.view(m, 1, 1, n), w.view(n, 1, 1, k), (1, 1), 1, 0).view(m, k)


def linear_wgrad(dy2d, x2d, dw: Optional[torch.Tensor] = None, accumulate: bool = False, dbias: Optional[torch.Tensor] = None):
    m, n = dy2d.shape
    k = x2d.shape[1]
    out = conv2d_wgrad(dy2d.view(m, 1, 1, n), x2d.view(m, 1, 1, k), (n, 1, 1, k), 1, 0,
                       None if dw is None else dw.view(n, 1, 1, k), accumulate, dbias)
    return out.view(n, k)


def linear_bwd_fusable(m: int, k: int, n: int) -> bool:
    return bool(lib().phnet_linear_bwd_fusable(m, k, n))


def linear_bwd(dy2d, x2d, w, dw: torch.Tensor, dbias: Optional[torch.Tensor], accumulate: bool, relu_y: Optional[torch.Tensor] = None):
    """dx = dy @ w and dw (+)= dy.T @ x (+ dbias) in one launch (few-rows Linear layers); returns dx.
    relu_y: saved output of a layer that ended in a ReLU - dy is masked by relu_y > 0 inside the kernel."""
    _req(dy2d, name="dy"); _req(x2d, name="x"); _req(w, name="w"); _req(dw, name="dw")
    _forward_only("linear_bwd")
    m, n = dy2d.shape
    k = x2d.shape[1]
    dx = torch.empty((m, k), dtype=torch.float32, device=dy2d.device)
    _timed_launch(lambda: _kernel(lib().phnet_linear_bwd_kernel, m, k, n, int(relu_y is not None), has_splits=False), 4.0 * m * n * k,
                  lambda: check(lib().phnet_linear_bwd(_ptr(dy2d), _ptr(x2d), _ptr(w), _ptr(relu_y), _ptr(dx), _ptr(dw), _ptr(dbias), m, k, n,
                                                       int(accumulate), _stream()), "phnet_linear_bwd"), shape=("linbwd", m, n, k, 1))
    return dx


def nchw3_to_nhwc4(x):
    _req(x, name="frames")
    n, c, h, w = x.shape
    assert c == 3
    y = torch.empty((n, h, w, 4), dtype=torch.float32, device=x.device)
    check(lib().phnet_nchw3_to_nhwc4(_ptr(x), _ptr(y), n, h, w, _stream()), "phnet_nchw3_to_nhwc4")
    return y


def pad_channels(src2d, cd: int):
    _req(src2d, name="src")
    rows, cs = src2d.shape
    dst = torch.empty((rows, cd), dtype=torch.float32, device=src2d.device)
    check(lib().phnet_pad_channels(_ptr(src2d), _ptr(dst), rows, cs, cd, _stream()), "phnet_pad_channels")
    return dst


# ------------------------------------------------------------------------------------------------ BN / pool / FPN
def _partials(m, c, device, slot=1):
    nfloats = lib().phnet_channel_partials_size(m, c)
    return workspace(nfloats * 4, device, slot)


def bn_fwd(x, gamma, beta, running_mean, running_var, training: bool, eps: float, momentum: float,
           residual=None, relu: bool = True, partials=None):
    """x [..., C] NHWC conv output.  Returns (y, save_mean, save_invstd); stats tensors are None in eval.
    partials = (partial, nblk) from conv2d_fwd(..., stats=True): the batch statistics come from the convolution's epilogue."""
    _req(x, name="x")
    c = x.shape[-1]
    m = x.numel() // c
    dev = x.device
    scale = torch.empty(c, dtype=torch.float32, device=dev)
    shift = torch.empty(c, dtype=torch.float32, device=dev)
    sm = torch.empty(c, dtype=torch.float32, device=dev) if training else None
    si = torch.empty(c, dtype=torch.float32, device=dev) if training else None
    if training and partials is not None:
        check(lib().phnet_bn_finalize_partials(_ptr(partials[0]), int(partials[1]), m, c, eps, momentum, _ptr(gamma), _ptr(beta),
                                               _ptr(running_mean), _ptr(running_var), _ptr(sm), _ptr(si), _ptr(scale), _ptr(shift),
                                               _stream()), "phnet_bn_finalize_partials")
    else:
        part = _partials(m, c, dev) if training else None
        check(lib().phnet_bn_fwd_stats(_ptr(x), m, c, eps, momentum, _ptr(gamma), _ptr(beta), _ptr(running_mean),
                                       _ptr(running_var), _ptr(sm), _ptr(si), _ptr(scale), _ptr(shift), _ptr(part),
                                       int(training), _stream()), "phnet_bn_fwd_stats")
    y = torch.empty_like(x)
    check(lib().phnet_bn_apply(_ptr(x), _ptr(scale), _ptr(shift), _ptr(residual), _ptr(y), m, c, int(relu), _stream()),
          "phnet_bn_apply")
    return y, sm, si


def bn_bwd(dy, x, y, save_mean, save_invstd, gamma, relu: bool, dres: Optional[torch.Tensor] = None,
           dres_accumulate: bool = False, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None,
           param_accumulate: bool = False):
    """Returns (dx, dgamma, dbeta); writes/accumulates the residual-branch gradient into dres when given.
    dgamma/dbeta may be caller-provided destinations: overwritten, or added to with param_accumulate (gradient arena)."""
    _req(dy, name="dy")
    c = x.shape[-1]
    m = x.numel() // c
    dev = x.device
    dx = torch.empty_like(x)
    dgamma = torch.empty(c, dtype=torch.float32, device=dev) if dgamma is None else dgamma
    dbeta = torch.empty(c, dtype=torch.float32, device=dev) if dbeta is None else dbeta
    c12 = torch.empty(2, c, dtype=torch.float32, device=dev)
    part = _partials(m, c, dev)
    check(lib().phnet_bn_bwd(_ptr(dy), _ptr(x), _ptr(y), _ptr(save_mean), _ptr(save_invstd), _ptr(gamma), _ptr(dx),
                             _ptr(dres), _ptr(dgamma), _ptr(dbeta), _ptr(part), _ptr(c12[0]), _ptr(c12[1]),
                             m, c, int(relu), int(dres_accumulate), int(param_accumulate), _stream()), "phnet_bn_bwd")
    return dx, dgamma, dbeta


def bn_fwd_sync(x, gamma, beta, running_mean, running_var, eps: float, momentum: float, residual=None, relu: bool = True,
                group=None, partials=None):
    """Training-mode BatchNorm whose statistics span the ranks of `group` (nn.SyncBatchNorm, trainOL.py:141), without any
    host round trip: local fp64 (sum x, sum x^2, count) -> ONE all-reduce of 2C+1 doubles -> statistics of the union batch,
    running statistics, scale / shift on the device.  Returns (y, mean, invstd, count) with `count` a device view (fp64[1])
    of the reduced element count, which the backward reads on the device too."""
    from . import parallel
    _req(x, name="x")
    c = x.shape[-1]
    m = x.numel() // c
    dev = x.device
    stats = torch.empty(4, c, dtype=torch.float32, device=dev)          # mean, invstd, scale, shift
    sums = torch.empty(2 * c + 1, dtype=torch.float64, device=dev)
    if partials is not None and partials[0] is not None:                # (sum, sum of squares) partials from the conv epilogue
        check(lib().phnet_bn_partials_to_sums(_ptr(partials[0]), int(partials[1]), m, c, _ptr(sums), _stream()), "phnet_bn_partials_to_sums")
    else:
        part = _partials(m, c, dev)
        check(lib().phnet_bn_local_sums(_ptr(x), m, c, _ptr(part), _ptr(sums), _stream()), "phnet_bn_local_sums")
    parallel.allreduce_sum_(sums, group)
    check(lib().phnet_bn_finalize_sums(_ptr(sums), c, eps, momentum, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                       _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]), _ptr(stats[3]), _stream()), "phnet_bn_finalize_sums")
    y = torch.empty_like(x)
    check(lib().phnet_bn_apply(_ptr(x), _ptr(stats[2]), _ptr(stats[3]), _ptr(residual), _ptr(y), m, c, int(relu), _stream()),
          "phnet_bn_apply")
    return y, stats[0], stats[1], sums[2 * c:]


def bn_bwd_sync(dy, x, y, mean, invstd, gamma, relu: bool, count, dres: Optional[torch.Tensor] = None, group=None,
                dres_accumulate: bool = False, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None,
                param_accumulate: bool = False):
    """SyncBatchNorm backward: local (sum g*xhat, sum g) -> ONE all-reduce of 2C floats -> dx with the global means (count is
    the device scalar of the forward).  dgamma / dbeta stay LOCAL sums (the gradient averaging across ranks treats them like
    every other parameter gradient, as with torch.nn.SyncBatchNorm under DDP); they are written / added to the given
    destinations."""
    from . import parallel
    _req(dy, name="dy")
    c = x.shape[-1]
    m = x.numel() // c
    dev = x.device
    sums = torch.empty(2, c, dtype=torch.float32, device=dev)
    scratch = torch.empty(2, c, dtype=torch.float32, device=dev)
    part = _partials(m, c, dev)
    check(lib().phnet_bn_bwd_reduce(_ptr(dy), _ptr(x), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(sums), _ptr(part),
                                    _ptr(scratch[0]), _ptr(scratch[1]), m, c, int(relu), _stream()), "phnet_bn_bwd_reduce")
    if dgamma is None:
        dgamma, dbeta = sums[0].clone(), sums[1].clone()
    elif param_accumulate:
        dgamma.add_(sums[0]); dbeta.add_(sums[1])
    else:
        dgamma.copy_(sums[0]); dbeta.copy_(sums[1])
    parallel.allreduce_sum_(sums, group)
    dx = torch.empty_like(x)
    check(lib().phnet_bn_bwd_apply_sums(_ptr(dy), _ptr(x), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(sums), _ptr(count),
                                        _ptr(scratch[0]), _ptr(scratch[1]), _ptr(dx), _ptr(dres), m, c, int(relu),
                                        int(dres_accumulate), _stream()), "phnet_bn_bwd_apply_sums")
    return dx, dgamma, dbeta


def maxpool_fwd(x):
    _req(x, name="x")
    n, hi, wi, c = x.shape
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    y = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    arg = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
    check(lib().phnet_maxpool3x3s2_fwd(_ptr(x), _ptr(y), _ptr(arg), n, hi, wi, c, _stream()), "phnet_maxpool3x3s2_fwd")
    return y, arg


def maxpool_bwd(dy, arg, in_shape):
    n, hi, wi, c = in_shape
    dx = torch.empty(in_shape, dtype=torch.float32, device=dy.device)
    check(lib().phnet_maxpool3x3s2_bwd(_ptr(_req(dy)), _ptr(arg), _ptr(dx), n, hi, wi, c, _stream()), "phnet_maxpool3x3s2_bwd")
    return dx


def upsample_add_(fine, coarse):
    n, H, W, c = fine.shape
    _, h, w, _ = coarse.shape
    check(lib().phnet_upsample_add(_ptr(_req(fine)), _ptr(_req(coarse)), n, H, W, h, w, c, _stream()), "phnet_upsample_add")
    return fine


def upsample_add_bwd_(dfine, dcoarse):
    n, H, W, c = dfine.shape
    _, h, w, _ = dcoarse.shape
    check(lib().phnet_upsample_add_bwd(_ptr(_req(dfine)), _ptr(_req(dcoarse)), n, H, W, h, w, c, _stream()),
          "phnet_upsample_add_bwd")
    return dcoarse


def colsum(a2d, out: Optional[torch.Tensor] = None, accumulate: bool = False):
    _req(a2d, name="a")
    m, c = a2d.shape
    if out is None:
        out = torch.empty(c, dtype=torch.float32, device=a2d.device)
        accumulate = False
    ws = workspace(lib().phnet_colsum_workspace(m, c), a2d.device, 2)
    check(lib().phnet_colsum(_ptr(a2d), _ptr(out), m, c, int(accumulate), _ptr(ws), ws.numel(), _stream()), "phnet_colsum")
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm / gate
def layernorm_fwd(x, w, b, eps: float = 1e-5, res=None, relu: bool = False, save_stats: bool = True):
    """LayerNorm over the trailing w.numel() elements.  Returns (y, mean, rstd)."""
    _req(x, name="x")
    L = w.numel()
    rows = x.numel() // L
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    check(lib().phnet_layernorm_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(res), _ptr(y), _ptr(mean), _ptr(rstd), rows, L, eps,
                                    int(relu), _stream()), "phnet_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, y, w, mean, rstd, relu: bool, need_dres: bool = False,
                  dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None, accumulate: bool = False):
    """Returns (dx, dres or None, dw, db).  dw/db may be caller-provided [L] destinations (accumulated into when asked)."""
    _req(dy, name="dy")
    L = w.numel()
    rows = x.numel() // L
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if need_dres else None
    if dw is None:
        dw, db, accumulate = torch.empty_like(w), torch.empty_like(w), False
    ws = workspace(lib().phnet_layernorm_bwd_workspace(rows, L), x.device, 2)
    check(lib().phnet_layernorm_bwd(_ptr(dy), _ptr(x), _ptr(y), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dres),
                                    _ptr(dw), _ptr(db), rows, L, int(relu), int(accumulate), _ptr(ws), ws.numel(), _stream()),
          "phnet_layernorm_bwd")
    return dx, dres, dw, db


def dyn_bmm_ln_relu_fwd(x, w, gamma, beta, eps: float, save_stats: bool = True):
    """x [N,P,K], w [N,K,J] -> (y [N,P,J], stats [N,P,2] or None)."""
    _req(x, name="x"); _req(w, name="w")
    n, p, k = x.shape
    j = w.shape[2]
    if w.shape[0] != n or w.shape[1] != k or gamma.numel() != j:
        raise ValueError(f"dyn_bmm_ln_relu: x {tuple(x.shape)} / w {tuple(w.shape)} / gamma {tuple(gamma.shape)} mismatch")
    y = torch.empty((n, p, j), dtype=torch.float32, device=x.device)
    stats = torch.empty((n, p, 2), dtype=torch.float32, device=x.device) if save_stats else None
    check(lib().phnet_dyn_bmm_ln_relu_fwd(_ptr(x), _ptr(w), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(stats), n, p, k, j, eps, _stream()),
          "phnet_dyn_bmm_ln_relu_fwd")
    return y, stats


def dyn_bmm_ln_relu_bwd(dy, x, w, y, stats, gamma, eps: float, need_dx: bool = True,
                        dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None, accumulate: bool = False):
    """Returns (dx or None, dw, dgamma, dbeta)."""
    _req(dy, name="dy")
    n, p, k = x.shape
    j = w.shape[2]
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w)
    if dgamma is None:
        dgamma, dbeta, accumulate = torch.empty_like(gamma), torch.empty_like(gamma), False
    ws = workspace(n * 2 * j * 4, x.device, 2)
    check(lib().phnet_dyn_bmm_ln_relu_bwd(_ptr(dy), _ptr(x), _ptr(w), _ptr(y), _ptr(stats), _ptr(gamma), _ptr(dx), _ptr(dw),
                                          _ptr(dgamma), _ptr(dbeta), n, p, k, j, eps, int(accumulate), _ptr(ws), ws.numel(), _stream()),
          "phnet_dyn_bmm_ln_relu_bwd")
    return dx, dw, dgamma, dbeta


def dwconv3x3(x, w, bias, flip: bool = False):
    """x [N,C,P] planes, w [N,3,3] (or [N,1,3,3]), bias [N] or None."""
    _req(x, name="x"); _req(w, name="w")
    n, c, p = x.shape
    y = torch.empty_like(x)
    check(lib().phnet_dwconv3x3(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), n, c, p, int(flip), _stream()), "phnet_dwconv3x3")
    return y


def dwconv3x3_wgrad(dy, x, dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None, accumulate: bool = False):
    _req(dy, name="dy")
    n, c, p = x.shape
    if dw is None:
        dw = torch.empty((n, 1, 3, 3), dtype=torch.float32, device=x.device)
        db = torch.empty((n,), dtype=torch.float32, device=x.device)
        accumulate = False
    check(lib().phnet_dwconv3x3_wgrad(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), n, c, p, int(accumulate), _stream()),
          "phnet_dwconv3x3_wgrad")
    return dw, db


def relu_bwd(dy, y):
    _req(dy, name="dy")
    dx = torch.empty_like(dy)
    check(lib().phnet_relu_bwd(_ptr(dy), _ptr(y), _ptr(dx), dy.numel(), _stream()), "phnet_relu_bwd")
    return dx


def lane_assign(pred, tgt, img_w: int, img_h: int, want_cost: bool = False):
    """pred [N,6+S], tgt [L,6+S] -> (rows_by_col [L] i64, rows_sorted [L] i64, n_valid [] i32[, cost [N,L]])."""
    _req(pred, name="pred"); _req(tgt, name="tgt")
    n, w = pred.shape
    L = tgt.shape[0]
    rows = torch.empty(L, dtype=torch.int64, device=pred.device)
    srt = torch.empty(L, dtype=torch.int64, device=pred.device)
    nv = torch.empty((), dtype=torch.int32, device=pred.device)
    cost = torch.empty((n, L), dtype=torch.float32, device=pred.device) if want_cost else None
    check(lib().phnet_lane_assign(_ptr(pred), _ptr(tgt), n, L, w - 6, float(img_w), float(img_h), _ptr(rows), _ptr(srt),
                                  _ptr(nv), _ptr(cost), _stream()), "phnet_lane_assign")
    return (rows, srt, nv, cost) if want_cost else (rows, srt, nv)


def lane_assign_tokens(pred, tgt, img_w: int, img_h: int, feat, out):
    """lane_assign(pred, tgt) + memory_tokens(feat, matched anchors, out=out) in one launch; out = (tokens [L+1,E] view, valid bool [L+1]).
    Returns rows_sorted (i64[L], -1 padded)."""
    _req(pred, name="pred"); _req(tgt, name="tgt"); _req(feat, name="feat")
    n, w = pred.shape
    L = tgt.shape[0]
    e = feat.shape[-1]
    tokens, valid = out
    _req(tokens, name="tokens out")
    if tokens.numel() != (L + 1) * e or valid.numel() != L + 1 or valid.dtype != torch.bool or not valid.is_contiguous() or feat.numel() != n * e:
        raise ValueError("lane_assign_tokens: out buffers do not match (tokens [L+1,E] f32, valid [L+1] bool, contiguous)")
    rows = torch.empty(L, dtype=torch.int64, device=pred.device)
    srt = torch.empty(L, dtype=torch.int64, device=pred.device)
    check(lib().phnet_lane_assign_tokens(_ptr(pred), _ptr(tgt), n, L, w - 6, float(img_w), float(img_h), _ptr(rows), _ptr(srt), _ptr(feat), e,
                                         _ptr(tokens), _ptr(valid), _stream()), "phnet_lane_assign_tokens")
    return srt


def lane_assign_one2many(pred, tgt, img_w: int, img_h: int):
    """pred [N,6+S], tgt [L<=4,6+S] (all label rows, valid flag in column 1) -> (rows i64[16], cols i64[16], n i32[]): the
    (anchor, label row) pairs of dynamic_assign.assignOne2Many in the reference's order, -1 padded; no host sync."""
    _req(pred, name="pred"); _req(tgt, name="tgt")
    n, w = pred.shape
    rows = torch.empty(16, dtype=torch.int64, device=pred.device)
    cols = torch.empty(16, dtype=torch.int64, device=pred.device)
    cnt = torch.empty((), dtype=torch.int32, device=pred.device)
    check(lib().phnet_lane_assign_one2many(_ptr(pred), _ptr(tgt), n, tgt.shape[0], w - 6, float(img_w), float(img_h), _ptr(rows), _ptr(cols),
                                           _ptr(cnt), _stream()), "phnet_lane_assign_one2many")
    return rows, cols, cnt


def frame_loss_variant(variant: int, preds, gates, tgt, img_w, img_h, cls_w, reg_w, iou_w):
    """The loss4OL (variant 1) / loss4OLV2 (variant 2) criterion of one frame in two launches (csrc/loss_variants.hip).
    preds: 6 x [N,6+S], gates: 3 x [N], tgt [L,6+S] -> (loss [1], dpred [6,N,6+S], dgate [3,N], pair_rows [6,16] i64,
    pair_cols [6,16] i64, rows_sorted [6,L] i64)."""
    import ctypes
    for t in list(preds) + list(gates) + [tgt]:
        _req(t, name="loss input")
    n, w = preds[0].shape
    L = tgt.shape[0]
    dev = tgt.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dpred = torch.empty((6, n, w), dtype=torch.float32, device=dev)
    dgate = torch.empty((3, n), dtype=torch.float32, device=dev)
    prow = torch.empty((6, 16), dtype=torch.int64, device=dev)
    pcol = torch.empty((6, 16), dtype=torch.int64, device=dev)
    srt = torch.full((6, L), -1, dtype=torch.int64, device=dev)
    scratch = torch.empty(6 * n + 192, dtype=torch.float32, device=dev)
    P = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in preds])
    G = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in gates])
    D = (ctypes.c_void_p * 6)(*[dpred[i].data_ptr() for i in range(6)])
    check(lib().phnet_frame_loss_variant(int(variant), P, G, _ptr(tgt), n, L, w - 6, float(img_w), float(img_h), float(cls_w), float(reg_w),
                                         float(iou_w), _ptr(loss), D, _ptr(dgate), _ptr(prow), _ptr(pcol), _ptr(srt), _ptr(scratch),
                                         _stream()), "phnet_frame_loss_variant")
    return loss, dpred, dgate, prow, pcol, srt


def frame_loss(preds, gates, tgt, img_w, img_h, cls_w, reg_w, iou_w, liou_hw, liou_h, liou_w):
    """preds: 6 x [N,6+S] (branch A stages 0..2, branch B stages 0..2), gates: 3 x [N], tgt [L,6+S].
    Returns (loss [1], dpred [6,N,6+S], dgate [3,N], rows_by_col [6,L] i64, rows_sorted [6,L] i64)."""
    import ctypes
    for t in list(preds) + list(gates) + [tgt]:
        _req(t, name="loss input")
    n, w = preds[0].shape
    L = tgt.shape[0]
    dev = tgt.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dpred = torch.empty((6, n, w), dtype=torch.float32, device=dev)
    dgate = torch.empty((3, n), dtype=torch.float32, device=dev)
    rows = torch.empty((6, L), dtype=torch.int64, device=dev)
    srt = torch.empty((6, L), dtype=torch.int64, device=dev)
    scratch = torch.empty(6 * n + 12, dtype=torch.float32, device=dev)
    P = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in preds])
    G = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in gates])
    D = (ctypes.c_void_p * 6)(*[dpred[i].data_ptr() for i in range(6)])
    check(lib().phnet_frame_loss(P, G, _ptr(tgt), n, L, w - 6, float(img_w), float(img_h), float(cls_w), float(reg_w),
                                 float(iou_w), float(liou_hw), float(liou_h), float(liou_w), _ptr(loss), D, _ptr(dgate),
                                 _ptr(rows), _ptr(srt), _ptr(scratch), _ptr(scratch[6 * n:]), _stream()), "phnet_frame_loss")
    return loss, dpred, dgate, rows, srt


def clip_loss(preds, gates, tgt, img_w, img_h, cls_w, reg_w, iou_w, liou_hw, liou_h, liou_w):
    """frame_loss for the T frames of a clip in the same two launches.  preds: T x 6 x [N,6+S], gates: T x 3 x [N], tgt [T,L,6+S].
    Returns (loss [T], dpred [T,6,N,6+S], dgate [T,3,N], rows_by_col [T,6,L] i64, rows_sorted [T,6,L] i64)."""
    import ctypes
    T = len(preds)
    flat_p = [t for fr in preds for t in fr]
    flat_g = [t for fr in gates for t in fr]
    for t in flat_p + flat_g + [tgt]:
        _req(t, name="loss input")
    if len(flat_p) != 6 * T or len(flat_g) != 3 * T or tgt.shape[0] != T:
        raise ValueError("clip_loss: 6 predictions and 3 gates per frame, one label block per frame")
    n, w = flat_p[0].shape
    L = tgt.shape[1]
    dev = tgt.device
    loss = torch.empty(T, dtype=torch.float32, device=dev)
    dpred = torch.empty((T, 6, n, w), dtype=torch.float32, device=dev)
    dgate = torch.empty((T, 3, n), dtype=torch.float32, device=dev)
    rows = torch.empty((T, 6, L), dtype=torch.int64, device=dev)
    srt = torch.empty((T, 6, L), dtype=torch.int64, device=dev)
    scratch = torch.empty(T * (6 * n + 12), dtype=torch.float32, device=dev)
    P = (ctypes.c_void_p * (6 * T))(*[t.data_ptr() for t in flat_p])
    G = (ctypes.c_void_p * (3 * T))(*[t.data_ptr() for t in flat_g])
    D = (ctypes.c_void_p * (6 * T))(*[dpred[f, i].data_ptr() for f in range(T) for i in range(6)])
    check(lib().phnet_clip_loss(P, G, _ptr(tgt), T, n, L, w - 6, float(img_w), float(img_h), float(cls_w), float(reg_w),
                                float(iou_w), float(liou_hw), float(liou_h), float(liou_w), _ptr(loss), D, _ptr(dgate),
                                _ptr(rows), _ptr(srt), _ptr(scratch), _ptr(scratch[T * 6 * n:]), _stream()), "phnet_clip_loss")
    return loss, dpred, dgate, rows, srt


def lane_update_fwd(priors, head, ys, img_w, img_h):
    """priors [N,6+S], head [N,HW] -> (preds, lines) [N,6+S]."""
    _req(priors, name="priors"); _req(head, name="head")
    n, w = priors.shape
    preds, lines = torch.empty_like(priors), torch.empty_like(priors)
    check(lib().phnet_lane_update_fwd(_ptr(priors), _ptr(head), _ptr(ys), _ptr(preds), _ptr(lines), n, w - 6, head.shape[1],
                                      float(img_w), float(img_h), _stream()), "phnet_lane_update_fwd")
    return preds, lines


def lane_update_bwd(dpreds, dlines, lines, head, ys, img_w, img_h, need_dpriors: bool):
    n, w = lines.shape
    dhead = torch.empty_like(head)
    dpriors = torch.empty_like(lines) if need_dpriors else None
    check(lib().phnet_lane_update_bwd(_ptr(dpreds), _ptr(dlines), _ptr(lines), _ptr(head), _ptr(ys), _ptr(dhead), _ptr(dpriors),
                                      n, w - 6, head.shape[1], float(img_w), float(img_h), _stream()), "phnet_lane_update_bwd")
    return dhead, dpriors


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def gate_stack_fwd(x, params, eps: float, save: bool, anchors: Optional[int] = None):
    """x [N,C,P] (N a multiple of `anchors`: planes of several frames); params: the 34 tensors in the C-ABI order.
    Returns (out, saved or None)."""
    _req(x, name="x")
    n, c, p = x.shape
    anchors = n if anchors is None else anchors
    out = torch.empty_like(x)
    saved = torch.empty(lib().phnet_gate_stack_saved_floats(n, c, p), dtype=torch.float32, device=x.device) if save else None
    check(lib().phnet_gate_stack_fwd(_ptr(x), _ptr_array(params), _ptr(out), _ptr(saved), n, anchors, c, p, eps, _stream()),
          "phnet_gate_stack_fwd")
    return out, saved


def gate_stack_bwd(gout, x, out, params, saved, grads, eps: float, accumulate: bool, anchors: Optional[int] = None):
    _req(gout, name="gout")
    n, c, p = x.shape
    anchors = n if anchors is None else anchors
    ws = workspace(lib().phnet_gate_stack_bwd_workspace(n, c, p), x.device, 3)
    check(lib().phnet_gate_stack_bwd(_ptr(gout), _ptr(x), _ptr(out), _ptr_array(params), _ptr(saved), _ptr_array(grads),
                                     n, anchors, c, p, eps, int(accumulate), _ptr(ws), ws.numel(), _stream()), "phnet_gate_stack_bwd")


def _rng_args(rng, width: int = 0):
    """rng = None | (state int64[1] device tensor, site id, drop probability[, item0, item_rows]) -> the three C arguments.
    Items (csrc/common.h): item0 = number of the first item of this launch, item_rows = rows per item when the launch covers a
    batch of items (0: the launch is one item); packed into the 64-bit call argument as site | item0 << 20 | item_elems << 32
    with item_elems = item_rows * width (width = elements per row of the tensor the mask is drawn for)."""
    if rng is None:
        return None, 0, 0.0
    state, call, p = rng[:3]
    item0, item_rows = (rng[3], rng[4]) if len(rng) > 3 else (0, 0)
    elems = int(item_rows) * int(width)
    assert 0 <= call < (1 << 20) and 0 <= item0 < (1 << 12) and 0 <= elems < (1 << 32), (call, item0, elems)
    return _ptr(state), int(call) | (int(item0) << 20) | (elems << 32), float(p)


def attention_fwd(q, k, v, heads: int, key_valid=None, keep=None, keep_scale: float = 1.0, rng=None, batch: int = 1):
    """q [Lq,E], k/v [Lk,E] (any row stride, unit column stride) -> (o [Lq,E], lse [H,Lq]).  Dropout of the attention
    weights: explicit `keep` u8[H,Lq,Lk] (+ keep_scale), or `rng` for the in-kernel counter-based mask."""
    e = q.shape[1]
    lq, lk = q.shape[0] // batch, k.shape[0] // batch          # `batch` clips: contiguous row blocks of q and of k / v
    assert q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1 and q.shape[0] == lq * batch and k.shape[0] == lk * batch
    out = torch.empty((lq * batch, e), dtype=torch.float32, device=q.device)
    lse = torch.empty((batch * heads, lq), dtype=torch.float32, device=q.device)
    check(lib().phnet_attention_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(key_valid), _ptr(keep), _ptr(out), _ptr(lse), batch, lq, lk, heads, e,
                                    q.stride(0), k.stride(0), v.stride(0), out.stride(0), float(keep_scale), *_rng_args(rng), _stream()),
          "phnet_attention_fwd")
    return out, lse


def attention_bwd(q, k, v, o, dout, lse, heads: int, dq, dk, dv, key_valid=None, keep=None, keep_scale: float = 1.0, rng=None,
                  batch: int = 1):
    """Writes dq/dk/dv (views with arbitrary row stride)."""
    e = q.shape[1]
    lq, lk = q.shape[0] // batch, k.shape[0] // batch
    check(lib().phnet_attention_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(dout), _ptr(lse), _ptr(key_valid), _ptr(keep),
                                    _ptr(dq), _ptr(dk), _ptr(dv), batch, lq, lk, heads, e, q.stride(0), k.stride(0), v.stride(0),
                                    o.stride(0), dq.stride(0), dk.stride(0), dv.stride(0), float(keep_scale), *_rng_args(rng),
                                    _stream()), "phnet_attention_bwd")


def memory_tokens(feat, rows, out=None):
    """feat [N,E] / [N,1,E] with rows i64[L] (-1 padded) -> (tokens [L+1,1,E], valid bool[L+1]); or a batch of clips:
    feat [B,N,E] with rows i64[B,L] -> (tokens [B,L+1,E], valid bool[B,L+1]).  One launch.  out = (tokens, valid): write into
    caller-provided contiguous tensors (a slot of a ring buffer) instead of allocating."""
    _req(feat, name="feat"); _req(rows, torch.int64, "rows")
    batched = rows.dim() == 2
    b = rows.shape[0] if batched else 1
    l, e = rows.shape[-1], feat.shape[-1]
    n = feat.numel() // (b * e)
    if out is not None:
        tokens, valid = out
        _req(tokens, name="tokens out")
        if tokens.numel() != b * (l + 1) * e or valid.numel() != b * (l + 1) or valid.dtype != torch.bool or not valid.is_contiguous():
            raise ValueError("memory_tokens: out buffers do not match (tokens [..,L+1,E] f32, valid [..,L+1] bool, contiguous)")
    else:
        tokens = torch.empty((b, l + 1, e) if batched else (l + 1, 1, e), dtype=torch.float32, device=feat.device)
        valid = torch.empty((b, l + 1) if batched else (l + 1,), dtype=torch.bool, device=feat.device)
    check(lib().phnet_memory_tokens(_ptr(feat), _ptr(rows), _ptr(tokens), _ptr(valid), b, n, e, l, _stream()), "phnet_memory_tokens")
    return tokens, valid


def _stream_dims(ring, ring_valid, n, cursor):
    """(S, B, W, L, E) of a token ring [S,B,W,L+1,E] after checking the state tensors that go with it."""
    _req(ring, name="ring"); _req(n, torch.int32, "n"); _req(cursor, torch.int32, "cursor")
    if ring.dim() != 5:
        raise ValueError("stream: ring must be [S,B,W,L+1,E]")
    s, b, w, l1, e = ring.shape
    if (ring_valid.dtype != torch.bool or not ring_valid.is_contiguous() or tuple(ring_valid.shape) != (s, b, w, l1)
            or n.numel() != b or cursor.numel() != b or l1 < 2):
        raise ValueError("stream: ring_valid must be bool [S,B,W,L+1] (contiguous), n and cursor int32 [B], L >= 1")
    return s, b, w, l1 - 1, e


def stream_window(ring, ring_valid, n, cursor, out=None):
    """The memory the next frame of every stream attends to, in logical order (oldest first, empty slots last and invalid):
    (window [S,B,W*(L+1),E], window_valid bool [S,B,W*(L+1)], has_memory bool [B]).  Publishes cursor = n.  One launch."""
    s, b, w, l, e = _stream_dims(ring, ring_valid, n, cursor)
    m = w * (l + 1)
    if out is not None:
        window, valid, has = out
        _req(window, name="window out")
        if (tuple(window.shape) != (s, b, m, e) or valid.dtype != torch.bool or has.dtype != torch.bool or not valid.is_contiguous()
                or not has.is_contiguous() or tuple(valid.shape) != (s, b, m) or has.numel() != b):
            raise ValueError("stream_window: out = (window [S,B,W*(L+1),E] f32, window_valid bool [S,B,W*(L+1)], has_memory bool [B])")
    else:
        window = torch.empty((s, b, m, e), dtype=torch.float32, device=ring.device)
        valid = torch.empty((s, b, m), dtype=torch.bool, device=ring.device)
        has = torch.empty((b,), dtype=torch.bool, device=ring.device)
    check(lib().phnet_stream_window(_ptr(ring), _ptr(ring_valid), _ptr(n), _ptr(cursor), _ptr(window), _ptr(valid), _ptr(has),
                                    s, b, w, e, l, _stream()), "phnet_stream_window")
    return window, valid, has


def stream_push(feat, anchors_sorted, ring, ring_valid, n, cursor):
    """feat [S,B,N,E] and anchors_sorted i64[B,L] (-1 padded) -> the memory entry of this frame (memory_tokens of every stage and
    stream) in ring slot cursor % W, then n = cursor + 1.  One launch; needs a stream_window since the last push."""
    s, b, w, l, e = _stream_dims(ring, ring_valid, n, cursor)
    _req(feat, name="feat"); _req(anchors_sorted, torch.int64, "anchors_sorted")
    if feat.dim() != 4 or feat.shape[0] != s or feat.shape[1] != b or feat.shape[3] != e or tuple(anchors_sorted.shape) != (b, l):
        raise ValueError(f"stream_push: feat {tuple(feat.shape)} / anchors {tuple(anchors_sorted.shape)} vs ring {tuple(ring.shape)}")
    check(lib().phnet_stream_push(_ptr(feat), _ptr(anchors_sorted), _ptr(ring), _ptr(ring_valid), _ptr(cursor), _ptr(n),
                                  s, b, w, feat.shape[2], e, l, _stream()), "phnet_stream_push")


def stream_select(attn, has_memory, feat):
    """feat[b] = attn[b] (both [B,N,E]) for the streams with has_memory[b] == False, in place; returns feat.  One launch."""
    _req(attn, name="attn"); _req(feat, name="feat")
    if attn.dim() != 3 or attn.shape != feat.shape or has_memory.dtype != torch.bool or has_memory.numel() != attn.shape[0] \
            or not has_memory.is_contiguous() or has_memory.device != attn.device:
        raise ValueError("stream_select: attn / feat [B,N,E] f32 and has_memory bool [B] expected")
    check(lib().phnet_stream_select(_ptr(attn), _ptr(has_memory), _ptr(feat), attn.shape[0], attn.shape[1], attn.shape[2], _stream()),
          "phnet_stream_select")
    return feat


def stream_keys(local, pos, window, window_valid, cursor, min_frames: int, tgt=None, out=None):
    """Key set of the Router4OLV2 cross-frame decoder for one stage of B streams (csrc/stream_v2.hip): local [B,N,E], pos [N,E],
    window [B,M,E] / window_valid bool [B,M] (one stage of stream_window's output), cursor int32 [B] ->
    (tgt = local + pos [B,N,E], keys [B,Kmax,E], keys_valid bool [B,Kmax]), Kmax = max(N, M).  A stream with
    0 < cursor >= min_frames gets its window (then zero / invalid rows), the others their own tgt rows, valid (then zero /
    invalid).  tgt / out = (keys, keys_valid): caller-provided buffers.  One launch."""
    _req(local, name="local"); _req(pos, name="pos"); _req(window, name="window"); _req(cursor, torch.int32, "cursor")
    if local.dim() != 3 or window.dim() != 3:
        raise ValueError("stream_keys: local [B,N,E] and window [B,M,E] expected")
    b, n, e = local.shape
    m = window.shape[1]
    if (tuple(pos.shape) != (n, e) or window.shape[0] != b or window.shape[2] != e or window_valid.dtype != torch.bool
            or tuple(window_valid.shape) != (b, m) or not window_valid.is_contiguous() or window_valid.device != local.device
            or cursor.numel() != b or int(min_frames) < 0):
        raise ValueError(f"stream_keys: local {tuple(local.shape)} vs pos {tuple(pos.shape)} / window {tuple(window.shape)} / "
                         f"window_valid {tuple(window_valid.shape)} / cursor {tuple(cursor.shape)}, min_frames {min_frames}")
    kmax = max(n, m)
    if tgt is None:
        tgt = torch.empty_like(local)
    else:
        _req(tgt, name="tgt out")
        if tgt.shape != local.shape:
            raise ValueError("stream_keys: tgt must be [B,N,E] like local")
    if out is None:
        keys = torch.empty((b, kmax, e), dtype=torch.float32, device=local.device)
        valid = torch.empty((b, kmax), dtype=torch.bool, device=local.device)
    else:
        keys, valid = out
        _req(keys, name="keys out")
        if (keys.dim() != 3 or keys.shape[0] != b or keys.shape[1] < kmax or keys.shape[2] != e or valid.dtype != torch.bool
                or not valid.is_contiguous() or valid.device != local.device or tuple(valid.shape) != tuple(keys.shape[:2])):
            raise ValueError("stream_keys: out = (keys [B,Kmax,E] f32, keys_valid bool [B,Kmax]) with Kmax >= max(N, M)")
    check(lib().phnet_stream_keys(_ptr(local), _ptr(pos), _ptr(window), _ptr(window_valid), _ptr(cursor), _ptr(tgt), _ptr(keys),
                                  _ptr(valid), b, n, m, keys.shape[1], e, int(min_frames), _stream()), "phnet_stream_keys")
    return tgt, keys, valid


def gate_tail_fwd(h, w, b):
    _req(h, name="h"); _req(w, name="w"); _req(b, name="b")
    n, k = h.shape
    if w.numel() != k or b.numel() != 1:
        raise ValueError(f"gate_tail: h {tuple(h.shape)} vs w {tuple(w.shape)} / b {tuple(b.shape)}")
    out = torch.empty((n,), dtype=torch.float32, device=h.device)
    check(lib().phnet_gate_tail_fwd(_ptr(h), _ptr(w), _ptr(b), _ptr(out), n, k, _stream()), "phnet_gate_tail_fwd")
    return out


def gate_tail_bwd(dout, out, h, w, need_dh: bool = True, dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None,
                  accumulate: bool = False):
    _req(dout, name="dout")
    n, k = h.shape
    dh = torch.empty_like(h) if need_dh else None
    if dw is None:
        dw = torch.empty((k,), dtype=torch.float32, device=h.device)
        db = torch.empty((1,), dtype=torch.float32, device=h.device)
        accumulate = False
    check(lib().phnet_gate_tail_bwd(_ptr(dout), _ptr(out), _ptr(h), _ptr(w), _ptr(dh), _ptr(dw), _ptr(db), n, k, int(accumulate),
                                    _stream()), "phnet_gate_tail_bwd")
    return dh, dw, db


def blend_priors(gate, a, b, idx):
    """gate [N] (or [1,N,1]), a/b [1,N,W], idx i64[P] -> (priors [1,N,W], on_map [1,N,P])."""
    _req(gate, name="gate"); _req(a, name="lines_a"); _req(b, name="lines_b"); _req(idx, torch.int64, "idx")
    w = a.shape[-1]
    n = a.numel() // w                                   # all leading dimensions are rows (frames / clips x anchors)
    p = idx.numel()
    priors = torch.empty_like(a)
    on_map = torch.empty(a.shape[:-1] + (p,), dtype=torch.float32, device=a.device)
    check(lib().phnet_blend_priors(_ptr(gate), _ptr(a), _ptr(b), _ptr(idx), _ptr(priors), _ptr(on_map), n, w, p, _stream()),
          "phnet_blend_priors")
    return priors, on_map


def adamw_step(p, g, m, v, n_decay: int, step, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, lr_dev=None):
    """In-place AdamW over flat fp32 buffers (all the same length, a multiple of 4); step = int64[1] device tensor.
    lr_dev (optional float32[1] device tensor) replaces `lr` (read on the device: capturable LR schedules)."""
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, name=name)
    _req(step, torch.int64, "step")
    if not (p.numel() == g.numel() == m.numel() == v.numel()):
        raise ValueError("adamw_step: p/g/m/v lengths differ")
    if lr_dev is not None:
        _req(lr_dev, name="lr_dev")
    check(lib().phnet_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), int(n_decay), _ptr(step), float(lr), _ptr(lr_dev),
                                 float(beta1), float(beta2), float(eps), float(weight_decay), _stream()), "phnet_adamw_step")


GUARD_CHUNK = 131072             # PHNET_GUARD_CHUNK of include/phnet_hip.h: elements per chunk partial of the guard's reduction
GUARD_WS_BYTES_PER_CHUNK = 12    # PHNET_GUARD_WS_BYTES_PER_CHUNK: one float64 partial and one uint32 count
GUARD_STATS_WORDS = 4            # PHNET_GUARD_STATS_WORDS: {f32 norm, f32 mult} | last step skipped | non-finite count | skipped steps
GUARD_SKIP_NONFINITE, GUARD_CLIP = 1, 2


def grad_guard_workspace_bytes(n: int) -> int:
    """Bytes of workspace phnet_grad_guard needs for an arena of n elements."""
    return GUARD_WS_BYTES_PER_CHUNK * max(1, -(-int(n) // GUARD_CHUNK))


def grad_guard(g, workspace, stats, step, max_norm: Optional[float], skip_nonfinite: bool, grad_scale=None, found_inf=None):
    """Rules 1-7 of the guarded step (include/phnet_hip.h) over the flat gradient buffer g, on the device: writes
    stats (int64[GUARD_STATS_WORDS]) and advances step (int64[1]) unless the step is to be skipped.  g is only read.
    workspace: uint8 tensor of >= grad_guard_workspace_bytes(g.numel()); grad_scale / found_inf: float32 scalars on the
    device as torch.amp.GradScaler hands them over, or None."""
    _req(g, name="g"); _req(workspace, torch.uint8, "workspace"); _req(stats, torch.int64, "stats"); _req(step, torch.int64, "step")
    if stats.numel() != GUARD_STATS_WORDS or step.numel() != 1:
        raise ValueError("grad_guard: stats must have GUARD_STATS_WORDS elements and step one")
    for t, name in ((grad_scale, "grad_scale"), (found_inf, "found_inf")):
        if t is not None:
            _req(t, name=name)
            if t.numel() != 1:
                raise ValueError(f"grad_guard: {name} must hold one element")
    flags = (GUARD_SKIP_NONFINITE if skip_nonfinite else 0) | (GUARD_CLIP if max_norm is not None else 0)
    check(lib().phnet_grad_guard(_ptr(g), g.numel(), _ptr(workspace), workspace.numel(), _ptr(stats), _ptr(step),
                                 float(max_norm) if max_norm is not None else 0.0, flags, _ptr(grad_scale), _ptr(found_inf), _stream()),
          "phnet_grad_guard")


def adamw_step_guarded(p, g, m, v, n_decay: int, step, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                       mult, skip, lr_dev=None):
    """adamw_step on fl32(g * mult[0]), or nothing at all when skip[0] != 0; mult (float32[1]) and skip (int64[1]) are read on the
    device - the views of grad_guard's stats.  step has already been advanced by grad_guard."""
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (mult, "mult")):
        _req(t, name=name)
    _req(step, torch.int64, "step"); _req(skip, torch.int64, "skip")
    if not (p.numel() == g.numel() == m.numel() == v.numel()):
        raise ValueError("adamw_step_guarded: p/g/m/v lengths differ")
    if lr_dev is not None:
        _req(lr_dev, name="lr_dev")
    check(lib().phnet_adamw_step_guarded(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), int(n_decay), _ptr(step), float(lr), _ptr(lr_dev),
                                         float(beta1), float(beta2), float(eps), float(weight_decay), _ptr(mult), _ptr(skip), _stream()),
          "phnet_adamw_step_guarded")


def dropout_add(x, res=None, rng=None):
    """res + dropout(x) (either part optional) in one launch; dropout_add(dy, None, rng) is the backward of the dropout."""
    _req(x, name="x")
    y = torch.empty_like(x)
    check(lib().phnet_dropout_add(_ptr(x), _ptr(res), _ptr(y), x.numel(), *_rng_args(rng, x.shape[-1]), _stream()), "phnet_dropout_add")
    return y


def dropout_add_ln_fwd(x, res, w, b, eps: float, rng=None, save_stats: bool = True):
    """t = res + dropout(x), h = LayerNorm(t)*w + b over the last w.numel() (<= 256) elements -> (t, h, mean, rstd)."""
    _req(x, name="x"); _req(res, name="res")
    L = w.numel()
    rows = x.numel() // L
    t, h = torch.empty_like(x), torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    check(lib().phnet_dropout_add_ln_fwd(_ptr(x), _ptr(res), _ptr(w), _ptr(b), _ptr(t), _ptr(h), _ptr(mean), _ptr(rstd), rows, L, eps,
                                         *_rng_args(rng, L), _stream()), "phnet_dropout_add_ln_fwd")
    return t, h, mean, rstd


def dropout_add_ln_bwd(dh, dt, t, w, mean, rstd, rng=None, dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None,
                       accumulate: bool = False):
    """Returns (dres, dx, dw, db); dt (gradient on the residual stream) may be None."""
    _req(dh, name="dh")
    L = w.numel()
    rows = t.numel() // L
    dres, dx = torch.empty_like(t), torch.empty_like(t)
    if dw is None:
        dw, db, accumulate = torch.empty_like(w), torch.empty_like(w), False
    ws = workspace(lib().phnet_layernorm_bwd_workspace(rows, L), t.device, 2)
    check(lib().phnet_dropout_add_ln_bwd(_ptr(dh), _ptr(dt), _ptr(t), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dres), _ptr(dx), _ptr(dw),
                                         _ptr(db), rows, L, int(accumulate), *_rng_args(rng, L), _ptr(ws), ws.numel(), _stream()),
          "phnet_dropout_add_ln_bwd")
    return dres, dx, dw, db


def gelu_dropout_fwd(x, rng=None):
    _req(x, name="x")
    y = torch.empty_like(x)
    check(lib().phnet_gelu_dropout_fwd(_ptr(x), _ptr(y), x.numel(), *_rng_args(rng, x.shape[-1]), _stream()), "phnet_gelu_dropout_fwd")
    return y


def gelu_dropout_bwd(dy, x, rng=None):
    _req(dy, name="dy")
    dx = torch.empty_like(x)
    check(lib().phnet_gelu_dropout_bwd(_ptr(dy), _ptr(x), _ptr(dx), x.numel(), *_rng_args(rng, x.shape[-1]), _stream()), "phnet_gelu_dropout_bwd")
    return dx


def lane_decode(lines, conf_thresh: float, nms_thresh: float, top_k: int, img_w: int):
    """lines [N,6+S] or [F,N,6+S] -> dict(keep_mask u8, num i64, keep_c, anchors, anchors_sorted i64 [..,top_k],
    kept_rows [..,top_k,6+S]); everything stays on the device (no sync)."""
    _req(lines, name="lines")
    batched = lines.dim() == 3
    f = lines.shape[0] if batched else 1
    n, w = lines.shape[-2], lines.shape[-1]
    dev = lines.device
    out = dict(keep_mask=torch.empty((f, n), dtype=torch.uint8, device=dev), num=torch.empty((f,), dtype=torch.int64, device=dev),
               keep_c=torch.empty((f, top_k), dtype=torch.int64, device=dev), anchors=torch.empty((f, top_k), dtype=torch.int64, device=dev),
               anchors_sorted=torch.empty((f, top_k), dtype=torch.int64, device=dev),
               kept_rows=torch.empty((f, top_k, w), dtype=torch.float32, device=dev))
    check(lib().phnet_lane_decode(_ptr(lines), f, n, w - 6, float(conf_thresh), float(nms_thresh), int(top_k), float(img_w),
                                  _ptr(out["keep_mask"]), _ptr(out["num"]), _ptr(out["keep_c"]), _ptr(out["anchors"]),
                                  _ptr(out["anchors_sorted"]), _ptr(out["kept_rows"]), _stream()), "phnet_lane_decode")
    return out if batched else {k: v[0] for k, v in out.items()}


LANE_POINTS_MAX_LANES, LANE_POINTS_MAX_OFFSETS = 64, 256      # limits of phnet_lane_points (csrc/lane_points.hip)


def lane_points(kept_rows, num, prior_ys, out=None):
    """kept_rows [L,6+S] or [F,L,6+S] and num i64 [] / [F] as lane_decode returns them, prior_ys [S] -> dict(points f32 [..,L,S,2],
    count i32 [..,L], lanes_num i32 [..], slot i32 [..,L]): the (x, y) polylines of DetNetV2.predictions_to_pred, packed per
    frame, in one launch; everything stays on the device (no sync).  out: such a dict (of the [F,...] shapes) to write into."""
    _req(kept_rows, name="kept_rows"); _req(num, torch.int64, "num"); _req(prior_ys, name="prior_ys")
    if kept_rows.dim() not in (2, 3):
        raise ValueError("lane_points: kept_rows [L,6+S] or [F,L,6+S] expected")
    batched = kept_rows.dim() == 3
    f = kept_rows.shape[0] if batched else 1
    l, s = kept_rows.shape[-2], kept_rows.shape[-1] - 6
    if num.numel() != f or prior_ys.numel() != s or num.device != kept_rows.device or prior_ys.device != kept_rows.device:
        raise ValueError(f"lane_points: kept_rows {tuple(kept_rows.shape)} vs num {tuple(num.shape)} / prior_ys {tuple(prior_ys.shape)}")
    dev = kept_rows.device
    shapes = dict(points=((f, l, s, 2), torch.float32), count=((f, l), torch.int32), lanes_num=((f,), torch.int32),
                  slot=((f, l), torch.int32))
    if out is None:
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    else:
        for k, (shape, dt) in shapes.items():
            _req(out[k], dt, k + " out")
            if tuple(out[k].shape) != shape or out[k].device != dev:
                raise ValueError(f"lane_points: out[{k!r}] must be {shape}, got {tuple(out[k].shape)}")
        out = {k: out[k] for k in shapes}
    check(lib().phnet_lane_points(_ptr(kept_rows), _ptr(num), _ptr(prior_ys), f, l, s, _ptr(out["points"]), _ptr(out["count"]),
                                  _ptr(out["lanes_num"]), _ptr(out["slot"]), _stream()), "phnet_lane_points")
    return out if batched else {k: v[0] for k, v in out.items()}


LANE_TRACK_MAX_TRACKS, LANE_TRACK_MAX_OFFSETS = 64, 256       # limits of phnet_lane_track (csrc/lane_track.hip)
LANE_TRACK_MAX_LDS_WORDS = 15360                              # (L + M) * S + 2 * L * M, the kernel's LDS staging


def lane_track(kept_rows, num, state, thr: float, max_age: int, out=None):
    """kept_rows [B,L,6+S] and num i64 [B] (one frame of B streams, T = 1) or [B,T,L,6+S] and [B,T] (T frames of each) as
    lane_decode returns them; state: a phnet_amd.tracking.TrackState of those B streams (id, missed, hits i32 [B,M], ext i32
    [B,M,2], x [B,M,S], next_id i32 [B]), advanced in place -> dict(track_id i32 [..,L], hits i32 [..,L]) shaped like num.
    The rules are those of include/phnet_hip.h; thr is in the units of kept_rows.  One launch, everything stays on the device
    (no sync).  out: such a dict to write into."""
    _req(kept_rows, name="kept_rows"); _req(num, torch.int64, "num")
    if kept_rows.dim() not in (3, 4):
        raise ValueError("lane_track: kept_rows [B,L,6+S] or [B,T,L,6+S] expected")
    b, t = kept_rows.shape[0], (kept_rows.shape[1] if kept_rows.dim() == 4 else 1)
    l, s = kept_rows.shape[-2], kept_rows.shape[-1] - 6
    lead = tuple(kept_rows.shape[:-2])
    dev = kept_rows.device
    if tuple(num.shape) != lead or num.device != dev:
        raise ValueError(f"lane_track: kept_rows {tuple(kept_rows.shape)} vs num {tuple(num.shape)}")
    m = state.id.shape[-1]
    shapes = dict(id=((b, m), torch.int32), missed=((b, m), torch.int32), hits=((b, m), torch.int32), ext=((b, m, 2), torch.int32),
                  x=((b, m, s), torch.float32), next_id=((b,), torch.int32))
    for k, (shape, dt) in shapes.items():
        v = _req(getattr(state, k), dt, "state." + k)
        if tuple(v.shape) != shape or v.device != dev:
            raise ValueError(f"lane_track: state.{k} must be {shape} on {dev}, got {tuple(v.shape)} on {v.device}")
    if not (1 <= l <= m <= LANE_TRACK_MAX_TRACKS and 2 <= s <= LANE_TRACK_MAX_OFFSETS and (l + m) * s + 2 * l * m <= LANE_TRACK_MAX_LDS_WORDS):
        raise ValueError(f"lane_track: L = {l}, M = {m}, S = {s} outside 1 <= L <= M <= 64, 2 <= S <= 256, (L + M) * S + 2 * L * M <= 15360")
    outs = dict(track_id=(lead + (l,), torch.int32), hits=(lead + (l,), torch.int32))
    if out is None:
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in outs.items()}
    else:
        for k, (shape, dt) in outs.items():
            _req(out[k], dt, k + " out")
            if tuple(out[k].shape) != shape or out[k].device != dev:
                raise ValueError(f"lane_track: out[{k!r}] must be {shape}, got {tuple(out[k].shape)}")
        out = {k: out[k] for k in outs}
    check(lib().phnet_lane_track(_ptr(kept_rows), _ptr(num), b, t, l, s, m, float(thr), int(max_age), _ptr(state.id), _ptr(state.missed),
                                 _ptr(state.hits), _ptr(state.ext), _ptr(state.x), _ptr(state.next_id), _ptr(out["track_id"]),
                                 _ptr(out["hits"]), _stream()), "phnet_lane_track")
    return out


LANE_DRAW_MAX_SIZE, LANE_DRAW_MAX_WIDTH, LANE_DRAW_COORD_BOUND = 4096, 256, 8192     # limits of phnet_lane_draw (csrc/lane_draw.hip)
LANE_DRAW_FORMATS = {"none": 0, "rgb": 1, "nv12": 2, "yuyv": 3}


def lane_draw(points, count, lanes_num, out_hw, sx: float, sy: float, oy: float, lane_width: int = 12, slot=None, track_id=None,
              src=None, src_format: str = "none", pitch: int = 0, chroma_offset: int = 0, csc=None, palette=None, alpha: int = 256,
              label_map=True, overlay=False):
    """points f32 [F,L,S,2], count i32 [F,L], lanes_num i32 [F] (and slot i32 [F,L]) as lane_points returns them; track_id i32 [F,L]
    as lane_track does -> dict(label_map u8 [F,H,W] or None, overlay u8 [F,H,W,3] or None) with (H, W) = out_hw: the lanes drawn by
    the rules of include/phnet_hip.h (phnet_lane_draw), one launch, everything stays on the device (no sync).
    label_map / overlay: True allocates, a tensor is written into, False / None leaves that output out.  src: u8 [F, ...] frames of
    H x W pixels under the overlay (any shape; the frame stride is the bytes of src[0]), src_format "rgb" | "nv12" | "yuyv", with
    pitch, chroma_offset and csc (10 ints, yuv_matrix) as ClipPreprocessor passes them to phnet_preprocess_yuv; palette u8 [256,3]."""
    import ctypes
    _req(points, name="points"); _req(count, torch.int32, "count"); _req(lanes_num, torch.int32, "lanes_num")
    if points.dim() != 4 or points.shape[-1] != 2:
        raise ValueError("lane_draw: points [F,L,S,2] expected")
    f, l, s = points.shape[:3]
    dev = points.device
    h, w = int(out_hw[0]), int(out_hw[1])
    if tuple(count.shape) != (f, l) or tuple(lanes_num.shape) != (f,) or count.device != dev or lanes_num.device != dev:
        raise ValueError(f"lane_draw: points {tuple(points.shape)} vs count {tuple(count.shape)} / lanes_num {tuple(lanes_num.shape)}")
    for name, t in (("slot", slot), ("track_id", track_id)):
        if t is not None:
            _req(t, torch.int32, name)
            if tuple(t.shape) != (f, l) or t.device != dev:
                raise ValueError(f"lane_draw: {name} must be int32 {(f, l)} on {dev}, got {tuple(t.shape)}")
    if track_id is not None and slot is None:
        raise ValueError("lane_draw: track_id needs the slot of lane_points")
    if src_format not in LANE_DRAW_FORMATS:
        raise ValueError(f"lane_draw: src_format must be one of {sorted(LANE_DRAW_FORMATS)}, got {src_format!r}")
    if (src is None) != (src_format == "none"):
        raise ValueError("lane_draw: src and src_format go together")
    stride = 0
    if src is not None:
        _req(src, torch.uint8, "src")
        if src.dim() < 2 or src.shape[0] != f or src.device != dev:
            raise ValueError(f"lane_draw: src must hold {f} frames on {dev}, got {tuple(src.shape)}")
        stride = src[0].numel()
        if src_format == "rgb" and not pitch:
            pitch = 3 * w
    outs = {}
    for name, want, shape in (("label_map", label_map, (f, h, w)), ("overlay", overlay, (f, h, w, 3))):
        if want is None or want is False:
            outs[name] = None
        elif want is True:
            outs[name] = torch.empty(shape, dtype=torch.uint8, device=dev)
        else:
            _req(want, torch.uint8, name)
            if tuple(want.shape) != shape or want.device != dev:
                raise ValueError(f"lane_draw: {name} must be uint8 {shape} on {dev}, got {tuple(want.shape)}")
            outs[name] = want
    if palette is not None:
        _req(palette, torch.uint8, "palette")
        if tuple(palette.shape) != (256, 3) or palette.device != dev:
            raise ValueError(f"lane_draw: palette must be uint8 [256,3] on {dev}")
    csc_arr = None if csc is None else (ctypes.c_int32 * 10)(*[int(v) for v in csc])
    check(lib().phnet_lane_draw(_ptr(points), _ptr(count), _ptr(lanes_num), _ptr(slot), _ptr(track_id), f, l, s, float(sx), float(sy),
                                float(oy), h, w, int(lane_width), _ptr(src), LANE_DRAW_FORMATS[src_format], stride, int(pitch),
                                int(chroma_offset), None if csc_arr is None else ctypes.cast(csc_arr, ctypes.c_void_p), _ptr(palette),
                                int(alpha), _ptr(outs["label_map"]), _ptr(outs["overlay"]), _stream()), "phnet_lane_draw")
    return outs


LANE_TARGETS_MAX_IN_LANES, LANE_TARGETS_MAX_POINTS = 64, 256       # limits of phnet_lane_targets (csrc/lane_targets.hip)
LANE_TARGETS_MAX_ROWS, LANE_TARGETS_MAX_OFFSETS = 64, 256
LANE_TARGETS_MAX_POINTS_CLIP = 254                                # with rule 0c: a fragment has up to P + 2 points


def lane_targets(points, counts, lanes_num, offsets_ys, max_lanes: int, img_h: float, img_w: float, strip_size: float,
                 crop: float = 0.0, src_w: float = 0.0, scale_x: float = 1.0, scale_y: float = 1.0, flip: bool = False, out=None,
                 _aug=None, _clip=None):
    """points [F,Lin,P,2], counts i32 [F,Lin], lanes_num i32 [F], offsets_ys f64 [S] (the reference's np.arange table, on the
    device) -> label rows [F,max_lanes,6+S] by the rules of include/phnet_hip.h.  One launch, no allocation with out=, no sync.
    (_aug: lane_targets_aug's (flip2, fwd); None is phnet_lane_targets itself.  _clip: lane_targets_clip's (clip, frag_count).)"""
    _req(points, name="points"); _req(counts, torch.int32, "counts"); _req(lanes_num, torch.int32, "lanes_num")
    _req(offsets_ys, torch.float64, "offsets_ys")
    if points.dim() != 4 or points.shape[-1] != 2 or offsets_ys.dim() != 1:
        raise ValueError("lane_targets: points [F,Lin,P,2] and offsets_ys [S] expected")
    f, lin, p, _ = points.shape
    s, r, dev = offsets_ys.shape[0], int(max_lanes), points.device
    if tuple(counts.shape) != (f, lin) or tuple(lanes_num.shape) != (f,) or any(t.device != dev for t in (counts, lanes_num, offsets_ys)):
        raise ValueError(f"lane_targets: points {tuple(points.shape)} vs counts {tuple(counts.shape)}, lanes_num {tuple(lanes_num.shape)}")
    if not (1 <= f < 2 ** 31 and 1 <= lin <= LANE_TARGETS_MAX_IN_LANES and 2 <= p <= LANE_TARGETS_MAX_POINTS
            and 1 <= r <= LANE_TARGETS_MAX_ROWS and 2 <= s <= LANE_TARGETS_MAX_OFFSETS):
        raise ValueError(f"lane_targets: F = {f}, Lin = {lin}, P = {p}, R = {r}, S = {s} outside 1 <= F < 2^31, 1 <= Lin <= 64, "
                         "2 <= P <= 256, 1 <= R <= 64, 2 <= S <= 256")
    if out is None:
        out = torch.empty((f, r, 6 + s), dtype=torch.float32, device=dev)
    else:
        _req(out, name="out")
        if tuple(out.shape) != (f, r, 6 + s) or out.device != dev:
            raise ValueError(f"lane_targets: out must be {(f, r, 6 + s)} on {dev}, got {tuple(out.shape)} on {out.device}")
    args = (_ptr(points), _ptr(counts), _ptr(lanes_num), _ptr(offsets_ys), _ptr(out), f, lin, p, r, s, float(img_h), float(img_w),
            float(strip_size), float(crop), float(src_w), float(scale_x), float(scale_y), int(bool(flip)))
    if _aug is None and _clip is None:
        check(lib().phnet_lane_targets(*args, _stream()), "phnet_lane_targets")
    else:
        flip2, fwd = _aug if _aug is not None else (None, None)
        if flip2 is not None:
            _req(flip2, torch.int32, "flip2")
        if fwd is not None:
            _req(fwd, torch.float64, "fwd")
        if (flip2 is not None and (tuple(flip2.shape) != (f,) or flip2.device != dev)) or \
                (fwd is not None and (tuple(fwd.shape) != (f, 6) or fwd.device != dev)):
            raise ValueError(f"lane_targets_aug: flip2 i32 [{f}] and fwd f64 [{f},6] on {dev} expected")
        if _clip is None:
            check(lib().phnet_lane_targets_aug(*args, _ptr(flip2), _ptr(fwd), _stream()), "phnet_lane_targets_aug")
            return out
        clip, frag_count = _clip
        if clip and p > LANE_TARGETS_MAX_POINTS_CLIP:
            raise ValueError(f"lane_targets_clip: P = {p} outside 2 <= P <= 254 with clip")
        if frag_count is not None:
            _req(frag_count, torch.int32, "frag_count")
            if tuple(frag_count.shape) != (f,) or frag_count.device != dev:
                raise ValueError(f"lane_targets_clip: frag_count i32 [{f}] on {dev} expected")
        check(lib().phnet_lane_targets_clip(*args, _ptr(flip2), _ptr(fwd), int(bool(clip)), _ptr(frag_count), _stream()),
              "phnet_lane_targets_clip")
    return out


def lane_targets_aug(points, counts, lanes_num, offsets_ys, max_lanes: int, img_h: float, img_w: float, strip_size: float, flip2, fwd,
                     **kw):
    """lane_targets behind an augmented image: rule 0b of include/phnet_hip.h with flip2 i32 [F] and fwd f64 [F,6] (the source -> output
    matrices) on the device; either may be None (its step is skipped).  Keywords as lane_targets."""
    return lane_targets(points, counts, lanes_num, offsets_ys, max_lanes, img_h, img_w, strip_size, _aug=(flip2, fwd), **kw)


def lane_targets_clip(points, counts, lanes_num, offsets_ys, max_lanes: int, img_h: float, img_w: float, strip_size: float, flip2=None,
                      fwd=None, clip: bool = True, frag_count=None, **kw):
    """lane_targets_aug with rule 0c of include/phnet_hip.h: clip = True cuts every lane at the image border and encodes each fragment
    of more than 2 points as a lane of its own (P <= 254); clip = False is lane_targets_aug bit for bit.  frag_count i32 [F] on the
    device, or None: written with the surviving fragments of each frame before the max_lanes cap.  Keywords as lane_targets."""
    return lane_targets(points, counts, lanes_num, offsets_ys, max_lanes, img_h, img_w, strip_size, _aug=(flip2, fwd),
                        _clip=(clip, frag_count), **kw)


AUGMENT_TABLE_COLS, AUGMENT_MAX_SIDE = 16, 32768                  # the i32 table of phnet_augment_u8 (csrc/augment.hip)


AUGMENT_STENCIL_COLS = 40                                         # the i32 stencil table of phnet_augment_stencil_u8 (csrc/augment_stencil.hip)


def augment_u8(frames_u8, flip2, inv, table, mean3, std3, layout: str = "nchw", out=None, out_u8=None, stencil=None, staged=None):
    """frames_u8 u8 [T,H,W,3] (resized frames) -> the augmented, normalised clip f32 [T,3,H,W] ("nchw") or [T,H,W,4] ("nhwc4") by the
    rules of include/phnet_hip.h, with flip2 i32 [T], inv f64 [T,6], table i32 [T,16] on the device and mean3 / std3 ctypes float[3] on
    the host.  out / out_u8: buffers to write into (out_u8 = None: the 8-bit image is not written).  One launch, no sync.
    stencil: i32 [T,40] on the device, the neighbourhood ops of rule 7 - then phnet_augment_stencil_u8 runs (two launches) and staged,
    a u8 [T,H,W,3] scratch buffer on the device that is neither the input nor out_u8, is required."""
    import ctypes
    _req(frames_u8, torch.uint8, "frames_u8"); _req(flip2, torch.int32, "flip2"); _req(inv, torch.float64, "inv"); _req(table, torch.int32, "table")
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError("augment_u8: frames_u8 [T,H,W,3] expected")
    if layout not in ("nchw", "nhwc4"):
        raise ValueError("layout must be 'nchw' or 'nhwc4'")
    t, h, w, _ = frames_u8.shape
    dev = frames_u8.device
    if tuple(flip2.shape) != (t,) or tuple(inv.shape) != (t, 6) or tuple(table.shape) != (t, AUGMENT_TABLE_COLS) or \
            any(x.device != dev for x in (flip2, inv, table)):
        raise ValueError(f"augment_u8: flip2 [{t}], inv [{t},6], table [{t},{AUGMENT_TABLE_COLS}] on {dev} expected, got "
                         f"{tuple(flip2.shape)}, {tuple(inv.shape)}, {tuple(table.shape)}")
    shape = (t, 3, h, w) if layout == "nchw" else (t, h, w, 4)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        _req(out, name="out")
        if tuple(out.shape) != shape or out.device != dev:
            raise ValueError(f"augment_u8: out must be {shape} on {dev}, got {tuple(out.shape)} on {out.device}")
    if out_u8 is not None:
        _req(out_u8, torch.uint8, "out_u8")
        if tuple(out_u8.shape) != (t, h, w, 3) or out_u8.device != dev:
            raise ValueError(f"augment_u8: out_u8 must be {(t, h, w, 3)} on {dev}")
        if out_u8.data_ptr() == frames_u8.data_ptr() and t:
            raise ValueError("augment_u8: out_u8 must not be the input (a warp reads other pixels than it writes)")
    mean_p, std_p = ctypes.cast(mean3, ctypes.c_void_p), ctypes.cast(std3, ctypes.c_void_p)
    if stencil is None:
        check(lib().phnet_augment_u8(_ptr(frames_u8), _ptr(out), _ptr(out_u8), _ptr(flip2), _ptr(inv), _ptr(table), t, h, w,
                                     0 if layout == "nchw" else 1, mean_p, std_p, _stream()), "phnet_augment_u8")
        return out
    _req(stencil, torch.int32, "stencil")
    if tuple(stencil.shape) != (t, AUGMENT_STENCIL_COLS) or stencil.device != dev:
        raise ValueError(f"augment_u8: stencil must be [{t},{AUGMENT_STENCIL_COLS}] on {dev}, got {tuple(stencil.shape)}")
    if staged is None:
        raise ValueError("augment_u8: a stencil table needs a staged buffer")
    _req(staged, torch.uint8, "staged")
    if tuple(staged.shape) != (t, h, w, 3) or staged.device != dev:
        raise ValueError(f"augment_u8: staged must be {(t, h, w, 3)} on {dev}")
    if t and (staged.data_ptr() == frames_u8.data_ptr() or (out_u8 is not None and staged.data_ptr() == out_u8.data_ptr())):
        raise ValueError("augment_u8: staged must be neither the input nor out_u8 (both launches read other pixels than they write)")
    check(lib().phnet_augment_stencil_u8(_ptr(frames_u8), _ptr(out), _ptr(out_u8), _ptr(flip2), _ptr(inv), _ptr(table), _ptr(stencil),
                                         _ptr(staged), t, h, w, 0 if layout == "nchw" else 1, mean_p, std_p, _stream()),
          "phnet_augment_stencil_u8")
    return out


# ------------------------------------------------------------------------------------------------ Router4OLV2 family (inference)
def gate_v2_fwd(x_cp, w1, s1, t1, w2, s2, t2, wl, bl, out: Optional[torch.Tensor] = None):
    """x_cp [M,C,P] -> sigmoid(mean(Linear(flatten(conv-bn-relu x2)))) [M]  (csrc/v2head.hip)."""
    for t, nm in ((x_cp, "x"), (w1, "w1"), (s1, "s1"), (t1, "t1"), (w2, "w2"), (s2, "s2"), (t2, "t2"), (wl, "wl"), (bl, "bl")):
        _req(t, name=nm)
    m, c, p = x_cp.shape
    c1, c2 = w1.shape[0], w2.shape[0]
    if w1.numel() != c1 * c * 3 or w2.numel() != c2 * c1 or wl.numel() != p * c2 * p or bl.numel() != p:
        raise RuntimeError("gate_v2_fwd: parameter shapes do not match the feature map")
    if out is None:
        out = torch.empty((m,), dtype=torch.float32, device=x_cp.device)
    check(lib().phnet_gate_v2_fwd(_ptr(x_cp), _ptr(w1), _ptr(s1), _ptr(t1), _ptr(w2), _ptr(s2), _ptr(t2), _ptr(wl), _ptr(bl), _ptr(out),
                                  m, c, p, c1, c2, _stream()), "phnet_gate_v2_fwd")
    return out


def dyn_bmm_ln_relu_fwd_any(x, w, gamma, beta, eps: float):
    """x [N,P,K], w [N,K,J] -> relu(LayerNorm(x @ w)) [N,P,J] at run-time shapes (forward only)."""
    _req(x, name="x"); _req(w, name="w"); _req(gamma, name="gamma"); _req(beta, name="beta")
    n, p, k = x.shape
    j = w.shape[2]
    assert w.shape[0] == n and w.shape[1] == k and gamma.numel() == j
    y = torch.empty((n, p, j), dtype=torch.float32, device=x.device)
    check(lib().phnet_dyn_bmm_ln_relu_fwd_any(_ptr(x), _ptr(w), _ptr(gamma), _ptr(beta), _ptr(y), n, p, k, j, float(eps), _stream()),
          "phnet_dyn_bmm_ln_relu_fwd_any")
    return y


def route_lines(gates, a, b, hard: bool):
    """gates [S,M] (one row per refinement stage), a / b [M,W] -> [M,W]: hard selection or soft blend by the mean gate."""
    _req(gates, name="gates"); _req(a, name="a"); _req(b, name="b")
    s, m = gates.shape
    w = a.shape[-1]
    assert a.numel() == m * w and b.numel() == m * w
    out = torch.empty_like(a)
    check(lib().phnet_route_lines(_ptr(gates), _ptr(a), _ptr(b), _ptr(out), s, m, w, int(bool(hard)), _stream()), "phnet_route_lines")
    return out


def rowchain_fwd(x, resid=None, wa=None, ba=None, ln1=None, ffn=None, ln2=None, wg=None, bg=None, eps: float = 1e-5,
                 rng_a=None, rng_f=None, rng_3=None, want_t: bool = True, want_h: bool = False):
    """Row-local chain of a transformer layer in one launch (csrc/rowchain.hip), forward only.  x [R,E]; wa / ba: out-projection
    (then t = resid + dropout_a(.)); ln1 = (w, b); ffn = (W1, b1, W2, b2) with ln2 = (w, b); wg / bg: next projection.
    rng_*: DropoutStream.site tuples (None = no dropout at that site; all sites share one probability).  -> (t, h, y), each None
    when not produced."""
    _req(x, name="x")
    r, e = x.shape
    dev = x.device
    t = torch.empty((r, e), dtype=torch.float32, device=dev) if want_t else None
    h = torch.empty((r, e), dtype=torch.float32, device=dev) if want_h else None
    ng = wg.shape[0] if wg is not None else 0
    y = torch.empty((r, ng), dtype=torch.float32, device=dev) if wg is not None else None
    w1 = b1 = w2 = b2 = None
    ff = 0
    if ffn is not None:
        w1, b1, w2, b2 = ffn
        ff = w1.shape[0]
    sites = [s for s in (rng_a, rng_f, rng_3) if s is not None]
    state, p = (sites[0][0], sites[0][2]) if sites else (None, 0.0)
    assert all(s[2] == p and s[0].data_ptr() == state.data_ptr() for s in sites), "rowchain_fwd: the dropout sites of one launch share one counter and one probability"

    def call(rng, width):
        return 0 if rng is None else _rng_args(rng, width)[1]
    for tns in (resid, wa, ba, w1, b1, w2, b2, wg, bg) + tuple(ln1) + (tuple(ln2) if ln2 is not None else ()):
        if tns is not None:
            _req(tns, name="rowchain operand")
    check(lib().phnet_rowchain_fwd(_ptr(x), _ptr(resid), _ptr(wa), _ptr(ba), _ptr(ln1[0]), _ptr(ln1[1]), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                                   _ptr(ln2[0]) if ln2 is not None else None, _ptr(ln2[1]) if ln2 is not None else None, _ptr(wg), _ptr(bg),
                                   _ptr(t), _ptr(h), _ptr(y), r, e, ff, ng, float(eps), _ptr(state), call(rng_a, e), call(rng_f, ff), call(rng_3, e),
                                   float(p), _stream()), "phnet_rowchain_fwd")
    return t, h, y


ROWCHAIN_ATTN_MAX_KEYS = 64       # csrc/rowchain.hip: LKMAX


def rowchain_attn_ok(e: int, ff: int, heads: int, lk: int) -> bool:
    """The shapes phnet_rowchain_attn_fwd takes (everything else: PHNET_ERR_ARG - the caller keeps the three launches)."""
    return e == 128 and ff == 256 and heads * 16 == e and 1 <= lk <= ROWCHAIN_ATTN_MAX_KEYS


def rowchain_attn_fwd(x, resid, k, v, heads: int, wa, ba, ln1, ffn, ln2, chain_a=None, key_valid=None, wg=None, bg=None,
                      eps: float = 1e-5, eps_a: float = 1e-5, rng_a0=None, rng_c=None, rng_a=None, rng_f=None, rng_3=None,
                      batch: int = 1, want_t: bool = True, want_h: bool = False, out=None):
    """[chain A] -> cross-attention core -> [chain B] in one launch (csrc/rowchain.hip), forward only: the bits of
    rowchain_fwd -> attention_fwd -> rowchain_fwd.  chain_a = (wa0, ba0, ln0w, ln0b, wq, bq): x [R,E] = the self-attention output,
    resid its residual (dropout site rng_a0); chain_a = None: x = q and resid = t of an earlier launch.  k / v [batch*Lk, E] (any
    row stride), key_valid u8[batch*Lk]; rng_c: dropout site of the attention weights.  The rest as rowchain_fwd with the
    feed-forward block.  out = (t, h, y): caller-provided outputs (None entries are not produced).  -> (t, h, y)."""
    _req(x, name="x"); _req(resid, name="resid")
    r, e = x.shape
    lq, lk = r // batch, k.shape[0] // batch
    assert r == lq * batch and k.shape[0] == lk * batch and v.shape[0] == k.shape[0] and k.stride(1) == 1 and v.stride(1) == 1
    dev = x.device
    ng = wg.shape[0] if wg is not None else 0
    if out is not None:
        t, h, y = out
    else:
        t = torch.empty((r, e), dtype=torch.float32, device=dev) if want_t else None
        h = torch.empty((r, e), dtype=torch.float32, device=dev) if want_h else None
        y = torch.empty((r, ng), dtype=torch.float32, device=dev) if wg is not None else None
    w1, b1, w2, b2 = ffn
    ff = w1.shape[0]
    a6 = tuple(chain_a) if chain_a is not None else (None,) * 6
    for tns in a6 + (wa, ba, w1, b1, w2, b2, wg, bg, t, h, y) + tuple(ln1) + tuple(ln2):
        if tns is not None:
            _req(tns, name="rowchain operand")
    if key_valid is not None:
        _req(key_valid, torch.uint8, "key_valid")
    sites = [s for s in (rng_a0, rng_a, rng_f, rng_3) if s is not None]
    state, p = (sites[0][0], sites[0][2]) if sites else (None, 0.0)
    if state is None and rng_c is not None:
        state = rng_c[0]
    assert all(s[2] == p for s in sites), "rowchain_attn_fwd: the dropout sites of the chains share one probability (rng_c has its own)"
    assert all(s[0].data_ptr() == state.data_ptr() for s in sites + ([rng_c] if rng_c is not None else [])), "one dropout counter per launch"

    def call(rng, width):
        return 0 if rng is None else _rng_args(rng, width)[1]
    check(lib().phnet_rowchain_attn_fwd(_ptr(x), _ptr(resid), *[_ptr(a) for a in a6], float(eps_a), _ptr(k), _ptr(v), k.stride(0), v.stride(0),
                                        _ptr(key_valid), _ptr(wa), _ptr(ba), _ptr(ln1[0]), _ptr(ln1[1]), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                                        _ptr(ln2[0]), _ptr(ln2[1]), _ptr(wg), _ptr(bg), _ptr(t), _ptr(h), _ptr(y), batch, lq, lk, heads, e, ff, ng,
                                        float(eps), _ptr(state), call(rng_a0, e), call(rng_c, 0), call(rng_a, e), call(rng_f, ff), call(rng_3, e),
                                        float(p), float(rng_c[2]) if rng_c is not None else 0.0, _stream()), "phnet_rowchain_attn_fwd")
    return t, h, y


def tower_layout(n_towers: int, c: int, head_out):
    """-> (total floats, offsets[6] of w1 | b1 | w2 | b2 | wh | bh, HW) of the assembled tower weights (csrc/towers.hip)."""
    import ctypes
    ho = (ctypes.c_int32 * n_towers)(*[int(v) for v in head_out])
    offs = (ctypes.c_int64 * 6)()
    hw = ctypes.c_int32()
    total = int(lib().phnet_tower_layout(n_towers, c, ho, offs, ctypes.byref(hw)))
    if total == 0:
        raise RuntimeError("phnet_tower_layout: bad arguments")
    return total, list(offs), int(hw.value)


def assemble_towers(params, n_towers: int, c: int, head_out, dst):
    import ctypes
    ho = (ctypes.c_int32 * n_towers)(*[int(v) for v in head_out])
    check(lib().phnet_assemble_towers(_ptr_array([_req(p, name="tower parameter") for p in params]), n_towers, c, ho, _ptr(dst), _stream()),
          "phnet_assemble_towers")
    return dst


def scatter_tower_grads(src, grads, n_towers: int, c: int, head_out, accumulate: bool):
    import ctypes
    ho = (ctypes.c_int32 * n_towers)(*[int(v) for v in head_out])
    table = (ctypes.c_void_p * len(grads))(*[None if g is None else _req(g, name="tower gradient").data_ptr() for g in grads])
    check(lib().phnet_scatter_tower_grads(_ptr(src), table, n_towers, c, ho, int(accumulate), _stream()), "phnet_scatter_tower_grads")


def tower_chain_fwd(x, params, head_out, priors, ys, img_w, img_h):
    """x [R,C], params = 6*T tower tensors, priors [R,6+S] -> (preds, lines) [R,6+S]: towers + heads + lane prior update in one
    launch (csrc/rowchain.hip), forward only."""
    import ctypes
    _req(x, name="x"); _req(priors, name="priors")
    r, c = x.shape
    t = len(params) // 6
    ho = (ctypes.c_int32 * t)(*[int(v) for v in head_out])
    preds, lines = torch.empty_like(priors), torch.empty_like(priors)
    check(lib().phnet_tower_chain_fwd(_ptr(x), _ptr_array([_req(p, name="tower parameter") for p in params]), t, c, ho, _ptr(priors), _ptr(ys),
                                      _ptr(preds), _ptr(lines), r, priors.shape[1] - 6, float(img_w), float(img_h), _stream()),
          "phnet_tower_chain_fwd")
    return preds, lines


DEFAULT_MMA = "bf16x3"


def lane_raster(segs, n_lanes: int, height: int, width: int, lane_width: int, masks=None):
    """Bit masks [n_lanes][height][ceil(width/32)] (int32 words) of the thick poly-lines: segs [S][5] int32 = (x0, y0, x1, y1, lane)
    (csrc/lane_iou.hip; the evaluator's cv::line canvases, evaluation/culane/src/lane_compare.cpp:17-49).  masks: such a tensor,
    zeroed by the caller, to OR the lines into (a captured graph keeps its address)."""
    _req(segs, torch.int32, "segs")
    assert segs.dim() == 2 and segs.shape[1] == 5
    if masks is None:
        masks = torch.zeros((n_lanes, height, (width + 31) // 32), dtype=torch.int32, device=segs.device)
    else:
        _req(masks, torch.int32, "masks")
        assert tuple(masks.shape) == (n_lanes, height, (width + 31) // 32) and masks.device == segs.device
    check(lib().phnet_lane_raster(_ptr(segs), segs.shape[0], _ptr(masks), n_lanes, height, width, lane_width, _stream()), "phnet_lane_raster")
    return masks


def lane_mask_stats(masks, pairs, width: int):
    """(area [n_lanes], inter [n_pairs]) int64: set bits of every mask and of masks[pairs[p, 0]] & masks[pairs[p, 1]]
    (lane_compare.cpp:51-55: cv::sum of the canvases and of their product)."""
    _req(masks, torch.int32, "masks"); _req(pairs, torch.int32, "pairs")
    n_lanes, height = masks.shape[0], masks.shape[1]
    assert masks.shape[2] == (width + 31) // 32 and pairs.dim() == 2 and pairs.shape[1] == 2
    area = torch.zeros(n_lanes, dtype=torch.int64, device=masks.device)
    inter = torch.zeros(pairs.shape[0], dtype=torch.int64, device=masks.device)
    check(lib().phnet_lane_mask_stats(_ptr(masks), n_lanes, height, width, _ptr(pairs), pairs.shape[0], _ptr(area), _ptr(inter),
                                      _stream()), "phnet_lane_mask_stats")
    return area, inter


def lane_mask_iou(segs, n_lanes: int, pairs, height: int, width: int, lane_width: int):
    """Areas of the drawn lanes and the pairwise intersections the IoU matrices need, two launches."""
    return lane_mask_stats(lane_raster(segs, n_lanes, height, width, lane_width), pairs, width)


def check_iou_groups(groups, n_lanes: int):
    """Host check of a `phnet_lane_iou_groups` table -> (int32 [G, 5] array, n_entries).  Rows are (row_first, n_rows, col_first,
    n_cols, out_first): counts >= 0, lane ranges inside [0, n_lanes), out_first = 0 and then ascending without gaps."""
    import numpy as np
    g = np.asarray(groups)
    if g.size == 0:
        g = np.zeros((0, 5), np.int32)
    if g.ndim != 2 or g.shape[1] != 5 or g.dtype.kind not in "iu":
        raise ValueError("lane_iou_groups: groups must be an integer table [n_groups, 5]")
    g = g.astype(np.int64)
    total = 0
    for k, (r0, nr, c0, nc, out) in enumerate(g.tolist()):
        if nr < 0 or nc < 0:
            raise ValueError(f"lane_iou_groups: group {k} has a negative count")
        if (nr and (r0 < 0 or r0 + nr > n_lanes)) or (nc and (c0 < 0 or c0 + nc > n_lanes)):
            raise ValueError(f"lane_iou_groups: group {k} addresses a lane outside [0, {n_lanes})")
        if out != total:
            raise ValueError(f"lane_iou_groups: group {k} has out_first {out}, contiguous output wants {total}")
        total += nr * nc
    if total + n_lanes >= 1 << 31:
        raise ValueError("lane_iou_groups: too many entries for one launch")
    return np.ascontiguousarray(g.astype(np.int32)), total


def lane_iou_groups(masks, groups, width: int, scale: int = 1, eps: float = 0.0, want_area: bool = False):
    """IoU matrices of the masks of `lane_raster`, one launch (csrc/lane_iou.hip): `groups` is a HOST integer table [G][5] =
    (row_first, n_rows, col_first, n_cols, out_first), checked here before it is uploaded; -> iou float64 [n_entries], entry
    (r, c) of group g at out_first + r * n_cols + c = scale * I / (scale * (A + B - I) + eps) (and area int64 [n_lanes])."""
    n_lanes = int(masks.shape[0])
    table, n_entries = check_iou_groups(groups, n_lanes)
    if int(scale) < 1 or not (0.0 <= float(eps) < float("inf")):
        raise ValueError("lane_iou_groups: scale must be >= 1 and eps finite and >= 0")
    _req(masks, torch.int32, "masks")
    height = masks.shape[1]
    assert masks.dim() == 3 and masks.shape[2] == (width + 31) // 32
    dev_groups = torch.from_numpy(table).to(masks.device)
    iou = torch.empty(n_entries, dtype=torch.float64, device=masks.device)
    area = torch.empty(n_lanes, dtype=torch.int64, device=masks.device) if want_area else None
    check(lib().phnet_lane_iou_groups(_ptr(masks), n_lanes, height, width, _ptr(dev_groups), table.shape[0], n_entries, int(scale),
                                      float(eps), _ptr(iou), _ptr(area), _stream()), "phnet_lane_iou_groups")
    return (iou, area) if want_area else iou


LANE_EVAL_MAX_LANES, LANE_EVAL_MAX_POINTS, LANE_EVAL_TIMES = 16, 256, 50     # limits of phnet_lane_eval_* (csrc/lane_eval.hip)
LANE_EVAL_RELABEL_CAP = 1024                                                 # PHNET_LANE_EVAL_RELABEL_CAP of include/phnet_hip.h
LANE_EVAL_MODES = {"wire": 0, "raw": 1}


def lane_eval_rows(n_offsets: int, max_gt_points: int) -> int:
    """C: the rows a lane owns in the segment table of `lane_eval_segments`."""
    return (max(int(n_offsets), int(max_gt_points)) - 1) * LANE_EVAL_TIMES


def _out_dict(name, out, shapes, dev):
    if out is None:
        return {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    for k, (shape, dt) in shapes.items():
        _req(out[k], dt, k + " out")
        if tuple(out[k].shape) != shape or out[k].device != dev:
            raise ValueError(f"{name}: out[{k!r}] must be {shape} on {dev}, got {tuple(out[k].shape)} on {out[k].device}")
    return {k: out[k] for k in shapes}


def lane_eval_segments(points, count, lanes_num, gt_points, gt_count, gt_num, mode: str, size, crop_top: float, out=None):
    """points f32 [F,L,S,2], count i32 [F,L], lanes_num i32 [F] as lane_points returns them and the annotations gt_points f32
    [F,G,P,2], gt_count i32 [F,G], gt_num i32 [F] in evaluator coordinates -> dict(segs i32 [F*(G+L), C, 5], lane_pts i32 [F, G+L]):
    the evaluator's cv::line table (spline, 50 segments per interval) by the rules of include/phnet_hip.h, one launch, no sync
    (csrc/lane_eval.hip).  mode "wire": the predictions go through the .lines.txt round trip with size = (H_crop, W_org) and
    crop_top; "raw": they are evaluator coordinates already.  Annotation g of image f is lane f*(G+L)+g, prediction k lane
    f*(G+L)+G+k; unused rows carry lane -1.  out: such a dict to write into."""
    _req(points, name="points"); _req(count, torch.int32, "count"); _req(lanes_num, torch.int32, "lanes_num")
    _req(gt_points, name="gt_points"); _req(gt_count, torch.int32, "gt_count"); _req(gt_num, torch.int32, "gt_num")
    if mode not in LANE_EVAL_MODES:
        raise ValueError(f"lane_eval_segments: mode must be one of {sorted(LANE_EVAL_MODES)}, got {mode!r}")
    if points.dim() != 4 or gt_points.dim() != 4 or points.shape[-1] != 2 or gt_points.shape[-1] != 2:
        raise ValueError("lane_eval_segments: points [F,L,S,2] and gt_points [F,G,P,2] expected")
    f, l, s = points.shape[:3]
    g, p = gt_points.shape[1:3]
    dev = points.device
    if (gt_points.shape[0] != f or tuple(count.shape) != (f, l) or tuple(lanes_num.shape) != (f,) or tuple(gt_count.shape) != (f, g)
            or tuple(gt_num.shape) != (f,) or any(t.device != dev for t in (count, lanes_num, gt_points, gt_count, gt_num))):
        raise ValueError(f"lane_eval_segments: points {tuple(points.shape)} / count {tuple(count.shape)} / lanes_num "
                         f"{tuple(lanes_num.shape)} / gt_points {tuple(gt_points.shape)} / gt_count {tuple(gt_count.shape)} / gt_num "
                         f"{tuple(gt_num.shape)} do not belong together")
    if not (1 <= g <= LANE_EVAL_MAX_LANES and 1 <= l <= LANE_EVAL_MAX_LANES and 2 <= s <= LANE_EVAL_MAX_POINTS
            and 2 <= p <= LANE_EVAL_MAX_POINTS and f >= 1):
        raise ValueError(f"lane_eval_segments: F = {f}, G = {g}, L = {l}, S = {s}, P = {p} outside 1 <= F, 1 <= G, L <= 16, 2 <= S, P <= 256")
    c = lane_eval_rows(s, p)
    if f * (g + l) * c >= 1 << 31:
        raise ValueError("lane_eval_segments: F * (G + L) * C must stay below 2^31")
    out = _out_dict("lane_eval_segments", out, dict(segs=((f * (g + l), c, 5), torch.int32), lane_pts=((f, g + l), torch.int32)), dev)
    check(lib().phnet_lane_eval_segments(_ptr(points), _ptr(count), _ptr(lanes_num), _ptr(gt_points), _ptr(gt_count), _ptr(gt_num),
                                         f, g, l, s, p, LANE_EVAL_MODES[mode], float(size[0]), float(size[1]), float(crop_top),
                                         _ptr(out["segs"]), _ptr(out["lane_pts"]), _stream()), "phnet_lane_eval_segments")
    return out


def lane_eval_count(iou, lane_pts, n_gt: int, threshold: float, totals, iou_tot, overflow, video=None, out=None):
    """iou f64 [F,G,L] (lane_iou_groups with scale = 1, eps = 0 on the table of one group per image) and lane_pts i32 [F,G+L] of
    lane_eval_segments -> dict(tp, fp, fn i32 [F], iou_im f64 [F], anno_match i32 [F,G]): the evaluator's matching and counters
    per image (count_im_pair / make_match as written; the rules are in include/phnet_hip.h), one launch, no sync.  The images are
    ADDED, in ascending order, to totals i64 [V,4] = (tp, fp, fn, images) and iou_tot f64 [V] in the row video i32 [F] names (row
    0 without it); overflow i32 [1] counts the images that reached the relabelling cap.  out: such a dict to write into."""
    _req(iou, torch.float64, "iou"); _req(lane_pts, torch.int32, "lane_pts")
    _req(totals, torch.int64, "totals"); _req(iou_tot, torch.float64, "iou_tot"); _req(overflow, torch.int32, "overflow")
    if iou.dim() != 3 or lane_pts.dim() != 2:
        raise ValueError("lane_eval_count: iou [F,G,L] and lane_pts [F,G+L] expected")
    f, g, l = iou.shape
    dev = iou.device
    if g != int(n_gt) or tuple(lane_pts.shape) != (f, g + l) or lane_pts.device != dev:
        raise ValueError(f"lane_eval_count: iou {tuple(iou.shape)} vs lane_pts {tuple(lane_pts.shape)} with G = {n_gt}")
    if not (1 <= g <= LANE_EVAL_MAX_LANES and 1 <= l <= LANE_EVAL_MAX_LANES and 1 <= f < 1 << 22):
        raise ValueError(f"lane_eval_count: F = {f}, G = {g}, L = {l} outside 1 <= F < 2^22, 1 <= G, L <= 16")
    v = totals.shape[0]
    if totals.dim() != 2 or totals.shape[1] != 4 or v < 1 or tuple(iou_tot.shape) != (v,) or overflow.numel() != 1 or \
            any(t.device != dev for t in (totals, iou_tot, overflow)):
        raise ValueError(f"lane_eval_count: totals i64 [V,4], iou_tot f64 [V] and overflow i32 [1] on {dev} expected")
    if video is not None:
        _req(video, torch.int32, "video")
        if tuple(video.shape) != (f,) or video.device != dev:
            raise ValueError(f"lane_eval_count: video must be int32 [{f}] on {dev}")
    out = _out_dict("lane_eval_count", out, dict(tp=((f,), torch.int32), fp=((f,), torch.int32), fn=((f,), torch.int32),
                                                 iou_im=((f,), torch.float64), anno_match=((f, g), torch.int32)), dev)
    check(lib().phnet_lane_eval_count(_ptr(iou), _ptr(lane_pts), f, g, l, float(threshold), _ptr(video), v, _ptr(out["tp"]),
                                      _ptr(out["fp"]), _ptr(out["fn"]), _ptr(out["iou_im"]), _ptr(out["anno_match"]), _ptr(totals),
                                      _ptr(iou_tot), _ptr(overflow), _stream()), "phnet_lane_eval_count")
    return out


def lane_iou_groups_device(masks, dev_groups, n_entries: int, width: int, out):
    """lane_iou_groups for a caller that keeps its (host-checked, see check_iou_groups) table on the device and owns the output:
    dev_groups i32 [n_groups, 5], out f64 with n_entries elements; scale = 1, eps = 0.  Nothing is allocated or copied."""
    _req(masks, torch.int32, "masks"); _req(dev_groups, torch.int32, "groups"); _req(out, torch.float64, "out")
    n_lanes, height = int(masks.shape[0]), masks.shape[1]
    assert masks.dim() == 3 and masks.shape[2] == (width + 31) // 32 and dev_groups.dim() == 2 and dev_groups.shape[1] == 5
    assert out.numel() == n_entries and out.device == masks.device and dev_groups.device == masks.device
    check(lib().phnet_lane_iou_groups(_ptr(masks), n_lanes, height, width, _ptr(dev_groups), dev_groups.shape[0], int(n_entries), 1, 0.0,
                                      _ptr(out), None, _stream()), "phnet_lane_iou_groups")
    return out


MASK_METRICS_MAX_RADIUS, MASK_METRICS_MAX_SIZE = 127, 4096     # PHNET_MASK_METRICS_MAX_RADIUS / _MAX_SIZE of include/phnet_hip.h
MASK_METRICS_COUNTS = ("area_pred", "area_gt", "area_both", "n_fg", "n_gt", "fg_match", "gt_match")


def mask_metric_counts(pred, gt, radius: int, out=None):
    """pred, gt u8 [.., H, W] (any leading dimensions, the same on both; a non-zero byte is foreground) -> int64 [.., 7]: the counts
    of MASK_METRICS_COUNTS per frame by the rules of include/phnet_hip.h (phnet_mask_metrics; csrc/mask_metrics.hip) - the areas of
    the two masks and of their intersection, the sizes of the two boundary maps, and how much of each boundary lies within `radius`
    pixels of the other.  Three graph nodes, no sync; the boundary words live in the shared workspace.  `out`: an int64
    [.., 7] tensor to write into (a captured graph keeps its address)."""
    _req(pred, torch.uint8, "pred"); _req(gt, torch.uint8, "gt")
    if pred.dim() < 2 or pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError(f"mask_metric_counts: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be u8 [.., H, W] of one shape on one device")
    lead, (h, w) = tuple(pred.shape[:-2]), pred.shape[-2:]
    radius = int(radius)
    if not (1 <= h <= MASK_METRICS_MAX_SIZE and 1 <= w <= MASK_METRICS_MAX_SIZE):
        raise ValueError(f"mask_metric_counts: height and width must be in 1..{MASK_METRICS_MAX_SIZE}, got {h} x {w}")
    if not 0 <= radius <= MASK_METRICS_MAX_RADIUS:
        raise ValueError(f"mask_metric_counts: radius must be in 0..{MASK_METRICS_MAX_RADIUS}, got {radius}")
    n = 1
    for d in lead:
        n *= int(d)
    if out is None:
        out = torch.empty(lead + (7,), dtype=torch.int64, device=pred.device)
    else:
        _req(out, torch.int64, "out")
        if tuple(out.shape) != lead + (7,) or out.device != pred.device:
            raise ValueError(f"mask_metric_counts: out must be int64 {lead + (7,)} on {pred.device}, got {tuple(out.shape)}")
    if n == 0:
        return out
    nbytes = lib().phnet_mask_metrics_workspace(n, h, w, radius)
    ws = workspace(nbytes, pred.device)
    check(lib().phnet_mask_metrics(_ptr(pred), _ptr(gt), n, h, w, radius, _ptr(ws), ws.numel(), _ptr(out), _stream()), "phnet_mask_metrics")
    return out


def tune_k_tile(code: int) -> None:
    """Benchmark aid (process-global): phnet_tune_force_k_tile; -5 / -6 switch the three-taps 3x3 forward / dgrad kernel off / on,
    -300 / -301 the tall-tile kernel of the many-row Linear layers (csrc/linrows.hip), -302 takes it for every Linear launch
    without addend / statistics that it can run, whatever the size or the forced plan."""
    check(lib().phnet_tune_force_k_tile(code), "phnet_tune_force_k_tile")


def tune_wgrad(flags: int = 1, target: int = 768) -> None:
    """Benchmark aid (process-global): phnet_tune_wgrad - bit 3 of `flags` switches the three-taps 3x3 weight-gradient kernel off,
    bit 4 gives it 32-pixel steps, bit 5 switches its producer / consumer variant (csrc/wgrad3s.hip) off; a negative `target` is ITS workgroup target, a positive one the generic kernel's."""
    check(lib().phnet_tune_wgrad(flags, target), "phnet_tune_wgrad")


def tune_reset() -> None:
    """Every switch of include/phnet_hip_tuning.h (arithmetic mode included) back to its default."""
    check(lib().phnet_tune_reset(), "phnet_tune_reset")


MMA_MODES = {"f32": 0, "split_bf16": 1, "split3_bf16": 2, "bf16x3": 3, "bf16": 4}


def mma_mode() -> int:
    """The library's current GEMM arithmetic (phnet_tune_mma code; 3 = "bf16x3", 4 = "bf16")."""
    return int(lib().phnet_tune_mma_get())


def set_mma_mode(mode: str) -> None:
    """Arithmetic of the conv / linear GEMM kernels (process-global; set it before a step is captured in a hipGraph):
    "bf16x3" (default) - see below; "f32" = f32-input MFMA (v_mfma_f32_32x32x2_f32, the round-1 default); "split_bf16" = operands split into two bf16 terms in registers, 3 bf16 MFMAs per
    product, f32 accumulation (~4x the rounding noise of "f32"); "split3_bf16" = three bf16 terms (an exact split of the
    f32 value), 6 bf16 MFMAs per product, dropped terms <= 2^-24: the accuracy of "f32" (csrc/igemm.h); "bf16x3" = the same
    exact three-term arithmetic with the split done ONCE while a tile is staged into LDS (bf16 planes, transposed fragment
    reads): the fast form of "split3_bf16"; "bf16" = the inference arithmetic (forward only): every operand element rounded to
    bf16 once while it is staged, one bf16 MFMA per product, f32 accumulation and epilogues (include/phnet_hip_tuning.h has the rule)."""
    if mode not in MMA_MODES:
        raise ValueError(f"unknown GEMM arithmetic {mode!r}: one of {sorted(MMA_MODES)}")
    check(lib().phnet_tune_mma(MMA_MODES[mode]), "phnet_tune_mma")


@contextlib.contextmanager
def mma(mode: str):
    """Runs the block in GEMM arithmetic `mode` (a set_mma_mode name) and puts the previous mode back, also when the block raises.
    Only the arithmetic code is saved and restored, through phnet_tune_mma - which also gives the mode its register ring depth."""
    if mode not in MMA_MODES:
        raise ValueError(f"unknown GEMM arithmetic {mode!r}: one of {sorted(MMA_MODES)}")
    before = mma_mode()
    check(lib().phnet_tune_mma(MMA_MODES[mode]), "phnet_tune_mma")
    try:
        yield
    finally:
        check(lib().phnet_tune_mma(before), "phnet_tune_mma")


PRECISIONS = {"fp32": "bf16x3", "bf16": "bf16"}


def precision_mode(precision: str, training: bool = False) -> str:
    """The set_mma_mode name behind the `precision` keyword of the inference entry points ("fp32" | "bf16")."""
    if precision not in PRECISIONS:
        raise ValueError(f'precision must be "fp32" or "bf16", not {precision!r}')
    if precision == "bf16" and training:
        raise RuntimeError('precision="bf16" is an inference arithmetic (forward-only): call model.eval() first')
    return PRECISIONS[precision]


@contextlib.contextmanager
def precision_scope(precision: str, training: bool = False):
    """`mma(...)` for the `precision` keyword.  "fp32" keeps whichever f32-accurate arithmetic the process is in - the entry points
    behave as they did before the keyword existed, including under a mode a benchmark has set - and leaves only "bf16" for the default."""
    mode = precision_mode(precision, training)
    if precision == "fp32" and mma_mode() != MMA_MODES["bf16"]:
        yield
    else:
        with mma(mode):
            yield
