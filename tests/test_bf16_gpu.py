"""The "bf16" inference arithmetic (phnet_tune_mma(4); precision="bf16" on the inference entry points) on the MI355X.

Kernels: every forward family the mode has (conv_igemm_kernel<..., 4, ...> with and without buffer loads, K tiles 16 and 64,
split-K; conv3p_bf16_kernel in both column widths, single-job and job-table packing; linrows_bf16_kernel) against the fp64
convolution of the bf16-ROUNDED operands (tests/bf16_cases.py) at the 2e-5 of tests/test_kernels_gpu.py - after the rounding every
product is exact in f32 and only the f32 accumulation is left - and, so that the reference is known to discriminate, the default
arithmetic's result of the same launch must FAIL that comparison (it multiplies the unrounded operands: ~1e-3 of the scale).
Integer operands in [-4, 4] are bf16-exact with partial sums below 2^24: there the result must equal the int64 convolution and the
default arithmetic's result bit for bit.  The backward entry points raise.

Model: the eval trunk record by record (own input, folded weight, bias, residual) at the same 2e-5; no cache leak between the
precisions; bit-equal repeats; graph replay == eager; stream == clip as tests/test_stream_gpu.py / test_stream_v2_gpu.py hold the
fp32 ones; captured graphs keep their arithmetic; training untouched by a bf16 inference call; bad arguments raise."""
import functools

import numpy as np
import pytest
import torch

from tests import bf16_cases as C
from tests import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops
    return hip_ops


@pytest.fixture
def bf16(ops):
    """The process in arithmetic mode 4 for one test; every tuning switch back to its default afterwards."""
    ops.tune_reset()
    ops.set_mma_mode("bf16")
    yield ops
    ops.tune_reset()
    assert ops.mma_mode() == 3


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def err_of(got, want):
    """(max |got - want|, the scale close() of tests/test_kernels_gpu.py judges it against)."""
    got = got.detach().cpu().double().numpy().reshape(want.shape)
    return float(np.abs(got - want).max()), max(1.0, float(np.abs(want).max()))


def assert_close(got, want, what):
    err, scale = err_of(got, want)
    print(f"{what}: max err {err:.3e} = {err / scale:.3e} of the scale (bound {C.TOL:g})")
    assert err <= C.TOL * scale, (what, err, scale)


@functools.lru_cache(maxsize=None)
def operands(name, integers=False):
    return C.make_operands(C.case(name), seed=len(name), integers=integers)


@functools.lru_cache(maxsize=None)
def reference(name, bias=False, addend=False, relu=False):
    """fp64 on rounded operands; computed once per (case, epilogue) and shared."""
    c = C.case(name)
    x, w, b, a = operands(name)
    ref = C.conv_ref64(x, w, b if bias else None, a if addend else None, relu, stride=c[7], pad=c[8])
    ref.setflags(write=False)
    return ref


def kernel_name(ops, c, packed):
    _, n, hi, wi, ci, co, r, stride, pad = c
    lib = ops.lib()
    if packed:
        return ops._kernel(lib.phnet_conv3p_kernel, n * hi * wi, ci, co, ops.splitk_workspace_bytes(n * hi * wi, co))
    ho, wo = C.out_hw(hi, wi, r, stride, pad)
    co4 = co + (-co) % 4
    return ops._kernel(lib.phnet_conv2d_kernel, 0, n, hi, wi, ci, co4, r, r, stride, pad, ops.splitk_workspace_bytes(n * ho * wo, co4))


def launch(ops, c, x, w, bias=None, addend=None, relu=False, stats=False, packed=False, image=None):
    """One forward launch of the case in the CURRENT arithmetic.  packed: through conv3p on the image the arithmetic takes."""
    name, n, hi, wi, ci, co, r, stride, pad = c
    xd, wd = cuda(x), cuda(w)
    bd = None if bias is None else cuda(bias)
    ad = None if addend is None else cuda(addend)
    if packed:
        img = ops.conv3p_pack(wd, False) if image is None else image
        return ops.conv3p(xd, img, co, bias=bd, addend=ad, relu=relu, stats=stats)
    if co % 4:                                                    # the 6-wide head output: the public Linear pads it (bf16_cases.py)
        from phnet_amd import functional as PF
        assert r == 1 and ad is None and not stats
        with torch.no_grad():
            return PF.linear(xd.view(n, ci), wd.view(co, ci), bd, relu).view(n, 1, 1, co)
    return ops.conv2d_fwd(xd, wd, bd, stride, pad, relu=relu, addend=ad, stats=stats)


KERNEL_RUNS = [(c[0], False) for c in C.GPU_CASES] + [(n, True) for n in C.PACKED]


@pytest.mark.parametrize("name,packed", KERNEL_RUNS, ids=[f"{n}-{'packed' if p else 'generic'}" for n, p in KERNEL_RUNS])
def test_kernel_vs_fp64_on_rounded_operands(ops, bf16, name, packed):
    c = C.case(name)
    x, w, _, _ = operands(name)
    ref = reference(name)
    if name == "lin_tall":
        ops.tune_k_tile(-302)
    if name == "l4_3x3_splitk":
        ops.tune_k_tile(-401)                                     # mode 4 does not split K on its own: mode 3's split plan for this case
    kn, splits = kernel_name(ops, c, packed)
    print(f"{name}: {kn} x {splits}")
    want = "conv3p_bf16_kernel<" if packed else "linrows_bf16_kernel<" if name == "lin_tall" else "conv_igemm_kernel<"
    assert kn.startswith(want) and (not kn.startswith("conv_igemm") or kn.split(", ")[5] == "4"), kn
    assert (splits > 1) == (name == "l4_3x3_splitk"), (kn, splits)
    assert_close(launch(ops, c, x, w, packed=packed), ref, f"{name} bf16")
    # the same launch in the default arithmetic multiplies the UNROUNDED operands: it must miss this reference (~1e-3 of the scale)
    ops.set_mma_mode("bf16x3")
    if name == "lin_tall":
        ops.tune_k_tile(-302)
    err, scale = err_of(launch(ops, c, x, w, packed=packed), ref)
    print(f"{name} default arithmetic against the rounded reference: {err / scale:.3e} of the scale")
    assert err > C.TOL * scale, (name, err, scale)


EPILOGUES = [("l2_3x3_s2", False), ("lat_1x1", False), ("l1_3x3_rows", True), ("l2_3x3_128", True), ("l4_3x3_splitk", True),
             ("l4_3x3_splitk", False)]


@pytest.mark.parametrize("name,packed", EPILOGUES, ids=[f"{n}-{'packed' if p else 'generic'}" for n, p in EPILOGUES])
def test_epilogues_stay_f32(ops, bf16, name, packed):
    """bias; bias + addend (residual) + ReLU; the statistics rows = (sum, sum of squares) of the f32 outputs, per channel."""
    c = C.case(name)
    x, w, b, a = operands(name)
    if name == "l4_3x3_splitk":
        ops.tune_k_tile(-401)                                     # epilogues of the split path: bias / addend / ReLU / statistics in the reduce
        assert kernel_name(ops, c, packed)[1] > 1
    assert_close(launch(ops, c, x, w, bias=b, packed=packed), reference(name, bias=True), f"{name} bias")
    assert_close(launch(ops, c, x, w, bias=b, addend=a, relu=True, packed=packed), reference(name, True, True, True), f"{name} bias+addend+relu")
    co = c[5]
    y, (part, nblk) = launch(ops, c, x, w, stats=True, packed=packed)
    assert_close(y, reference(name), f"{name} with statistics")
    sums = part[:nblk * 2 * co * 4].view(torch.float32).view(nblk, 2, co).double().sum(0).cpu()
    yd = y.double().cpu().reshape(-1, co)
    for what, got, want, scale in (("sum", sums[0], yd.sum(0), yd.abs().sum(0).max()), ("sum of squares", sums[1], (yd ** 2).sum(0), (yd ** 2).sum(0).max())):
        e = float((got - want).abs().max())
        print(f"{name} statistics {what}: {e / float(scale):.3e} of the scale")
        assert e <= C.TOL * float(scale), (name, what, e, float(scale))


def test_forced_split_counts_and_tiles(ops, bf16):
    """phnet_tune_force_conv_tile: a split count the heuristic does not pick (3), and the three larger tiles of the generic kernel."""
    c = C.case("l2_3x3_s2")
    x, w, b, _ = operands("l2_3x3_s2")
    for bm, bn, sp in ((64, 64, 3), (128, 128, 2), (128, 64, 1), (64, 128, 4)):
        ops.check(ops.lib().phnet_tune_force_conv_tile(bm, bn, sp), "phnet_tune_force_conv_tile")
        kn, splits = kernel_name(ops, c, False)
        assert kn.startswith(f"conv_igemm_kernel<{bm}, {bn}, false, ") and kn.split(", ")[5] == "4" and splits == sp, (kn, splits)
        assert_close(launch(ops, c, x, w, bias=b), reference("l2_3x3_s2", bias=True), f"{bm}x{bn} split {sp}")
    ops.check(ops.lib().phnet_tune_force_conv_tile(0, 0, 0), "phnet_tune_force_conv_tile")


def test_packed_wide_tile_and_job_table(ops, bf16):
    """conv3p_bf16_kernel<2> (the dispatch takes it from 16384 pixels on: here through a lowered pixel count is not possible, so at
    that size, one launch) and the one-plane images of a Conv3pPackPlan: byte for byte the single-job images."""
    lib = ops.lib()
    n, hi, wi, ci, co = 2, 64, 128, 128, 128                      # 16384 pixels
    rng = np.random.default_rng(5)
    x = rng.integers(-4, 5, size=(n, hi, wi, ci)).astype(np.float32)
    w = rng.integers(-4, 5, size=(co, 3, 3, ci)).astype(np.float32)
    kn, _ = ops._kernel(lib.phnet_conv3p_kernel, n * hi * wi, ci, co, ops.splitk_workspace_bytes(n * hi * wi, co))
    assert kn == "conv3p_bf16_kernel<2>", kn
    got = ops.conv3p(cuda(x), ops.conv3p_pack(cuda(w), False), co)
    want = torch.nn.functional.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double().permute(0, 3, 1, 2),
                                      padding=1).permute(0, 2, 3, 1)
    assert torch.equal(got.cpu().double(), want)                  # integers: exact
    # ---- job table against single jobs ----
    ws = [cuda(operands(nm)[1]) for nm in ("l1_3x3", "l2_3x3_128", "l4_3x3_splitk")]
    plan = ops.Conv3pPackPlan(ws, with_dgrad=False, planes=1)
    plan.refresh()
    assert plan.buf.numel() * 3 == sum(ops.conv3p_packed_bytes(t.shape[0], t.shape[3]) for t in ws)
    for t, img in zip(ws, plan.images):
        single = ops.conv3p_pack(t, False, planes=1)
        assert single.numel() * 3 == ops.conv3p_packed_bytes(t.shape[0], t.shape[3]) and torch.equal(img[False], single)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.Conv3pPackPlan(ws, with_dgrad=True, planes=1)
    c = C.case("l1_3x3")
    assert_close(launch(ops, c, *operands("l1_3x3")[:2], packed=True, image=plan.images[0][False]), reference("l1_3x3"), "job-table image")


EXACT = [("l2_3x3_s2", False), ("l1_3x3_rows", True), ("lin_tall", False), ("stem_7x7", False), ("lin_head", False)]


@pytest.mark.parametrize("name,packed", EXACT, ids=[f"{n}-{'packed' if p else 'generic'}" for n, p in EXACT])
def test_integer_operands_are_exact(ops, bf16, name, packed):
    """Operands in [-4, 4]: nothing rounds anywhere, so any indexing or layout slip of the one-plane paths shows with zero tolerance.
    (The 128-column packed tile's exact case is in test_packed_wide_tile_and_job_table, at the size the dispatch takes it.)"""
    c = C.case(name)
    x, w, b, a = operands(name, True)
    can_add = not name.startswith("lin_tall")                     # the tall tile takes launches without addend
    want = C.conv_ref64(x, w, b, a if can_add else None, False, stride=c[7], pad=c[8], rounded=False)
    assert float(np.abs(want).max()) < 2 ** 24 and np.array_equal(want, np.rint(want))
    if name == "lin_tall":
        ops.tune_k_tile(-302)
        assert kernel_name(ops, c, False)[0].startswith("linrows_bf16_kernel<")
    got = launch(ops, c, x, w, bias=b, addend=a if can_add else None, packed=packed)
    assert np.array_equal(got.cpu().double().numpy(), want), name
    ops.set_mma_mode("bf16x3")
    if name == "lin_tall":
        ops.tune_k_tile(-302)
    default = launch(ops, c, x, w, bias=b, addend=a if can_add else None, packed=packed)
    assert torch.equal(got, default), name


def test_backward_entry_points_raise_and_the_process_survives(ops, bf16):
    c = C.case("l1_3x3")
    x, w, _, _ = operands("l1_3x3")
    xd, wd = cuda(x), cuda(w)
    dy = torch.randn(2, 16, 20, 64, device="cuda")
    with pytest.raises(RuntimeError, match="bf16"):
        ops.conv2d_dgrad(dy, wd, (16, 20), 1, 1)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.conv2d_wgrad(dy, xd, tuple(wd.shape), 1, 1)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.linear_bwd(torch.randn(240, 64, device="cuda"), torch.randn(240, 64, device="cuda"), torch.randn(64, 64, device="cuda"),
                       torch.zeros(64, 64, device="cuda"), None, False)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.conv3p(dy, ops.conv3p_pack(wd, False), 64, dgrad=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.conv3p_pack(wd, True)
    # the library itself: PHNET_ERR_ARG, nothing launched
    lib = ops.lib()
    dx = torch.empty_like(xd)
    assert lib.phnet_conv2d_dgrad(dy.data_ptr(), wd.data_ptr(), None, dx.data_ptr(), 2, 16, 20, 64, 64, 3, 3, 1, 1, None, 0, None) == -1
    dw = torch.empty_like(wd)
    assert lib.phnet_conv2d_wgrad(dy.data_ptr(), xd.data_ptr(), dw.data_ptr(), None, 2, 16, 20, 64, 64, 3, 3, 1, 1, 0, None, 0, None) == -1
    torch.cuda.synchronize()
    ops.tune_reset()
    ref = C.conv_ref64(x, w, stride=1, pad=1, rounded=False)
    assert_close(ops.conv2d_fwd(xd, wd, None, 1, 1), ref, "default-mode forward afterwards")
    got = ops.conv2d_dgrad(dy, wd, (16, 20), 1, 1)
    want = torch.nn.functional.conv_transpose2d(dy.cpu().double().permute(0, 3, 1, 2), wd.cpu().double().permute(0, 3, 1, 2), padding=1)
    assert_close(got, want.permute(0, 2, 3, 1).contiguous().numpy(), "default-mode data gradient afterwards")


# ------------------------------------------------------------------------------------------------------ trunk
def _tiny_v1(arch="resnet18"):
    from oracle import phnet_cpu as O
    return O.Geometry(img_h=64, img_w=160, arch=arch, conf_threshold=0.3)


def _build_v1(arch="resnet18", calibrated=None):
    import tests.test_stream_gpu as S1
    g = _tiny_v1(arch)
    model = S1._build(g, conf_threshold=0.3)
    if calibrated is not None:                                   # running statistics that match the weights: activations O(1-10)
        sd = synth.make_state(g)
        synth.calibrate_running_stats_(sd, calibrated, g.arch)
        model.load_state_dict(sd, strict=True)
    return g, model


def _build_v2():
    import tests.test_stream_v2_gpu as S2
    g = S2._tiny()
    return g, S2._build(g)


@pytest.mark.parametrize("arch", ["resnet18", "resnet34"])
def test_trunk_record_by_record_and_no_cache_leak(ops, arch):
    from phnet_amd import trunk
    g = _tiny_v1(arch)
    frames = synth.make_clip(g, 2)
    _, model = _build_v1(arch, calibrated=frames)
    recs = []
    real = trunk._conv_bn

    def recording(tape, x, conv, bn, training, relu, residual=None, **kw):
        y = real(tape, x, conv, bn, training, relu, residual=residual, **kw)
        rec = tape[-1]
        wf, bf, pk = trunk._folded(conv, bn, rec.w)               # the cache entry the launch used (this arithmetic's slot)
        recs.append((conv, rec.x_in, wf, bf, residual, relu, rec.stride, rec.pad, y, pk))
        return y
    x = frames.cuda()
    with torch.no_grad():
        fp32_a = [f.clone() for f in model.backbone(x)]
        trunk._conv_bn = recording
        try:
            with ops.mma("bf16"):
                bf = [f.clone() for f in model.backbone(x)]
        finally:
            trunk._conv_bn = real
        assert ops.mma_mode() == 3
        fp32_b = [f.clone() for f in model.backbone(x)]
        with ops.mma("bf16"):
            bf_b = [f.clone() for f in model.backbone(x)]
    assert len(recs) == {"resnet18": 20, "resnet34": 36}[arch]
    packed = 0
    for i, (conv, xin, wf, bfold, res, relu, stride, pad, y, pk) in enumerate(recs):
        if pk is not None:
            packed += 1
            assert pk.numel() * 3 == ops.conv3p_packed_bytes(wf.shape[0], wf.shape[3]), i      # the one-plane image
        ref = C.conv_ref64(xin.cpu().numpy(), wf.cpu().numpy(), bfold.cpu().numpy(), None if res is None else res.cpu().numpy(), relu,
                           stride=stride, pad=pad)
        assert_close(y, ref, f"{arch} record {i} ({tuple(wf.shape)}, stride {stride}{', packed' if pk is not None else ''})")
    assert packed >= 8, packed
    for a, b, c, d in zip(fp32_a, fp32_b, bf, bf_b):
        assert torch.equal(a, b) and torch.equal(c, d) and not torch.equal(a, c)


# ------------------------------------------------------------------------------------------------------ model
def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_model_precision_keyword(ops, family):
    """Repeatability, graph == eager, a replay keeps the arithmetic of its capture, bf16 != fp32, the process mode stays 3."""
    from phnet_amd.graphed import GraphedInference
    g, model = _build_v1() if family == "v1" else _build_v2()
    clip = synth.make_clip(g, 4, seed=40).cuda()
    clips = torch.stack([clip, synth.make_clip(g, 4, seed=41).cuda()])
    with torch.no_grad():
        fp32 = model.infer_device(clip)
        a = model.infer_device(clip, precision="bf16")
        assert ops.mma_mode() == 3
        b = model.infer_device(clip, precision="bf16")
        assert _same(a, b)                                        # repeatability
        assert _same(fp32, model.infer_device(clip)) and _same(fp32, model.infer_device(clip, precision="fp32"))
        assert not torch.equal(a[0], fp32[0])                     # the keyword did something
        ca = model.infer_clips_device(clips, precision="bf16")
        assert ops.mma_mode() == 3
        assert _same(ca, model.infer_clips_device(clips, precision="bf16")) and not torch.equal(ca[0], model.infer_clips_device(clips)[0])
        pa = model.infer_points_device(clip, precision="bf16")
        assert ops.mma_mode() == 3 and _same(pa, a)
        tr = model.track_clips(a[0], a[1], precision="bf16")
        assert ops.mma_mode() == 3 and all(torch.equal(x, y) for x, y in zip(tr, model.track_clips(a[0], a[1])))
    gb = GraphedInference(model, clip, precision="bf16")
    assert ops.mma_mode() == 3
    assert _same(gb(clip), a)                                     # replay under process mode 3: still the bf16 result, bit for bit
    gf = GraphedInference(model, clip)
    with ops.mma("bf16"):
        assert _same(gf(clip), fp32)                              # captured in fp32, replayed inside mma("bf16"): still fp32
        assert _same(gb(clip), a)
    assert ops.mma_mode() == 3
    gp = GraphedInference(model, clips, polylines=True, precision="bf16")
    assert _same(gp(clips), ca) and ops.mma_mode() == 3


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_bf16_stream_equals_bf16_clip(ops, family):
    """As test_stream_equals_clip of tests/test_stream_gpu.py / test_stream_v2_gpu.py, both sides in precision="bf16": counts and
    kept anchors equal, kept rows within that file's BATCH_TOL (2e-4 / 2e-3).

    Why this holds: mode 4 does not split K on its own (csrc/conv.hip plan_conv).  The step of a stream runs the trunk on one frame,
    the clip on T; with mode 3's plan the two cut K into different numbers of slabs, an activation comes out with other last bits
    (fp32: 9e-7 of the FPN maps' maximum) and the next layer ROUNDS it to bf16 - one bf16 ulp (4e-3) apart where it sits at a rounding
    boundary, which the cascade amplifies.  Measured with that plan (tune_k_tile(-401)) on this geometry: FPN maps of frame 0 3.8e-3
    (v1) / 5.1e-3 (v2) of their maximum apart, kept anchors equal on 0/11 and 1/12 frames, kept rows up to 3.8e-2 apart.  Unsplit,
    every output's accumulation chain is the same whatever the batch, and the stream equals the clip bit for bit (difference 0.0 in
    FPN maps, counts, anchors and rows, both families)."""
    import tests.test_stream_gpu as S1
    import tests.test_stream_v2_gpu as S2
    S = S1 if family == "v1" else S2
    g, model = _build_v1() if family == "v1" else _build_v2()
    T = 11 if family == "v1" else 12
    if family == "v2":
        model.faithful_memory = False
    clip = synth.make_clip(g, T, seed=40).cuda()
    with torch.no_grad():
        rows_c, nums_c, anch_c = model.infer_device(clip, precision="bf16")[:3]
    s = model.open_stream(streams=1, frame_hw=(g.img_h, g.img_w), graph=True, precision="bf16")
    assert ops.mma_mode() == 3
    e = model.open_stream(streams=1, frame_hw=(g.img_h, g.img_w), graph=False, precision="bf16")
    kept_late = 0
    for t in range(T):
        rows, num, anchors = s.step(clip[t:t + 1])
        assert ops.mma_mode() == 3
        rows_e, num_e, anch_e = e.step(clip[t:t + 1])
        assert ops.mma_mode() == 3
        assert torch.equal(num, num_e) and torch.equal(anchors, anch_e)
        S._close(rows, rows_e, S.GRAPH_TOL, f"frame {t} graph vs eager")
        k = S._same_frame((rows[0], num[0], anchors[0]), (rows_c[t], nums_c[t], anch_c[t]), S.BATCH_TOL, f"frame {t}")
        if t >= model.save_freq_max:
            kept_late += k
    assert kept_late > 0


def test_training_is_untouched_by_a_bf16_inference_call(ops):
    """One training step on the tiny model: loss and every gradient bit-equal before and after a precision="bf16" inference call on
    the same model (the fold cache, the pack plans and the process mode are all the call could have left behind)."""
    import tests.test_model_gpu as TM
    from oracle import phnet_cpu as O
    g = O.Geometry(img_h=64, img_w=160, arch="resnet18")
    model = TM._build(g).train()
    frames, lanes = synth.make_clip(g, 2).cuda(), synth.make_targets(g, 2).cuda()
    stats = {k: v.clone() for k, v in model.state_dict().items()}

    def step():
        model.load_state_dict(stats, strict=True)                 # the running statistics a training forward moves
        model.train()
        model.zero_grad(set_to_none=True)
        loss = model({"frame": frames, "lanes": lanes})
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}
    loss0, grads0 = step()
    model.eval()
    with torch.no_grad():
        model.infer_device(frames, precision="bf16")
    assert ops.mma_mode() == 3
    loss1, grads1 = step()
    worst = max(float((grads0[n] - grads1[n]).abs().max()) for n in grads0)
    print(f"loss {float(loss0)!r} / {float(loss1)!r}; largest gradient difference {worst:.3e}")
    assert torch.equal(loss0, loss1)
    differ = [n for n in grads0 if not torch.equal(grads0[n], grads1[n])]
    assert not differ, differ[:5]


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_bad_arguments(ops, family):
    from phnet_amd.graphed import GraphedInference
    g, model = _build_v1() if family == "v1" else _build_v2()
    clip = synth.make_clip(g, 2).cuda()
    with torch.no_grad():
        for call in (lambda p: model.infer_device(clip, precision=p), lambda p: model.infer_clips_device(clip[None], precision=p),
                     lambda p: model.infer_points_device(clip, precision=p), lambda p: model.open_stream(streams=1, precision=p),
                     lambda p: GraphedInference(model, clip, precision=p),
                     lambda p: model.track_clips(torch.zeros(2, 4, 78, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), precision=p)):
            model.eval()
            with pytest.raises(ValueError):
                call("fp16")
            model.train()
            with pytest.raises(RuntimeError, match="bf16"):
                call("bf16")
            assert ops.mma_mode() == 3
    model.eval()
