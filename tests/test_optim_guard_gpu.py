"""The guarded AdamW step on a real MI355X (include/phnet_hip.h, "guarded step"): the norm and the flags of every case of
tests/guard_cases.py, the update and the skip bit for bit, torch's clip_grad_norm_ + AdamW and GradScaler as twins, a captured step
replayed over a poisoned gradient, and the whole training step of the tiny model.  Run with -m gpu."""
import numpy as np
import pytest
import torch

from tests import guard_cases as GC

pytestmark = pytest.mark.gpu

HYPER = dict(lr=5e-3, betas=(0.9, 0.99), eps=1e-8)
START_STEP = 3                     # the bias corrections of a run that is under way


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from phnet_amd import hip_ops
    return hip_ops


def close(a, b, tol=2e-4, what=""):                     # tests/test_kernels_gpu.py close()
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * scale, (what, err, scale)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    """Bit for bit, except that two NaNs count as equal whatever their payloads (which operand's payload a multiply passes on is the
    hardware's business, not rule 5's)."""
    a, b = a.detach(), b.detach()
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool(((bits(a) == bits(b)) | both_nan).all())


def ulps(a: np.float32, b: np.float32) -> int:
    """Distance in float32 steps between two values of one sign; 0 for two NaNs, a large number for a NaN against a number."""
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 30
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ------------------------------------------------------------------------------------------------ items 1-3: every case, run once
_RUNS = {}


def run_case(ops, name):
    """One guarded step of case `name` on raw buffers (no model), next to the unguarded kernel fed fl32(g * mult) computed by torch."""
    if name in _RUNS:
        return _RUNS[name]
    c = GC.case(name)
    n, dev = c["n"], "cuda"
    gen = torch.Generator().manual_seed(n % 1000 + len(name))
    g = torch.from_numpy(c["grad"]).to(dev)
    p0 = torch.randn(n, generator=gen).to(dev)
    m0 = (torch.randn(n, generator=gen) * 0.1).to(dev)
    v0 = (torch.rand(n, generator=gen) * 0.01).to(dev)
    scale = None if c["grad_scale"] is None else torch.full((), c["grad_scale"], dtype=torch.float32, device=dev)
    found = None if c["found_inf"] is None else torch.full((), c["found_inf"], dtype=torch.float32, device=dev)
    out = {"case": c}
    stats_runs = []
    for rep in range(2):                                                       # two calls on the same buffer: the same bits
        stats = torch.zeros(ops.GUARD_STATS_WORDS, dtype=torch.int64, device=dev)
        stats[3] = 7                                                           # a run that has skipped before
        ws = torch.full((ops.grad_guard_workspace_bytes(n),), 0xA5 if rep else 0x5A, dtype=torch.uint8, device=dev)     # never zeroed
        step = torch.full((1,), START_STEP, dtype=torch.int64, device=dev)
        ops.grad_guard(g, ws, stats, step, c["max_norm"], c["skip_nonfinite"], scale, found)
        stats_runs.append((stats, step))
    (stats, step), (stats2, step2) = stats_runs
    out["stats_bits_repeat"] = torch.equal(stats, stats2) and torch.equal(step, step2)
    f = stats.view(torch.float32)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.adamw_step_guarded(p, g, m, v, c["n_decay"], step, HYPER["lr"], *HYPER["betas"], HYPER["eps"], 0.05, f[1:2], stats[1:2])
    # the unguarded kernel on the pre-multiplied gradient
    mult = f[1:2].clone()
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    ops.adamw_step(pr, g * mult, mr, vr, c["n_decay"], torch.full((1,), START_STEP + 1, dtype=torch.int64, device=dev),
                   HYPER["lr"], *HYPER["betas"], HYPER["eps"], 0.05)
    torch.cuda.synchronize()
    host = stats.cpu()
    out.update(norm=np.float32(host[0:1].view(torch.float32)[0].item()), mult=np.float32(host[0:1].view(torch.float32)[1].item()),
               last_skipped=int(host[1]), nonfinite=int(host[2]), skipped_steps=int(host[3]), step=int(step),
               arena_untouched=torch.equal(bits(g), bits(torch.from_numpy(c["grad"]).to(dev))),
               state_untouched=all(torch.equal(bits(a), bits(b)) for a, b in ((p, p0), (m, m0), (v, v0))),
               equals_unguarded=all(same_bits(a, b) for a, b in ((p, pr), (m, mr), (v, vr))),
               moved=not torch.equal(bits(p), bits(p0)))
    _RUNS[name] = out
    return out


@pytest.mark.parametrize("name", GC.NAMES)
def test_norm_and_flags(ops, name):
    """nonfinite / last_skipped / skipped_steps exact; grad_norm within ONE float32 ulp of fl32(sqrt(sum (double)g^2) * inv) from torch in
    float64 (a fixed-order float64 sum differs from any other by ~1e-14 relative, which can move the result across at most one float32
    rounding boundary) and, beyond what that asks, equal in every bit to the numpy restatement of the header's summation order; a second
    call over a differently filled workspace gives the same bits.  (The implementation has no grid parameter: one workgroup per chunk.)"""
    r, c = run_case(ops, name), GC.case(name)
    g64 = torch.from_numpy(c["grad"]).double()
    inv = float(np.float32(1.0) / np.float32(c["grad_scale"])) if c["grad_scale"] is not None else 1.0
    want = np.float32((g64.square().sum().sqrt() * inv).to(torch.float32).item())
    restated = GC.guard(c["grad"], c["max_norm"], c["skip_nonfinite"], c["grad_scale"], c["found_inf"])
    print(name, "norm", r["norm"], "torch f64", want, "restated", restated["norm"], "mult", r["mult"], restated["mult"])
    assert r["nonfinite"] == c["nonfinite"] and r["last_skipped"] == int(c["skip"]) and r["skipped_steps"] == 7 + int(c["skip"])
    assert r["step"] == START_STEP + (0 if c["skip"] else 1)
    assert ulps(r["norm"], want) <= 1, (r["norm"], want)
    assert ulps(r["norm"], restated["norm"]) == 0 and ulps(r["mult"], restated["mult"]) == 0, (r["norm"], restated["norm"], r["mult"], restated["mult"])
    assert r["stats_bits_repeat"]


@pytest.mark.parametrize("name", GC.NAMES)
def test_update_equals_unguarded_kernel_on_premultiplied_gradient(ops, name):
    """With mult read back from the device, the guarded step on (p, g, m, v) is, bit for bit, phnet_adamw_step on (p, fl32(g * mult), m, v);
    where nothing triggers (mult == 1) that says guarded == unguarded."""
    r, c = run_case(ops, name), GC.case(name)
    if c["skip"]:
        assert r["state_untouched"]
        return
    assert r["equals_unguarded"] and r["moved"]
    if name.startswith("quiet") or name == "clip_below":
        assert r["mult"] == 1.0


@pytest.mark.parametrize("name", GC.NAMES)
def test_skip_keeps_every_bit_and_the_arena_is_never_written(ops, name):
    r, c = run_case(ops, name), GC.case(name)
    assert r["arena_untouched"]
    if c["skip"]:
        assert r["state_untouched"] and r["step"] == START_STEP and not r["moved"]


# ------------------------------------------------------------------------------------------------ items 4-6: the small net
def make_net():
    torch.manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Conv2d(8, 12, 3, bias=False), torch.nn.BatchNorm2d(12), torch.nn.Flatten(), torch.nn.Linear(12 * 36, 7)).cuda()
    net[0].weight.data = net[0].weight.data.contiguous(memory_format=torch.channels_last)
    return net


def torch_adamw(ref):
    from phnet_amd.optim import split_decay
    decay, no_decay = split_decay(ref)
    return torch.optim.AdamW([{"params": decay, "weight_decay": 0.05}, {"params": no_decay, "weight_decay": 0.0}], **HYPER)


def accumulate(net, loss):
    """What the HIP backward kernels do: accumulate into the arena's .grad views."""
    for p, gr in zip(net.parameters(), torch.autograd.grad(loss, list(net.parameters()))):
        p.grad.add_(gr)


def test_clipping_matches_clip_grad_norm_and_torch_adamw(ops):
    """The net of test_flat_adamw_matches_torch_adamw, four steps, the loss of steps 1 and 3 a hundred times that of steps 0 and 2;
    max_grad_norm = 10 x the first step's norm, so torch's own returned norms say: clip on 1 and 3, not on 0 and 2."""
    from phnet_amd.optim import FlatAdamW
    ref, net = make_net(), make_net()
    topt = torch_adamw(ref)
    gen = torch.Generator(device="cuda").manual_seed(9)
    xs = [torch.randn(5, 8, 8, 8, device="cuda", generator=gen) for _ in range(4)]
    ref(xs[0]).square().mean().backward()
    max_norm = 10.0 * float(torch.nn.utils.clip_grad_norm_(list(ref.parameters()), float("inf")))
    fopt, arena = FlatAdamW.for_model(net, weight_decay=0.05, max_grad_norm=max_norm, **HYPER)
    try:
        clipped = []
        for step, k in enumerate((1.0, 100.0, 1.0, 100.0)):
            topt.zero_grad(set_to_none=True)
            fopt.zero_grad()
            (ref(xs[step]).square().mean() * k).backward()
            accumulate(net, net(xs[step]).square().mean() * k)
            raw = arena.flat.clone()
            tnorm = float(torch.nn.utils.clip_grad_norm_(list(ref.parameters()), max_norm, norm_type=2))
            topt.step()
            fopt.step()
            s = fopt.guard_stats()
            print("step", step, "torch norm", tnorm, "ours", s, "max_norm", max_norm)
            clipped.append(tnorm > max_norm)
            assert (s["clip_coef"] < 1.0) == (tnorm > max_norm) and s["last_skipped"] == 0 and s["nonfinite"] == 0
            assert abs(s["grad_norm"] - tnorm) <= 4e-6 * tnorm                   # torch: float32 norm of per-tensor float32 norms
            assert torch.equal(bits(arena.flat), bits(raw))                      # .grad keeps the raw gradient
            for a, b in zip(ref.parameters(), net.parameters()):
                close(b, a, 2e-6, f"step {step}")
        assert clipped == [False, True, False, True]
        assert int(fopt.step_count) == 4 and fopt.guard_stats()["skipped_steps"] == 0
    finally:
        arena.release()


def test_gradscaler_runs_sync_free_and_skips_with_torch(ops):
    """The reference's loop (scaler.scale(loss).backward(); scaler.step(opt); scaler.update()) around FlatAdamW(skip_nonfinite=True) and
    around torch.optim.AdamW; on step 2 one gradient element of each is inf.  scaler.step + update on our side run with torch's
    synchronisation check set to raise."""
    from phnet_amd.optim import FlatAdamW
    ref, net = make_net(), make_net()
    topt = torch_adamw(ref)
    fopt, arena = FlatAdamW.for_model(net, weight_decay=0.05, skip_nonfinite=True, **HYPER)
    tscaler, fscaler = (torch.amp.GradScaler("cuda", init_scale=65536.0) for _ in range(2))
    gen = torch.Generator(device="cuda").manual_seed(11)
    try:
        skipped = []
        for step in range(4):
            x = torch.randn(5, 8, 8, 8, device="cuda", generator=gen)
            topt.zero_grad(set_to_none=True)
            fopt.zero_grad()
            tscaler.scale(ref(x).square().mean()).backward()
            fscaler.scale(net(x).square().mean()).backward()
            if step == 2:
                arena.flat[5] = float("inf")
                next(iter(ref.parameters())).grad[0, 0, 0, 0] = float("inf")
            scale_before = fscaler.get_scale()
            before = arena.flat_params.clone()
            tbefore = [p.detach().clone() for p in ref.parameters()]
            tscaler.step(topt)
            tscaler.update()
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                fscaler.step(fopt)
                fscaler.update()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            s = fopt.guard_stats()
            print("step", step, s, "scale", scale_before, "->", fscaler.get_scale())
            ours_skipped = torch.equal(bits(before), bits(arena.flat_params))
            torch_skipped = all(torch.equal(a, b.detach()) for a, b in zip(tbefore, ref.parameters()))
            skipped.append(ours_skipped)
            assert ours_skipped == torch_skipped == bool(s["last_skipped"]) == (step == 2)
            assert fscaler.get_scale() == tscaler.get_scale() == (scale_before / 2 if step == 2 else scale_before)
            assert s["nonfinite"] == (1 if step == 2 else 0)
            assert abs(s["clip_coef"] * scale_before - 1.0) == 0.0                # mult = 1 / scale
            if step != 2:
                for a, b in zip(ref.parameters(), net.parameters()):
                    close(b, a, 2e-6, f"step {step}")
        assert skipped == [False, False, True, False]
        assert int(fopt.step_count) == 3 == int(topt.state[next(iter(ref.parameters()))]["step"])
        assert fopt.guard_stats()["skipped_steps"] == 1
        for a, b in zip(ref.parameters(), net.parameters()):
            close(b, a, 2e-6, "end")
    finally:
        arena.release()


def test_captured_guarded_step_replays_over_a_poisoned_gradient(ops):
    """One captured guarded step(), replayed over a clean, a poisoned (one inf written into the arena between the replays) and a clean
    gradient: step_count 1, 1, 2, skipped_steps 0, 1, 1, and the parameters equal, bit for bit, an eager guarded optimizer's."""
    from phnet_amd.optim import FlatAdamW
    neta, netb = make_net(), make_net()
    kw = dict(weight_decay=0.05, max_grad_norm=0.05, skip_nonfinite=True, **HYPER)
    (fa, arena_a), (fb, arena_b) = FlatAdamW.for_model(neta, **kw), FlatAdamW.for_model(netb, **kw)
    try:
        n = arena_a.flat.numel()
        gen = torch.Generator(device="cuda").manual_seed(13)
        grads = [torch.randn(n, device="cuda", generator=gen) * 0.01 for _ in range(3)]
        grads[1][n // 3] = float("inf")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            with torch.cuda.graph(graph, stream=st):
                fa.step()
        torch.cuda.current_stream().wait_stream(st)
        assert int(fa.step_count) == 0                                       # capturing executes nothing
        seen = []
        for g in grads:
            arena_a.flat.copy_(g)
            arena_b.flat.copy_(g)
            fa.sync_lr()
            graph.replay()
            fb.step()
            sa, sb = fa.guard_stats(), fb.guard_stats()
            seen.append((int(fa.step_count), sa["skipped_steps"], sa["last_skipped"]))
            assert sa == sb or (np.isnan(sa["grad_norm"]) and np.isnan(sb["grad_norm"])), (sa, sb)
        print(seen)
        assert seen == [(1, 0, 0), (1, 1, 1), (2, 1, 0)]
        assert int(fb.step_count) == 2
        assert sa["clip_coef"] < 1.0                                         # the clean steps were clipped as well
        for a, b in ((arena_a.flat_params, arena_b.flat_params), (fa.exp_avg, fb.exp_avg), (fa.exp_avg_sq, fb.exp_avg_sq)):
            assert torch.equal(bits(a), bits(b))
    finally:
        arena_a.release(); arena_b.release()


# ------------------------------------------------------------------------------------------------ item 7: the real step
def test_graphed_train_step_skips_a_poisoned_step_and_goes_on():
    """GraphedTrainStep(between=hook) on the tiny ResNet-18 64x160 model with a clipped, skipping FlatAdamW: the hook writes inf into the
    gradient arena on its second call only (plain arithmetic in a float buffer).  That step leaves every weight bit alone, the next one
    moves them."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import phnet_cpu as O
    from phnet_amd.config import make_cfg
    from phnet_amd.graphed import GraphedTrainStep
    from phnet_amd.libs.models.Router4OL import RouterOL
    from phnet_amd.libs.utils.loss4OLV3 import Criterion4OL
    from phnet_amd.optim import FlatAdamW
    from tests import synth
    g = O.Geometry(img_h=64, img_w=160, arch="resnet18")
    cfg = make_cfg(img_h=g.img_h, img_w=g.img_w, arch=g.arch)
    model = RouterOL(cfg, Criterion4OL(cfg))
    model.load_state_dict(synth.make_state(g), strict=True)
    model = model.cuda().train()
    T = 2
    frames, lanes = synth.make_clip(g, T).cuda(), synth.make_targets(g, T).cuda()
    opt, arena = FlatAdamW.for_model(model, lr=1e-4, max_grad_norm=10.0, skip_nonfinite=True)
    calls = []

    def hook():
        calls.append(len(calls))
        if len(calls) == 2:
            arena.flat[arena.flat.numel() // 2] = float("inf")

    try:
        step = GraphedTrainStep(model, opt, frames, lanes, loss_divisor=T, warmup=1, arena=arena, between=hook)      # call 1: the eager warm-up
        assert len(calls) == 1 and opt.guard_stats()["skipped_steps"] == 0 and int(opt.step_count) == 1
        w0 = arena.flat_params.clone()
        step(frames)                                                          # call 2: poisoned
        s1 = opt.guard_stats()
        w1 = arena.flat_params.clone()
        step(frames)                                                          # call 3: clean
        s2 = opt.guard_stats()
        print(s1, s2)
        assert len(calls) == 3
        assert torch.equal(bits(w0), bits(w1)) and s1["last_skipped"] == 1 and s1["nonfinite"] == 1 and s1["skipped_steps"] == 1
        assert not torch.equal(bits(w1), bits(arena.flat_params)) and s2["last_skipped"] == 0 and s2["nonfinite"] == 0
        assert s2["skipped_steps"] == 1 and int(opt.step_count) == 2 and np.isfinite(s2["grad_norm"]) and s2["grad_norm"] > 0
        assert bool(torch.isfinite(arena.flat_params).all())
    finally:
        arena.release()
