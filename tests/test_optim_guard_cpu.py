"""The guarded AdamW step, the part that needs no GPU: both entry points are declared, exported and refuse bad arguments before any
launch; the numpy restatement of tests/guard_cases.py is held to torch on the CPU (clip_grad_norm_ + AdamW + GradScaler); and an
optimizer built without the two new arguments is today's, attribute for attribute."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from phnet_amd import build as hip_build
from tests import guard_cases as GC

ERR_ARG, ERR_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


def close(a, b, tol=2e-4, what=""):                     # the project's AdamW metric (tests/test_kernels_gpu.py close(), used there at 2e-6)
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------------------ the entry points
def test_both_symbols_are_declared_and_exported(built):
    names = {n: a for n, _, a in _lib.declared_functions(_lib.HEADER)}
    assert len(names["phnet_grad_guard"]) == 11 and len(names["phnet_adamw_step_guarded"]) == 16 and len(names["phnet_adamw_step"]) == 14
    assert hasattr(built, "phnet_grad_guard") and hasattr(built, "phnet_adamw_step_guarded")
    assert built.phnet_abi_version() == 1
    header = open(_lib.HEADER).read()
    for rule in ("element -> lane -> wavefront -> chunk partial -> ascending chunk index", "exponent field is all ones",
                 "norm = fl32(sqrt(S) * (double)inv)", "coef = min(1, max_norm / (norm + 1e-6f))", "g itself is never written",
                 "skip = PHNET_GUARD_SKIP_NONFINITE && (nonfinite > 0 ||", "p, m, v and step keep their bits", "step[0] += 1"):
        assert rule in header, rule


def test_published_constants_match_the_python_side():
    from phnet_amd import hip_ops
    defines = dict(re.findall(r"#define (PHNET_GUARD_\w+) (\d+)", open(_lib.HEADER).read()))
    assert int(defines["PHNET_GUARD_CHUNK"]) == hip_ops.GUARD_CHUNK == GC.CHUNK
    assert int(defines["PHNET_GUARD_WS_BYTES_PER_CHUNK"]) == hip_ops.GUARD_WS_BYTES_PER_CHUNK
    assert int(defines["PHNET_GUARD_STATS_WORDS"]) == hip_ops.GUARD_STATS_WORDS
    assert (int(defines["PHNET_GUARD_SKIP_NONFINITE"]), int(defines["PHNET_GUARD_CLIP"])) == (hip_ops.GUARD_SKIP_NONFINITE, hip_ops.GUARD_CLIP)
    assert hip_ops.grad_guard_workspace_bytes(GC.CHUNK) == 12 and hip_ops.grad_guard_workspace_bytes(GC.CHUNK + 4) == 24


def test_grad_guard_validates_without_a_gpu(built):
    """Each refusal comes before any launch (no device is touched: this runs without one).  Non-null pointers are made-up addresses - a
    call that got past the checks would try to launch."""
    p = 0x1000

    def guard(g=p, n=GC.CHUNK + 4, ws=p, ws_bytes=24, stats=p, step=p, max_norm=1.0, flags=3, scale=None, found=None):
        return built.phnet_grad_guard(g, n, ws, ws_bytes, stats, step, max_norm, flags, scale, found, None)

    for key in ("g", "ws", "stats", "step"):
        assert guard(**{key: None}) == ERR_ARG, key
        assert guard(**{key: None}, n=0) == ERR_ARG, key
    assert guard(n=-4) == ERR_ARG and guard(n=-1) == ERR_ARG
    for n in (1, 2, 3, GC.CHUNK + 1, GC.CHUNK + 6):
        assert guard(n=n) == ERR_ARG, n
    for bad in (-1.0, -1e-30, float("nan"), float("-inf")):
        assert guard(max_norm=bad) == ERR_ARG, bad
        assert guard(max_norm=bad, flags=1) == ERR_ARG, bad
    assert guard(flags=4) == ERR_ARG and guard(flags=-1) == ERR_ARG
    assert guard(ws_bytes=23) == ERR_WORKSPACE and guard(n=GC.CHUNK, ws_bytes=11) == ERR_WORKSPACE


def test_adamw_step_guarded_validates_without_a_gpu(built):
    p = 0x1000

    def step(ptrs=(p,) * 4, n=64, n_decay=33, stepc=p, mult=p, skip=p):
        return built.phnet_adamw_step_guarded(*ptrs, n, n_decay, stepc, 1e-3, None, 0.9, 0.999, 1e-8, 0.01, mult, skip, None)

    for i in range(4):
        assert step(tuple(None if j == i else p for j in range(4))) == ERR_ARG, i
    assert step(stepc=None) == ERR_ARG and step(mult=None) == ERR_ARG and step(skip=None) == ERR_ARG
    assert step(n=-4, n_decay=0) == ERR_ARG and step(n=62) == ERR_ARG and step(n=63) == ERR_ARG
    assert step(n_decay=-1) == ERR_ARG and step(n_decay=65) == ERR_ARG
    assert step(n=0, n_decay=0) == 0 and step((None,) * 4, n=0, n_decay=0) == 0        # a no-op, as phnet_adamw_step
    # the unguarded entry point answers the same way
    assert built.phnet_adamw_step(p, p, p, p, 64, 65, p, 1e-3, None, 0.9, 0.999, 1e-8, 0.01, None) == ERR_ARG
    assert built.phnet_adamw_step(p, p, p, p, 62, 0, p, 1e-3, None, 0.9, 0.999, 1e-8, 0.01, None) == ERR_ARG


def test_guard_kernels_compile_without_scratch_or_spills(tmp_path):
    import subprocess
    src = os.path.join(hip_build.CSRC, "optim_guard.hip")
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "optim_guard.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", out.stderr)
    assert sum("guard_reduce_kernel" in k for k in kernels) == 1 and sum("adamw_guarded_kernel" in k for k in kernels) == 1
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)] == [0] * len(kernels)
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)] == [0] * len(kernels)


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_case_table_is_complete_and_does_what_it_says():
    cs = GC.cases()
    assert [c["name"] for c in cs] == list(GC.NAMES)
    assert {c["n"] for c in cs} >= set(GC.LENGTHS) and all(c["n"] % 4 == 0 and c["n_decay"] % 4 != 0 for c in cs)
    for c in cs:
        r = GC.guard(c["grad"], c["max_norm"], c["skip_nonfinite"], c["grad_scale"], c["found_inf"])
        assert r["skip"] == c["skip"] and r["nonfinite"] == c["nonfinite"], c["name"]
        want = GC.f64_norm(c)                                                              # numpy's pairwise float64 sum
        assert (np.isnan(want) and np.isnan(r["norm"])) or abs(int(r["norm"].view(np.int32)) - int(want.view(np.int32))) <= 1, c["name"]
    by = {c["name"]: GC.guard(c["grad"], c["max_norm"], c["skip_nonfinite"], c["grad_scale"], c["found_inf"]) for c in cs}
    assert all(abs(by[f"len_{n}"]["mult"] - 0.5) < 1e-5 for n in GC.LENGTHS)                  # (the 1e-6 of rule 4 shows on a norm of ~0.5)
    assert by["quiet_4"]["mult"] == 1 and by["clip_below"]["mult"] == 1
    assert abs(by["clip_above"]["mult"] - 0.5) < 1e-6 and abs(by["clip_above_1e4"]["mult"] - 1e-4) < 1e-9
    assert np.isinf(by["overflow_norm"]["norm"]) and np.isfinite(by["overflow_norm"]["S"]) and by["overflow_norm"]["nonfinite"] == 0
    assert 0 < by["denormals"]["norm"] < 1e-36 and by["denormals"]["S"] > 0 and not by["denormals"]["skip"]
    assert np.isnan(by["clip_nan_no_skip"]["mult"]) and not by["clip_nan_no_skip"]["skip"]
    assert abs(by["scale_clean"]["mult"] - 0.5 / 65536) < 1e-11 and not by["scale_clean"]["skip"]
    assert by["scale_found_inf"]["skip"] and by["scale_found_inf"]["nonfinite"] == 0 and by["scale_found_inf"]["mult"] == np.float32(1 / 65536)
    for v in ("pinf", "ninf"):
        assert np.isinf(by[f"{v}_first"]["norm"])
    assert np.isnan(by["nan_last"]["norm"]) and np.isnan(by["nan_and_inf"]["norm"])


def test_sum_order_is_fixed_and_sensitive_to_nothing_but_the_data():
    g = GC.case(f"len_{3 * GC.CHUNK + 260}")["grad"]
    a, b = GC.sum_squares(g), GC.sum_squares(g.copy())
    assert a[0].tobytes() == b[0].tobytes() and a[1] == 0
    assert GC.sum_squares(np.zeros(4, np.float32))[0] == 0.0
    one = np.zeros(GC.CHUNK + 4, np.float32)
    one[GC.CHUNK + 3] = 3.0
    assert GC.sum_squares(one) == (9.0, 0)


def _problem(seed=0):
    """Three 'parameters' (a matrix with weight decay, a bias and a 3-D tensor without), their flat layout padded to a multiple of 4."""
    r = np.random.default_rng(seed)
    shapes = [(40, 30), (17,), (5, 7, 3)]
    values = [r.standard_normal(s).astype(np.float32) for s in shapes]
    n = sum(v.size for v in values)
    flat = np.zeros((n + 3) // 4 * 4, np.float32)
    flat[:n] = np.concatenate([v.ravel() for v in values])
    return shapes, values, flat, values[0].size, n


HYPER = dict(lr=5e-3, betas=(0.9, 0.99), eps=1e-8)


def _torch_twin(values, dtype=torch.float32):
    params = [torch.nn.Parameter(torch.from_numpy(v).to(dtype)) for v in values]
    opt = torch.optim.AdamW([{"params": params[:1], "weight_decay": 0.05}, {"params": params[1:], "weight_decay": 0.0}], **HYPER)
    return params, opt


def _set_grads(params, shapes, flat_grad):
    off = 0
    for p, s in zip(params, shapes):
        k = int(np.prod(s))
        p.grad = torch.from_numpy(flat_grad[off:off + k].reshape(s).copy()).to(p.dtype)
        off += k


def _flat(params, n_flat):
    out = torch.zeros(n_flat, dtype=torch.float64)
    cat = torch.cat([p.detach().double().reshape(-1) for p in params])
    out[:cat.numel()] = cat
    return out


def test_restatement_matches_clip_grad_norm_and_adamw_over_four_steps():
    """torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on the CPU, gradient scales chosen so that steps 1 and 3 clip and steps 0 and 2
    do not.  torch clips in float32 from a norm of per-tensor norms; the restatement's norm is the float64 one: they agree to a few
    float32 ulps, and the parameters at the project's AdamW bound (close(), 2e-6)."""
    shapes, values, flat, n_decay, n = _problem()
    params, topt = _torch_twin(values)
    ours = GC.Restated(flat, n_decay, HYPER["lr"], HYPER["betas"], HYPER["eps"], 0.05, max_norm=10.0)
    r = np.random.default_rng(1)
    clipped = []
    for step, scale in enumerate((0.1, 3.0, 0.1, 3.0)):
        g = np.zeros_like(flat)
        g[:n] = r.standard_normal(n).astype(np.float32) * np.float32(scale)
        _set_grads(params, shapes, g)
        keep = g.copy()
        tnorm = float(torch.nn.utils.clip_grad_norm_(params, max_norm=10.0, norm_type=2))
        topt.step()
        got = ours.step(g)
        assert np.array_equal(g, keep)                                       # rule 5: the gradient is not rewritten
        clipped.append(tnorm > 10.0)
        assert (got["mult"] < 1.0) == (tnorm > 10.0) and not got["skip"]
        assert abs(float(got["norm"]) - tnorm) <= 4e-6 * tnorm, (step, got["norm"], tnorm)
        assert ours.step_count == step + 1 == int(topt.state[params[0]]["step"])
        close(torch.from_numpy(ours.p), _flat(params, flat.size), 2e-6, f"step {step}")
    assert clipped == [False, True, False, True]


def test_restatement_matches_gradscaler_skips_over_four_steps():
    """torch.amp.GradScaler('cpu') around torch.optim.AdamW, with clipping between unscale_ and step as torch's recipe has it; the
    restatement takes the SCALED gradient and the scale (rules 3-5).  Step 1 carries an inf, step 2 a NaN: both skip, the scale halves
    each time, and the step counters stay behind exactly as torch's do."""
    shapes, values, flat, n_decay, n = _problem(2)
    params, topt = _torch_twin(values)
    scaler = torch.amp.GradScaler("cpu", init_scale=65536.0)
    scaler.scale(torch.ones(()))                                             # builds the scale tensor
    ours = GC.Restated(flat, n_decay, HYPER["lr"], HYPER["betas"], HYPER["eps"], 0.05, max_norm=10.0, skip_nonfinite=True)
    r = np.random.default_rng(3)
    skips, scales = [], []
    for step, (mag, poison) in enumerate(((0.1, None), (0.1, np.inf), (3.0, np.nan), (3.0, None))):
        s = scaler.get_scale()
        scales.append(s)
        g = np.zeros_like(flat)
        g[:n] = r.standard_normal(n).astype(np.float32) * np.float32(mag) * np.float32(s)
        if poison is not None:
            g[n // 2] = poison
        _set_grads(params, shapes, g)
        before = _flat(params, flat.size)
        scaler.unscale_(topt)
        torch.nn.utils.clip_grad_norm_(params, max_norm=10.0, norm_type=2)
        scaler.step(topt)
        scaler.update()
        torch_skipped = torch.equal(before, _flat(params, flat.size))
        got = ours.step(g, grad_scale=s, found_inf=0.0)
        skips.append(got["skip"])
        assert got["skip"] == torch_skipped == (poison is not None), step
        tstep = int(topt.state[params[0]]["step"]) if topt.state else 0
        assert ours.step_count == tstep, (step, ours.step_count, tstep)
        close(torch.from_numpy(ours.p), _flat(params, flat.size), 2e-6, f"step {step}")
    assert skips == [False, True, True, False] and ours.skipped_steps == 2 and ours.step_count == 2
    assert scales == [65536.0, 65536.0, 32768.0, 16384.0] and scaler.get_scale() == 16384.0
    # found_inf alone (a finite gradient): skipped as well, nothing moves
    keep = ours.p.copy()
    got = ours.step(np.ones_like(flat), grad_scale=16384.0, found_inf=1.0)
    assert got["skip"] and got["nonfinite"] == 0 and np.array_equal(keep, ours.p) and ours.step_count == 2 and ours.skipped_steps == 3


# ------------------------------------------------------------------------------------------------------------ the host side
def _net():
    torch.manual_seed(4)
    return torch.nn.Sequential(torch.nn.Conv2d(8, 12, 3, bias=False), torch.nn.BatchNorm2d(12), torch.nn.Flatten(), torch.nn.Linear(12 * 36, 7))


def test_defaults_stay_todays():
    from phnet_amd.optim import FlatAdamW
    sig = inspect.signature(FlatAdamW.__init__).parameters
    assert sig["max_grad_norm"].default is None and sig["skip_nonfinite"].default is False
    opt, arena = FlatAdamW.for_model(_net())
    try:
        assert "_step_supports_amp_scaling" not in vars(opt) and not getattr(opt, "_step_supports_amp_scaling", False)
        assert not opt.guarded and opt.max_grad_norm is None and opt.skip_nonfinite is False
        for name in ("_guard_ws", "_guard_stats", "grad_norm", "clip_coef", "last_skipped", "nonfinite", "skipped_steps"):
            assert not hasattr(opt, name), name
        with pytest.raises(RuntimeError):
            opt.guard_stats()
        plain_keys = {k: sorted(v) for k, v in opt.state_dict()["state"].items()}
        plain_groups = [sorted(g) for g in opt.state_dict()["param_groups"]]
    finally:
        arena.release()
    for kw in (dict(max_grad_norm=10.0), dict(skip_nonfinite=True), dict(max_grad_norm=0.0, skip_nonfinite=True)):
        opt, arena = FlatAdamW.for_model(_net(), **kw)
        try:
            assert opt.guarded and vars(opt)["_step_supports_amp_scaling"] is True
            assert "grad_scaler" not in inspect.signature(opt.step).parameters
            assert (opt.grad_norm.dtype, opt.clip_coef.dtype) == (torch.float32, torch.float32)
            assert all(t.dtype == torch.int64 and t.shape == (1,) for t in (opt.last_skipped, opt.nonfinite, opt.skipped_steps))
            assert opt.grad_norm.shape == opt.clip_coef.shape == (1,)
            assert opt._guard_ws.numel() >= 12 * -(-arena.flat.numel() // GC.CHUNK)
            sd = opt.state_dict()                                                 # torch's own layout, nothing of the guard in it
            assert set(sd) == {"state", "param_groups"} and {k: sorted(v) for k, v in sd["state"].items()} == plain_keys
            assert [sorted(g) for g in sd["param_groups"]] == plain_groups
            opt.skipped_steps.fill_(5)
            opt.load_state_dict(sd)
            assert int(opt.skipped_steps) == 0 and int(opt.step_count) == 0
        finally:
            arena.release()
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            FlatAdamW.for_model(_net(), max_grad_norm=bad)
