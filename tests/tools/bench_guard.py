"""What the guarded optimizer step costs (csrc/optim_guard.hip; include/phnet_hip.h "guarded step") at the arena length of the ResNet-34
model (counted from the module tree on the CPU; --elements overrides), random finite gradients, max_grad_norm = 10 and skip_nonfinite
on - so every step clips and none is skipped.

Two FlatAdamW over one flat parameter each, one unguarded and one guarded; `step()` of each captured in a hipGraph of its own.  ms per
step from device events around STEPS back-to-back replays after a warm-up, ROUNDS rounds, the two alternated inside every round, one
process: median (min - max).  Then, launches alone (eager, back to back, the same event bracket): phnet_adamw_step, phnet_grad_guard
(phase A + phase B - the library has no entry point for one phase) and phnet_adamw_step_guarded, with the GB/s of the bytes each must
move (adamw: 7 streams of 4 n bytes; guard: one read of 4 n bytes).  Last, in a pass of its own, torch's profiler splits the guard launch
into its two kernels (device durations of guard_reduce_kernel = phase A and guard_finalize_kernel = phase B, and of adamw_kernel); where
the profiler reports no kernels the split is null = not measured.  Prints one JSON line."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from phnet_amd import hip_ops as K
from phnet_amd.arena import GradArena
from phnet_amd.optim import FlatAdamW

ROUNDS, STEPS, WARMUP = 3, 200, 20


def resnet34_arena_elements() -> int:
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import RouterOL
    from phnet_amd.libs.utils.loss4OLV3 import Criterion4OL
    cfg = make_cfg(arch="resnet34")
    model = RouterOL(cfg, Criterion4OL(cfg))
    n = sum(p.numel() for p in model.parameters() if p.requires_grad)
    return (n + 3) // 4 * 4


def _events(call, reps, warmup):
    for _ in range(warmup):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _summary(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def _optimizer(n, grad, **kw):
    p = torch.nn.Parameter(torch.randn(n, device="cuda") * 0.05)
    arena = GradArena([p], flatten_params=True)
    opt = FlatAdamW(arena, n_decay=n - n // 300, lr=1e-4, **kw)          # 0.3 % of the elements are undecayed 1-D parameters
    arena.flat.copy_(grad)
    opt.step()                                                          # eager once: lr on the device, kernels loaded
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            opt.step()
    torch.cuda.current_stream().wait_stream(st)
    return opt, arena, graph


def _kernel_split(calls, reps):
    """{kernel name fragment: mean device us} from torch's profiler, or None where it saw no kernels."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            for call in calls:
                call()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for frag in ("guard_reduce_kernel", "guard_finalize_kernel", "adamw_guarded_kernel", "adamw_kernel"):
            if frag in ev.key:
                total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                if ev.count and total:
                    out[frag] = total / ev.count
                break
    return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=0, help="arena length (default: the ResNet-34 model's)")
    ap.add_argument("--no-profiler", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guard: needs a GPU")
    n = (args.elements + 3) // 4 * 4 if args.elements else resnet34_arena_elements()
    grad = torch.randn(n, device="cuda") * 0.01                          # norm = 0.01 sqrt(n) > 10 from n = 1e6 on
    plain, arena_p, graph_p = _optimizer(n, grad)
    guarded, arena_g, graph_g = _optimizer(n, grad, max_grad_norm=10.0, skip_nonfinite=True)
    steps = {"unguarded": [], "guarded": []}
    for _ in range(ROUNDS):
        steps["unguarded"].append(_events(graph_p.replay, STEPS, WARMUP))
        steps["guarded"].append(_events(graph_g.replay, STEPS, WARMUP))
    stats = guarded.guard_stats()
    hyper = (1e-4, 0.9, 0.999, 1e-8, 1e-2)
    launches = {
        "adamw": lambda: K.adamw_step(arena_p.flat_params, arena_p.flat, plain.exp_avg, plain.exp_avg_sq, plain.n_decay, plain.step_count,
                                      *hyper, lr_dev=plain.lr_dev),
        "guard": lambda: K.grad_guard(arena_g.flat, guarded._guard_ws, guarded._guard_stats, guarded.step_count, 10.0, True),
        "adamw_guarded": lambda: K.adamw_step_guarded(arena_g.flat_params, arena_g.flat, guarded.exp_avg, guarded.exp_avg_sq, guarded.n_decay,
                                                      guarded.step_count, *hyper, guarded.clip_coef, guarded.last_skipped, lr_dev=guarded.lr_dev)}
    alone = {k: [] for k in launches}
    for _ in range(ROUNDS):
        for k, call in launches.items():
            alone[k].append(_events(call, STEPS, WARMUP))
    nbytes = {"adamw": 7 * 4 * n, "guard": 4 * n, "adamw_guarded": 7 * 4 * n}
    med = {k: statistics.median(v) for k, v in steps.items()}
    out = {"workload": f"FlatAdamW.step() over {n} elements ({4 * n / 1e6:.1f} MB per stream), captured; ms per step from device events around "
                       f"{STEPS} back-to-back replays, {ROUNDS} alternated rounds: median (min - max)",
           "elements": n, "chunks": -(-n // K.GUARD_CHUNK),
           "step_ms": {k: _summary(v) for k, v in steps.items()},
           "guard_cost_ms": round(med["guarded"] - med["unguarded"], 4), "guard_cost_ratio": round(med["guarded"] / med["unguarded"], 4),
           "launch_ms": {k: _summary(v) for k, v in alone.items()},
           "launch_GBps": {k: round(nbytes[k] / (statistics.median(v) * 1e-3) / 1e9, 1) for k, v in alone.items()},
           "last_step": stats}
    split = None
    if not args.no_profiler:
        split = _kernel_split(list(launches.values()), 20)
    if split:
        out["kernel_us"] = {k: round(v, 2) for k, v in split.items()}
        out["kernel_GBps"] = {k: round({"guard_reduce_kernel": 4 * n, "adamw_kernel": 28 * n, "adamw_guarded_kernel": 28 * n}[k] / (v * 1e-6) / 1e9, 1)
                              for k, v in split.items() if k != "guard_finalize_kernel"}
    else:
        out["kernel_us"] = out["kernel_GBps"] = None
    print(json.dumps(out))
    arena_p.release(); arena_g.release()


if __name__ == "__main__":
    main()
