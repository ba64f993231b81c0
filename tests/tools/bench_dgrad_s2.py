"""The six stride-2 data gradients of the trunk backward at one 5-frame 320 x 800 clip (ResNet-34: the 3x3 / pad 1 and the 1x1
downsample convolution of the layer1->2, layer2->3 and layer3->4 transitions), every one the launch phnet_conv2d_dgrad makes for it
(conv_igemm_kernel<64, 64, true, 16, true, 3, 4, false>, split counts 1 / 1, 2 / 1, 4 / 2) with its split-K reduce: csrc/igemm_tile.h DIL.
Device time per call in us from a hipGraph of LAUNCHES calls (no launch gaps of the host), ROUNDS rounds with all variants
alternated inside every round, one process: median (min - max).
  * baseline: phnet_conv2d_dgrad of the library named by --baseline-lib (a build of the parent commit, `python -m phnet_amd.build` in
    a checkout of it: phnet_amd/lib/libphnet_hip.so), through ctypes with the same pointers; left out when no library is named;
  * branch: this tree's phnet_conv2d_dgrad through the same bare ctypes call.
Before timing the two outputs are compared (max |difference| over max |baseline|; unsplit launches add the same products in the
same order and must be bit-equal).  --mma f32: the f32-input MFMA arithmetic.  Prints one JSON line."""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from phnet_amd import _lib
from phnet_amd import hip_ops as K

ROUNDS, LAUNCHES, REPLAYS = 5, 20, 5
SHAPES = [  # name, (N, Hi, Wi, Ci, Co, R, stride, pad) of the forward convolution
    ("layer2 3x3", (5, 80, 200, 64, 128, 3, 2, 1)), ("layer2 1x1", (5, 80, 200, 64, 128, 1, 2, 0)),
    ("layer3 3x3", (5, 40, 100, 128, 256, 3, 2, 1)), ("layer3 1x1", (5, 40, 100, 128, 256, 1, 2, 0)),
    ("layer4 3x3", (5, 20, 50, 256, 512, 3, 2, 1)), ("layer4 1x1", (5, 20, 50, 256, 512, 1, 2, 0)),
]
MMA = {"bf16x3": 3, "f32": 0}


def _declare(handle, name):
    fn = getattr(handle, name)
    fn.restype, fn.argtypes = next((r, a) for n, r, a in _lib.declared_functions() if n == name)
    return fn


def _graph(call):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            call()
    g.replay()
    torch.cuda.synchronize()
    return g


def _time(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPLAYS):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (REPLAYS * LAUNCHES) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None, help="a libphnet_hip.so built from the parent commit")
    ap.add_argument("--mma", default="bf16x3", choices=sorted(MMA))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dgrad_s2: needs a GPU")
    libs = {"branch": _lib.lib()}
    if args.baseline_lib:
        libs = {"baseline": ctypes.CDLL(args.baseline_lib), **libs}
    for handle in libs.values():
        _lib.check(_declare(handle, "phnet_tune_mma")(MMA[args.mma]), "phnet_tune_mma")
    out = {"workload": f"stride-2 data gradients of a 5-frame 320x800 clip, {args.mma}; us per call (reduce included) from a hipGraph of "
                       f"{LAUNCHES} calls replayed {REPLAYS} times, {ROUNDS} alternated rounds: median (min - max)", "launches": {}}
    torch.manual_seed(5)
    for name, (n, hi, wi, ci, co, r, stride, pad) in SHAPES:
        ho, wo = K.conv_out_hw(hi, wi, r, r, stride, pad)
        dy = torch.randn(n, ho, wo, co, device="cuda")
        w = torch.randn(co, r, r, ci, device="cuda") * (ci * r * r) ** -0.5
        need = K.splitk_workspace_bytes(n * hi * wi, ci)
        ws = K.workspace(need, dy.device) if need else None
        kernel, splits = K._kernel(libs["branch"].phnet_conv2d_kernel, 1, n, hi, wi, ci, co, r, r, stride, pad, need)
        dx = {k: torch.full((n, hi, wi, ci), float("nan"), device="cuda") for k in libs}
        calls = {k: (lambda f=_declare(h, "phnet_conv2d_dgrad"), o=dx[k]: _lib.check(
            f(dy.data_ptr(), w.data_ptr(), None, o.data_ptr(), n, hi, wi, ci, co, r, r, stride, pad, K._ptr(ws), need, K._stream()),
            "phnet_conv2d_dgrad")) for k, h in libs.items()}
        graphs = {k: _graph(c) for k, c in calls.items()}
        rec = {"kernel": kernel, "splits": splits}
        if "baseline" in dx:
            diff = float((dx["branch"] - dx["baseline"]).abs().max()) / float(dx["baseline"].abs().max())
            rec["max_diff_over_max_baseline"] = diff
            rec["bit_equal"] = bool(torch.equal(dx["branch"], dx["baseline"]))
        times = {k: [] for k in graphs}
        for _ in range(ROUNDS):
            for k, g in graphs.items():
                times[k].append(_time(g))
        rec["us"] = {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}
        if "baseline" in times:
            rec["branch_over_baseline"] = round(statistics.median(times["branch"]) / statistics.median(times["baseline"]), 3)
        out["launches"][name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
