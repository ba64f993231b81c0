"""What the input format costs (phnet_amd/libs/dataset/openlane/preprocess.py, csrc/preprocess.hip): the workload's geometry,
1280x1920 -> 320x800 with crop 480, B = 32 frames per launch (one step of a 32-stream LaneStream), "nhwc4" output.  Per format
(packed RGB, NV12 at pitch 1920, YUYV at pitch 3840):
  * us per launch from device events around LAUNCHES back-to-back launches (launch gaps included - not a profiler's kernel
    time), after a warm-up, ROUNDS rounds with the three formats alternated inside every round, all in this process.  The launches
    of a run cycle through SETS different input buffers, so that together they exceed the 256 MiB Infinity Cache and the source is
    not simply re-read from it (the buffers hold seeded random bytes: every byte pattern is a valid surface);
  * the bytes of one step's frames, and ms / GB/s of their pinned host -> device copy (device events around COPIES copies).
The expectation stated with the kernel: the NV12 launch reads half the bytes of the RGB launch on the same geometry and should not
be slower; `nv12_vs_rgb` reports the ratio of the medians either way.  Prints one JSON line.  --frames B (default 32)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor

ROUNDS, LAUNCHES, COPIES, WARMUP = 5, 200, 20, 20
GEOM = dict(src_h=1280, src_w=1920, crop_size=480)
OUT_HW = (320, 800)
FORMATS = ("rgb", "nv12", "yuyv")


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def _events(fn, n):
    """Device-event time of n back-to-back calls of fn(i) -> ms per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess: needs an MI355X; nothing is measured without one")
    B = int(_arg("--frames", 32))
    gen = torch.Generator().manual_seed(0)
    pre, bufs, host, nbytes = {}, {}, {}, {}
    for f in FORMATS:
        pre[f] = ClipPreprocessor(*OUT_HW, **GEOM, **({} if f == "rgb" else {"pixel_format": f}))
        shape = (B, *pre[f].frame_shape)
        nbytes[f] = int(torch.tensor(shape).prod())
        sets = max(2, -(-(320 << 20) // nbytes[f]))                        # > 256 MiB of distinct source per cycle
        host[f] = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8).pin_memory()
        bufs[f] = [host[f].roll(s, 0).cuda() for s in range(sets)]
    run = {f: (lambda i, f=f: pre[f](bufs[f][i % len(bufs[f])], layout="nhwc4")) for f in FORMATS}
    for f in FORMATS:
        _events(run[f], WARMUP)
    us = {f: [] for f in FORMATS}
    for _ in range(ROUNDS):
        for f in FORMATS:
            us[f].append(_events(run[f], LAUNCHES) * 1e3)
    copy_ms = {f: [] for f in FORMATS}
    for f in FORMATS:
        _events(lambda i, f=f: bufs[f][0].copy_(host[f], non_blocking=True), 3)
    for _ in range(ROUNDS):
        for f in FORMATS:
            copy_ms[f].append(_events(lambda i, f=f: bufs[f][0].copy_(host[f], non_blocking=True), COPIES))
    out = {"workload": f"pre-processing 1280x1920 -> 320x800, crop 480, {B} frames per launch, nhwc4; {LAUNCHES} launches per run, "
                       f"{ROUNDS} rounds, formats alternated; device events, launch gaps included",
           "out_bytes_per_launch": B * OUT_HW[0] * OUT_HW[1] * 16}
    for f in FORMATS:
        lu, cm = _spread(us[f]), _spread(copy_ms[f])
        out[f] = {"frame_bytes": nbytes[f] // B, "step_bytes": nbytes[f], "input_sets": len(bufs[f]), "us_per_launch": lu,
                  "frames_per_s_launch_only": round(B / (lu["median"] * 1e-6)), "h2d_ms_per_step": cm,
                  "h2d_GB_per_s": round(nbytes[f] / (cm["median"] * 1e-3) / 1e9, 2)}
    out["nv12_vs_rgb"] = round(out["nv12"]["us_per_launch"]["median"] / out["rgb"]["us_per_launch"]["median"], 3)
    out["yuyv_vs_rgb"] = round(out["yuyv"]["us_per_launch"]["median"] / out["rgb"]["us_per_launch"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
