"""What drawing the lanes costs (phnet_amd/overlay.py, csrc/lane_draw.hip) at the camera's 1280 x 1920, lanes of 72 points, width 12.
  * the launch alone, us per frame, with 4 and 8 lanes, one frame per launch and eight: the label map alone, and the overlay drawn
    on packed RGB, NV12 (pitch 2048) and YUYV frames.  Next to each figure the FLOOR it is compared with: the bytes the launch must
    move (source pixels read once, output written once; the points are a few KB) over the HBM bandwidth a copy achieves on this
    part (6.29 TB/s measured, 8 TB/s on the data sheet), and the achieved fraction of it.  At one frame per launch the figure is
    mostly the launch itself: nothing of this size reaches its floor.
  * HOST BASELINE, labelled as such: the numpy restatement of the same rules (tests/overlay_cases.py draw_reference) on the
    polylines copied to the host - what a caller without this launch would do; cv2 is not available here.
  * the stream step (ResNet-34, 3x320x800, NV12 camera frames in, polylines and tracks on) WITHOUT and WITH render=, three
    alternated runs of each in this process; the step without render= is the parent's step - the option adds one launch to it and
    changes nothing else.
Prints one JSON line.  --frames F (default 240 timed steps / 400 timed launches); --no-stream skips the model."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from phnet_amd import hip_ops as K
from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
from phnet_amd.overlay import LaneRenderer
from bench_stream import _arg, _timed                       # the stream tool beside this file: same arguments, same clock
from bench_polylines import _spread, ROUNDS

H0, W0, CROP, S, WIDTH = 1280, 1920, 480, 72, 12
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12                    # bytes / s: a float4 copy on this part; the data sheet


def synthetic_polylines(F, L, n_lanes, device):
    """n_lanes straight lanes per frame from the bottom edge to a vanishing point, S points each, laid out as lane_points does."""
    ys = np.linspace(1.0, 0.05, S, dtype=np.float64)
    pts = np.zeros((F, L, S, 2), dtype=np.float32)
    for k in range(n_lanes):
        x_bottom = (k + 0.5) / n_lanes
        pts[:, k, :, 0] = 0.5 + (x_bottom - 0.5) * (ys - 0.05) / 0.95 * 1.4
        pts[:, k, :, 1] = ys
    count = np.zeros((F, L), dtype=np.int32)
    count[:, :n_lanes] = S
    return dict(points=torch.from_numpy(pts).to(device), count=torch.from_numpy(count).to(device),
                lanes_num=torch.full((F,), n_lanes, dtype=torch.int32, device=device),
                slot=torch.arange(L, dtype=torch.int32, device=device).repeat(F, 1))


def kernel_rows(reps):
    out = {}
    pres = {"rgb": ClipPreprocessor(320, 800), "nv12": ClipPreprocessor(320, 800, pixel_format="nv12", pitch=2048),
            "yuyv": ClipPreprocessor(320, 800, pixel_format="yuyv")}
    px = H0 * W0
    moved = {"label_map": px, "overlay_rgb": 6 * px, "overlay_nv12": px * 3 // 2 + 3 * px, "overlay_yuyv": 5 * px}
    for n_lanes in (4, 8):
        for F in (1, 8):
            pl = synthetic_polylines(F, 8, n_lanes, "cuda")
            for name in moved:
                fmt = name.split("_")[1] if name != "label_map" else "rgb"
                r = LaneRenderer.for_preprocessor(pres[fmt], lane_width=WIDTH, alpha=128, label_map=name == "label_map", overlay=name != "label_map")
                frames = torch.randint(0, 256, (F, *r.frame_shape), dtype=torch.uint8, device="cuda") if r.overlay else None
                bufs = r.buffers((F,), "cuda")
                for _ in range(10):
                    r.render(pl, frames=frames, out=bufs)
                us = _timed(lambda i: r.render(pl, frames=frames, out=bufs), reps) * 1e3 / F
                floor = moved[name] / HBM_MEASURED * 1e6
                out[f"{name}_lanes{n_lanes}_F{F}"] = {"us_per_frame": round(us, 2), "bytes_per_frame": moved[name],
                                                      "floor_us_6.29TBps": round(floor, 2), "floor_us_8TBps": round(moved[name] / HBM_SPEC * 1e6, 2),
                                                      "fraction_of_floor": round(floor / us, 3)}
    return out


def host_baseline(reps=3):
    """numpy on the copied polylines (tests/overlay_cases.py), label map only: the copy is inside the timed region."""
    import time
    from tests import overlay_cases as OC
    out = {}
    for n_lanes in (4, 8):
        pl = synthetic_polylines(1, 8, n_lanes, "cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            host = {k: v.cpu().numpy() for k, v in pl.items()}
            OC.draw_reference(host["points"], host["count"], host["lanes_num"], (H0, W0), W0, H0 - CROP, CROP, WIDTH)
        out[f"host_numpy_label_map_lanes{n_lanes}_ms_per_frame"] = round((time.perf_counter() - t0) / reps * 1e3, 2)
    return out


def stream_rows(frames_timed, H=320, W=800, arch="resnet34"):
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import RouterOL
    from phnet_amd.synthetic import spread_scores_
    torch.manual_seed(0)
    model = RouterOL(make_cfg(img_h=H, img_w=W, arch=arch), None).cuda().eval()
    spread_scores_(model)                                   # about half of the anchors pass conf_threshold: lanes are kept
    pre = ClipPreprocessor(H, W, pixel_format="nv12", pitch=2048)
    T, out = 16, {}
    frames = torch.randint(0, 256, (T, 1, *pre.frame_shape), dtype=torch.uint8, device="cuda")
    for name, kw in (("label_map", dict(label_map=True, overlay=False)), ("overlay_nv12", dict(label_map=False, overlay=True, alpha=128))):
        r = LaneRenderer.for_preprocessor(pre, lane_width=WIDTH, **kw)
        plain = model.open_stream(streams=1, frame_hw=(H, W), graph=True, raw=pre, polylines=True, track=True)
        drawn = model.open_stream(streams=1, frame_hw=(H, W), graph=True, raw=pre, polylines=True, track=True, render=r)
        for t in range(2 * model.save_freq_max + 4):
            plain.step(frames[t % T]); drawn.step(frames[t % T])
        ms_plain, ms_drawn = [], []
        for _ in range(ROUNDS):
            ms_plain.append(_timed(lambda i: plain.step(frames[i % T]), frames_timed))
            ms_drawn.append(_timed(lambda i: drawn.step(frames[i % T]), frames_timed))
        lanes = int(drawn.polylines["lanes_num"][0])
        del plain, drawn
        out[name] = {"ms_per_step": _spread(ms_plain), "ms_per_step_render": _spread(ms_drawn), "lanes_in_last_frame": lanes,
                     "added_us": round((_spread(ms_drawn)["median"] - _spread(ms_plain)["median"]) * 1e3, 1)}
    return out


def main():
    frames_timed = int(_arg("--frames", 240))
    out = {"workload": f"lanes on a {H0}x{W0} picture, {S} points per lane, width {WIDTH}; stream: resnet34 3x320x800 from NV12 {H0}x{W0}, "
                       f"hipGraph, {frames_timed} timed steps per run, {ROUNDS} alternated runs"}
    out["launch"] = kernel_rows(max(400, frames_timed))
    out["host_baseline"] = host_baseline()
    if "--no-stream" not in sys.argv:
        out["stream_B1"] = stream_rows(frames_timed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
