"""What lanes cost the caller (phnet_amd/polylines.py, csrc/lane_points.hip): ResNet-34, 3x320x800, V1 streams at B = 1 and B = 32
and one 5-frame clip.  Per row:
  * ms per step of the replayed stream graph WITHOUT and WITH polylines=True, three alternated runs of each in this process (the
    step without polylines is the parent's step: the option adds one launch to it and changes nothing else);
  * host ms per frame of `lanes()` (copy + DetNetV2.predictions_to_pred + one scipy spline per lane) against `lanes_fast()` (one
    packed copy + numpy slicing) on the SAME step outputs;
  * end-to-end frames/s with the result construction INSIDE the timed loop, for both.
The clip row does the same with GraphedInference(polylines=...) / lanes_from_device / polylines_from_device.
Prints one JSON line.  --frames F (default 240, after a warm-up of 2W + 4 frames); --streams 1,32."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from phnet_amd.config import make_cfg
from phnet_amd.graphed import GraphedInference
from phnet_amd.libs.models.Router4OL import RouterOL
from phnet_amd.synthetic import make_clip, spread_scores_
from bench_stream import _arg, _timed                       # the stream tool beside this file: same arguments, same clock

ROUNDS = 3


def _spread(xs):
    return {"runs": [round(x, 3) for x in xs], "median": round(sorted(xs)[len(xs) // 2], 3), "spread": round(max(xs) - min(xs), 3)}


def main(H=320, W=800, arch="resnet34"):
    frames_timed = int(_arg("--frames", 240))
    streams = [int(b) for b in str(_arg("--streams", "1,32")).split(",")]
    torch.manual_seed(0)
    model = RouterOL(make_cfg(img_h=H, img_w=W, arch=arch), None).cuda().eval()
    spread_scores_(model)                                   # about half of the anchors pass conf_threshold: lanes are kept
    T = 16
    out = {"workload": f"lanes to the caller, {arch}, 3x{H}x{W}, eval, hipGraph, {frames_timed} timed frames per run, {ROUNDS} alternated runs"}
    for B in streams:
        clips = torch.stack([make_clip(H, W, T, seed=100 + b) for b in range(B)]).cuda()      # [B,T,3,H,W]
        plain = model.open_stream(streams=B, frame_hw=(H, W), graph=True)
        poly = model.open_stream(streams=B, frame_hw=(H, W), graph=True, polylines=True)
        for t in range(2 * model.save_freq_max + 4):
            plain.step(clips[:, t % T]); poly.step(clips[:, t % T])
        ms_plain, ms_poly = [], []
        for _ in range(ROUNDS):
            ms_plain.append(_timed(lambda i: plain.step(clips[:, i % T]), frames_timed))
            ms_poly.append(_timed(lambda i: poly.step(clips[:, i % T]), frames_timed))
        rows, num, _ = poly.step(clips[:, 0])
        reps = max(4, frames_timed // (4 * B))
        host_slow = _timed(lambda i: poly.lanes(rows, num), reps) / B
        host_fast = _timed(lambda i: poly.lanes_fast(), reps) / B
        lanes = [len(x) for x in poly.lanes_fast()]
        e2e_n = max(8, frames_timed // 4)
        e2e_slow = _timed(lambda i: plain.lanes(*plain.step(clips[:, i % T])[:2]), e2e_n)
        e2e_fast = _timed(lambda i: (poly.step(clips[:, i % T]), poly.lanes_fast()), e2e_n)
        del plain, poly
        out[f"B{B}"] = {"ms_per_step": _spread(ms_plain), "ms_per_step_polylines": _spread(ms_poly),
                        "host_ms_per_frame_lanes": round(host_slow, 4), "host_ms_per_frame_lanes_fast": round(host_fast, 4),
                        "host_ratio": round(host_slow / host_fast, 1), "lanes_per_stream": lanes,
                        "frames_per_s_device_only": round(B * 1e3 / _spread(ms_plain)["median"], 1),
                        "frames_per_s_end_to_end_lanes": round(B * 1e3 / e2e_slow, 1),
                        "frames_per_s_end_to_end_lanes_fast": round(B * 1e3 / e2e_fast, 1)}
    clip = make_clip(H, W, 5, seed=100).cuda()
    g_plain, g_poly = GraphedInference(model, clip), GraphedInference(model, clip, polylines=True)
    for _ in range(3):
        g_plain(clip); g_poly(clip)
    n = max(4, frames_timed // 5)
    ms_plain, ms_poly = [], []
    for _ in range(ROUNDS):
        ms_plain.append(_timed(lambda i: g_plain(clip), n))
        ms_poly.append(_timed(lambda i: g_poly(clip), n))
    rows, num, _ = g_poly(clip)
    host_slow = _timed(lambda i: model.lanes_from_device(rows, num), 20) / 5
    host_fast = _timed(lambda i: model.polylines_from_device(g_poly.polylines, rows), 20) / 5
    e2e_slow = _timed(lambda i: model.lanes_from_device(*g_plain(clip)[:2]), n)
    e2e_fast = _timed(lambda i: model.polylines_from_device(g_poly.polylines, g_poly(clip)[0]), n)
    out["clip5"] = {"ms_per_clip": _spread(ms_plain), "ms_per_clip_polylines": _spread(ms_poly),
                    "host_ms_per_frame_lanes": round(host_slow, 4), "host_ms_per_frame_lanes_fast": round(host_fast, 4),
                    "host_ratio": round(host_slow / host_fast, 1),
                    "lanes_per_frame": [len(x) for x in model.polylines_from_device(g_poly.polylines, rows)],
                    "frames_per_s_end_to_end_lanes": round(5e3 / e2e_slow, 1), "frames_per_s_end_to_end_lanes_fast": round(5e3 / e2e_fast, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
