"""Streaming inference latency (phnet_amd/stream.py): ResNet-34, 3x320x800, B in {1, 4, 8} live streams - ms per frame of the
replayed stream step (one hipGraph for every frame, the cross-frame memory on the device), next to two numbers from
GraphedInference taken in the same process: a 5-frame clip (ms per clip / 5: the throughput shape, a caller waits for 5 frames)
and a 1-frame clip (the latency floor: it has no memory and skips the cross-frame decoder, so the stream step is expected to cost
MORE than it).  Prints one JSON line.  --frames F (default 240, timed after a warm-up of 2W + 4 frames so that the ring is full
and has wrapped); --streams 1,4,8."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from phnet_amd.config import make_cfg
from phnet_amd.graphed import GraphedInference
from phnet_amd.libs.models.Router4OL import RouterOL
from phnet_amd.synthetic import make_clip, spread_scores_


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _timed(fn, reps):
    """Host clock around `reps` calls that end in a device synchronise -> ms per call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main(H=320, W=800, arch="resnet34"):
    frames_timed = int(_arg("--frames", 240))
    streams = [int(b) for b in str(_arg("--streams", "1,4,8")).split(",")]
    torch.manual_seed(0)
    model = RouterOL(make_cfg(img_h=H, img_w=W, arch=arch), None).cuda().eval()
    spread_scores_(model)                                   # about half of the anchors pass conf_threshold: lanes are kept, memories carry positives
    T = 16
    out = {"workload": f"stream step, {arch}, 3x{H}x{W}, eval, hipGraph, {frames_timed} timed frames per row"}
    for B in streams:
        clips = torch.stack([make_clip(H, W, T, seed=100 + b) for b in range(B)]).cuda()      # [B,T,3,H,W]
        s = model.open_stream(streams=B, frame_hw=(H, W), graph=True)
        for t in range(2 * model.save_freq_max + 4):
            rows, num, _ = s.step(clips[:, t % T])
        kept = num.cpu().tolist()
        ms_stream = _timed(lambda i: s.step(clips[:, i % T]), frames_timed)
        lanes = s.lanes(*s.step(clips[:, 0])[:2])
        del s
        g5 = GraphedInference(model, clips[0, :5] if B == 1 else clips[:, :5])
        five = clips[0, :5] if B == 1 else clips[:, :5]
        for _ in range(3):
            g5(five)
        ms_clip5 = _timed(lambda i: g5(five), max(1, frames_timed // 5))
        del g5
        one = clips[0, :1] if B == 1 else clips[:, :1]
        g1 = GraphedInference(model, one)
        for _ in range(3):
            g1(one)
        ms_clip1 = _timed(lambda i: g1(one), frames_timed)
        del g1
        out[f"B{B}"] = {"ms_per_frame_stream": round(ms_stream, 3), "ms_per_frame_clip5_graph": round(ms_clip5 / 5, 3),
                        "ms_first_lane_clip5_graph": round(ms_clip5, 3), "ms_per_frame_clip1_graph_no_memory": round(ms_clip1, 3),
                        "frames_per_s_stream": round(B * 1e3 / ms_stream, 1), "kept_last_warmup_frame": kept,
                        "lanes_last_frame": [len(x) for x in lanes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
