"""Streaming inference latency of the Router4OLV2 family (phnet_amd/stream.py LaneStreamV2): ResNet-18, 3x320x800, B in {1, 8, 32}
live streams - ms per frame of the replayed stream step (one hipGraph for every frame, keys and memory on the device), next to
GraphedInference on 5-frame clips in the same process: at B = 1 `infer_device` (the only way to run this family before it had a
stream), at B > 1 `infer_clips_device`; and on a 1-frame clip.  Same output keys as tests/tools/bench_stream.py, which stays the
V1 tool.  Prints one JSON line.  --frames F (default 240, timed after a warm-up of 2W + 4 frames so that the ring is full and has
wrapped); --streams 1,8,32."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from phnet_amd.config import make_cfg_v2
from phnet_amd.graphed import GraphedInference
from phnet_amd.libs.models.Router4OLV2 import RouterOL
from phnet_amd.synthetic import make_clip, spread_scores_
from bench_stream import _arg, _timed                       # the V1 tool beside this file: same arguments, same clock

def main(H=320, W=800, arch="resnet18"):
    frames_timed = int(_arg("--frames", 240))
    streams = [int(b) for b in str(_arg("--streams", "1,8,32")).split(",")]
    torch.manual_seed(0)
    model = RouterOL(make_cfg_v2(img_h=H, img_w=W, arch=arch)).cuda().eval()
    spread_scores_(model)                                   # about half of the anchors pass conf_threshold: lanes are kept
    T = 16
    out = {"workload": f"stream step, Router4OLV2, {arch}, 3x{H}x{W}, eval, hipGraph, {frames_timed} timed frames per row"}
    for B in streams:
        clips = torch.stack([make_clip(H, W, T, seed=100 + b) for b in range(B)]).cuda()      # [B,T,3,H,W]
        s = model.open_stream(streams=B, frame_hw=(H, W), graph=True)
        for t in range(2 * model.save_freq_max + 4):
            rows, num, _ = s.step(clips[:, t % T])
        kept = num.cpu().tolist()
        ms_stream = _timed(lambda i: s.step(clips[:, i % T]), frames_timed)
        lanes = s.lanes(*s.step(clips[:, 0])[:2])
        del s
        five = clips[0, :5] if B == 1 else clips[:, :5]
        g5 = GraphedInference(model, five)
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
                        "frames_per_s_stream": round(B * 1e3 / ms_stream, 1), "frames_per_s_clip5_graph": round(B * 5e3 / ms_clip5, 1),
                        "kept_last_warmup_frame": kept, "lanes_last_frame": [len(x) for x in lanes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
