"""What lane identities cost per step (phnet_amd/tracking.py, csrc/lane_track.hip): ResNet-34, 3x320x800, V1 streams at B = 1 and
B = 32.  Per row:
  * ms per step of the replayed stream graph WITHOUT and WITH track=True, three alternated runs of each in this process (the
    step without tracking is the parent's step: the option adds one launch after the decode and changes nothing else);
  * the kernel alone, us per launch for T = 1 (the streaming step) and T = 16 (a clip), from device events around a run of
    back-to-back launches on one state - this includes the launch gaps, it is not a profiler's kernel time - on the stream's own
    kept rows and on the synthetic sequences of tests/track_cases.py (S = 72, L = 4, M = 8: four rows against up to eight live
    slots on every frame, whatever the randomly initialised model's rows look like);
  * what the tracker saw on the model's rows (rows that rule 1 calls trackable, distinct ids, the largest hits).
Prints one JSON line.  --frames F (default 240, after a warm-up of 2W + 4 frames); --streams 1,32."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from phnet_amd import hip_ops as K
from phnet_amd.config import make_cfg
from phnet_amd.libs.models.Router4OL import RouterOL
from phnet_amd.synthetic import make_clip, spread_scores_
from phnet_amd.tracking import TrackState, track_defaults
from bench_stream import _arg, _timed                       # the stream tool beside this file: same arguments, same clock
from bench_polylines import _spread
from tests import track_cases as C

ROUNDS = 3


def _kernel_us(rows, num, M, thr, age, launches=200):
    """rows [B,T,L,6+S], num [B,T]: device-event time of `launches` back-to-back hip_ops.lane_track calls -> us per launch."""
    state = TrackState(rows.shape[0], M, rows.shape[-1] - 6, rows.device)
    out = K.lane_track(rows, num, state, thr, age)
    for _ in range(20):
        K.lane_track(rows, num, state, thr, age, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        K.lane_track(rows, num, state, thr, age, out=out)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


def _trackable(rows, nums):
    """Rows per frame that rule 1 of the tracker accepts (torch restatement: finite r[2], r[5], end >= start, index < num)."""
    S = rows.shape[-1] - 6
    r2, r5 = rows[..., 2].double(), rows[..., 5].double()
    start = torch.clamp(torch.round(r2 * (S - 1)), 0, S - 1)
    end = torch.clamp(start + torch.round(r5) - 1, max=S - 1)
    inside = torch.arange(rows.shape[-2], device=rows.device) < nums[..., None].clamp(0, rows.shape[-2])
    return float((torch.isfinite(r2) & torch.isfinite(r5) & (end >= start) & inside).sum(-1).float().mean())


def _synthetic(B, T0=16):
    """Frames [T0, 2 * T0) of B streams of tests/track_cases.py (S = 72) on the device; _kernel_us replays them on one state, so
    the slots are live from its warm-up launches on."""
    seqs = [C.random_sequence(72, C.random_seed(72, b)) for b in range(B)]
    rows = torch.stack([torch.from_numpy(s[0]) for s in seqs]).cuda()
    nums = torch.stack([torch.from_numpy(s[1]) for s in seqs]).cuda()
    return rows[:, T0:2 * T0].contiguous(), nums[:, T0:2 * T0].contiguous()


def main(H=320, W=800, arch="resnet34"):
    frames_timed = int(_arg("--frames", 240))
    streams = [int(b) for b in str(_arg("--streams", "1,32")).split(",")]
    torch.manual_seed(0)
    model = RouterOL(make_cfg(img_h=H, img_w=W, arch=arch), None).cuda().eval()
    spread_scores_(model)                                   # about half of the anchors pass conf_threshold: lanes are kept
    M, age, thr = track_defaults(model)
    T = 16
    out = {"workload": f"lane identities, {arch}, 3x{H}x{W}, eval, hipGraph, {frames_timed} timed frames per run, {ROUNDS} alternated runs; "
                       f"max_tracks {M}, max_age {age}, thr {thr:.6f}"}
    for B in streams:
        clips = torch.stack([make_clip(H, W, T, seed=100 + b) for b in range(B)]).cuda()      # [B,T,3,H,W]
        plain = model.open_stream(streams=B, frame_hw=(H, W), graph=True)
        tracked = model.open_stream(streams=B, frame_hw=(H, W), graph=True, track=True)
        for t in range(2 * model.save_freq_max + 4):
            plain.step(clips[:, t % T]); tracked.step(clips[:, t % T])
        ms_plain, ms_track = [], []
        for _ in range(ROUNDS):
            ms_plain.append(_timed(lambda i: plain.step(clips[:, i % T]), frames_timed))
            ms_track.append(_timed(lambda i: tracked.step(clips[:, i % T]), frames_timed))
        rows, nums, ids, hits = [], [], [], []
        for t in range(T):                                                                     # the kept rows of one pass over the clip
            r, n, _ = tracked.step(clips[:, t])
            rows.append(r.clone()); nums.append(n.clone())
            ids.append(tracked.tracks["track_id"].clone()); hits.append(tracked.tracks["hits"].clone())
        rows, nums, ids = torch.stack(rows, 1).contiguous(), torch.stack(nums, 1).contiguous(), torch.stack(ids, 1)
        us1 = _kernel_us(rows[:, :1].contiguous(), nums[:, :1].contiguous(), M, thr, age)
        us16 = _kernel_us(rows, nums, M, thr, age)
        srows, snums = _synthetic(B)
        sus1 = _kernel_us(srows[:, :1].contiguous(), snums[:, :1].contiguous(), 8, float(C.THR), 3)
        sus16 = _kernel_us(srows, snums, 8, float(C.THR), 3)
        del plain, tracked
        a, b = _spread(ms_plain), _spread(ms_track)
        out[f"B{B}"] = {"ms_per_step": a, "ms_per_step_track": b, "track_minus_plain_us": round((b["median"] - a["median"]) * 1e3, 1),
                        "kernel_us_per_launch_T1": round(us1, 2), "kernel_us_per_launch_T16": round(us16, 2),
                        "synthetic_kernel_us_per_launch_T1": round(sus1, 2), "synthetic_kernel_us_per_launch_T16": round(sus16, 2),
                        "synthetic_rows_per_frame_mean": round(float(snums.float().mean()), 2),
                        "lanes_per_frame_mean": round(float(nums.float().mean()), 2), "trackable_rows_per_frame_mean": round(_trackable(rows, nums), 2),
                        "distinct_ids_stream0": len(set(ids[0][ids[0] > 0].tolist())), "max_hits": int(torch.stack(hits).max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
