"""What the training targets cost (phnet_amd/libs/dataset/openlane/targets.py, csrc/lane_targets.hip): 320 x 800, S = 36, R = 4,
source annotations at 1280 x 1920 with crop 480 (tests/target_cases.source_frames: 1 - 4 lanes of 3 - 24 points per frame), for
one clip (5 frames x 4 rows) and for a batch of 32 clips (32 x 5 frames x 4 rows).  Per row:
  * the launch alone, us per launch, from device events around a run of back-to-back TargetEncoder calls with out= - this
    includes the launch gaps, it is not a profiler's kernel time; three runs, and the same with 24-point lanes replaced by
    256-point lanes (the serial solve at its longest);
  * the numpy / Python restatement of tests/target_cases.py on the host for the same frames, ms (one run: it is slow) - the
    restatement is written for clarity, the reference's own scipy path is not installed behind imgaug here;
  * pack_annotations on the host, ms, and the copy of its three pinned tensors, us.
Prints one JSON line."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
from tests import target_cases as C

ROUNDS = 3


def _launch_us(enc, pts, cnt, num, launches=200):
    out = enc(pts, cnt, num)
    for _ in range(20):
        enc(pts, cnt, num, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        enc(pts, cnt, num, out=out)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


def _long_frames(n_frames):
    return [[C.curve(300 + 400 * k, 500, -200, 1270, 500, 256) for k in range(4)] for _ in range(n_frames)]


def main():
    enc = TargetEncoder(320, 800, 36, 4, device="cuda")
    mp = C.map_for(320, 800, 1280, 1920, 480)
    out = {"workload": "training targets, 320x800, S 36, R 4, annotations at 1280x1920 crop 480; us per launch from device events "
                       f"over 200 back-to-back launches, {ROUNDS} runs"}
    for clips in (1, 32):
        frames = C.source_frames(7, clips * 5)
        t0 = time.perf_counter()
        packed = pack_annotations(frames, 4, 256)
        t_pack = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pts, cnt, num = (t.cuda(non_blocking=True) for t in packed)
        torch.cuda.synchronize()
        t_copy = time.perf_counter() - t0
        us = [_launch_us(enc, pts, cnt, num) for _ in range(ROUNDS)]
        lpts, lcnt, lnum = (t.cuda() for t in pack_annotations(_long_frames(clips * 5), 4, 256))
        us_long = [_launch_us(enc, lpts, lcnt, lnum) for _ in range(ROUNDS)]
        t0 = time.perf_counter()
        want = np.stack([C.encode_frame(lanes, 320, 800, 36, 4, mapping=mp)[0] for lanes in frames])
        t_host = time.perf_counter() - t0
        got = enc(pts, cnt, num).cpu().numpy()
        out[f"clips{clips}"] = {"frames": clips * 5, "rows": clips * 5 * 4, "valid_rows": int(want[..., 1].sum()),
                                "launch_us": [round(v, 2) for v in us], "launch_us_256_point_lanes": [round(v, 2) for v in us_long],
                                "restatement_host_ms": round(t_host * 1e3, 2), "pack_annotations_ms": round(t_pack * 1e3, 2),
                                "copy_us": round(t_copy * 1e6, 1), "worst_ulps_vs_restatement": int(C.ulps(got, want).max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
