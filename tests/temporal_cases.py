"""Shared by tests/test_temporal_cpu.py and tests/test_temporal_gpu.py: the reference fixture (tests/golden/temporal_tiny.json,
written by tests/golden/make_goldens_temporal.py from the reference's executed Python), a plain numpy stand-in for the one
device step of phnet_amd.evaluation.temporal, and hand-made matrices for the counting rules."""
import json
import os

import numpy as np

from oracle import culane_cpu as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_tiny.json")


def fixture():
    with open(GOLD) as fh:
        return json.load(fh)


def numpy_ious(segments, groups, height, width, lane_width):
    """What `temporal.device_ious` computes, on the host: oracle.culane_cpu.raster_lane on the module's own segments and
    3 I / (3 U + 1e-10) in the reference's order of operations (evalTemporalOLV2.py:26-35: integer sums of three-channel
    canvases, one double add, one double divide)."""
    masks = [O.raster_lane([tuple(int(v) for v in s) for s in seg], height, width, lane_width) for seg in segments]
    out = []
    for r0, nr, c0, nc, first in np.asarray(groups).reshape(-1, 5).tolist():
        assert first == len(out)
        for r in range(r0, r0 + nr):
            for c in range(c0, c0 + nc):
                inter, union = int((masks[r] & masks[c]).sum()), int((masks[r] | masks[c]).sum())
                out.append(float(3 * inter) / (float(3 * union) + 1e-10))
    return np.asarray(out, np.float64)


def frames_of(fx, video, T):
    return [(T.lanes_from_text(f["anno"]), T.lanes_from_text(f["pred"])) for f in fx["videos"][video]]


def write_files(fx, root):
    """The fixture as label files under root/anno and root/pred -> (anno_dir, pred_dir, names).  A frame without predictions
    gets no prediction file (a missing file is a frame without lanes)."""
    names = []
    for video, frames in fx["videos"].items():
        for side in ("anno", "pred"):
            os.makedirs(os.path.join(root, side, video), exist_ok=True)
        for f in frames:
            names.append(f["name"])
            with open(os.path.join(root, "anno", f["name"] + ".lines.txt"), "w") as fh:
                fh.write(f["anno"])
            if f["pred"]:
                with open(os.path.join(root, "pred", f["name"] + ".lines.txt"), "w") as fh:
                    fh.write(f["pred"])
    return os.path.join(root, "anno"), os.path.join(root, "pred"), names


def check_against_fixture(res, want):
    assert {v: [list(t) for t in trios] for v, trios in res["per_video"].items()} == want["per_video"]
    assert (res["Ns"], res["Nj"], res["Nm"]) == (want["Ns"], want["Nj"], want["Nm"])
    assert (res["Rs"], res["Rj"], res["Rm"]) == (want["Rs"], want["Rj"], want["Rm"])           # equal as doubles


def synthetic_video(n_frames=6, n_lanes=4, height=640, width=960, seed=3):
    """One small video at the OpenLane-V canvas: n_lanes annotated and n_lanes predicted lanes per frame (lists of points)."""
    rng = np.random.default_rng(seed)
    base = np.linspace(0.2 * width, 0.8 * width, n_lanes)
    frames = []
    for t in range(n_frames):
        anno, pred = [], []
        for k in range(n_lanes):
            ys = np.linspace(height - 10, 0.35 * height, 8)
            xs = base[k] + 3.0 * t + (k - 1.5) * 0.25 * (ys - ys[0]) + rng.normal(0, 1.0, len(ys))
            anno.append([(float(x), float(y)) for x, y in zip(xs, ys)])
            shift = (0.0, 6.0, 14.0, 45.0)[int(rng.integers(0, 4))]
            pred.append([(float(x + shift), float(y)) for x, y in zip(xs[::-1], ys[::-1])])
        frames.append((anno, pred))
    return frames
