"""What line clipping costs in the target launch (csrc/lane_targets.hip rule 0c, phnet_lane_targets_clip): 320 x 800, S = 36, R = 4,
annotations at 1280 x 1920 with crop 480 (tests/target_cases.source_frames: 1 - 4 lanes of 3 - 24 points per frame, Lin = 4, P = 32)
behind the draws of AugmentSampler('basic'), for a batch of 5 frames and one of 40.  Per batch, us per launch from device events
around a run of back-to-back launches with out= (launch gaps included - not a profiler's kernel time) after a warm-up, ROUNDS rounds
with all variants alternated inside every round, one process:
  * baseline: phnet_lane_targets_aug of the library named by --baseline-lib (a build of the parent commit's csrc/lane_targets.hip),
    called through ctypes with the same pointers; left out when no library is named.  That file and its common.h in one directory,
    `hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -shared -I include lane_targets.hip -o libparent.so`;
  * aug_ctypes: this tree's phnet_lane_targets_aug through the same bare ctypes call (the like-for-like comparison with baseline);
  * aug: this tree's phnet_lane_targets_aug through hip_ops;  clip0 / clip1: phnet_lane_targets_clip with clip off / on, frag_count written.
Before timing, the outputs are compared: baseline, aug and clip0 bit for bit, clip1 against the restatement of tests/clip_cases.py.
Prints one JSON line."""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from phnet_amd import _lib
from phnet_amd import hip_ops as K
from phnet_amd.libs.dataset.openlane.augment import AugmentSampler
from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
from tests import clip_cases as CC
from tests import target_cases as C

ROUNDS, LAUNCHES, WARMUP = 5, 500, 50


def _baseline(path):
    handle = ctypes.CDLL(path)
    fn = handle.phnet_lane_targets_aug
    fn.restype, fn.argtypes = next((r, a) for n, r, a in _lib.declared_functions(_lib.HEADER) if n == "phnet_lane_targets_aug")
    return fn


def _time(call):
    for _ in range(WARMUP):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / LAUNCHES * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None, help="a shared library with the parent commit's phnet_lane_targets_aug")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lane_clip: needs a GPU")
    base = _baseline(args.baseline_lib) if args.baseline_lib else None
    enc = TargetEncoder(320, 800, 36, 4, device="cuda")
    mp = C.map_for(320, 800, 1280, 1920, 480)
    out = {"workload": "target launch with and without rule 0c, 320x800, S 36, R 4, Lin 4, P 32, annotations at 1280x1920 crop 480 behind "
                       f"'basic' draws; us per launch from device events over {LAUNCHES} back-to-back launches, {ROUNDS} alternated rounds: "
                       "median (min - max)"}
    for frames_n in (5, 40):
        frames = C.source_frames(7, frames_n)
        table = AugmentSampler("basic", 320, 800, seed=11).sample(frames_n)
        host = table.numpy()
        dev = table.to("cuda")
        pts, cnt, num = (t.cuda() for t in pack_annotations(frames, 4, 32, clip=True))
        rows = {k: torch.empty((frames_n, 4, 6 + 36), device="cuda") for k in ("baseline", "aug", "clip0", "clip1")}
        frag = torch.zeros(frames_n, dtype=torch.int32, device="cuda")
        a = (pts, cnt, num, enc.offsets_ys, 4, 320, 800, enc.strip_size)
        kw = dict(crop=enc.crop, src_w=enc.src_w, scale_x=enc.scale_x, scale_y=enc.scale_y)
        raw = (pts.data_ptr(), cnt.data_ptr(), num.data_ptr(), enc.offsets_ys.data_ptr(), rows["baseline"].data_ptr(), frames_n, 4, 32, 4, 36,
               320.0, 800.0, float(enc.strip_size), float(enc.crop), float(enc.src_w), float(enc.scale_x), float(enc.scale_y), 0,
               dev.flip2.data_ptr(), dev.fwd.data_ptr(), K._stream())
        calls = {"aug": lambda: K.lane_targets_aug(*a, dev.flip2, dev.fwd, out=rows["aug"], **kw),
                 "clip0": lambda: K.lane_targets_clip(*a, dev.flip2, dev.fwd, clip=False, frag_count=frag, out=rows["clip0"], **kw),
                 "clip1": lambda: K.lane_targets_clip(*a, dev.flip2, dev.fwd, clip=True, frag_count=frag, out=rows["clip1"], **kw)}
        if base is not None:                                                          # both through the same bare ctypes call
            rows["aug_ctypes"] = torch.empty_like(rows["aug"])
            mine = raw[:4] + (rows["aug_ctypes"].data_ptr(),) + raw[5:]
            calls = {"baseline": lambda: _lib.check(base(*raw), "baseline phnet_lane_targets_aug"),
                     "aug_ctypes": lambda: _lib.check(_lib.lib().phnet_lane_targets_aug(*mine), "phnet_lane_targets_aug"), **calls}
        for call in calls.values():
            call()
        torch.cuda.synchronize()
        got = {k: rows[k].cpu().numpy() for k in calls}
        same = all(np.array_equal(got[k].view(np.int32), got["aug"].view(np.int32)) for k in calls if k != "clip1")
        want = [CC.encode_frame_clipped(lanes, 320, 800, 36, 4, int(host["flip2"][t]), [float(v) for v in host["fwd"][t]], mapping=mp)
                for t, lanes in enumerate(frames)]
        want_rows = np.stack([w[0] for w in want])
        pattern = np.array_equal(got["clip1"] == C.INVALID, want_rows == C.INVALID)
        times = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, call in calls.items():
                times[k].append(_time(call))
        rec = {"frames": frames_n, "rows": frames_n * 4, "unclipped_entries_bit_equal": bool(same),
               "clip1_invalid_pattern_equals_restatement": bool(pattern),
               "clip1_worst_ulps_vs_restatement": int(C.ulps(got["clip1"], want_rows).max()) if pattern else None,
               "clip1_frag_count_equals_restatement": frag.tolist() == [w[2] for w in want],
               "frames_changed_by_clipping": int((got["clip1"] != got["aug"]).any(axis=(1, 2)).sum()),
               "us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}}
        ref = "baseline" if base is not None else "aug"
        rec["ratio_to_" + ref] = {k: round(statistics.median(times[k]) / statistics.median(times[ref]), 3) for k in calls if k != ref}
        out[f"frames{frames_n}"] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
