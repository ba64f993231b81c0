"""What the training augmentation costs (phnet_amd/libs/dataset/openlane/augment.py, csrc/augment.hip, csrc/lane_targets.hip rule 0b) at
the workload's geometry: 1280 x 1920 frames, crop 480, resized to 320 x 800, 1 - 4 annotated lanes per frame, S = 36, R = 4, for one clip
(T = 5) and for 32 clips (T = 160).  In one process, alternated inside every round:
  * resize: the phnet_preprocess_u8 launch of the same clip with out_u8 (what runs in front of the augment launch), "nchw" output;
  * augment: the phnet_augment_u8 launch on those 8-bit frames with an identity table (one tap per pixel, every op skipped), with an
    affine-only table (four taps), with every op switched on in every frame (four taps, colour, per-channel pixel dropout), and with
    the tables AugmentSampler draws per frame for "basic" and "complex" (seed 5; `ops_on` counts the frames each op is on in);
  * targets / targets_aug: the phnet_lane_targets launch and phnet_lane_targets_aug with the same affine table.
us per launch from device events around back-to-back calls with out= (launch gaps included - not a profiler's kernel time), ROUNDS
rounds, median (min - max).  The augment launch reads 3 B and writes 12 B (+ 3 with out_u8) per pixel with at most 12 byte loads per
pixel; the resize launch issues 48 loads per pixel, so the augment launch is expected below it.  Prints one JSON line."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from phnet_amd.libs.dataset.openlane.augment import AugmentParams, AugmentSampler, ClipAugmenter
from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
from phnet_amd.libs.dataset.openlane.targets import TargetEncoder, pack_annotations
from tests import augment_cases as AC
from tests import target_cases as C

ROUNDS, LAUNCHES = 5, 500


def _us(fn, launches=LAUNCHES):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


def _tables(T):
    affine = [dict(rotate=3.7 * (-1) ** t, scale=1.0 + 0.01 * (t % 9), translate=(0.05, -0.03)) for t in range(T)]
    every = [dict(a, flip=bool(t % 2), perm=(1, 2, 0), mul=1.05, add=-4, value=6, dropout=dict(mode="pixel", p=0.03, per_channel=True, seed=1000 + t))
             for t, a in enumerate(affine)]
    return {"identity": AugmentParams.identity(T), "affine": AugmentParams.build(affine, 320, 800), "every_op": AugmentParams.build(every, 320, 800),
            "sampled_basic": AugmentSampler("basic", 320, 800, seed=5).sample(T), "sampled_complex": AugmentSampler("complex", 320, 800, seed=5).sample(T)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs an MI355X; nothing is measured without one")
    pre = ClipPreprocessor(320, 800, device="cuda")
    aug = ClipAugmenter.for_preprocessor(pre)
    enc = TargetEncoder.for_preprocessor(pre, 36, 4)
    out = {"workload": f"training augmentation, 1280x1920 crop 480 -> 320x800, S 36, R 4; us per launch from device events over {LAUNCHES} "
                       f"back-to-back launches, {ROUNDS} alternated rounds: median, min, max"}
    rng = np.random.default_rng(1)
    for clips in (1, 32):
        T = clips * 5
        frames = torch.from_numpy(rng.integers(0, 256, (T, 1280, 1920, 3), dtype=np.uint8)).cuda()
        pts, cnt, num = (t.cuda() for t in pack_annotations(C.source_frames(7, T), 4, 256))
        tables = {k: v.to("cuda") for k, v in _tables(T).items()}
        clip = torch.empty((T, 3, 320, 800), device="cuda")
        rows = torch.empty((T, 4, 6 + 36), device="cuda")
        _, u8 = pre(frames, return_u8=True)
        u8_out = torch.empty_like(u8)
        runs = {"resize_preprocess_u8": lambda: pre(frames, out=clip, augment=None, return_u8=True)}
        for k, tab in tables.items():
            runs[f"augment_{k}"] = (lambda tab: lambda: aug(u8, tab, out=clip))(tab)
        runs["augment_every_op_with_out_u8"] = lambda: aug(u8, tables["every_op"], out=clip, out_u8=u8_out)
        runs["targets"] = lambda: enc(pts, cnt, num, out=rows)
        runs["targets_aug"] = lambda: enc(pts, cnt, num, out=rows, augment=tables["affine"])
        us = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, fn in runs.items():
                us[k].append(_us(fn))
        n = tables["every_op"].numpy()
        want_u8, _ = AC.augment(u8[:1].cpu().numpy(), n["flip2"][:1], n["inv"][:1], n["table"][:1])
        got_u8 = aug(u8[:1].contiguous(), AugmentParams(*[x[:1].contiguous() for x in tables["every_op"].tensors()]), return_u8=True)[1]
        ops_on = {}
        for k in ("sampled_basic", "sampled_complex"):
            m = tables[k].numpy()
            ident = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
            ops_on[k] = {"flip": int(m["flip2"].sum()), "shuffle": int((m["table"][:, :3] != [0, 1, 2]).any(axis=1).sum()),
                         "brightness": int(((m["table"][:, 3] != 256) | (m["table"][:, 4] != 0)).sum()), "hue_sat": int((m["table"][:, 5] != 0).sum()),
                         "dropout": int((m["table"][:, 6] != 0).sum()), "affine": int((m["inv"] != ident).any(axis=1).sum())}
        out[f"clips{clips}"] = {"frames": T, "pixels": T * 320 * 800, "ops_on": ops_on,
                                "us": {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in us.items()},
                                "frame0_every_op_equals_restatement": bool(np.array_equal(got_u8.cpu().numpy(), want_u8))}
        del frames
    print(json.dumps(out))


if __name__ == "__main__":
    main()
