"""What the neighbourhood ops of the training augmentation cost (csrc/augment_stencil.hip, `phnet_augment_stencil_u8`) on one clip of the
workload's geometry, 5 x 320 x 800, "nchw" output, every other op neutral (identity matrices: one tap per pixel).  In one process,
alternated inside every round:
  * plain:        the phnet_augment_u8 launch (no stencil table) - the launch as it was before the neighbourhood ops existed;
  * no_op:        phnet_augment_stencil_u8 with a stencil table in which no frame has an op: the staging launch whose workgroups all
                  return at once, and the warp launch with its per-frame switch.  This is the case that matters for the training step:
                  81 % of the frames of 'complex' draw neither group;
  * median5_one:  one frame of the five with a 5 x 5 median;
  * gauss9_edge:  all five frames with the 9-tap Gaussian and an edge filter.
us per call from device events around back-to-back calls with out= (launch gaps included - not a profiler's kernel time), ROUNDS
rounds, median (min - max).  Checks while it is there that `no_op` gives the bytes of `plain`.  Prints one JSON line."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from phnet_amd.libs.dataset.openlane.augment import AugmentParams, ClipAugmenter, edge_kernel, gaussian_kernel

ROUNDS, LAUNCHES = 7, 500
T, H, W = 5, 320, 800


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment_stencil: needs an MI355X; nothing is measured without one")
    aug = ClipAugmenter(H, W, device="cuda")
    u8 = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (T, H, W, 3), dtype=np.uint8)).cuda()
    both = dict(edge=dict(weights=edge_kernel(0.1)), blur=dict(kind="gaussian", k=9, weights=gaussian_kernel(2.9)))
    tables = {"plain": AugmentParams.identity(T), "no_op": AugmentParams.identity(T, stencil=True),
              "median5_one": AugmentParams.build([{}, {}, dict(blur=dict(kind="median", k=5)), {}, {}], H, W, stencil=True),
              "gauss9_edge": AugmentParams.build([both] * T, H, W)}
    tables = {k: v.to("cuda") for k, v in tables.items()}
    clip = torch.empty((T, 3, H, W), device="cuda")
    runs = {k: (lambda tab: lambda: aug(u8, tab, out=clip))(tab) for k, tab in tables.items()}
    us = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            us[k].append(_us(fn))
    same = torch.equal(aug(u8, tables["plain"]).view(torch.int32), aug(u8, tables["no_op"]).view(torch.int32))
    differs = not torch.equal(aug(u8, tables["plain"]).view(torch.int32), aug(u8, tables["gauss9_edge"]).view(torch.int32))
    print(json.dumps({"workload": f"augment launch(es) on {T}x{H}x{W}, identity matrices, nchw; us per call from device events over {LAUNCHES} "
                                  f"back-to-back calls, {ROUNDS} alternated rounds: median, min, max",
                      "us": {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in us.items()},
                      "no_op_equals_plain": bool(same), "gauss9_edge_differs": bool(differs)}))


if __name__ == "__main__":
    main()
