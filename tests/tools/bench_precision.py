"""precision="fp32" against precision="bf16" (phnet_tune_mma(4), DESIGN.md "bf16 inference") on ResNet-34 at 5 x 3 x 320 x 800:

  * hipGraph replay of one clip, of 32 clips batched (GraphedInference) and of a B = 1 and a B = 8 stream step (open_stream): ms per
    replay, median and [min, max] of --repeats windows; the two precisions alternate window by window in one process, so they see
    the same machine state.  The fp32 figure is the baseline: that code path does not change with the keyword.
  * per-layer time of the trunk + FPN forward GEMMs (every distinct launch of one 5-frame clip and of one frame, as hip_ops recorded
    them) in both arithmetics: each launch replayed --inner times inside a small hipGraph, median and [min, max] over --repeats.
  * how far the bf16 outputs of the synthetic clip move from the fp32 ones: FPN levels, kept rows, kept lane sets.  Recorded, not
    asserted: random weights put scores next to the threshold.

Prints one JSON line.  --repeats R (7), --inner N (20), --frames F (120 timed stream frames per window), --quick (one clip and the
layers only), --bf16-splitk (A/B: bf16 with mode 3's split-K plan, phnet_tune_force_k_tile(-401), instead of its own unsplit,
batch-invariant one; the fp32 column is the same baseline in both runs)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from phnet_amd import hip_ops as K
from phnet_amd.config import make_cfg
from phnet_amd.graphed import GraphedInference
from phnet_amd.libs.models.Router4OL import RouterOL
from phnet_amd.synthetic import make_clip, spread_scores_

PRECISIONS = ("fp32", "bf16")


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _window(fn, reps):
    """Host clock around `reps` calls that end in a device synchronise -> ms per call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _spread(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def _alternate(runners, reps, repeats):
    """runners: {precision: fn(i)} -> {precision: spread of ms per call}, the precisions taking turns window by window."""
    for fn in runners.values():
        _window(fn, max(3, reps // 4))                                            # warm-up of every shape the windows use
    got = {p: [] for p in runners}
    for _ in range(repeats):
        for p, fn in runners.items():
            got[p].append(_window(fn, reps))
    out = {p: _spread(v) for p, v in got.items()}
    out["bf16_over_fp32"] = round(out["bf16"]["median"] / out["fp32"]["median"], 3)
    return out


def _layers(model, frames, inner, repeats):
    """Every distinct forward GEMM launch of the trunk + FPN on `frames`, timed alone in both arithmetics."""
    rec = {}
    for p in PRECISIONS:
        with torch.no_grad(), K.precision_scope(p):
            model.backbone(frames)                                                # folds / packs of this arithmetic exist before the recording
            K.TIMER = []
            try:
                model.backbone(frames)
            finally:
                rec[p], K.TIMER = K.TIMER, None
    assert [r[6] for r in rec["fp32"]] == [r[6] for r in rec["bf16"]]             # the same launches, in the same order
    rows, seen = [], {}
    for a, b in zip(rec["fp32"], rec["bf16"]):
        key = (a[6], a[0], b[0])
        if key in seen:
            seen[key]["count"] += 1
            continue
        graphs = {}
        for p, r in (("fp32", a), ("bf16", b)):
            with K.precision_scope(p):                                            # the launch closure reads the mode when it runs
                for _ in range(3):
                    r[5]()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(inner):
                        r[5]()
            graphs[p] = g
        times = {p: [] for p in PRECISIONS}
        for _ in range(repeats):
            for p in PRECISIONS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); graphs[p].replay(); e1.record()
                torch.cuda.synchronize()
                times[p].append(e0.elapsed_time(e1) / inner * 1e3)                # us per launch (with its split-K reduce)
        row = {"gemm": "x".join(str(v) for v in a[6][1:4]), "filter": a[6][4], "count": 1, "gflop": round(a[2] / 1e9, 3)}
        for p, r in (("fp32", a), ("bf16", b)):
            row[p] = {"kernel": r[0], "splits": r[1], "us": _spread(times[p], 2)}
        row["bf16_over_fp32"] = round(row["bf16"]["us"]["median"] / row["fp32"]["us"]["median"], 3)
        seen[key] = row
        rows.append(row)
    total = {p: round(sum(r[p]["us"]["median"] * r["count"] for r in rows), 1) for p in PRECISIONS}
    return {"layers": rows, "sum_us": total, "bf16_over_fp32": round(total["bf16"] / total["fp32"], 3)}


def _deviation(model, clip):
    with torch.no_grad():
        feats = {p: [f.clone() for f in (model.backbone(clip) if p == "fp32" else _bf16_backbone(model, clip))] for p in PRECISIONS}
        out = {p: model.infer_device(clip, precision=p) for p in PRECISIONS}
    fpn = [float((a - b).abs().max() / a.abs().max()) for a, b in zip(feats["fp32"], feats["bf16"])]
    (ra, na, aa), (rb, nb, ab) = out["fp32"], out["bf16"]
    same, rows_dev, kept = [], 0.0, []
    for t in range(clip.shape[0]):
        ka, kb = int(na[t]), int(nb[t])
        kept.append([ka, kb])
        eq = ka == kb and torch.equal(aa[t, :ka], ab[t, :kb])
        same.append(bool(eq))
        if eq and ka:
            rows_dev = max(rows_dev, float(((ra[t, :ka] - rb[t, :ka]).abs() / (1 + ra[t, :ka].abs())).max()))
    return {"fpn_levels_max_abs_over_max": [float(f"{v:.3e}") for v in fpn], "kept_fp32_bf16_per_frame": kept,
            "kept_lane_sets_agree_per_frame": same, "kept_rows_max_dev_over_1_plus_abs_where_sets_agree": float(f"{rows_dev:.3e}")}


def _bf16_backbone(model, clip):
    with K.mma("bf16"):
        return model.backbone(clip)


def main(H=320, W=800, arch="resnet34", T=5):
    repeats, inner, frames_timed = int(_arg("--repeats", 7)), int(_arg("--inner", 20)), int(_arg("--frames", 120))
    quick, splitk = "--quick" in sys.argv, "--bf16-splitk" in sys.argv
    if splitk:
        K.tune_k_tile(-401)
    torch.manual_seed(0)
    model = RouterOL(make_cfg(img_h=H, img_w=W, arch=arch), None).cuda().eval()
    spread_scores_(model)                                   # about half of the anchors pass conf_threshold: lanes are kept, memories carry positives
    clip = make_clip(H, W, T, seed=0).cuda()
    out = {"workload": f"{arch}, {T} x 3 x {H} x {W}, eval, hipGraph replay; ms per replay, median [min, max] of {repeats} windows",
           "bf16_plan": "mode 3's split-K plan" if splitk else "unsplit (default: batch-invariant)",
           "deviation_bf16_from_fp32": _deviation(model, clip)}
    g = {p: GraphedInference(model, clip, precision=p) for p in PRECISIONS}
    out["clip_1"] = _alternate({p: (lambda i, p=p: g[p](clip)) for p in PRECISIONS}, 20, repeats)
    del g
    out["trunk_gemms_5_frames"] = _layers(model, clip, inner, repeats)
    out["trunk_gemms_1_frame"] = _layers(model, clip[:1].contiguous(), inner, repeats)
    if not quick:
        big = torch.stack([make_clip(H, W, T, seed=i % 4) for i in range(32)]).cuda()
        g = {p: GraphedInference(model, big, precision=p) for p in PRECISIONS}
        out["clips_32_batched"] = _alternate({p: (lambda i, p=p: g[p](big)) for p in PRECISIONS}, 3, repeats)
        del g, big
        for B in (1, 8):
            clips = torch.stack([make_clip(H, W, 16, seed=100 + b) for b in range(B)]).cuda()
            s = {p: model.open_stream(streams=B, frame_hw=(H, W), graph=True, precision=p) for p in PRECISIONS}
            for p in PRECISIONS:
                for t in range(2 * model.save_freq_max + 4):                      # the ring is full and has wrapped
                    s[p].step(clips[:, t % 16])
            out[f"stream_B{B}"] = _alternate({p: (lambda i, p=p: s[p].step(clips[:, i % 16])) for p in PRECISIONS}, frames_timed, repeats)
            del s, clips
    K.tune_reset()
    assert K.mma_mode() == 3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
