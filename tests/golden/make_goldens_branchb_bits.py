"""Records what branch B's forward computes, bit for bit, into tests/golden/branchb_parent_bits.npz.

Run on the GPU at the commit whose results are to be pinned (the parent of a change to csrc/attention.hip / attn_device.h /
rowchain.hip or to the launches of TransformerDecoder._forward_row_chains):

    python tests/golden/make_goldens_branchb_bits.py [--out FILE]

Two parts, both through public entry points only:
  * hip_ops.attention_fwd (outputs and lse) on the cases of ATTN_CASES: cross-attention of R query rows per item against Lk keys
    with a key mask and the counter-based dropout, and one self-attention at 240 x 240;
  * DetNetV2.forward_second (pred_b, line_b) of the small model (resnet18, 64 x 160) in train mode with dropout 0.1, for two stages
    and the two frames of a T = 3 clip that have a memory, each as its own dropout item.
The inputs are drawn on the host from numpy seeds (the tests regenerate them from the recorded case list); the outputs are kept
as raw bits (floats as uint32).  tests/test_rowchain_attn_gpu.py holds a later build to these bits, tests/test_branchb_bits_cpu.py
checks that the fixture is there and covers the shapes."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "branchb_parent_bits.npz")
E, H = 128, 8
RNG_STATE = 0x5DEECE66D          # value of the dropout counter the attention cases run with
ROWS, KEYS, MASKS, PS = (1, 16, 17, 240), (1, 16, 17, 41), ("all", "few", "none"), (0.0, 0.1)

# cross-attention: R query rows and Lk keys per item, `mask`: "all" keys valid | a "few" masked | "none" valid (rows of zeros through
# l = 0), dropout p, `batch` items.  Not the full product (the fixture stays small): every (R, Lk) pair of the small R with the
# (mask, p) combinations dealt round-robin, R = 240 with a few keys masked and with none valid, batch 2 at the ragged R = 17.
ATTN_CASES = []
_combos = [(m, p) for m in MASKS for p in PS]
for _i, (_r, _lk) in enumerate((r, lk) for r in ROWS[:3] for lk in KEYS):
    _m, _p = _combos[_i % len(_combos)]
    ATTN_CASES.append(dict(R=_r, Lk=_lk, mask=_m, p=_p, batch=1))
ATTN_CASES += [dict(R=240, Lk=41, mask="few", p=0.1, batch=1), dict(R=240, Lk=17, mask="none", p=0.0, batch=1),
               dict(R=17, Lk=41, mask="few", p=0.1, batch=2), dict(R=17, Lk=17, mask="all", p=0.0, batch=2),
               dict(R=240, Lk=240, mask="all", p=0.1, batch=1, self_attn=True)]
for _i, _c in enumerate(ATTN_CASES):
    _c.setdefault("self_attn", False); _c["seed"] = 8200 + _i; _c["site"] = 3 + _i

MODEL = dict(img_h=64, img_w=160, arch="resnet18", T=3, stages=[0, 1], frames=[1, 2], p=0.1, seed=8300, torch_seed=20240)


def key_mask(c):
    """u8[batch*Lk] of a case: 1 = valid."""
    n = c["batch"] * c["Lk"]
    m = np.ones(n, np.uint8)
    if c["mask"] == "few":
        m[::3] = 0
        if c["Lk"] > 1:
            m[1::c["Lk"]] = 1          # every item keeps a valid key
    elif c["mask"] == "none":
        m[:] = 0
    return m


def attn_inputs(c):
    """(q [batch*R,E], kv [batch*Lk,2E], key mask u8[batch*Lk]) float32 of one case, from its seed alone.  A self-attention case
    takes q | k | v as the column blocks of one [R,3E] array (kv then holds all three)."""
    r = np.random.default_rng(c["seed"])
    if c["self_attn"]:
        return None, r.normal(size=(c["R"], 3 * E)).astype(np.float32), key_mask(c)
    q = r.normal(size=(c["batch"] * c["R"], E)).astype(np.float32)
    kv = r.normal(size=(c["batch"] * c["Lk"], 2 * E)).astype(np.float32)
    return q, kv, key_mask(c)


def bits(t):
    """A device tensor as a host array of raw bits (floats as uint32)."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def rng_state(torch):
    return torch.tensor([RNG_STATE], dtype=torch.int64, device="cuda")


def run_attn_case(c, K, torch):
    q, kv, mask = attn_inputs(c)
    kv = torch.from_numpy(kv).cuda()
    rng = (rng_state(torch), c["site"], c["p"]) if c["p"] > 0 else None
    if c["self_attn"]:
        o, lse = K.attention_fwd(kv[:, :E], kv[:, E:2 * E], kv[:, 2 * E:], H, None, rng=rng, batch=1)
    else:
        o, lse = K.attention_fwd(torch.from_numpy(q).cuda(), kv[:, :E], kv[:, E:], H, torch.from_numpy(mask).cuda(), rng=rng, batch=c["batch"])
    torch.cuda.synchronize()
    return dict(o=bits(o), lse=bits(lse))


def build_model(torch, root):
    """The small model of the model tests with its decoder's dropout at MODEL['p'], in train mode on the GPU."""
    if root not in sys.path:
        sys.path.insert(0, root)
    from oracle import phnet_cpu as O
    from phnet_amd.config import make_cfg
    from phnet_amd.libs.models.Router4OL import RouterOL
    from phnet_amd.libs.utils.loss4OLV3 import Criterion4OL
    from tests import synth
    g = O.Geometry(img_h=MODEL["img_h"], img_w=MODEL["img_w"], arch=MODEL["arch"])
    cfg = make_cfg(img_h=g.img_h, img_w=g.img_w, arch=g.arch)
    model = RouterOL(cfg, Criterion4OL(cfg))
    model.load_state_dict(synth.make_state(g), strict=True)
    for m in model.detNet.transformer_Dec.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = MODEL["p"]
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = MODEL["p"]
    return model.cuda().train()


def model_inputs(det, save_freq_max, max_lanes):
    """{(stage, frame): (tokens [N,1,E], memory [M,1,E], valid bool[M], priors [1,N,6+S])} as host arrays, from MODEL['seed']."""
    r = np.random.default_rng(MODEL["seed"])
    N, M = det.num_priors, save_freq_max * (max_lanes + 1)
    width = det.priors.shape[-1]
    out = {}
    for s in MODEL["stages"]:
        for t in MODEL["frames"]:
            tok = r.normal(size=(N, 1, E)).astype(np.float32)
            mem = r.normal(size=(M, 1, E)).astype(np.float32)
            valid = np.zeros(M, bool)
            valid[-t * (max_lanes + 1):] = r.uniform(size=t * (max_lanes + 1)) < 0.7        # the slots of the t frames before
            valid[-1] = True
            pri = r.uniform(0.1, 0.9, size=(1, N, width)).astype(np.float32)
            out[(s, t)] = (tok, mem, valid, pri)
    return out


def run_model(model, torch, hoisted=False):
    """forward_second of every (stage, frame) of MODEL as the training schedule calls it -> {"s{stage}_t{frame}_pred" / "_line": bits}.
    The dropout counter is set from MODEL['torch_seed'] (and put back).  hoisted: layer 1's prefix of a stage's frames as one batch
    (builds that have TransformerDecoder.decoder_prefix)."""
    from phnet_amd import functional as PF
    from phnet_amd.libs.models.Router4OL import BRANCH_B_SITES
    det, DS = model.detNet, PF.DropoutStream
    T, N = MODEL["T"], model.detNet.num_priors
    ins = model_inputs(det, model.save_freq_max, 4)
    saved = (dict(DS._state), dict(DS._slot), DS._calls)
    out = {}
    try:
        DS._state.clear(); DS._slot.clear()
        with torch.random.fork_rng(devices=[0]):
            torch.manual_seed(MODEL["torch_seed"])
            DS.begin_step("cuda:0")
        with torch.no_grad():
            for s in MODEL["stages"]:
                prefix = None
                if hoisted:
                    with DS.items(BRANCH_B_SITES, s * (T - 1), N):
                        tgt = torch.cat([torch.from_numpy(ins[(s, t)][0]).cuda().view(N, E) for t in MODEL["frames"]])
                        prefix = [x.view(len(MODEL["frames"]), N, E) for x in det.transformer_Dec.decoder_prefix(tgt, batch=len(MODEL["frames"]))]
                for j, t in enumerate(MODEL["frames"]):
                    tok, mem, valid, pri = (torch.from_numpy(a).cuda() for a in ins[(s, t)])
                    with DS.items(BRANCH_B_SITES, s * (T - 1) + t - 1, 0):
                        if hoisted:
                            pred, line = det.forward_second((mem, valid), tok, s, pri, (prefix[0][j], prefix[1][j]))
                        else:
                            pred, line = det.forward_second((mem, valid), tok, s, pri)
                    out[f"s{s}_t{t}_pred"], out[f"s{s}_t{t}_line"] = bits(pred), bits(line)
        torch.cuda.synchronize()
    finally:
        DS._state.clear(); DS._state.update(saved[0]); DS._slot.clear(); DS._slot.update(saved[1]); DS._calls = saved[2]
    return out


def load(path=FIXTURE):
    """([(case dict, {name: array})] of the attention cases, (MODEL dict, {name: array}) of the model part)."""
    z = np.load(path)
    cases = json.loads(str(z["attn_cases"]))
    attn = [(c, {k[len(f"a{i}_"):]: z[k] for k in z.files if k.startswith(f"a{i}_")}) for i, c in enumerate(cases)]
    return attn, (json.loads(str(z["model"])), {k[len("m_"):]: z[k] for k in z.files if k.startswith("m_")})


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, root)
    import torch
    from phnet_amd import hip_ops as K
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    arrays = {"attn_cases": np.asarray(json.dumps(ATTN_CASES)), "model": np.asarray(json.dumps(MODEL))}
    for i, c in enumerate(ATTN_CASES):
        for k, v in run_attn_case(c, K, torch).items():
            arrays[f"a{i}_{k}"] = v
    for k, v in run_model(build_model(torch, root), torch).items():
        arrays[f"m_{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(ATTN_CASES)} attention cases + {len(MODEL['stages']) * len(MODEL['frames'])} model passes, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
