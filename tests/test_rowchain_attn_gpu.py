"""The row chain with the cross-attention core as a stage (csrc/rowchain.hip: rowchain_attn_kernel) against the three launches it
replaces, rowchain_fwd -> attention_fwd -> rowchain_fwd: `torch.equal` on every output - the same rows through the same
instructions.  And the attention forward after its body moved into csrc/attn_device.h, and the decoder's forward through the new
launches, against the bits recorded at the parent commit (tests/golden/branchb_parent_bits.npz, make_goldens_branchb_bits.py)."""
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_goldens_branchb_bits", os.path.join(HERE, "golden", "make_goldens_branchb_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

E, FF, H = 128, 256, 8
PAD = 3                      # rows past the end of every input (NaN) and output (sentinel)
SENTINEL = -12345.5
_W = {}


def _weights():
    """The parameters of one decoder layer's chains, drawn once."""
    if not _W:
        r = np.random.default_rng(8100)
        dev = "cuda"
        mat = lambda n, k: torch.from_numpy((r.normal(size=(n, k)) / np.sqrt(k)).astype(np.float32)).to(dev)      # noqa: E731
        vec = lambda n, s=0.1: torch.from_numpy((r.normal(size=n) * s).astype(np.float32)).to(dev)                # noqa: E731
        lnw = lambda: torch.from_numpy((1.0 + 0.1 * r.normal(size=E)).astype(np.float32)).to(dev)                 # noqa: E731
        _W.update(wa0=mat(E, E), ba0=vec(E), ln0=(lnw(), vec(E)), wq=mat(E, E), bq=vec(E),
                  wo=mat(E, E), bo=vec(E), ln1=(lnw(), vec(E)), w1=mat(FF, E), b1=vec(FF), w2=mat(E, FF), b2=vec(E), ln2=(lnw(), vec(E)),
                  wg=mat(3 * E, E), bg=vec(3 * E), state=torch.tensor([0x1234567], dtype=torch.int64, device=dev))
    return _W


def _padded(a, rows):
    """`a` [rows, w] followed by PAD rows of NaN in one allocation -> the view of the first `rows`."""
    buf = torch.full((rows + PAD, a.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    buf[:rows] = a
    return buf[:rows]


def _outputs(rows, ng):
    full = [torch.full((rows + PAD, w), SENTINEL, dtype=torch.float32, device="cuda") for w in (E, E, max(ng, 1))]
    return full, [f[:rows] for f in full]


def _run_both(R, Lk, batch, mask, p, chain_a, nxt, seed):
    from phnet_amd import hip_ops as K
    W = _weights()
    r = np.random.default_rng(seed)
    rows, keys = batch * R, batch * Lk
    rnd = lambda n, w: torch.from_numpy(r.normal(size=(n, w)).astype(np.float32)).cuda()       # noqa: E731
    x, resid = _padded(rnd(rows, E), rows), _padded(rnd(rows, E), rows)
    kv = _padded(rnd(keys, 2 * E), keys)
    kvalid = torch.from_numpy(G.key_mask(dict(batch=batch, Lk=Lk, mask=mask))).cuda()
    item = (0, R) if batch > 1 else (5, 0)
    site = (lambda i: (W["state"], 40 + i, p) + item) if p > 0 else (lambda i: None)        # noqa: E731
    r0, rc, ra, rf, r3 = (site(i) for i in range(5))
    wg, bg = (W["wg"], W["bg"]) if nxt else (None, None)
    chain_b = dict(wa=W["wo"], ba=W["bo"], ln1=W["ln1"], ffn=(W["w1"], W["b1"], W["w2"], W["b2"]), ln2=W["ln2"], wg=wg, bg=bg, eps=1e-5,
                   rng_a=ra, rng_f=rf, rng_3=r3)
    # today's three launches
    if chain_a:
        t, _, q = K.rowchain_fwd(x, resid=resid, wa=W["wa0"], ba=W["ba0"], ln1=W["ln0"], wg=W["wq"], bg=W["bq"], eps=1e-5, rng_a=r0)
    else:
        q, t = x, resid
    a2, _ = K.attention_fwd(q, kv[:, :E], kv[:, E:], H, kvalid, rng=rc, batch=batch)
    ref = K.rowchain_fwd(a2, resid=t, want_t=True, want_h=not nxt, **chain_b)
    # the one launch
    full, views = _outputs(rows, 3 * E if nxt else 0)
    out = (views[0], None if nxt else views[1], views[2] if nxt else None)
    got = K.rowchain_attn_fwd(x, resid, kv[:, :E], kv[:, E:], H, key_valid=kvalid, rng_c=rc, rng_a0=r0 if chain_a else None, batch=batch,
                              chain_a=(W["wa0"], W["ba0"], *W["ln0"], W["wq"], W["bq"]) if chain_a else None, eps_a=1e-5, out=out, **chain_b)
    torch.cuda.synchronize()
    return ref, got, full


SHAPES = [(R, Lk, 1) for R in G.ROWS for Lk in G.KEYS] + [(17, Lk, 2) for Lk in G.KEYS]


@pytest.mark.parametrize("R,Lk,batch", SHAPES)
def test_one_launch_gives_the_bits_of_the_three(R, Lk, batch):
    """Key masks all valid / a few masked / none valid (rows of zeros through l = 0), p in {0, 0.1} with a live counter, with and
    without chain A, with and without the next projection (last layer: h_out).  Inputs carry NaN rows past their end, outputs
    sentinel rows past theirs: neither may be touched."""
    for n, (mask, p, chain_a, nxt) in enumerate(itertools.product(G.MASKS, G.PS, (True, False), (True, False))):
        ref, got, full = _run_both(R, Lk, batch, mask, p, chain_a, nxt, 8110 + n)
        what = (R, Lk, batch, mask, p, chain_a, nxt)
        for name, a, b in zip("thy", ref, got):
            assert (a is None) == (b is None), (what, name)
            if a is not None:
                assert bool(torch.isfinite(a).all()), (what, name, "reference not finite")
                assert torch.equal(a, b), (what, name, float((a - b).abs().max()))
        for f in full:
            assert bool((f[batch * R:] == SENTINEL).all()), (what, "rows past the end written")
        if nxt:
            assert bool((full[1] == SENTINEL).all()), (what, "h written although not asked for")


def test_all_keys_masked_is_the_zero_attention_row():
    """With no valid key the attention stage hands zeros to the out-projection (the l = 0 branch), whatever K / V hold."""
    from phnet_amd import hip_ops as K
    W = _weights()
    r = np.random.default_rng(8150)
    q, t = (torch.from_numpy(r.normal(size=(17, E)).astype(np.float32)).cuda() for _ in range(2))
    kv = torch.from_numpy(r.normal(size=(16, 2 * E)).astype(np.float32)).cuda()
    zero = torch.zeros((17, E), dtype=torch.float32, device="cuda")
    chain_b = dict(wa=W["wo"], ba=W["bo"], ln1=W["ln1"], ffn=(W["w1"], W["b1"], W["w2"], W["b2"]), ln2=W["ln2"], want_h=True)
    ref = K.rowchain_fwd(zero, resid=t, **chain_b)
    got = K.rowchain_attn_fwd(q, t, kv[:, :E], kv[:, E:], H, key_valid=torch.zeros(16, dtype=torch.uint8, device="cuda"), **chain_b)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])


@pytest.mark.parametrize("what", ["too many keys", "head width 32", "E = 256"])
def test_unsupported_shapes_are_refused_before_any_launch(what):
    from phnet_amd import hip_ops as K
    W = _weights()
    lk, heads = (K.ROWCHAIN_ATTN_MAX_KEYS + 1, H) if what == "too many keys" else (16, 4 if what == "head width 32" else H)
    assert not K.rowchain_attn_ok(E if what != "E = 256" else 256, FF, heads, lk)
    q, t = torch.randn(17, E, device="cuda"), torch.randn(17, E, device="cuda")
    kv = torch.randn(lk, 2 * E, device="cuda")
    full, views = _outputs(17, 3 * E)
    kw = dict(wa=W["wo"], ba=W["bo"], ln1=W["ln1"], ffn=(W["w1"], W["b1"], W["w2"], W["b2"]), ln2=W["ln2"], wg=W["wg"], bg=W["bg"])
    if what == "E = 256":
        q, t, kv = torch.randn(17, 256, device="cuda"), torch.randn(17, 256, device="cuda"), torch.randn(lk, 512, device="cuda")
        e = 256
    else:
        e = E
    with pytest.raises(RuntimeError, match="PHNET_ERR_ARG"):
        K.rowchain_attn_fwd(q, t, kv[:, :e], kv[:, e:], heads, out=tuple(views), **kw)
    torch.cuda.synchronize()
    assert all(bool((f == SENTINEL).all()) for f in full)


_FIX = {}


def _fixture():
    if not _FIX:
        _FIX["attn"], _FIX["model"] = G.load()
    return _FIX


def test_attention_forward_keeps_the_parents_bits():
    """attn_fwd_kernel through the shared body: outputs and lse of every recorded case, bit for bit."""
    from phnet_amd import hip_ops as K
    for c, rec in _fixture()["attn"]:
        got = G.run_attn_case(c, K, torch)
        assert np.array_equal(got["o"], rec["o"]), (c, "o")
        assert np.array_equal(got["lse"], rec["lse"]), (c, "lse")


@pytest.mark.parametrize("fuse,hoisted", [(True, False), (True, True), (False, True), (False, False)])
def test_forward_second_keeps_the_parents_bits(fuse, hoisted):
    """pred_b / line_b of the small model's branch B (train mode, p = 0.1, two stages, the frames with a memory) through the fused
    launch and / or the batched prefix of layer 1 are the bits the parent's launches gave."""
    meta, rec = _fixture()["model"]
    assert meta == G.MODEL
    model = G.build_model(torch, os.path.dirname(HERE))
    dec = model.detNet.transformer_Dec
    dec.fuse_cross_attention = fuse             # (an instance attribute: the class default stays)
    got = G.run_model(model, torch, hoisted=hoisted)
    assert sorted(got) == sorted(rec)
    for k in sorted(rec):
        assert np.array_equal(got[k], rec[k]), k
