"""The head-backward harness (tests/head_cases.py) proves itself on the CPU, with plain torch fp32 standing in for the device.

  * every statement run in fp32 through its own ReLU masks sits at the fp32 floor against fp64 through the same masks
    (<= 1.5e-5 for both measures: 2.5x the worst value measured when the cases were chosen, 6.0e-6 in the two-frame gate), the masks pass the mask
    conditions, and the bound finds nothing;
  * the masked, batched attention / decoder statement equals nn.MultiheadAttention and oracle.temporal_decoder in fp64 where those
    apply (no mask, batch 1), a masked key carries no weight and no gradient, and a clip batch equals clip by clip;
  * the gate-stack, dynamic-head and branch statements equal oracle.routing_gate / dynamic_head / branch_heads in fp64;
  * the mask conditions reject a mask flipped at a unit far from zero;
  * the seed conditions of the hidden-ReLU cases hold (and reject a case that has a unit at zero);
  * the recovered-mask logic for dropout is right on a synthetic mask;
  * a gradient off by 1e-4, a missing bias gradient and a destination added twice trip the bound.
"""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from oracle import phnet_cpu as O
from tests import head_cases as H

FLOOR = 1.5e-5

GROUPS = (H.LINEAR, H.LAYER_NORM, H.DYN, H.DWCONV, H.GATE_TAIL, H.gate_stack_pieces(), H.ROI_POOL, H.LANE_UPDATE, H.DROPOUT,
          H.DROPOUT_LN_WAYS, H.ATTENTION, H.TOWERS, H.DECODER, H.router_pieces())
ALL = [p for g in GROUPS for p in g]


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    yield
    H.release()


def stand_in(piece):
    """torch fp32 run free: (its outputs, its gradients, its own ReLU masks or None)."""
    if piece.kind.startswith(("dropout", "gelu")) and piece.opts["p"] > 0:
        gen = torch.Generator().manual_seed(piece.seed)
        keep = (torch.rand(piece.tensors["x"].shape, generator=gen) >= piece.opts["p"]).double()
        piece = piece.with_tensors(keep=keep)
    run = H.Run(piece, torch.float32)
    masks = None if piece.hidden else (run.relus.masks or None)
    return piece, run, masks


@pytest.mark.parametrize("piece", ALL, ids=[f"{p.kind}-{p.name}" for p in ALL])
def test_fp32_statement_sits_inside_its_own_bound(piece):
    piece, run, masks = stand_in(piece)
    rep = H.compare(piece, run.outs, run.grads, masks)
    print(rep.line(f"{piece.kind} {piece.name}"))
    assert rep.bad == []
    assert max(rep.f_l2.values()) <= FLOOR and max(rep.f_max.values()) <= FLOOR, (rep.f_l2, rep.f_max)
    assert rep.e_l2 == rep.f_l2 and rep.e_max == rep.f_max                        # the stand-in IS the floor
    n_grads = sum(k.startswith("grad:") for k in rep.e_l2)
    if piece.cot_on is None or piece.cot_on:
        assert n_grads >= len(piece.diff) - len(piece.zero_noise)
    else:
        assert n_grads == 0


@pytest.mark.parametrize("make", [lambda: H.dynconv_piece(1), lambda: H.dynconv_piece(2), lambda: H.branch_piece(False), lambda: H.branch_piece(True)],
                         ids=["dynconv-B1", "dynconv-B2", "branch-fir", "branch-sec"])
def test_fp32_module_statement_sits_inside_its_own_bound(make):
    test_fp32_statement_sits_inside_its_own_bound(make())


def test_decoder_cases_cover_every_parameter_and_row_block():
    names = H.decoder_param_names()
    assert len(names) == 2 * 18 + 2
    for piece in H.DECODER:
        piece, run, masks = stand_in(piece)
        rep = H.compare(piece, run.outs, run.grads, masks)
        grads = [k for k in rep.e_l2 if k.startswith("grad:")]
        assert len(grads) == 2 * 26 + 2 + 2                                      # in_proj weight and bias as three row blocks each; d tgt, d memory
        ref, _ = H.reference_and_floor(piece, masks)
        for k in names:
            if k.endswith("in_proj_weight"):
                e = ref.grads[k].shape[0] // 3
                assert all(float(ref.grads[k][i * e:(i + 1) * e].abs().max()) > 1e-3 for i in range(3)), k
            elif k.endswith("self_attn.in_proj_bias") or k.endswith("multihead_attn.in_proj_bias"):
                e = ref.grads[k].shape[0] // 3
                assert float(ref.grads[k][e:2 * e].abs().max()) < 1e-12, k        # why the k block is judged in units of the whole bias gradient
                assert float(ref.grads[k][:e].abs().max()) > 1e-3 and float(ref.grads[k][2 * e:].abs().max()) > 1e-3, k
            else:
                assert float(ref.grads[k].abs().max()) > 1e-3, k


# ------------------------------------------------------------------------------------------------ the statements themselves
@pytest.mark.parametrize("e,lq,lk", [(128, 7, 3), (256, 37, 11)])
def test_attention_statement_equals_torch_multihead_attention(e, lq, lk):
    gen = torch.Generator().manual_seed(e + lq)
    m = torch.nn.MultiheadAttention(e, 8).double()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(H.rn(gen, *p.shape, scale=0.2))
    t = {k: v.detach() for k, v in m.named_parameters()}
    q_in, kv_in = H.rn(gen, lq, e), H.rn(gen, lk, e)
    with torch.no_grad():
        want, _ = m(q_in[:, None], kv_in[:, None], kv_in[:, None], need_weights=False)
    got = H.mha(t, "", q_in, kv_in, 8)
    assert float((got - want[:, 0]).abs().max()) <= 1e-12
    # a key mask: torch's key_padding_mask is True where a key is IGNORED
    valid = torch.ones(lk, dtype=torch.bool)
    valid[0] = False
    with torch.no_grad():
        want, _ = m(q_in[:, None], kv_in[:, None], kv_in[:, None], key_padding_mask=~valid[None], need_weights=False)
    assert float((H.mha(t, "", q_in, kv_in, 8, valid) - want[:, 0]).abs().max()) <= 1e-12


def test_attention_statement_mask_and_batch():
    gen = torch.Generator().manual_seed(5)
    e, b, lq, lk = 128, 3, 5, 4
    q, k, v = H.rn(gen, b * lq, e), H.rn(gen, b * lk, e).requires_grad_(True), H.rn(gen, b * lk, e).requires_grad_(True)
    valid = torch.tensor([[True, False, True, True], [False, False, True, False], [True, True, True, True]]).reshape(-1)
    out = H.attention(q, k, v, 8, valid, b)
    for i in range(b):                                                           # clip by clip over the valid keys only
        rows = valid[i * lk:(i + 1) * lk]
        one = H.attention(q[i * lq:(i + 1) * lq], k[i * lk:(i + 1) * lk][rows], v[i * lk:(i + 1) * lk][rows], 8)
        assert float((out[i * lq:(i + 1) * lq] - one).detach().abs().max()) <= 1e-12
    assert float((out[lq:2 * lq] - v[lk + 2]).detach().abs().max()) <= 1e-12     # a single valid key: its value, for every query
    gk, gv = torch.autograd.grad(out, (k, v), H.rn(gen, *out.shape))
    assert not gk[~valid].any() and not gv[~valid].any() and bool(gv[valid].abs().amax(dim=1).min() > 0)


def test_decoder_statement_equals_the_oracle_decoder():
    piece = H.DECODER[1]
    t = piece.tensors
    l, m = t["tgt"].shape[0] // 3, t["memory"].shape[0] // 3
    want = O.temporal_decoder(t, t["tgt"][:l], t["memory"][:m], prefix="")
    got = H.decoder(t, t["tgt"][:l], t["memory"][:m], 8, 2)
    assert float((got - want).abs().max()) <= 1e-12
    whole = H.decoder(t, t["tgt"], t["memory"], 8, 2, None, 3)                    # three clips at once == clip by clip
    assert float((whole[:l] - want).abs().max()) <= 1e-12


def test_gate_stack_statement_equals_the_oracle_gate():
    piece = H.gate_stack_pieces()[1]
    gen = torch.Generator().manual_seed(1)
    c, p = piece.tensors["x"].shape[1:]
    sd = H.gate_sd(piece.tensors, stage=1)
    sd["layers.1.0.weight"], sd["layers.1.0.bias"] = H.rn(gen, 96, c * p, scale=(c * p) ** -0.5), H.rn(gen, 96, scale=0.1)
    sd["layers.1.2.weight"], sd["layers.1.2.bias"] = H.rn(gen, 1, 96, scale=0.1), H.rn(gen, 1, scale=0.1)
    x = piece.tensors["x"]
    s = H.STATEMENTS["gate_stack"](piece.tensors, H.Relus(), piece.opts)["y"]
    h = F.relu(F.linear(s.flatten(1), sd["layers.1.0.weight"], sd["layers.1.0.bias"]))
    tail = H.STATEMENTS["gate_tail"](dict(h=h, w=sd["layers.1.2.weight"], b=sd["layers.1.2.bias"]), H.Relus(), {})["y"]
    for frame in range(2):                                                       # plane b * n + a uses the filters of anchor a
        want = O.routing_gate(sd, 1, x[3 * frame:3 * frame + 3][None], prefix="")
        assert float((tail[3 * frame:3 * frame + 3] - want[0, :, 0]).abs().max()) <= 1e-12


def test_dynamic_head_statement_equals_the_oracle():
    piece = H.dynconv_piece(2)
    sd = {"0." + k: v for k, v in piece.tensors.items() if k in H.DYNCONV_KEYS}
    got = H.STATEMENTS["dynconv"](piece.tensors, H.Relus(), piece.opts)
    for i in range(2):
        for b in range(2):                                                       # the oracle takes one frame at a time
            want = O.dynamic_head(sd, 0, piece.tensors[f"pro{i}"][b:b + 1], piece.tensors[f"roi{i}"][b:b + 1], prefix="")
            assert float((got[f"y{i}"][b:b + 1] - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("sec", [False, True], ids=["fir", "sec"])
def test_branch_statement_equals_the_oracle(sec):
    piece = H.branch_piece(sec)
    sd = {k: v.double() for k, v in H.tiny_state().items() if k.startswith("detNet.") and v.is_floating_point()}
    got = H.STATEMENTS["branch"](piece.tensors, H.Relus(), piece.opts)
    for i in range(2):
        preds, lines = O.branch_heads(sd, piece.tensors["feat"][i][None], piece.tensors["priors"], H.TINY, "_sec" if piece.opts["sec"] else "")
        assert float((got[f"preds{i}"] - preds).abs().max()) <= 1e-12 and float((got[f"lines{i}"] - lines).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ the conditions
def test_a_flipped_unit_trips_the_mask_condition():
    piece = H.TOWERS[0]
    piece, run, masks = stand_in(piece)
    ref, _ = H.reference_and_floor(piece, masks)
    pre = ref.relus.pre[1]
    rms = pre.pow(2).mean().sqrt()
    unit = int((pre.abs() - rms).abs().argmin())
    wrong = [m.clone() for m in masks]
    wrong[1].view(-1)[unit] ^= True
    base = H.mask_report(ref.relus, masks)
    units, worst = H.mask_report(ref.relus, wrong)
    assert units == base[0] + 1 and 0.9 <= worst <= 1.1
    with pytest.raises(AssertionError, match="not near zero"):
        H.compare(piece, run.outs, run.grads, wrong)
    with pytest.raises(AssertionError, match="too many"):
        H.check_masks((H.MASK_MAX_UNITS + 1, 1e-6))
    with pytest.raises(AssertionError):                                          # a statement with ReLUs is never compared without masks
        H.compare(piece, run.outs, run.grads, None)


def test_hidden_relu_seed_conditions_hold():
    for piece in H.GATE_TAIL + H.gate_stack_pieces() + H.router_pieces():
        assert piece.hidden
        ratio = H.seed_condition(piece)
        units = sum(p.numel() for p in H.reference_and_floor(piece)[0].relus.pre)
        print(f"{piece.kind} {piece.name}: {units} hidden ReLU units, smallest |pre| / rms {ratio:.1e}")
        assert ratio > H.MASK_NEAR
        closed = sum(int((~m).sum()) for m in H.reference_and_floor(piece)[0].relus.masks)
        assert 0.2 * units < closed < 0.8 * units                                # closed ReLUs are part of the case
    assert [sum(p.numel() for p in H.reference_and_floor(q)[0].relus.pre) for q in H.gate_stack_pieces()] == [9216, 18432]
    # a case with a unit AT zero is rejected
    tail = H.GATE_TAIL[0]
    t = tail.tensors
    pre0 = float(F.linear(t["h"][:1], t["w"], t["b"]))
    bad = dataclasses.replace(tail, name="tail_at_zero", tensors={**t, "b": t["b"] - pre0})
    with pytest.raises(AssertionError, match="near zero"):
        H.seed_condition(bad)


def test_recovered_dropout_mask():
    gen = torch.Generator().manual_seed(3)
    p = 0.3
    x, res = H.rn(gen, 37, 128).float(), H.rn(gen, 37, 128).float()
    keep = torch.rand(37, 128, generator=gen) >= p
    t = res + x * keep / (1 - p)                                                 # fp32, as the device computes it
    assert torch.equal(H.recovered_keep(t, res), keep.double())
    y = F.gelu(x) * keep / (1 - p)
    assert torch.equal(H.recovered_keep(y), keep.double())
    # through the statement: the gradient of x is the cotangent on the kept entries times 1 / (1 - p), zero elsewhere
    piece = H.DROPOUT[1].with_tensors(keep=keep.double())
    ref, _ = H.reference_and_floor(piece)
    cot = H.cotangents(piece, {"y": ref.outs["y"].shape})["y"]
    assert torch.equal(ref.grads["x"] != 0, keep) and torch.allclose(ref.grads["x"], cot * keep / (1 - p), rtol=1e-15, atol=0)
    assert torch.equal(ref.grads["res"], cot)
    # a backward that drew another mask is far outside the bound
    other = torch.rand(37, 128, generator=gen) >= p
    wrong = dict(ref.grads, x=(cot * other / (1 - p)))
    assert any(k == "grad:x" for k, *_ in H.compare(piece, ref.outs, wrong).bad)


def test_perturbations_trip_the_bound():
    piece, run, masks = stand_in(H.LINEAR[0])

    def bad(grads, **kw):
        return {(k, m) for k, m, _, _ in H.compare(piece, run.outs, grads, masks, **kw).bad}

    assert bad(run.grads) == set()
    assert bad(dict(run.grads, w=run.grads["w"] * (1 + 1e-4))) == {("grad:w", "l2"), ("grad:w", "max")}
    assert ("grad:b", "l2") in bad(dict(run.grads, b=torch.zeros_like(run.grads["b"])))          # the bias gradient never written
    assert ("grad:b", "l2") in bad(dict(run.grads, b=run.grads["b"] * 2))                         # ... or added once too often
    one = run.grads["w"].clone()
    one.view(-1)[int(one.abs().argmax())] *= 1 + 1e-4                                            # a single entry
    assert ("grad:w", "max") in bad(dict(run.grads, w=one))
    # arena destinations: g0 + gradient is expected, so an overwrite and a double add are both seen
    g0 = {k: H.g0_pattern(v.shape) for k, v in run.grads.items() if k in piece.params}
    acc = {k: v + g0[k] if k in g0 else v for k, v in run.grads.items()}
    assert bad(acc, g0=g0) == set()
    assert {"grad:w", "grad:b"} <= {k for k, _ in bad(run.grads, g0=g0)}
    assert {"grad:w", "grad:b"} <= {k for k, _ in bad({k: v + 2 * g0[k] if k in g0 else v for k, v in run.grads.items()}, g0=g0)}
    # a sink used twice holds the sum
    twice = {k: 2 * v for k, v in run.grads.items()}
    assert bad(twice, times=2.0) == set() and len(bad(run.grads, times=2.0)) == 6
    # one row block of a packed projection missing
    piece, run, masks = stand_in(H.DECODER[0])
    k = "layers.1.multihead_attn.in_proj_weight"
    g = run.grads[k].clone()
    g[128:256] = 0
    assert {x for x, *_ in H.compare(piece, run.outs, dict(run.grads, **{k: g}), masks).bad} == {f"grad:{k}[k]"}
    # one block of the packed bias missing; the k block, whose true gradient is zero, holding something
    k = "layers.0.self_attn.in_proj_bias"
    g = run.grads[k].clone()
    g[256:] = 0
    assert {x for x, *_ in H.compare(piece, run.outs, dict(run.grads, **{k: g}), masks).bad} == {f"grad:{k}[v]"}
    g = run.grads[k].clone()
    g[128:256] += 1e-5 * g.abs().max()
    assert {x for x, *_ in H.compare(piece, run.outs, dict(run.grads, **{k: g}), masks).bad} == {f"grad:{k}[k]/whole"}


def test_zero_gradients_are_judged_by_the_noise_rule():
    piece = H.gate_stack_pieces()[0]
    _, run, _ = stand_in(piece)
    assert len(piece.zero_noise) == 8
    assert H.compare(piece, run.outs, run.grads).bad == []
    wrong = dict(run.grads)
    wrong["2.b1"] = run.grads["2.b1"] + 1e-3
    assert [k for k, *_ in H.compare(piece, run.outs, wrong).bad] == ["grad:2.b1"]
