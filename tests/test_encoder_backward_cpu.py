"""The encoder-backward harness (tests/encoder_cases.py) proves itself on the CPU, with plain torch fp32 standing in for
the device: run free, its ReLU masks and max-pool winners forced onto the fp64 reference.

  * the forced-mask reference sits at the fp32 floor for every parameter (<= 2e-5 relative L2, <= 4e-5 entry-wise: 1.5-2x the
    worst values measured when the harness was designed, so this test is not itself a rounding lottery), where free fp64
    autograd is 1e-3 .. 2e-2 away whenever a unit flipped;
  * the mask conditions hold for the stand-in;
  * forcing the fp64 run's own masks changes nothing (bit-identical gradients);
  * a deliberately wrong stand-in is caught, by the mask conditions and by the gradient bound.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import encoder_cases as E

FLOOR_L2 = 2e-5
FLOOR_MAX = 4e-5


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_forced_masks_reach_the_fp32_floor(case):
    s = E.stand_in(case)
    n_params = {"resnet18": 72, "resnet34": 120}[case.arch]
    assert len(s.grads) == n_params and set(s.grads) == set(s.ref.grads)
    report = E.mask_report(s.ref.hooks, s.masks, s.winners)
    print(f"{case.name}: fp32 vs forced fp64, relative L2 median / max {E.summary(s.e_l2)}, entry-wise {E.summary(s.e_max)}; "
          f"forward {max(s.e_fwd):.1e}; running statistics {max(s.e_stats.values()):.1e}; "
          f"flipped units {report[0]} (|pre| / rms <= {report[1]:.1e}), pool gap {report[2]:.1e}")
    E.check_masks(report, case.name)
    assert max(s.e_l2.values()) <= FLOOR_L2, max(s.e_l2.items(), key=lambda kv: kv[1])
    assert max(s.e_max.values()) <= FLOOR_MAX, max(s.e_max.items(), key=lambda kv: kv[1])
    # the stand-in against its own floor: the bound rule of the device test holds trivially, and finds nothing
    assert E.grad_violations(s.grads, s.ref.grads, s.e_l2, s.e_max) == []


def test_forcing_its_own_masks_changes_nothing():
    """Forced with the masks and winners the fp64 run chose itself == free fp64 autograd, bit for bit."""
    case = E.CASES[2]
    free = E.free_reference(case)
    forced = E.forced_reference(case, free.hooks.masks, free.hooks.winners)
    assert E.mask_report(forced.hooks, free.hooks.masks, free.hooks.winners) == (0, 0.0, 0.0)
    for a, b in zip(forced.outs, free.outs):
        assert torch.equal(a, b)
    for k, g in free.grads.items():
        assert torch.equal(forced.grads[k], g), k
    for k, v in free.buffers.items():
        assert torch.equal(forced.buffers[k], v), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1


def test_a_flipped_unit_trips_the_mask_condition():
    """One unit whose |pre-activation| is about its tensor's RMS, taken the other way: the forcing must not absorb it."""
    case = E.CASES[2]
    s = E.stand_in(case)
    hooks = s.ref.hooks
    layer = len(hooks.pre) // 2
    pre = hooks.pre[layer]
    rms = pre.pow(2).mean().sqrt()
    unit = int((pre.abs() - rms).abs().argmin())
    masks = [m.clone() for m in s.masks]
    masks[layer].view(-1)[unit] ^= True
    units, worst, gap = E.mask_report(hooks, masks, s.winners)
    base = E.mask_report(hooks, s.masks, s.winners)
    assert units == base[0] + 1 and 0.9 <= worst <= 1.1 and gap == base[2]
    with pytest.raises(AssertionError, match="not near zero"):
        E.check_masks((units, worst, gap))
    # and a pool winner that is not the window's maximum
    x = hooks.pool_in
    top, idx = F.max_pool2d(x, kernel_size=3, stride=2, padding=1, return_indices=True)
    w = x.shape[3]
    inner = top[0, 0, 1:-1, 1:-1]                           # an interior window, the one with the largest maximum
    pos = (0, 0, 1 + int(inner.argmax()) // inner.shape[1], 1 + int(inner.argmax()) % inner.shape[1])
    centre = (2 * pos[2]) * w + 2 * pos[3]                  # its centre pixel, or the pixel right of it: both inside the window
    if int(idx[pos]) == centre:
        centre += 1
    assert float(top[pos]) > 0 and float(x[0, 0].view(-1)[centre]) < float(top[pos])
    winners = s.winners.clone()
    winners[pos] = centre
    with pytest.raises(AssertionError, match="not a maximum"):
        E.check_masks(E.mask_report(hooks, s.masks, winners))
    # too many near-zero units is a finding too
    with pytest.raises(AssertionError, match="too many"):
        E.check_masks((E.MASK_MAX_UNITS + 1, 1e-6, 0.0))


def test_a_perturbed_gradient_trips_the_bound():
    """One BatchNorm weight's gradient off by 1e-4 relative - far below what the end-to-end tests can see."""
    case = E.CASES[2]
    s = E.stand_in(case)
    key = E.TRUNK + "layer2.0.bn2.weight"
    wrong = dict(s.grads)
    wrong[key] = s.grads[key] * (1.0 + 1e-4)
    bad = E.grad_violations(wrong, s.ref.grads, s.e_l2, s.e_max)
    assert {(k, m) for k, m, _, _ in bad} == {(key, "l2"), (key, "max")}, bad
    # a single entry, too
    wrong[key] = s.grads[key].clone()
    i = int(s.grads[key].abs().argmax())
    wrong[key][i] *= 1.0 + 1e-4
    assert [k for k, m, _, _ in E.grad_violations(wrong, s.ref.grads, s.e_l2, s.e_max) if m == "max"] == [key]


def test_free_fp64_is_not_a_usable_reference():
    """Why the masks are forced: where the fp32 run flipped a unit, free fp64 autograd is orders of magnitude above the floor;
    where it flipped none, free and forced are the same run."""
    for case in (E.CASES[0], E.CASES[2]):
        s = E.stand_in(case)
        flipped = E.mask_report(s.ref.hooks, s.masks, s.winners)[0]
        if flipped == 0:
            assert torch.equal(s.winners, s.ref.hooks.winners)
            continue
        free = E.free_reference(case)
        worst = max(E.rel_l2(s.grads[k], free.grads[k]) for k in s.grads)
        print(f"{case.name}: {flipped} flipped units, fp32 vs free fp64 max relative L2 {worst:.1e}")
        assert worst > 10 * FLOOR_L2


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_nearest_index_rule(case):
    """The device's integer source-index rule of the top-down path == F.interpolate(mode="nearest") at the case's map sizes
    (3x6 -> 5x11 is not an integer factor)."""
    shapes = E.level_shapes(case)
    for fine, coarse in ((shapes[1], shapes[2]), (shapes[0], shapes[1])):
        (H, W), (h, w) = fine[2:], coarse[2:]
        ramp = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w)
        up = F.interpolate(ramp, size=(H, W), mode="nearest").long()[0, 0]
        sy, sx = E.nearest_source_index(H, h), E.nearest_source_index(W, w)
        assert torch.equal(up, sy.view(-1, 1) * w + sx.view(1, -1)), (fine, coarse)


def test_winner_translation_matches_aten():
    """Window slots r * 3 + q as the device stores them -> the positions F.max_pool2d reports."""
    x = torch.randn(2, 4, 9, 11)
    _, idx = F.max_pool2d(x, kernel_size=3, stride=2, padding=1, return_indices=True)
    w = x.shape[3]
    oy = torch.arange(idx.shape[2]).view(-1, 1)
    ox = torch.arange(idx.shape[3]).view(1, -1)
    slots = ((idx // w - (2 * oy - 1)) * 3 + (idx % w - (2 * ox - 1))).to(torch.uint8)
    assert torch.equal(E.winners_from_argmax(slots.permute(0, 2, 3, 1), x.shape[2:]), idx)
