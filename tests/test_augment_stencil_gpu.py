"""The neighbourhood ops of the training augmentation on the MI355X (csrc/augment_stencil.hip, the stencil switch of csrc/augment.hip,
`phnet_augment_stencil_u8`) against the restatement of tests/stencil_cases.py.

Bounds.  The augmented 8-bit image equals the restatement EXACTLY: rule 7 is integer arithmetic, and rules 1 - 3 and 6 behind it are
held as tests/test_augment_gpu.py holds them; the float output equals the float32 epilogue of those bytes bit for bit, in both layouts.
Launch shapes against each other (a null or all-zero stencil against `phnet_augment_u8`, a replayed graph against eager) are compared
bit for bit.  Properties that do not go through the restatement: a flat image stays flat, an impulse comes out as the point-reflected
weight pattern, an isolated pixel disappears under the median.

Flat images under the EDGE filters: the issue behind this file asks that a constant image stay constant under every op, and defines the
edge kernels by imgaug's formula, whose weights sum to 1 - alpha; both cannot hold (tests/test_augment_stencil_cpu.py says more).  The
formula is kept, and the check here is the exact consequence: a flat image of value v comes out flat, borders included, with the value
clamp((v * sum(e) + 2048) >> 12, 0, 255); under every blur it comes out as v."""
import ctypes

import numpy as np
import pytest
import torch

from tests import augment_cases as AC
from tests import stencil_cases as SC

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _augmenter(H, W):
    from phnet_amd.libs.dataset.openlane.augment import ClipAugmenter
    return ClipAugmenter(H, W, mean=AC.MEAN, std=AC.STD, device="cuda")


def _run(frames_np, params, layout="nchw"):
    """(float output, augmented u8) as numpy, through ClipAugmenter, with NaN-filled / 0xAB-filled buffers given."""
    frames = torch.from_numpy(np.array(frames_np)).cuda()
    T, H, W, _ = frames.shape
    out = torch.full((T, 3, H, W) if layout == "nchw" else (T, H, W, 4), float("nan"), device="cuda")
    out_u8 = torch.full_like(frames, 0xAB)
    got, got_u8 = _augmenter(H, W)(frames, params.to("cuda"), layout=layout, out=out, return_u8=True, out_u8=out_u8)
    assert got.data_ptr() == out.data_ptr() and got_u8.data_ptr() == out_u8.data_ptr()
    return got.cpu().numpy(), got_u8.cpu().numpy()


def _assert_image(got, got_u8, want_u8, layout, what):
    bad = np.argwhere(got_u8 != want_u8)
    assert len(bad) == 0, (what, layout, len(bad), bad[:4].tolist(), got_u8[tuple(bad[0])], want_u8[tuple(bad[0])])
    assert np.array_equal(got.view(np.int32), AC.epilogue(want_u8, layout).view(np.int32)), (what, layout)


@pytest.mark.parametrize("shape", list(SC.SHAPES))
@pytest.mark.parametrize("name", list(SC.PARAM_SETS))
def test_image_equals_the_restatement(shape, name):
    _need_gpu()
    want_u8 = SC.expected(shape, name)
    for layout in ("nchw", "nhwc4"):
        got, got_u8 = _run(SC.frames(shape), SC.params(shape, name), layout)
        _assert_image(got, got_u8, want_u8, layout, (shape, name))


def test_mixed_clip_frame_without_an_op_is_the_plain_entry():
    """Frame 0 of the mixed clip has no neighbourhood op: its bytes are phnet_augment_u8's on that frame."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    p = SC.params("tiny", "mixed")
    assert [SC.active(r) for r in p.numpy()["stencil"]] == [False, True, True]
    got, got_u8 = _run(SC.frames("tiny"), p)
    plain, plain_u8 = _run(SC.frames("tiny"), AugmentParams(*p.tensors()[:4]))
    assert np.array_equal(got_u8[0], plain_u8[0]) and np.array_equal(got[0].view(np.int32), plain[0].view(np.int32))
    assert not np.array_equal(got_u8[1], plain_u8[1]) and not np.array_equal(got_u8[2], plain_u8[2])


@pytest.mark.parametrize("shape", list(SC.SHAPES))
def test_flat_image_stays_flat(shape):
    _need_gpu()
    T, H, W = SC.SHAPES[shape]
    flat = np.full((T, H, W, 3), 93, np.uint8)
    for name in SC.SINGLE_OPS:
        p = SC.params(shape, name)
        want = 93
        if "edge" in name:
            want = int(np.clip((93 * int(p.numpy()["stencil"][0, 1:10].astype(np.int64).sum()) + 2048) >> 12, 0, 255))
            assert want != 93
        _, got_u8 = _run(flat, p)
        assert (got_u8 == want).all(), (shape, name, want, np.unique(got_u8).tolist())


@pytest.mark.parametrize("name", ["motion3", "motion5", "gauss3", "gauss5", "gauss7", "gauss9"])
def test_impulse_gives_the_weight_pattern(name):
    """One 255 pixel in the middle of a zero 11 x 11 image: B(c + R - j, c + R - i) = (w[j][i] * 255 + half) >> shift, the weights
    point-reflected about the centre (the filters are correlations), and zero elsewhere."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    img = np.zeros((1, 11, 11, 3), np.uint8)
    img[0, 5, 5] = 255
    p = AugmentParams.build([SC.PARAM_SETS[name]], 11, 11)
    s = SC.row(p.numpy()["stencil"][0])
    k, R = s["k"], s["k"] // 2
    if s["kind"] == 1:
        w, half, shift = s["weights"], 2048, 12
    else:
        w, half, shift = np.outer(s["weights"], s["weights"]), 32768, 16
    want = np.zeros((11, 11), np.int64)
    for j in range(k):
        for i in range(k):
            want[5 + R - j, 5 + R - i] = (w[j, i] * 255 + half) >> shift
    assert want.max() > 0 and want.max() < 255
    _, got_u8 = _run(img, p)
    assert all(np.array_equal(got_u8[0, :, :, c], want) for c in range(3)), (name, got_u8[0, :, :, 0].tolist(), want.tolist())


@pytest.mark.parametrize("k", [3, 5])
def test_isolated_pixel_disappears_under_the_median(k):
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    img = np.zeros((1, 11, 11, 3), np.uint8)
    img[0, 5, 5] = 255
    _, got_u8 = _run(img, AugmentParams.build([dict(blur=dict(kind="median", k=k))], 11, 11))
    assert not got_u8.any()


def _entry(frames, p, stencil, staged, layout=0, T=None, H=None, W=None, std=AC.STD, out_u8=True, null=()):
    """phnet_augment_stencil_u8 called directly -> (rc, out, out_u8)."""
    from phnet_amd._lib import lib
    t, h, w, _ = frames.shape
    out = torch.full((t, 3, h, w) if layout == 0 else (t, h, w, 4), float("nan"), device="cuda")
    u8 = torch.full_like(frames, 0xAB) if out_u8 else None
    mean3, std3 = (ctypes.c_float * 3)(*AC.MEAN), (ctypes.c_float * 3)(*std)
    ptr = lambda name, x: None if x is None or name in null else x.data_ptr()          # noqa: E731
    rc = lib().phnet_augment_stencil_u8(ptr("frames", frames), ptr("out", out), ptr("out_u8", u8), ptr("flip2", p.flip2), ptr("inv", p.inv),
                                        ptr("table", p.table), ptr("stencil", stencil), ptr("staged", staged), t if T is None else T,
                                        h if H is None else H, w if W is None else W, layout, ctypes.cast(mean3, ctypes.c_void_p),
                                        ctypes.cast(std3, ctypes.c_void_p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out, u8


def test_null_and_zero_stencil_equal_the_plain_entry():
    """stencil = NULL and an all-zero stencil table against phnet_augment_u8, bit for bit, on every parameter set of augment_cases."""
    _need_gpu()
    from phnet_amd import hip_ops as K
    T, H, W = AC.SHAPES["tiny"]
    frames = torch.from_numpy(np.array(AC.frames("tiny"))).cuda()
    mean3, std3 = (ctypes.c_float * 3)(*AC.MEAN), (ctypes.c_float * 3)(*AC.STD)
    zeros = torch.zeros((T, K.AUGMENT_STENCIL_COLS), dtype=torch.int32, device="cuda")
    staged = torch.full_like(frames, 0x5C)                                             # never read: no frame has an op
    for name in AC.PARAM_SETS:
        p = AC.params("tiny", name).to("cuda")
        for layout in (0, 1):
            want_u8 = torch.full_like(frames, 0xAB)
            want = K.augment_u8(frames, p.flip2, p.inv, p.table, mean3, std3, layout="nchw" if layout == 0 else "nhwc4", out_u8=want_u8)
            for stencil, scratch in ((None, None), (None, staged), (zeros, staged)):
                rc, got, got_u8 = _entry(frames, p, stencil, scratch, layout)
                assert rc == 0 and torch.equal(_bits(got), _bits(want)) and torch.equal(got_u8, want_u8), (name, layout, stencil is None)
    assert (staged == 0x5C).all()                                                      # and never written


def test_argument_checks():
    _need_gpu()
    from phnet_amd import hip_ops as K
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    T, H, W = 2, 5, 7
    frames = torch.zeros((T, H, W, 3), dtype=torch.uint8, device="cuda")
    p = AugmentParams.identity(T, stencil=True).to("cuda")
    staged = torch.empty_like(frames)
    assert _entry(frames, p, p.stencil, staged)[0] == 0
    assert _entry(frames, p, p.stencil, None)[0] == ERR_ARG                            # a stencil without a staging buffer
    assert _entry(frames, p, None, None)[0] == 0
    assert _entry(frames, p, p.stencil, staged, out_u8=False)[0] == 0                  # out_u8 is optional, as before
    for kw in (dict(layout=2), dict(H=0), dict(W=0), dict(T=-1), dict(H=32769), dict(W=32769), dict(std=(0.2, 0.0, 0.2)),
               dict(null=("frames",)), dict(null=("out",)), dict(null=("flip2",)), dict(null=("inv",)), dict(null=("table",))):
        layout = kw.pop("layout", 0)
        assert _entry(frames, p, p.stencil, staged, layout, **kw)[0] == ERR_ARG, kw
    rc, out, _ = _entry(frames, p, p.stencil, staged, T=0, null=("frames", "out", "staged"))     # T == 0 is a no-op
    assert rc == 0 and torch.isnan(out).all()
    aug = _augmenter(H, W)
    with pytest.raises(ValueError):                                                    # the wrapper: staged must be its own buffer
        K.augment_u8(frames, p.flip2, p.inv, p.table, aug._mean, aug._std, stencil=p.stencil, staged=frames)
    with pytest.raises(ValueError):
        K.augment_u8(frames, p.flip2, p.inv, p.table, aug._mean, aug._std, stencil=p.stencil[:1], staged=staged)


def test_wild_table_is_clamped():
    """Kind 77, k = -3 and 1000, weights +-2^31, junk in the zero columns: the kernels clamp as rule 7 states, stay in bounds, and equal
    the restatement with the same clamps."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams
    T, H, W = SC.WILD_SHAPE
    frames = np.random.default_rng(16).integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    base = AugmentParams.build([dict(rotate=3.0), dict(flip=True), {}, dict(value=5)], H, W)
    stencil = SC.wild_stencil()
    rows = [SC.row(r) for r in stencil]
    assert [(r["edge"], r["kind"], r["k"]) for r in rows] == [(True, 0, 0), (False, 2, 3), (False, 3, 9), (True, 1, 5)]
    p = AugmentParams(*base.tensors(), torch.from_numpy(stencil))
    n = base.numpy()
    want_u8 = SC.augment(frames, n["flip2"], n["inv"], n["table"], stencil)
    plain = SC.augment(frames, n["flip2"], n["inv"], n["table"], None)
    assert all(not np.array_equal(want_u8[t], plain[t]) for t in range(T))
    # guard pages of known bytes around the staging buffer and the output: nothing outside is written
    dev = torch.from_numpy(frames).cuda()
    pad = H * W * 3
    big = torch.full((T * H * W * 3 + 2 * pad,), 0x77, dtype=torch.uint8, device="cuda")
    staged = big[pad:-pad].view(T, H, W, 3)
    rc, got, got_u8 = _entry(dev, p.to("cuda"), p.stencil.cuda(), staged)
    assert rc == 0
    _assert_image(got.cpu().numpy(), got_u8.cpu().numpy(), want_u8, "nchw", "wild")
    assert (big[:pad] == 0x77).all() and (big[-pad:] == 0x77).all()
    for t in range(T):
        assert np.array_equal(staged[t].cpu().numpy(), SC.staged(frames, n["flip2"], n["table"], stencil, t)), t


def test_captured_graph_reads_the_stencil_at_replay():
    """pre(frames, augment=params, out=...) captured; a replay after copy_into of a table that switches frame 1 from median to none
    and frame 0 from none to edge equals eager - the staging launch is in the graph whatever the table held at capture."""
    _need_gpu()
    from phnet_amd.libs.dataset.openlane.augment import AugmentParams, edge_kernel, gaussian_kernel
    from phnet_amd.libs.dataset.openlane.preprocess import ClipPreprocessor
    T, H, W = AC.SHAPES["tiny"]
    pre = ClipPreprocessor(H, W, src_h=100, src_w=200, crop_size=10, device="cuda")
    frames = torch.from_numpy(np.random.default_rng(34).integers(0, 256, (T, 100, 200, 3), dtype=np.uint8)).cuda()
    gauss = dict(kind="gaussian", k=5, weights=gaussian_kernel(1.0))
    first = [dict(rotate=3.0), dict(blur=dict(kind="median", k=5), flip=True), dict(blur=gauss)]
    second = [dict(rotate=3.0, edge=dict(weights=edge_kernel(0.2))), dict(flip=True), dict(blur=gauss)]
    tables = [AugmentParams.build(f, H, W, stencil=True) for f in (first, second)] + [AugmentParams.identity(T)]
    live = tables[0].to("cuda")
    clip = torch.full((T, 3, H, W), float("nan"), device="cuda")
    pre(frames, augment=live, out=clip)                                                # warm-up: both staging buffers exist
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    pre(frames, augment=live, out=clip)
    assert torch.cuda.memory_allocated() == before                                     # a second call allocates nothing
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pre(frames, augment=live, out=clip)
    seen = []
    for table in (tables[1], tables[0], tables[2]):
        table.copy_into(live)
        clip.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(clip), _bits(pre(frames, augment=table.to("cuda"))))
        seen.append(clip.clone())
    assert not torch.equal(_bits(seen[0][0]), _bits(seen[1][0])) and not torch.equal(_bits(seen[0][1]), _bits(seen[1][1]))
    assert torch.equal(_bits(seen[0][2]), _bits(seen[1][2])) and torch.equal(_bits(seen[2]), _bits(pre(frames)))
    # and the restatement, through the preprocessor, on the resized bytes
    _, u8 = pre(frames, return_u8=True)
    n = tables[1].numpy()
    want_u8 = SC.augment(u8.cpu().numpy(), n["flip2"], n["inv"], n["table"], n["stencil"])
    got, got_u8 = pre(frames, augment=tables[1].to("cuda"), return_u8=True)
    _assert_image(got.cpu().numpy(), got_u8.cpu().numpy(), want_u8, "nchw", "preprocessor")
