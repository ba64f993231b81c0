"""tests/golden/branchb_parent_bits.npz is there, loads, and covers the shapes tests/test_rowchain_attn_gpu.py holds the kernels to
(no GPU): a stale or truncated fixture fails here."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_goldens_branchb_bits", os.path.join(HERE, "golden", "make_goldens_branchb_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
ATTN, (MODEL, MODEL_REC) = G.load()


def test_fixture_was_recorded_from_the_case_list_of_its_recorder():
    assert [c for c, _ in ATTN] == G.ATTN_CASES
    assert MODEL == G.MODEL


def test_attention_cases_cover_the_shapes():
    cross = [c for c, _ in ATTN if not c["self_attn"]]
    assert {c["R"] for c in cross} >= set(G.ROWS) == {1, 16, 17, 240}
    assert {c["Lk"] for c in cross} >= set(G.KEYS) == {1, 16, 17, 41}
    assert {(c["R"], c["Lk"]) for c in cross} >= {(r, lk) for r in (1, 16, 17) for lk in G.KEYS}
    assert {c["mask"] for c in cross} == set(G.MASKS) and {c["p"] for c in cross} == set(G.PS)
    assert {(c["mask"], c["p"]) for c in cross} == {(m, p) for m in G.MASKS for p in G.PS}
    assert {c["mask"] for c in cross if c["R"] == 240} >= {"few", "none"}
    assert any(c["batch"] == 2 and c["R"] == 17 for c in cross)
    assert [(c["R"], c["Lk"]) for c, _ in ATTN if c["self_attn"]] == [(240, 240)]


def test_recorded_arrays_have_the_shapes_of_their_cases():
    for c, rec in ATTN:
        assert rec["o"].dtype == np.uint32 and rec["o"].shape == (c["batch"] * c["R"], G.E), c
        assert rec["lse"].dtype == np.uint32 and rec["lse"].shape == (c["batch"] * G.H, c["R"]), c
        o = rec["o"].view(np.float32)
        assert np.isfinite(o).all(), c
        if not G.key_mask(c).any():                            # no valid key ("none", and "few" at Lk = 1): rows of zeros
            assert not o.any(), c
        else:
            assert o.any(), c


def test_model_part_holds_two_stages_and_the_frames_with_a_memory():
    assert MODEL["stages"] == [0, 1] and MODEL["frames"] == [1, 2] and MODEL["T"] == 3 and MODEL["p"] == 0.1
    assert sorted(MODEL_REC) == sorted(f"s{s}_t{t}_{k}" for s in (0, 1) for t in (1, 2) for k in ("pred", "line"))
    shapes = {v.shape for v in MODEL_REC.values()}
    assert len(shapes) == 1 and all(v.dtype == np.uint32 for v in MODEL_REC.values())
    for s in (0, 1):
        for t in (1, 2):
            pred, line = (MODEL_REC[f"s{s}_t{t}_{k}"].view(np.float32) for k in ("pred", "line"))
            assert np.isfinite(pred[..., :6]).all()
            assert np.array_equal(pred[..., :6], line[..., :6])          # the lane update copies the head columns into both
    assert not np.array_equal(MODEL_REC["s0_t1_pred"], MODEL_REC["s0_t2_pred"])


def test_fixture_stays_well_under_the_size_limit_of_a_committed_file():
    """A committed file may be 1 MiB at the most; the fixture is held to two thirds of that."""
    assert os.path.getsize(G.FIXTURE) < 2 * (1 << 20) // 3
