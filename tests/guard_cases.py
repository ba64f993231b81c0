"""The guarded AdamW step (include/phnet_hip.h, "guarded step", rules 1-8) restated in numpy, and the table of cases that the CPU and
the GPU tests share.  The restatement follows the header to the letter: the sum of squares in the header's order (so its float64 bits are
the device's), the scalars of rules 3-5 in float32, the AdamW element update in float64."""
import numpy as np

CHUNK = 131072                   # PHNET_GUARD_CHUNK
LANES, WAVE = 256, 64
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ rules 1-2
def sum_squares(g: np.ndarray):
    """(S as float64, non-finite count) of a float32 vector whose length is a multiple of 4, in the order of rule 1."""
    assert g.dtype == np.float32 and g.ndim == 1 and g.size % 4 == 0
    nonfinite = int(((g.view(np.uint32) & 0x7F800000) == 0x7F800000).sum())
    chunks = -(-g.size // CHUNK)
    d = np.zeros(chunks * CHUNK, np.float64)                       # vectors past n add +0
    d[:g.size] = g
    with np.errstate(all="ignore"):
        sq = (d * d).reshape(chunks, CHUNK // (4 * LANES), LANES, 4)      # [chunk][round of a lane][lane][component]
        acc = np.zeros((chunks, LANES, 4))
        for j in range(sq.shape[1]):                               # a lane's vectors in ascending order, one accumulator per component
            acc += sq[:, j]
        lane = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
        w = lane.reshape(chunks, LANES // WAVE, WAVE)
        for dist in (32, 16, 8, 4, 2, 1):                          # xor butterfly: every lane ends with the same bits
            w = w + w[..., np.arange(WAVE) ^ dist]
        w = w[..., 0]
        part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        S = np.float64(0.0)
        for c in range(chunks):                                    # ascending chunk index
            S = S + part[c]
    return S, nonfinite


# ------------------------------------------------------------------------------------------------------------------ rules 3-6
def guard(g, max_norm=None, skip_nonfinite=False, grad_scale=None, found_inf=None) -> dict:
    S, nonfinite = sum_squares(g)
    with np.errstate(all="ignore"):
        inv = F32(1.0) / F32(grad_scale) if grad_scale is not None else F32(1.0)
        norm = F32(np.sqrt(S) * np.float64(inv))
        coef = F32(1.0)
        if max_norm is not None:
            c = F32(max_norm) / F32(norm + F32(1e-6))
            coef = F32(1.0) if c > 1.0 else c                      # a NaN stays a NaN
        mult = F32(coef * inv)
    skip = bool(skip_nonfinite and (nonfinite > 0 or (found_inf is not None and found_inf != 0) or not np.isfinite(norm)))
    return {"S": S, "nonfinite": nonfinite, "norm": norm, "coef": coef, "mult": mult, "skip": skip}


# ------------------------------------------------------------------------------------------------------------------ rules 5, 7, 8
class Restated:
    """A guarded FlatAdamW over flat float64 state.  step(g) returns the dict of guard(); g (float32) is never written."""

    def __init__(self, p, n_decay, lr, betas, eps, weight_decay, max_norm=None, skip_nonfinite=False):
        self.p = np.asarray(p, np.float64).copy()
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.n_decay, self.lr, self.betas, self.eps, self.wd = n_decay, lr, betas, eps, weight_decay
        self.max_norm, self.skip_nonfinite = max_norm, skip_nonfinite
        self.step_count = self.skipped_steps = 0

    def step(self, g, grad_scale=None, found_inf=None):
        r = guard(g, self.max_norm, self.skip_nonfinite, grad_scale, found_inf)
        if r["skip"]:
            self.skipped_steps += 1
            return r
        self.step_count += 1
        with np.errstate(all="ignore"):
            ge = (g * r["mult"]).astype(np.float32).astype(np.float64)       # rule 5: one rounded float32 multiply
            b1, b2 = self.betas
            t = self.step_count
            self.p[:self.n_decay] *= 1.0 - self.lr * self.wd
            self.m = b1 * self.m + (1.0 - b1) * ge
            self.v = b2 * self.v + (1.0 - b2) * ge * ge
            self.p -= (self.lr / (1.0 - b1 ** t)) * (self.m / (np.sqrt(self.v) / np.sqrt(1.0 - b2 ** t) + self.eps))
        return r


# ------------------------------------------------------------------------------------------------------------------ the cases
LENGTHS = (4, CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 260, (1 << 22) + 12)
N_RAGGED = 3 * CHUNK + 260


def _normal(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def _case(name, grad, clip=None, skip_nonfinite=False, grad_scale=None, found_inf=None, skip=False, nonfinite=0):
    """clip: max_grad_norm as a multiple of the gradient's own (unscaled) norm - 0.5 clips, 100 does not; None: no clipping."""
    max_norm = None
    if clip is not None:
        with np.errstate(all="ignore"):
            finite = np.where(np.isfinite(grad), grad, 0).astype(np.float64)
        max_norm = float(F32(clip * np.sqrt((finite * finite).sum()) / (grad_scale or 1.0)))
    return {"name": name, "grad": grad, "n": grad.size, "n_decay": grad.size // 2 + 1,      # n_decay falls inside a 4-vector
            "max_norm": max_norm, "skip_nonfinite": skip_nonfinite, "grad_scale": grad_scale, "found_inf": found_inf,
            "skip": skip, "nonfinite": nonfinite}


def _poisoned(values_at, seed):
    g = _normal(N_RAGGED, seed)
    for pos, val in values_at:
        g[pos] = val
    return g


def _build():
    cases = []
    for i, n in enumerate(LENGTHS):                                                   # every length: clipped (mult != 1), not skipped
        cases.append(_case(f"len_{n}", _normal(n, 10 + i, 0.3), clip=0.5, skip_nonfinite=True))
    for i, n in enumerate((4, CHUNK + 4)):                                            # nothing triggers: mult == 1
        cases.append(_case(f"quiet_{n}", _normal(n, 20 + i, 0.3), clip=100.0, skip_nonfinite=True))
    spots = {"first": 0, "last": N_RAGGED - 1, "chunk_end": CHUNK - 1}
    for vi, (vname, val) in enumerate((("pinf", np.inf), ("ninf", -np.inf), ("nan", np.nan))):
        for si, (sname, pos) in enumerate(spots.items()):
            cases.append(_case(f"{vname}_{sname}", _poisoned([(pos, val)], 30 + 3 * vi + si), skip_nonfinite=True, skip=True, nonfinite=1))
    cases.append(_case("nan_and_inf", _poisoned([(7, np.nan), (2 * CHUNK + 1, np.inf)], 40), skip_nonfinite=True, skip=True, nonfinite=2))
    big = np.zeros(CHUNK + 4, np.float32)
    big[3] = big[CHUNK + 1] = 3e38                                                    # S finite in float64, norm overflows float32
    cases.append(_case("overflow_norm", big, skip_nonfinite=True, skip=True, nonfinite=0))
    cases.append(_case("denormals", np.full(CHUNK + 4, 1e-40, np.float32), skip_nonfinite=True))       # S > 0: no skip
    for name, factor in (("clip_below", 100.0), ("clip_above", 0.5), ("clip_above_1e4", 1e-4)):
        cases.append(_case(name, _normal(N_RAGGED, 50, 2.0), clip=factor))
    cases.append(_case("clip_nan_no_skip", _poisoned([(11, np.nan)], 51), clip=1.0, nonfinite=1))    # NaN propagates, as in torch
    scaled = _normal(N_RAGGED, 52) * F32(65536.0)
    cases.append(_case("scale_clean", scaled, clip=0.5, skip_nonfinite=True, grad_scale=65536.0, found_inf=0.0))
    cases.append(_case("scale_found_inf", scaled, skip_nonfinite=True, grad_scale=65536.0, found_inf=1.0, skip=True))
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


NAMES = ([f"len_{n}" for n in LENGTHS] + ["quiet_4", f"quiet_{CHUNK + 4}"]
         + [f"{v}_{s}" for v in ("pinf", "ninf", "nan") for s in ("first", "last", "chunk_end")]
         + ["nan_and_inf", "overflow_norm", "denormals", "clip_below", "clip_above", "clip_above_1e4", "clip_nan_no_skip",
            "scale_clean", "scale_found_inf"])


def case(name):
    return next(c for c in cases() if c["name"] == name)


def f64_norm(c) -> np.float32:
    """fl32(sqrt(sum of (double)g^2) * inv) with numpy's own (pairwise) float64 sum: the independent figure the device's norm is held to."""
    with np.errstate(all="ignore"):
        d = c["grad"].astype(np.float64)
        inv = F32(1.0) / F32(c["grad_scale"]) if c["grad_scale"] is not None else F32(1.0)
        return F32(np.sqrt((d * d).sum()) * np.float64(inv))
