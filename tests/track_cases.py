"""Lane identities (csrc/lane_track.hip): a plain numpy restatement of the rules in include/phnet_hip.h and the test sequences.

The restatement is written from the rules, not from the kernel: Python loops, np.float32 for the sum of rule 2, Python floats
(doubles) for the ordering of rule 3, a sort where the kernel runs argmin rounds.  It also records what happened (`events`), so
that tests/test_track_cpu.py can show, without a GPU, that the sequences reach every branch.

Every built input is DYADIC: xs are multiples of 1/4096 in [0, 1], thr = 1/64, r[5] is an integer and r[2] = k / (S - 1) for a
small integer k (its product with S - 1 rounds to k).  Every sum, product and comparison is then exact in f32, so equality with
the kernel cannot depend on a summation order, and exact ties really occur."""
import functools

import numpy as np

THR = np.float32(1.0 / 64.0)
Q = 4096.0                                   # xs are integers / Q
ID_MAX = 2 ** 31 - 1
STATE_KEYS = ("id", "missed", "hits", "ext", "x", "next_id")


# ------------------------------------------------------------------------------------------------------------ the restatement
def new_state(M, S, next_id=1):
    """The state of ONE stream as numpy arrays (the layout of one row of tracking.TrackState)."""
    return dict(id=np.zeros(M, np.int32), missed=np.zeros(M, np.int32), hits=np.zeros(M, np.int32), ext=np.zeros((M, 2), np.int32),
                x=np.zeros((M, S), np.float32), next_id=np.array(next_id, np.int32))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def reset_state(st):
    st["id"][:] = 0                          # next_id is kept


def extent(r, S):
    """Rule 1 for one row -> (start, end) or None."""
    r2, r5 = float(r[2]), float(r[5])
    if not (np.isfinite(r2) and np.isfinite(r5)):
        return None
    start = min(max(float(np.rint(r2 * (S - 1))), 0.0), float(S - 1))
    end = min(start + float(np.rint(r5)) - 1.0, float(S - 1))
    return (int(start), int(end)) if end >= start else None


def pair_sum(a, b, lo, hi):
    """Rule 2: f32 accumulation, ascending."""
    s = np.float32(0.0)
    with np.errstate(all="ignore"):
        for i in range(lo, hi + 1):
            x, y = np.float32(a[i]), np.float32(b[i])
            s = np.float32(s + (np.float32(y - x) if x < y else np.float32(x - y)))
    return s


def _order(p, q):
    """Rule 3 on (sum, cnt, d, k) tuples."""
    l, r = float(p[0]) * q[1], float(q[0]) * p[1]
    if l < r:
        return -1
    if r < l:
        return 1
    return -1 if (p[2], p[3]) < (q[2], q[3]) else (1 if (p[2], p[3]) > (q[2], q[3]) else 0)


def track_frame(rows, num, st, thr, max_age):
    """One frame of one stream: rows f32 [L,6+S], num int; st is advanced in place -> (track_id [L], hits [L], events)."""
    L, S, M = rows.shape[0], rows.shape[1] - 6, len(st["id"])
    thr = np.float32(thr)
    ev = dict(skipped=[], disjoint=0, strict=0, nan_pair=0, tie_slots=0, tie_rows=0, matches=[], aged_out=[], births=[])
    kept = min(max(int(num), 0), L)
    ext = {}
    for d in range(L):
        if d >= kept:
            ev["skipped"].append("num")
            continue
        e = extent(rows[d], S)
        if e is None:
            ev["skipped"].append("nonfinite" if not (np.isfinite(rows[d, 2]) and np.isfinite(rows[d, 5])) else "empty")
        else:
            ext[d] = e
    cands = []
    for d, (ds, de) in ext.items():
        for k in range(M):
            if st["id"][k] == 0:
                continue
            lo, hi = max(ds, int(st["ext"][k, 0])), min(de, int(st["ext"][k, 1]))
            if hi < lo:
                ev["disjoint"] += 1
                continue
            s, cnt = pair_sum(rows[d, 6:], st["x"][k], lo, hi), hi - lo + 1
            bound = np.float32(thr * np.float32(cnt))
            if s < bound:
                cands.append((s, cnt, d, k))
            else:
                ev["strict"] += int(s == bound)
                ev["nan_pair"] += int(np.isnan(s))
    cands.sort(key=functools.cmp_to_key(_order))
    track_id, hits = np.full(L, -1, np.int32), np.zeros(L, np.int32)
    rows_taken, slots_taken = set(), set()
    for i, c in enumerate(cands):
        s, cnt, d, k = c
        if d in rows_taken or k in slots_taken:
            continue
        for o in cands[i + 1:]:                                                  # an exact tie that the (d, k) order decided
            if o[2] in rows_taken or o[3] in slots_taken or float(s) * o[1] != float(o[0]) * cnt:
                continue
            ev["tie_slots"] += int(o[2] == d)
            ev["tie_rows"] += int(o[3] == k)
        rows_taken.add(d); slots_taken.add(k)
        ev["matches"].append((d, k, int(st["missed"][k])))
        st["x"][k] = rows[d, 6:]
        st["ext"][k] = ext[d]
        st["missed"][k] = 0
        st["hits"][k] += 1
        track_id[d], hits[d] = st["id"][k], st["hits"][k]
    for k in range(M):
        if st["id"][k] != 0 and k not in slots_taken:
            st["missed"][k] += 1
            if st["missed"][k] > max_age:
                st["id"][k] = 0
                ev["aged_out"].append(k)
    filled = set()
    for d in sorted(ext):
        if d in rows_taken:
            continue
        free = [k for k in range(M) if st["id"][k] == 0]
        if free:
            k, how = free[0], "free"
        else:
            open_ = [k for k in range(M) if k not in slots_taken and k not in filled]
            oldest = max(int(st["missed"][k]) for k in open_)
            tied = [k for k in open_ if int(st["missed"][k]) == oldest]
            k, how = tied[0], ("evict_tie" if len(tied) > 1 else "evict")
        filled.add(k)
        nid = int(st["next_id"])
        st["id"][k], st["hits"][k], st["missed"][k] = nid, 1, 0
        st["ext"][k] = ext[d]
        st["x"][k] = rows[d, 6:]
        st["next_id"][...] = 1 if nid == ID_MAX else nid + 1
        track_id[d], hits[d] = nid, 1
        ev["births"].append((d, k, how))
    return track_id, hits, ev


def track_stream(kept, num, st, thr, max_age, resets=()):
    """T frames of one stream: kept [T,L,6+S], num [T]; a reset before every frame index in `resets`.  st is advanced in place
    -> (track_id [T,L], hits [T,L], list of events per frame)."""
    ids, hits, events = [], [], []
    for t in range(len(num)):
        if t in resets:
            reset_state(st)
        a, b, ev = track_frame(kept[t], int(num[t]), st, thr, max_age)
        ids.append(a); hits.append(b); events.append(ev)
    return np.stack(ids), np.stack(hits), events


# ------------------------------------------------------------------------------------------------------------------ hand cases
S_HAND, L_HAND = 12, 4


def row(S, x, start=0, length=None, conf=0.9):
    """A kept row with all xs = x / 4096 (x: a number or S numbers), extent [start, start + length - 1]."""
    r = np.zeros(6 + S, np.float32)
    r[1], r[2], r[5] = conf, np.float32(start / (S - 1)), S - start if length is None else length
    r[6:] = np.asarray(x, np.float64) / Q
    return r


def frames_of(S, L, frames, nums=None):
    """frames: a list of row lists -> (kept f32 [T,L,6+S], num i64 [T]); nums overrides the row counts."""
    kept = np.zeros((len(frames), L, 6 + S), np.float32)
    for t, rows in enumerate(frames):
        for d, r in enumerate(rows):
            kept[t, d] = r
    num = np.array([len(rows) for rows in frames] if nums is None else nums, np.int64)
    return kept, num


def _case(name, frames, M=8, max_age=2, nums=None, resets=(), next_id=1, S=S_HAND, L=L_HAND):
    kept, num = frames_of(S, L, frames, nums)
    return dict(name=name, S=S, L=L, M=M, max_age=max_age, kept=kept, num=num, resets=tuple(resets), next_id=next_id)


@functools.lru_cache(maxsize=None)
def hand_cases():
    S = S_HAND
    R = functools.partial(row, S)
    nan_x = np.full(S, 1000.0)
    nan_x[3] = np.nan
    A, B, C, D, E, F = (R(x) for x in (500, 1500, 2500, 3500, 4000, 100))
    empty = []
    return (
        # one row 20/4096 from two slots: the lower slot wins
        _case("tie_slots", [[R(1000), R(1040)], [R(1020)]]),
        # two rows 20/4096 from one slot: the lower row wins, the other is born
        _case("tie_rows", [[R(1020)], [R(1000), R(1040)]]),
        # sum == thr * cnt exactly: not a match
        _case("strict", [[R(1000)], [R(1064)]]),
        # equal xs, extents [0, 4] and [6, 10]
        _case("disjoint", [[R(1000, 0, 5)], [R(1000, 6, 5)]]),
        # a NaN x inside the common range, on the row's side and then (stored) on the slot's side
        _case("nan_x", [[R(1000)], [R(nan_x)], [R(1000)]]),
        # r[2] = inf, r[2] = NaN, r[5] = inf: not trackable, the fourth row is
        _case("nonfinite", [[_with(R(1000), 2, np.inf), _with(R(1000), 2, np.nan), _with(R(1000), 5, np.inf), R(1000)],
                            [_with(R(1000), 2, -np.inf), R(1000)]]),
        # length 0 and a negative length: end < start
        _case("empty_extent", [[R(1000, 3, 0), R(2000, 3, -4), R(3000, 3, 1)], [R(3000, 3, 0), R(3000)]]),
        # num = 0 on rows that look valid
        _case("num_zero", [[R(1000), R(2000)], [R(1000), R(2000)], [R(1000)]], nums=[2, 0, 1]),
        # num > L is clamped to L
        _case("num_above_L", [[R(500), R(1500), R(2500), R(3500)], [R(1500), R(500), R(3500), R(2500)]], nums=[7, 1 << 40]),
        # num < 0 is 0
        _case("num_negative", [[R(1000)], [R(1000)], [R(1000)]], nums=[1, -3, 1]),
        # missed == max_age at the re-acquisition: the id is kept
        _case("reacquire", [[R(1000)], empty, empty, [R(1000)]], max_age=2),
        # missed == max_age + 1: freed, a new id
        _case("aged_out", [[R(1000)], empty, empty, empty, [R(1000)]], max_age=2),
        # M = L = 4 slots all live: E evicts on a tie (slots 0 and 1 both missed twice -> slot 0), F the one largest missed
        _case("evict", [[A, B, C, D], [C, D], [C, D, E], [D, E, F]], M=4, max_age=5),
        # next_id = 2^31 - 1: the second birth gets 1
        _case("wrap", [[R(1000), R(2000)], [R(2000), R(1000), R(3000)]], next_id=ID_MAX),
        # a reset between the frames: no match, and the id is a new one
        _case("reset", [[R(1000)], [R(1000)], [R(1000)]], resets=(1,)),
    )


def _with(r, col, value):
    r = r.copy()
    r[col] = value
    return r


# ----------------------------------------------------------------------------------------------------------- random sequences
RANDOM_CONFIGS = tuple((S, M, age) for S in (72, 37) for M, age in ((8, 3), (4, 1)))
RANDOM_STREAMS, RANDOM_FRAMES, GROUND, L_RANDOM = 3, 40, 6, 4


@functools.lru_cache(maxsize=None)
def random_sequence(S, seed):
    """40 frames of 6 ground lanes >= 500/4096 apart, each visible with probability 0.75 and drawn with a per-offset jitter of
    +-8/4096; a frame keeps up to L = 4 of the visible ones in random order.  Rows beyond num are copies of row 0 (they would
    match if they were looked at).  -> (kept [T,4,6+S], num [T], ground int [T,4]: the ground lane of each row, -1 beyond num)."""
    rng = np.random.default_rng(seed)
    base = np.array([300 + 600 * g + int(rng.integers(0, 100)) for g in range(GROUND)])
    kept = np.zeros((RANDOM_FRAMES, L_RANDOM, 6 + S), np.float32)
    num = np.zeros(RANDOM_FRAMES, np.int64)
    ground = np.full((RANDOM_FRAMES, L_RANDOM), -1, np.int64)
    for t in range(RANDOM_FRAMES):
        seen = rng.permutation(np.flatnonzero(rng.random(GROUND) < 0.75))[:L_RANDOM]
        num[t] = len(seen)
        for d, g in enumerate(seen):
            start = int(rng.integers(0, 4))
            length = S - start - int(rng.integers(0, 4))
            kept[t, d] = row(S, base[g] + rng.integers(-8, 9, S), start, length, conf=0.5 + 0.1 * d)
            ground[t, d] = g
        for d in range(len(seen), L_RANDOM):
            kept[t, d] = kept[t, 0]
    return kept, num, ground


def random_seed(S, b):
    return 1000 * S + b


@functools.lru_cache(maxsize=None)
def random_expected(S, M, max_age, b):
    """The restatement on stream b of a random configuration, from a fresh state: (track_id, hits, events, final state)."""
    kept, num, _ = random_sequence(S, random_seed(S, b))
    st = new_state(M, S)
    ids, hits, events = track_stream(kept, num, st, THR, max_age)
    return ids, hits, events, st


@functools.lru_cache(maxsize=None)
def hand_expected(i):
    c = hand_cases()[i]
    st = new_state(c["M"], c["S"], c["next_id"])
    ids, hits, events = track_stream(c["kept"], c["num"], st, THR, c["max_age"], c["resets"])
    return ids, hits, events, st
