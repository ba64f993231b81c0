"""Golden fixtures under tests/golden/ are kept below 1 MiB per file.  A fixture too large for one .npz is stored as
`<stem>.partNN.npz`; an array too large for one part is cut along its first axis into members `<key>#<i>`.
`load(name)` returns the same dict of arrays whichever way the fixture is stored; `save` writes it that way."""
import glob
import io
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMIT = 900 << 10                     # bytes per part file: below 1 MiB with room for the zip directory


def _packed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def load(name):
    path = os.path.join(GOLD, name)
    if os.path.exists(path):
        return dict(np.load(path))
    parts = sorted(glob.glob(os.path.join(GOLD, name[:-len(".npz")] + ".part[0-9][0-9].npz")))
    if not parts:
        raise FileNotFoundError(path)
    out, pieces = {}, {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                if "#" in k:
                    key, i = k.rsplit("#", 1)
                    pieces.setdefault(key, {})[int(i)] = z[k]
                else:
                    out[k] = z[k]
    for key, ps in pieces.items():
        out[key] = np.concatenate([ps[i] for i in range(len(ps))])
    return out


def save(path, arrays):
    """np.savez_compressed(path, **arrays), or parts of at most LIMIT bytes when the whole would be larger."""
    stem = path[:-len(".npz")]
    for old in glob.glob(stem + ".part[0-9][0-9].npz"):
        os.remove(old)
    if _packed_size(arrays) <= LIMIT:
        np.savez_compressed(path, **arrays)
        return
    if os.path.exists(path):
        os.remove(path)
    members = []
    for k, a in arrays.items():
        chunks = [a]
        while a.ndim and len(chunks) < len(a) and any(_packed_size({k: c}) > LIMIT for c in chunks):
            chunks = np.array_split(a, len(chunks) + 1)
        members += [(k, a)] if len(chunks) == 1 else [(f"{k}#{i}", c) for i, c in enumerate(chunks)]
    part, parts = {}, []
    for k, a in members:
        if part and _packed_size({**part, k: a}) > LIMIT:
            parts.append(part)
            part = {}
        part[k] = a
    parts.append(part)
    for i, p in enumerate(parts):
        np.savez_compressed(f"{stem}.part{i:02d}.npz", **p)
