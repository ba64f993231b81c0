"""Builds phnet_amd/lib/libphnet_hip.so (gfx950) from phnet_amd/csrc/*.hip with hipcc.  In-tree, no JIT cache."""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "lib", "obj")
SO = os.path.join(HERE, "lib", "libphnet_hip.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]
# per-source additions.  SLP packs adjacent f32 adds into v_pk_add_f32, which costs more issue time beside MFMAs than the two plain adds
# it replaces (MI355X_MICROARCH.md): the producer waves of wgrad3s.hip / wgrad1s.hip / linrows.hip share their SIMDs with MFMA streams (50 -> 44 us per launch);
# measured on the other GEMM sources: -5 % (their split arithmetic sits in the MFMA waves themselves), so only there
EXTRA_FLAGS = {"wgrad3s.hip": ["-fno-slp-vectorize"], "wgrad1s.hip": ["-fno-slp-vectorize"], "linrows.hip": ["-fno-slp-vectorize"]}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    hdrs = glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(os.path.dirname(HERE), "include", "phnet_hip.h")]     # optim_guard.hip takes its constants from the public header
    newest_hdr = max([os.path.getmtime(h) for h in hdrs] + [0.0])
    objs, procs = [], []
    for s in srcs:
        o = os.path.join(OBJ, os.path.basename(s)[:-4] + ".o")
        objs.append(o)
        if force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(s), newest_hdr):
            if verbose:
                print("[phnet_amd.build] hipcc", os.path.basename(s), flush=True)
            procs.append((s, subprocess.Popen([_hipcc(), *FLAGS, *EXTRA_FLAGS.get(os.path.basename(s), []), "-c", s, "-o", o])))
    for s, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {s}")
    if procs or not os.path.exists(SO) or any(os.path.getmtime(o) > os.path.getmtime(SO) for o in objs):      # (an object another build left behind)
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO, *objs])
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
