"""Build libcae_hip.so in-tree with hipcc for gfx950.

    python -m cae_tools_amd.build            # (re)build what is older than its sources
    python -m cae_tools_amd.build --force

Each .hip source is compiled to an object under csrc/_obj/, the sources in parallel, then the objects are linked into
csrc/libcae_hip.so.  hipcc writes the files each object was compiled from beside it (-MD); an object is compiled again when
one of them is newer, or when it has no such list.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(CSRC, "libcae_hip.so")
ARCH = "gfx950"
SOURCES = ["engine.hip", "ctbwd.hip", "unet_engine.hip", "vae_engine.hip", "linear_engine.hip"]
FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-cuda-compat", "-Wno-pass-failed"]
FLAGS += os.environ.get("CAE_HIPCC_FLAGS", "").split()     # tuning experiments: e.g. CAE_HIPCC_FLAGS=-DIG_KCW=32


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build libcae_hip.so")


def _obj(src):
    return os.path.join(OBJ, os.path.splitext(src)[0] + ".o")


def _deps(obj):
    """The files hipcc read for obj, from the dependency file it wrote beside it (None: there is none)."""
    try:
        with open(obj + ".d") as f:
            rule = f.read().replace("\\\n", " ")
    except OSError:
        return None
    return rule.split(": ", 1)[1].split()


def _stale(src):
    """An object is stale without a dependency file, or when a file named there is newer or gone."""
    obj, deps = _obj(src), _deps(_obj(src))
    if deps is None or not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps)


def needs_build():
    if any(_stale(s) for s in SOURCES) or not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(_obj(s)) > t for s in SOURCES)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    jobs = []
    for src in SOURCES:
        if force or _stale(src):
            cmd = [hipcc] + FLAGS + ["-I" + INC, "-I" + CSRC, "-MD", "-MF", _obj(src) + ".d", "-c", os.path.join(CSRC, src), "-o", _obj(src)]
            if verbose:
                print(" ".join(cmd), flush=True)
            jobs.append((src, subprocess.Popen(cmd)))
    failed = [src for src, p in jobs if p.wait() != 0]
    if failed:
        raise RuntimeError("hipcc failed for " + ", ".join(failed))
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB + ".tmp"] + [_obj(s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(LIB + ".tmp", LIB)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
