"""Builds libconfignet_hip.so (gfx950) in-tree with hipcc.  Used by __graft_entry__.build()
and `python confignet_amd/build.py`.  No cmake, no JIT cache: the .so sits next to the sources
so it travels to the GPU box with the repo snapshot."""
import os
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libconfignet_hip.so")
SOURCES = ["prof.hip", "igemm_conv.hip", "small_conv.hip", "conv_dispatch.hip", "igemm_bf16.hip", "upfold.hip", "winograd.hip", "winograd4.hip", "c3_wgrad.hip", "thin_wgrad.hip", "wgrad2.hip", "fwd2.hip", "gemm.hip", "elementwise.hip", "norm_coef.hip", "rotate3d.hip", "depthwise.hip", "bn_train.hip", "hdri.hip", "dataset.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wall"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(CSRC), "..", "include", "confignet_hip.h"))
    objs = []
    procs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [hipcc] + FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on %s" % src)
    if force or procs or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    print(LIB)
