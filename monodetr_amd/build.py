"""Build libmonodetr_amd.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

    python -m monodetr_amd.build [--force] [--save-temps]      (--save-temps: recompile everything with register / LDS usage remarks)

The .so lands next to this file (monodetr_amd/libmonodetr_amd.so): git-ignored, but it travels to
the GPU box with the repo snapshot.  hipcc cross-compiles without a GPU.
"""
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
LIB = os.path.join(HERE, "libmonodetr_amd.so")
ARCH = "gfx950"


# .hip files that another translation unit includes (wpack.hip, ABI 19, and detect.hip, ABI 22: parts of capi.hip): dependencies, not sources
INCLUDED = [os.path.join(CSRC, "wpack.hip"), os.path.join(CSRC, "detect.hip")]


def sources():
    return sorted(set(glob.glob(os.path.join(CSRC, "*.hip"))) - set(INCLUDED))


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + INCLUDED + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h")) + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm); cannot build libmonodetr_amd.so")


def _flags():
    # -amdgpu-mfma-vgpr-form: MFMA accumulators live in ordinary VGPRs (unified register file on
    # gfx90a+).  Without it hipcc parks them in AGPRs and pays a v_accvgpr_read/write per element every
    # time the softmax touches a score: 14-19 % of the attention kernels' VALU instructions.
    return ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-mllvm",
            "-amdgpu-mfma-vgpr-form", "-Wno-pass-failed", "-I", INCLUDE, "-I", CSRC]


def _compile_one(args):
    src, obj, extra, verbose = args
    cmd = [hipcc()] + _flags() + extra + ["-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return obj


def _stamp():
    """What an object file depends on besides its source: compiler, architecture, flags (a change of any rebuilds everything)."""
    import hashlib
    return hashlib.sha256("\0".join([hipcc(), ARCH] + _flags()).encode()).hexdigest()[:16]


def build(force=False, save_temps=False, verbose=False):
    """One object per translation unit (kept under build_obj/, rebuilt when the source, any header, the compiler or a flag
    changed), compiled in parallel, then one link of EXACTLY the objects of sources(): a kernel edit costs one file's compile
    time; objects of deleted or renamed sources are removed."""
    objdir = os.path.join(HERE, "build_obj")
    os.makedirs(objdir, exist_ok=True)
    stamp_file = os.path.join(objdir, "flags.stamp")
    stamp = _stamp()
    same_flags = os.path.exists(stamp_file) and open(stamp_file).read().strip() == stamp
    if not force and same_flags and not _stale():
        return LIB
    hdr_t = max(os.path.getmtime(d) for d in INCLUDED + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h")) + [os.path.abspath(__file__)])
    extra = ["-Rpass-analysis=kernel-resource-usage"] if save_temps else []
    jobs, objs = [], []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if force or save_temps or not same_flags or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_t):
            jobs.append((src, obj, extra, verbose))
    for stale in set(glob.glob(os.path.join(objdir, "*.o"))) - set(objs):     # a deleted / renamed source's object must not be linked
        os.remove(stale)
    if jobs:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as ex:
            list(ex.map(_compile_one, jobs))
    with open(stamp_file, "w") as f:
        f.write(stamp)
    cmd = [hipcc(), "--offload-arch=" + ARCH, "-fPIC", "-shared", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, save_temps="--save-temps" in sys.argv, verbose=True))
