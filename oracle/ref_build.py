"""Recipe for oracle/_ref/libmccnn_ref.so: the REFERENCE's own kernels and host launchers (its six tf_ops/*.cu files),
compiled with hipcc for gfx950 so that its arithmetic can run on the MI355X beside ours (tests/test_gpu_reference.py).

TEST INFRASTRUCTURE ONLY. The TensorFlow dependency of the reference lives in its tf_ops/*.cc op wrappers alone; the
.cu files use plain pointers, __syncthreads, shared memory and atomicAdd / atomicCAS, and compile unchanged once the
cuda* names are mapped onto hip* (ref_shim.h, ref_shim_aabb.h -- our own text, names only).

The sources are read IN PLACE from the directory the environment variable MCCNN_REFERENCE_DIR names (the checkout
root, the one that holds tf_ops/); nothing of them is copied into this tree, and oracle/_ref/ is ignored by git. Where
that directory does not exist (a GPU box that only receives the built library) build() does nothing and leaves an
existing oracle/_ref/ alone.

The compile mirrors the reference's own (tf_ops/genCompileScript.py:27-32): -O2, -DBLOCK_MLP_SIZE=8, no
PRINT_CONV_INFO, floating-point contraction at the compiler's default (fused, as nvcc's is). Plain gfx950: no xnack
feature, no sanitizer.
"""
import os
import shutil
import subprocess

_DIR = os.path.dirname(os.path.abspath(__file__))
REF_ENV = "MCCNN_REFERENCE_DIR"
REF_DEFAULT = "/root/reference"
OUT_DIR = os.path.join(_DIR, "_ref")
LIB = os.path.join(OUT_DIR, "libmccnn_ref.so")
ARCH = "gfx950"
BLOCK_MLP_SIZE = 8
#: the six files of genCompileScript.py:27-32, each with the forced include it needs
SOURCES = [("aabb_gpu.cu", "ref_shim_aabb.h"), ("sort_gpu.cu", "ref_shim.h"), ("find_neighbors.cu", "ref_shim.h"),
           ("compute_pdf.cu", "ref_shim.h"), ("poisson_sampling.cu", "ref_shim.h"), ("spatial_conv.cu", "ref_shim.h")]


def reference_dir():
    return os.environ.get(REF_ENV, REF_DEFAULT)


def available():
    return os.path.exists(LIB)


def _hipcc():
    return shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def build(force=False, verbose=False):
    """Compile the reference library. Returns its path, or None when the reference sources are not on this machine
    (then an existing oracle/_ref/ is left exactly as it is)."""
    src_dir = os.path.join(reference_dir(), "tf_ops")
    srcs = [os.path.join(src_dir, s) for s, _ in SOURCES]
    if not all(os.path.isfile(s) for s in srcs):
        return None
    deps = srcs + [os.path.join(_DIR, h) for h in ("ref_shim.h", "ref_shim_aabb.h")] + [os.path.abspath(__file__)]
    if not force and os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return LIB
    os.makedirs(OUT_DIR, exist_ok=True)
    objs = []
    for (name, shim), src in zip(SOURCES, srcs):
        obj = os.path.join(OUT_DIR, name + ".o")
        cmd = [_hipcc(), "-x", "hip", "--offload-arch=" + ARCH, "-O2", "-fPIC", "-DBLOCK_MLP_SIZE=%d" % BLOCK_MLP_SIZE,
               "-I", _DIR, "-include", shim, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, stderr=None if verbose else subprocess.DEVNULL)
        objs.append(obj)
    tmp = LIB + ".tmp"
    subprocess.check_call([_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC"] + objs + ["-o", tmp])
    os.replace(tmp, LIB)
    for o in objs:
        os.remove(o)
    return LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
