"""Recipe for oracle/_ref/: the reference rasterizer's own CUDA sources, compiled for the CPU (TEST INFRASTRUCTURE ONLY).

The three translation units of the reference checkout (cuda_rasterizer/forward.cu, backward.cu, rasterizer_impl.cu) are read where they lie,
their kernel launches `k<<<g, b>>>(` -- also in the spaced form `k << <g, b >> > (` -- are rewritten into `REFCPU_LAUNCH(g, b, k)(`, and the
rewritten copies are compiled by g++ against the stand-in headers of oracle/ref_cpu/shim/ (see refcpu.h for what those decide), the
reference's own headers and its own copy of glm, together with runtime.cpp and entry.cpp.  Two builds, like the oracle's: operation by
operation (-ffp-contract=off) and with contraction left to the compiler (-ffp-contract=fast -mfma).

Everything this writes -- rewritten sources and libraries -- goes to oracle/_ref/, which git ignores: no program text of the reference, nor
anything compiled from it, belongs in this repository.  The rewrite below is a pattern; it holds no line of the reference.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "_ref")
GEN = os.path.join(OUT, "gen")
SO = os.path.join(OUT, "libibgs_ref_cpu.so")
SO_FMA = os.path.join(OUT, "libibgs_ref_cpu_fma.so")
UNITS = ("forward.cu", "backward.cu", "rasterizer_impl.cu")
OWN = [os.path.join(HERE, n) for n in ("entry.cpp", "runtime.cpp")]
SHIM = os.path.join(HERE, "shim")

# kernel name (with template arguments, if any), launch configuration, up to the opening parenthesis of the argument list
_LAUNCH = re.compile(r"([A-Za-z_]\w*(?:\s*<[^<>;(){}]*>)?)\s*<<\s*<\s*([^;{}]*?)\s*>>\s*>\s*\(")


_ROOT = []          # reference_root()'s answer, looked up once


def reference_root():
    """The reference checkout's rasterizer directory -- the checkout tests/golden/_ref_import.py names in its REF constant, read from that file's text so that
    nothing is imported for it --, or None where there is none."""
    if not _ROOT:
        d = None
        try:
            with open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests", "golden", "_ref_import.py"), encoding="utf-8") as f:
                m = re.search(r'^REF = "([^"]+)"', f.read(), re.M)
            d = os.path.join(m.group(1), "submodules", "diff-plane-rasterization")
            if not all(os.path.exists(os.path.join(d, "cuda_rasterizer", u)) for u in UNITS):
                d = None
        except (OSError, AttributeError):
            d = None
        _ROOT.append(d)
    return _ROOT[0]


def _dependencies(root):
    """Everything the libraries are compiled from: the three units and every header of the reference's rasterizer, this directory's sources, every stand-in header."""
    deps = list(OWN) + [os.path.abspath(__file__)]
    cr = os.path.join(root, "cuda_rasterizer")
    deps += [os.path.join(cr, n) for n in os.listdir(cr) if n.endswith((".cu", ".h"))]
    for base, _, names in os.walk(SHIM):
        deps += [os.path.join(base, n) for n in names]
    return deps


def rewrite_launches(text):
    return _LAUNCH.sub(lambda m: "REFCPU_LAUNCH(%s, %s)(" % (m.group(2), m.group(1)), text)


def available():
    return os.path.exists(SO) and os.path.exists(SO_FMA)


def build(force=False, verbose=False):
    """Build both libraries from the reference checkout; returns the plain one's path.  Without a checkout an existing oracle/_ref is left
    alone (and None is returned when there is none)."""
    root = reference_root()
    if root is None:
        return SO if available() else None
    srcs = [os.path.join(root, "cuda_rasterizer", u) for u in UNITS]
    newest = max(os.path.getmtime(p) for p in _dependencies(root))
    if (not force) and available() and min(os.path.getmtime(SO), os.path.getmtime(SO_FMA)) >= newest:
        return SO
    os.makedirs(GEN, exist_ok=True)
    gen = []
    for u, src in zip(UNITS, srcs):
        with open(src, encoding="utf-8") as f:
            text = rewrite_launches(f.read())
        assert "<<<" not in text.replace(" ", ""), "a kernel launch in %s escaped the rewrite" % u
        dst = os.path.join(GEN, u + ".cpp")
        with open(dst, "w", encoding="utf-8") as f:
            f.write(text)
        gen.append(dst)
    inc = ["-I", SHIM, "-I", os.path.join(root, "cuda_rasterizer"), "-I", os.path.join(root, "third_party", "glm")]
    common = ["g++", "-std=c++17", "-O2", "-fno-fast-math", "-DGLM_FORCE_PURE", "-w", "-shared", "-fPIC"] + inc
    for so, flags in ((SO, ["-ffp-contract=off"]), (SO_FMA, ["-ffp-contract=fast", "-mfma"])):
        cmd = common + flags + ["-o", so] + gen + OWN
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return SO


def sanitize(kind="undefined", verbose=True):
    """Build sanitize_driver.cpp -- a stand-alone program with its own main: forward and backward of a small 3-source geo scene in both texture modes and both block
    orders -- together with entry.cpp, runtime.cpp and the generated sources under -fsanitize=`kind` ("undefined" or "address") into oracle/_ref/, and run it.
    (ASan does not fully support swapcontext and says so at start-up; detect_stack_use_after_return stays off for the fibers' stacks.)"""
    root = reference_root()
    assert root is not None and build() is not None, "needs the reference checkout"
    gen = [os.path.join(GEN, u + ".cpp") for u in UNITS]
    exe = os.path.join(OUT, "sanitize_driver_" + kind)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + kind, "-fno-sanitize-recover=all", "-ffp-contract=off", "-DGLM_FORCE_PURE", "-w",
           "-I", SHIM, "-I", HERE, "-I", os.path.join(root, "cuda_rasterizer"), "-I", os.path.join(root, "third_party", "glm"), "-o", exe,
           os.path.join(HERE, "sanitize_driver.cpp")] + gen + OWN
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    subprocess.check_call([exe], env=dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0"))


if __name__ == "__main__":
    import sys
    if sys.argv[1:2] == ["--sanitize"]:
        for kind in sys.argv[2:] or ["undefined", "address"]:
            sanitize(kind)
    else:
        print(build(force=True, verbose=True))
