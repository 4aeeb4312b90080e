#!/usr/bin/env python3
"""Instruction counts of a kernel's innermost loops, from the assembly hipcc produces with the library's own flags.  Runs on the CPU.

    python tools/hot_loop_isa.py render_bwd render_bwd_color_kernel
    python tools/hot_loop_isa.py render_fwd 'render_fwd_kernel<0, 4, 4>' --blocks

One translation unit of ibgs_amd/csrc is compiled to assembly (device side only) in a temporary directory with exactly the flags of
ibgs_amd/_build.py.  In the named kernel the loops of the control-flow graph are found (strongly connected components, and those inside them), and those that
hold no other loop are printed with their instruction
counts by class.  An instruction's class is decided by the first letters of its mnemonic and nothing else:

    v_...                                   vector ALU
    ds_...                                  LDS
    global_ / flat_ / buffer_ / scratch_ / s_load / s_buffer_load     memory
    s_cbranch / s_branch / s_endpgm / s_setpc / s_swappc              branch
    s_... (everything else: s_waitcnt and s_nop included)             scalar

The counts are STATIC: every instruction of every block of the loop, rare side paths included (--blocks lists the basic blocks, so that the common path can be added up by hand).  The figures in DESIGN.md section 3
and docs/EXPERIMENTS.md section 7 are this tool's.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ibgs_amd import _build  # noqa: E402

CLASSES = ("valu", "scalar", "lds", "memory", "branch")
MEMORY = ("global_", "flat_", "buffer_", "scratch_", "s_load", "s_buffer_load")
BRANCH = ("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")


def classify(mnemonic):
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(MEMORY):
        return "memory"
    if mnemonic.startswith(BRANCH):
        return "branch"
    if mnemonic.startswith("s_"):
        return "scalar"
    return None


def compile_to_asm(unit, outdir):
    src = os.path.join(_build.CSRC, unit + ".hip")
    out = os.path.join(outdir, unit + ".s")
    cmd = [_build._hipcc()] + _build.compile_flags(unit) + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return out


def _mini_demangle(n):
    """ibgs::name<integer template arguments> of an Itanium-mangled kernel name (bools print as 0 / 1); enough to tell the instantiations apart"""
    m = re.match(r"^_ZN4ibgs(\d+)", n)
    if not m:
        return n
    k = int(m.group(1))
    ident, rest = n[m.end():m.end() + k], n[m.end() + k:]
    t = re.match(r"^I((?:L[a-z]\d+E)+)E", rest)
    if not t:
        return ident
    return ident + "<" + ", ".join(re.findall(r"L[a-z](\d+)E", t.group(1))) + ">"


def demangle(names):
    import shutil
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if filt:
        try:
            out = subprocess.run([filt] + names, capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            pass
    return {n: _mini_demangle(n) for n in names}


def functions(asm_text):
    """{mangled name: [lines of its body]} for every function of the assembly file."""
    out, name, body = {}, None, []
    for line in asm_text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(line)
    return out


def parse(body):
    """-> basic blocks [(label, [(mnemonic, operands)])] in layout order; a block ends at a label or behind a branch"""
    blocks, cur, n = [], ("entry", []), 0
    for line in body:
        m = re.match(r"^(\.LBB[\w]+):", line)
        if m:
            if cur[1] or "+" not in cur[0]:
                blocks.append(cur)
            cur = (m.group(1), [])
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        if classify(parts[0]) is None:
            continue
        cur[1].append((parts[0], parts[1].strip() if len(parts) > 1 else ""))
        if classify(parts[0]) == "branch":
            blocks.append(cur)
            n += 1
            cur = ("%s+%d" % (cur[0].split("+")[0], n), [])
    if cur[1]:
        blocks.append(cur)
    return blocks


def _sccs(nodes, succ):
    """strongly connected components (Tarjan, iterative) of the graph restricted to `nodes`; only those that hold a cycle"""
    idx, low, on, stack, out, n = {}, {}, set(), [], [], [0]
    for root in sorted(nodes):
        if root in idx:
            continue
        work = [(root, iter(succ[root]))]
        idx[root] = low[root] = n[0]; n[0] += 1; stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in nodes:
                    continue
                if w not in idx:
                    idx[w] = low[w] = n[0]; n[0] += 1; stack.append(w); on.add(w)
                    work.append((w, iter(succ[w])))
                    break
                if w in on:
                    low[v] = min(low[v], idx[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == idx[v]:
                    comp = set()
                    while True:
                        w = stack.pop(); on.discard(w); comp.add(w)
                        if w == v:
                            break
                    if len(comp) > 1 or v in succ[v]:
                        out.append(comp)
    return out


def loops(blocks):
    """Innermost loops of the control-flow graph: {first block: set of block indices}.  A loop is a strongly connected component; its inner loops
    are the components that remain when the edges into its head (the block it is entered at) are taken away -- which also copes with the loops
    that the compiler enters in the middle."""
    index = {lab: i for i, (lab, _) in enumerate(blocks)}
    succ = [[] for _ in blocks]
    for i, (_, insts) in enumerate(blocks):
        last = insts[-1] if insts else ("", "")
        if last[0].startswith(("s_cbranch", "s_branch")) and last[1] in index:
            succ[i].append(index[last[1]])
        if not last[0].startswith(("s_branch", "s_endpgm", "s_setpc")) and i + 1 < len(blocks):
            succ[i].append(i + 1)
    found, all_succ = {}, succ

    def descend(comp, succ):
        entries = [t for i, ss in enumerate(all_succ) if i not in comp for t in ss if t in comp]
        h = min(entries) if entries else min(comp)
        inner_succ = [[t for t in ss if t != h] for ss in succ]
        inner = _sccs(comp, inner_succ)
        if not inner:
            found[h] = comp
        for c in inner:
            descend(c, inner_succ)
    for c in _sccs(set(range(len(blocks))), succ):
        descend(c, succ)
    return found


def count(insts):
    c = dict.fromkeys(CLASSES, 0)
    for mn, _ in insts:
        c[classify(mn)] += 1
    return c


def fmt(c):
    return "  ".join("%s %4d" % (k, c[k]) for k in CLASSES) + "   total %4d" % sum(c.values())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", help="translation unit of ibgs_amd/csrc without .hip, e.g. render_bwd")
    ap.add_argument("kernel", help="kernel name: the demangled name or its beginning, e.g. 'render_fwd_kernel<0, 4, 4>'")
    ap.add_argument("--blocks", action="store_true", help="list the basic blocks of every loop")
    ap.add_argument("--min", type=int, default=8, help="leave out loops of fewer instructions (default 8)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    a = ap.parse_args()
    if a.unit not in _build.SOURCES:
        ap.error("unknown unit %r" % a.unit)
    with tempfile.TemporaryDirectory() as tmp:
        text = open(a.asm or compile_to_asm(a.unit, tmp)).read()
    funcs = functions(text)
    names = demangle(sorted(funcs))
    want = a.kernel.replace(" ", "")
    def plain(n):          # "void ibgs::k<0, 4, 4>(ibgs::FwdParams)" -> "k<0,4,4>"
        d = names[n].split("(")[0].replace(" ", "")
        return re.sub(r"^void", "", d).replace("ibgs::", "")
    hits = [n for n in funcs if plain(n) == want or n == a.kernel]
    if not hits:
        hits = [n for n in funcs if want in plain(n)]
    if len(hits) != 1:
        sys.exit("kernel %r: %d matches\n  %s" % (a.kernel, len(hits), "\n  ".join(names[n] for n in (hits or sorted(funcs)))))
    blocks = parse(funcs[hits[0]])
    print("%s  (%s, %s)" % (names[hits[0]], a.unit + ".hip", " ".join(_build.compile_flags(a.unit))))
    print("whole kernel: " + fmt(count([x for _, b in blocks for x in b])))
    for h, body in sorted(loops(blocks).items()):
        insts = [x for i in sorted(body) for x in blocks[i][1]]
        if len(insts) < a.min:
            continue
        print("loop at %s (%d blocks): %s" % (blocks[h][0], len(body), fmt(count(insts))))
        if a.blocks:
            for i in sorted(body):
                print("    %-14s %s" % (blocks[i][0], fmt(count(blocks[i][1]))))


if __name__ == "__main__":
    main()
