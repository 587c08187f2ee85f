#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same?  (CPU only.)

The check for a refactor of csrc/colbert_mi355x.hip that must not change a
kernel: compile both trees to device-only assembly, each with its own
_build.FLAGS, and compare kernel by kernel after dropping what only spells
names: comments, .ident / .file, the __hip_cuid_* symbol, the mangled symbols
(replaced by their demangled base names, template arguments dropped) and the
function index in local labels.  Kernels are compared as a multiset of
(code + descriptor, metadata entry) per base name, so the order of
instantiation is free but every instantiation must have its twin.
    python tools/device_code_diff.py PARENT_TREE BRANCH_TREE [--work DIR] [--jobs N]
Exit status 0: the four builds are identical; 1: a difference (printed).
"""
import argparse
import collections
import concurrent.futures
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

PRODUCT = os.path.join("hybrid-rag-colbertv2_amd", "csrc", "colbert_mi355x.hip")
BUILDS = (("product", PRODUCT, []), ("product+stamps", PRODUCT, ["-DCBV2_LAB_STAMPS=1"]),
          ("scan_lab", os.path.join("tools", "scan_lab.hip"), []), ("topk_lab", os.path.join("tools", "topk_lab.hip"), []))


def compile_asm(tree, src, defs, out):
    """Device-only assembly of tree/src with the tree's own flags; reused if newer than every .hip / .h of the tree."""
    spec = importlib.util.spec_from_file_location("_build", os.path.join(tree, "hybrid-rag-colbertv2_amd", "_build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    deps = [os.path.join(tree, s) for _, s, _ in BUILDS] + [os.path.join(tree, "include", "colbert_mi355x.h")]
    if os.path.exists(out) and os.path.getmtime(out) > max(map(os.path.getmtime, deps)):
        return
    flags = [f for f in B.FLAGS if f not in ("-shared", "-pthread")]
    r = subprocess.run([B.HIPCC, *flags, *defs, "-S", "--offload-device-only", "-I", os.path.join(tree, "include"),
                        os.path.join(tree, src), "-o", out], stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"{os.path.join(tree, src)} {' '.join(defs)}: hipcc failed\n{r.stderr}")


def base_name(demangled):
    """'void (anonymous namespace)::k<1, 2>(int*)::smem' -> 'k::smem'."""
    out, depth = [], 0
    for ch in demangled.replace("(anonymous namespace)::", ""):
        depth += ch in "<("
        if depth == 0:
            out.append(ch)
        depth -= ch in ">)"
    return "".join(out).split()[-1]


def normalise(text):
    lines = []
    for ln in text.splitlines():
        ln = ln.split(";", 1)[0].rstrip()
        if ln and "__hip_cuid_" not in ln and not re.match(r"\s*\.(ident|file)\b", ln):
            lines.append(re.sub(r"\.L(BB|func_begin|func_end|JTI)\d+", r".L\1", ln))
    text = "\n".join(lines)
    syms = sorted(set(re.findall(r"_Z[A-Za-z0-9_$]+", text)), key=len, reverse=True)
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    table = {s: base_name(d) for s, d in zip(syms, names)}
    full = dict(zip(syms, names))
    spelled = [full.get(k, k) for k in re.findall(r"(?m)^\t\.amdhsa_kernel (\S+)$", text)]   # for the report only
    return re.sub(r"_Z[A-Za-z0-9_$]+", lambda m: table[m.group(0)], text), spelled


def split_kernels(text, spelled):
    """-> (kernel count, Counter of (base name, code, metadata entry), text outside kernels, {kernel: demangled names})."""
    code, meta = text.split("\t.amdgpu_metadata\n")
    parts = re.split(r"(?m)^(?=\t(?:\.section\t\.text\.\S+|\.text)\n\t\.(?:globl|weak|protected)\t)", code)
    head, entries, tail = re.split(r"(?m)^amdhsa\.kernels:\n|^(?=amdhsa\.target:)", meta)
    metas = collections.defaultdict(list)
    for e in re.split(r"(?m)^(?=  - )", entries)[1:]:
        name = re.search(r"(?m)^    \.name:\s+(\S+)$", e).group(1)
        metas[name].append(re.sub(r"(?m)^    \.(name|symbol):.*\n", "", e))
    kernels, outside, who = collections.Counter(), [parts[0], head, tail], collections.defaultdict(list)
    for p in parts[1:]:
        m = re.search(r"(?m)^\t\.amdhsa_kernel (\S+)$", p)
        if m:
            key = (m.group(1), p, metas[m.group(1)].pop(0))
            kernels[key] += 1
            who[key].append(spelled.pop(0))
        else:
            outside.append(p)
    assert not any(metas.values()), "metadata entries without a kernel"
    return sum(kernels.values()), kernels, "\n".join(outside), who


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--work", default=None, help="keep the assembly here (and reuse what is newer than its sources)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="device_code_diff_")
    os.makedirs(work, exist_ok=True)
    jobs = {(side, b[0]): (tree, b[1], b[2], os.path.join(work, f"{side}_{b[0]}.s"))
            for side, tree in (("parent", a.parent), ("branch", a.branch)) for b in BUILDS}
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        for f in [pool.submit(compile_asm, *j) for j in jobs.values()]:
            f.result()
    bad = 0
    for build, _, _ in BUILDS:
        (np_, kp, op, wp), (nb, kb, ob, wb) = (split_kernels(*normalise(open(jobs[(s, build)][3]).read()))
                                               for s in ("parent", "branch"))
        only_p, only_b = kp - kb, kb - kp
        same = not only_p and not only_b and op == ob and np_ == nb
        print(f"{build}: parent {np_} kernels, branch {nb} kernels: {'identical' if same else 'DIFFERENT'}")
        bad += not same
        if op != ob:
            print("  outside the kernels:")
            sys.stdout.writelines("    " + d + "\n" for d in list(difflib.unified_diff(op.split("\n"), ob.split("\n"), lineterm="", n=0))[:20])
        for name in sorted({k[0] for k in only_p} | {k[0] for k in only_b}):
            p = [k for k in only_p.elements() if k[0] == name]
            b = [k for k in only_b.elements() if k[0] == name]
            print(f"  {name}: {len(p)} instantiation(s) only in the parent, {len(b)} only in the branch")
            sys.stdout.writelines(f"    {side} {n}\n" for side, ks, w in (("-", p, wp), ("+", b, wb)) for k in dict.fromkeys(ks) for n in w[k])
            if p and b:
                d = difflib.unified_diff("\n".join(p[0][1:]).split("\n"), "\n".join(b[0][1:]).split("\n"), lineterm="", n=0)
                sys.stdout.writelines("    " + x + "\n" for x in list(d)[:12])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
