#!/usr/bin/env python3
"""Per-kernel resources and instruction streams of two source trees, compared.

    python tools/kernel_isa_diff.py <parent tree> <branch tree> [--jobs N] [--keep DIR]

The check behind a structure-only change (a source split, a shared helper):
every kernel of libsmvs_hip.so must come out of the compiler as it did before.
For each tree every entry of smvs_amd/build.py's SOURCES is compiled with its
FLAGS plus --cuda-device-only -S.  From the assembly, per kernel:

  * the resources: VGPRs, AGPRs, total SGPRs, LDS bytes per workgroup, scratch
    bytes per lane, occupancy in waves per SIMD (the "; Kernel info:" block);
  * the instruction stream: the lines from the kernel's label to its end, the
    kernel descriptor included, comments dropped, basic-block labels renumbered
    per kernel (.LBB<function>_<block>: the function index changes when a kernel
    moves).  The file name and the __hip_cuid_<hash of the source> symbol sit
    outside every kernel and are not looked at.

Kernels are matched by name across files (a kernel may move between sources).
Prints the table of profiles/split_*_kernel_resources.txt with a verdict per
kernel: `same` (equal streams), `permuted` (equal resources, equally many
lines, and the same lines once the order of the lines and of the operands
inside a line does not count: what one more level of inlining does to an add's
operands), or `DIFFERENT`.  Exits non-zero if the kernel sets differ, or any
kernel's resources differ or its stream is DIFFERENT.  Nothing here looks for a
particular instruction: streams are only compared.

A tree is a checkout: `git worktree add ../parent HEAD~1`, or an export of a
commit (`git archive`).
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

MAX_JOBS = 16

_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$")
_FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
_BLOCK = re.compile(r"\.LBB\d+_\d+")
_INFO = {
    "vgpr": re.compile(r"^; NumVgprs: (\d+)"),
    "agpr": re.compile(r"^; NumAgprs: (\d+)"),
    "sgpr": re.compile(r"^; TotalNumSgprs: (\d+)"),
    "lds": re.compile(r"^; LDSByteSize: (\d+)"),
    "scratch": re.compile(r"^; ScratchSize: (\d+)"),
    "occ": re.compile(r"^; Occupancy: (\d+)"),
}
RESOURCES = ("vgpr", "agpr", "sgpr", "lds", "scratch", "occ")


def strip_comment(line):
    """An assembly line without its `; comment` and surrounding blanks, inner
    runs of blanks as one space.  (Quoted strings keep their semicolons.)"""
    out = []
    quoted = False
    for ch in line:
        if ch == '"':
            quoted = not quoted
        elif ch == ";" and not quoted:
            break
        out.append(ch)
    return " ".join("".join(out).split())


def normalise_stream(lines):
    """The instruction stream of ONE kernel (its lines from the label to the
    end): comments and empty lines dropped, blanks collapsed, the basic-block
    labels .LBB<f>_<b> renamed .LBB_0, .LBB_1 ... in the order they first
    appear.  Pure: text in, list of lines out."""
    names = {}

    def renumber(m):
        return names.setdefault(m.group(0), ".LBB_%d" % len(names))

    out = []
    for line in lines:
        line = strip_comment(line)
        if line:
            out.append(_BLOCK.sub(renumber, line))
    return out


def kernels_of(text):
    """Assembly of one translation unit -> {mangled kernel name: (resources,
    normalised stream)}, in the file's order.  `resources` maps RESOURCES to
    ints."""
    lines = text.splitlines()
    label_at = {}
    for i, line in enumerate(lines):
        if line and not line[0].isspace() and not line.startswith("."):
            m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
            if m:
                label_at.setdefault(m.group(1), i)
    found = {}
    for i, line in enumerate(lines):
        m = _KERNEL.match(line)
        if not m:
            continue
        name = m.group(1)
        if name not in label_at or label_at[name] > i:
            raise ValueError("kernel %s: no label before its descriptor" % name)
        end = i
        while end < len(lines) and not _FUNC_END.match(lines[end]):
            end += 1
        if end == len(lines):
            raise ValueError("kernel %s: no end of function" % name)
        stream = normalise_stream(lines[label_at[name]:end])
        res = {}
        j = end
        while j < len(lines) and not lines[j].startswith("; Kernel info:"):
            j += 1
        for line in lines[j:j + 40]:
            for key, rx in _INFO.items():
                mm = rx.match(line)
                if mm and key not in res:
                    res[key] = int(mm.group(1))
        if set(res) != set(RESOURCES):
            raise ValueError("kernel %s: incomplete kernel info" % name)
        found[name] = (res, stream)
    return found


def same_kernel(a, b):
    """(resources, stream) pairs of kernels_of() -> (same resources, same stream)"""
    return a[0] == b[0], a[1] == b[1]


def line_key(line):
    """A normalised line -> (mnemonic, sorted operand tokens): what is left of a
    line when the order of its operands does not count."""
    head, _, rest = line.partition(" ")
    return head, tuple(sorted(t.strip() for t in rest.split(",") if t.strip()))


def permuted_kernel(a, b):
    """(resources, stream) pairs of kernels_of() -> whether b is a's stream
    reordered: equal resources, equally many lines, and the same multiset of
    lines once each is reduced to line_key().  (An equal stream is one.)"""
    return a[0] == b[0] and len(a[1]) == len(b[1]) \
        and sorted(map(line_key, a[1])) == sorted(map(line_key, b[1]))


def verdict_of(a, b):
    """-> "same", "permuted" or "DIFFERENT" for the two kernels' streams, with
    " (resources differ)" behind it where they do"""
    same_res, same_stream = same_kernel(a, b)
    verdict = "same" if same_stream else ("permuted" if permuted_kernel(a, b) else "DIFFERENT")
    return verdict if same_res else verdict + " (resources differ)"


def load_build(tree):
    path = os.path.join(tree, "smvs_amd", "build.py")
    spec = importlib.util.spec_from_file_location("_isa_diff_build_%x" % abs(hash(path)), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_tree(tree, out_dir, jobs):
    """-> [(source stem, assembly text)] in the order of build.SOURCES"""
    build = load_build(tree)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(out_dir, exist_ok=True)

    def one(src):
        out = os.path.join(out_dir, src.replace(".hip", ".s"))
        cmd = [hipcc] + build.FLAGS + ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument",
                                       os.path.join(build.CSRC, src), "-o", out]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError("compiler failed: %s\n%s" % (" ".join(cmd), p.stdout))
        with open(out) as f:
            return src[:-len(".hip")], f.read()

    with ThreadPoolExecutor(max_workers=max(1, min(jobs, MAX_JOBS))) as pool:
        return list(pool.map(one, build.SOURCES))


def demangle(names):
    names = list(names)
    if not names:
        return {}
    tool = os.environ.get("CXXFILT", "/opt/rocm/llvm/bin/llvm-cxxfilt")
    if not os.path.exists(tool):
        tool = "c++filt"
    out = subprocess.run([tool] + names, stdout=subprocess.PIPE, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def short_name(demangled):
    """`void smvs_hip::k<4, true>(smvs_hip::Args)` -> `k<4, true>`"""
    s = demangled
    if s.startswith("void "):
        s = s[5:]
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            s = s[:i]
            break
    return s.replace("smvs_hip::", "")


def collect(units):
    """[(file, assembly)] -> {mangled name: (file, resources, stream)}; a name
    defined by two sources is an error (they are matched by name)"""
    table = {}
    for stem, text in units:
        for name, (res, stream) in kernels_of(text).items():
            if name in table:
                raise ValueError("kernel %s in both %s and %s" % (name, table[name][0], stem))
            table[name] = (stem, res, stream)
    return table


def report(parent, branch, out=None):
    """Prints the table; -> number of kernels that are missing on a side or differ"""
    out = out or sys.stdout
    names = demangle(set(parent) | set(branch))
    shown = {k: short_name(v) for k, v in names.items()}
    order = list(branch) + [k for k in parent if k not in branch]
    wf = max([12] + [len((branch.get(k) or parent[k])[0]) for k in order])
    wk = max([62] + [len(shown[k]) for k in order])
    head = "%7s%6s%6s%6s%8s%6s" % ("VGPR", "AGPR", "SGPR", "LDS", "scratch", "occ")
    print("kernels: parent %d, branch %d\n" % (len(parent), len(branch)), file=out)
    print("%-*s %-*s |%s |%s | instructions" % (wf, "file", wk, "kernel", head, head), file=out)
    bad = permuted = 0
    for k in order:
        cols = []
        for side in (parent, branch):
            cols.append("%7d%6d%6d%6d%8d%6d" % tuple(side[k][1][r] for r in RESOURCES)
                        if k in side else " " * len(head))
        if k in parent and k in branch:
            verdict = verdict_of(parent[k][1:], branch[k][1:])
            permuted += verdict == "permuted"
            bad += verdict not in ("same", "permuted")
        else:
            verdict = "only in the " + ("parent" if k in parent else "branch")
            bad += 1
        print("%-*s %-*s |%s |%s | %s" % (wf, (branch.get(k) or parent[k])[0], wk, shown[k],
                                             cols[0], cols[1], verdict), file=out)
    print("\n%d of %d kernels differ or are missing on one side, %d are permuted"
          % (bad, len(order), permuted), file=out)
    return bad


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent", help="source tree before the change")
    ap.add_argument("branch", help="source tree after it")
    ap.add_argument("--jobs", type=int, default=min(MAX_JOBS, os.cpu_count() or 1),
                    help="compilers at a time (at most %d)" % MAX_JOBS)
    ap.add_argument("--keep", metavar="DIR", help="leave the assembly in DIR/parent and DIR/branch")
    args = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        base = args.keep or tmp
        sides = [collect(compile_tree(os.path.abspath(t), os.path.join(base, side), args.jobs))
                 for side, t in (("parent", args.parent), ("branch", args.branch))]
    return 1 if report(sides[0], sides[1]) else 0


if __name__ == "__main__":
    sys.exit(main())
