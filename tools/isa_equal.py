#!/usr/bin/env python3
"""Are the device kernels of a revision and of the working tree the same?  CPU only.

    python tools/isa_equal.py <parent-rev> [--work DIR] [csrc/file.hip ...]

Compiles each .hip file (default: every file of rag4dyg_amd/csrc that differs from <parent-rev>, or all of them when a header
differs) with build.py's FLAGS plus `--offload-device-only -S`, once from a checkout of <parent-rev> and once from the working
tree, and compares the two assembly files kernel by kernel after
  - dropping lines that are only comments (and trailing comments),
  - dropping lines that name a __hip_cuid_ symbol (a hash of the source text),
  - dropping the function number from local labels (.LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end: it counts the functions in
    front of this one, so it shifts in every kernel behind one that was added or removed),
  - treating the two source operands of the scalar bitwise operations in COMMUTATIVE as unordered.
Everything else -- instructions, register / spill counts, LDS size, kernel descriptors, metadata -- must be equal.  Prints the
first differing lines per kernel; exit status 1 if anything differs.  `--work DIR` keeps the assembly there and reuses the
parent's from an earlier run.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rag4dyg_amd.build import FLAGS, HIPCC  # noqa: E402

CSRC = "rag4dyg_amd/csrc"
COMMUTATIVE = ("s_and_b64", "s_or_b64", "s_and_b32", "s_or_b32")
_LABEL = re.compile(r"\.LBB\d+_(\d+)")       # .LBB<function number>_<block>: the number shifts when a kernel in front is added or removed
_FUNC_END = re.compile(r"\.Lfunc_end\d+")
_COMM = re.compile(r"^(\s*(?:%s)\s+)([^,]+),\s*([^,]+),\s*([^,]+)$" % "|".join(COMMUTATIVE))


def normalise(text):
    out = []
    for ln in text.splitlines():
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip() or "__hip_cuid_" in ln:
            continue
        ln = _FUNC_END.sub(".Lfunc_end", _LABEL.sub(r".LBB_\1", ln))
        m = _COMM.match(ln)
        if m:
            a, b = sorted((m.group(3).strip(), m.group(4).strip()))
            ln = f"{m.group(1)}{m.group(2).strip()}, {a}, {b}"
        out.append(ln)
    return out


def sections(lines):
    """{label: lines}: the text before the first kernel, each kernel (from its .globl to the next), and the trailing metadata."""
    secs, name = {"<preamble>": []}, "<preamble>"
    for ln in lines:
        m = re.match(r"\s*\.globl\s+(\S+)", ln)
        if m:
            prev, name = secs[name], m.group(1)
            lead = []                             # the .section / .protected lines in front of a .globl belong to its kernel
            while prev and prev[-1].split()[0] in (".section", ".protected", ".weak", ".text"):
                lead.insert(0, prev.pop())
            secs.setdefault(name, []).extend(lead)
        elif ln.strip().startswith(".amdgpu_metadata"):
            name = "<metadata>"
        secs.setdefault(name, []).append(ln)
    return secs


def assemble(tree, rel, out):
    r = subprocess.run([HIPCC, *FLAGS, "--offload-device-only", "-S", os.path.join(tree, rel), "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc -S failed for {rel} in {tree}:\n{r.stderr}")


def main(argv):
    work = None
    if "--work" in argv:
        i = argv.index("--work")
        work = argv[i + 1]
        del argv[i:i + 2]
    if not argv:
        raise SystemExit(__doc__)
    rev = argv[0]
    files = [os.path.relpath(os.path.abspath(f), ROOT) for f in argv[1:]]      # given paths: against the current directory
    if not files:                                                              # the default list is relative to the repository root
        changed = subprocess.check_output(["git", "diff", "--name-only", rev, "--", CSRC, "include"], cwd=ROOT, text=True).split()
        untracked = subprocess.check_output(["git", "ls-files", "-o", "--exclude-standard", "--", CSRC], cwd=ROOT, text=True).split()
        every = sorted(f"{CSRC}/{f}" for f in os.listdir(os.path.join(ROOT, CSRC)) if f.endswith(".hip"))
        files = every if any(f.endswith(".h") for f in changed + untracked) else [f for f in every if f in changed]
    with tempfile.TemporaryDirectory() as td:
        work = work or td
        os.makedirs(os.path.join(work, "parent_tree"), exist_ok=True)
        sha = subprocess.check_output(["git", "rev-parse", rev], cwd=ROOT, text=True).strip()
        tree = os.path.join(work, "parent_tree", sha)
        if not os.path.isdir(tree):
            os.makedirs(tree)
            tar = subprocess.run(["git", "archive", sha, "--", CSRC, "include"], cwd=ROOT, capture_output=True, check=True).stdout
            subprocess.run(["tar", "-x", "-C", tree], input=tar, check=True)
        jobs = []
        for rel in files:
            base = os.path.basename(rel)[:-4]
            old, new = os.path.join(work, f"{base}.{sha[:12]}.s"), os.path.join(work, f"{base}.new.s")
            if not os.path.exists(old):
                jobs.append((tree, rel, old))
            jobs.append((ROOT, rel, new))
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            list(ex.map(lambda j: assemble(*j), jobs))
        bad = 0
        for rel in files:
            base = os.path.basename(rel)[:-4]
            old = sections(normalise(open(os.path.join(work, f"{base}.{sha[:12]}.s")).read()))
            new = sections(normalise(open(os.path.join(work, f"{base}.new.s")).read()))
            differing = 0
            for name in sorted(set(old) | set(new)):
                a, b = old.get(name), new.get(name)
                if a == b:
                    continue
                differing += 1
                if a is None or b is None:
                    print(f"{rel}: {name}: only in the {'new' if a is None else 'parent'} tree")
                    continue
                n = sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))
                print(f"{rel}: {name}: {n} differing lines ({len(a)} -> {len(b)} lines)")
                shown = 0
                for i, (x, y) in enumerate(zip(a, b)):
                    if x != y:
                        print(f"    line {i}: - {x.strip()}\n    line {i}: + {y.strip()}")
                        shown += 1
                        if shown == 3:
                            break
            kernels = len([k for k in old if not k.startswith("<")])
            print(f"{rel}: {'EQUAL' if not differing else 'DIFFERENT'} ({kernels} global symbols, {sum(map(len, old.values()))} normalised lines)")
            bad += differing
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
