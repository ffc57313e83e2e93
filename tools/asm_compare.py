#!/usr/bin/env python
"""Do the kernels a commit leaves alone still compile to the same instructions, in the
same place?  (DESIGN.md sections 26 and 29.)

Compiles one translation unit of maddpg_amd/csrc from two trees to gfx950 assembly and
compares them kernel by kernel: the instructions with their operands, local label
numbers normalised, and the order in which the kernels are emitted.  Every kernel of
the first tree must be found unchanged in the second, and the first tree's order must
be a prefix of the second's, so that new kernels lie behind the old ones in the code
object (a kernel that is no template is emitted ahead of every template instantiation,
which moves them all).  Exit status 0 if both hold.

    git worktree add /tmp/parent HEAD~1
    python tools/asm_compare.py /tmp/parent . mdp_grads.hip
"""
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "-O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 --offload-device-only -S".split()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def assembly(tree, unit, out):
    subprocess.run([HIPCC, *FLAGS, unit, "-o", out], check=True, cwd=os.path.join(tree, "maddpg_amd", "csrc"))
    return out


def kernels(path):
    """{name: [instruction lines]} in emission order (dicts keep it)"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        ln = re.sub(r";.*$", "", line).strip()
        if not ln or ln.startswith("."):
            continue
        ln = re.sub(r"\.LBB\d+_", "LBB_", ln)
        ln = re.sub(r"\.L__unnamed_\d+|\.Ltmp\d+|\.LJTI\d+_", "L_", ln)
        out[cur].append(ln)
    return out


def main():
    if len(sys.argv) != 4:
        raise SystemExit(__doc__)
    old_tree, new_tree, unit = sys.argv[1:]
    with tempfile.TemporaryDirectory() as d:
        a = kernels(assembly(os.path.abspath(old_tree), unit, os.path.join(d, "old.s")))
        b = kernels(assembly(os.path.abspath(new_tree), unit, os.path.join(d, "new.s")))
    bad = 0
    for name, code in a.items():
        if name not in b:
            print("missing in the second tree:", name)
            bad += 1
        elif b[name] != code:
            print("differs:", name, len(code), len(b[name]))
            bad += 1
    prefix = list(b)[:len(a)] == list(a)
    print(f"{unit}: {len(a)} kernels in the first tree, {len(a) - bad} unchanged in the second, "
          f"{len(set(b) - set(a))} new; the first tree's order is {'' if prefix else 'NOT '}a prefix of the second's")
    for name in b:
        if name not in a:
            print("new:", name, len(b[name]), "instructions")
    return 0 if bad == 0 and prefix else 1


if __name__ == "__main__":
    sys.exit(main())
