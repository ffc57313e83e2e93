"""mdp_variants.h's refusal() against the matrix the library had before it.

tests/native/variant_gate_check prints the pure function's verdict for every
cell of the variants x seams matrix; tests/golden/variant_matrix.json is what
tools/variant_matrix.py recorded, cell by cell on a GPU, from the commit whose
shim still spelled every refusal out by hand.  A call is refused after the
table exactly where it was before.  The table does not hold the refusals of a
call that merely came out of order (mdp_update_all before the mode is set, the
xGMI steps before mdp_dp_xgmi_open): those cells it must let through, and the
golden message must be that sequencing text (tools.variant_matrix.SEQUENCING).
"""
import json
import os
import shutil
import subprocess

import pytest

from tools import variant_matrix as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "native", "variant_gate_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "variant_matrix.json")


@pytest.fixture(scope="module")
def tables():
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        subprocess.run(["make", "-C", os.path.join(ROOT, "maddpg_amd", "csrc"), "variant-check"],
                       check=True, capture_output=True, timeout=300)
    if not os.path.exists(BIN):
        pytest.skip("variant_gate_check not built (no hipcc here)")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-2000:]
    with open(GOLDEN) as f:
        return json.loads(p.stdout), json.load(f)


def test_the_golden_matrix_is_whole(tables):
    got, want = tables
    assert list(want["cells"]) == [vm.key(s, c) for s, c in vm.cells()]
    assert len(want["cells"]) == 9 * 16 - 1
    assert set(want["cells"]) <= set(got)
    not_run = {k for k, v in want["cells"].items() if v["verdict"] == vm.BY_READING}
    assert not_run == {vm.key(s, c) for s, c in vm.NOT_EXECUTED}


def test_refused_exactly_where_the_shim_refused_before(tables):
    got, want = tables
    for state, call in vm.cells():
        k = vm.key(state, call)
        was, why = want["cells"][k]["verdict"] == "refused", got[k]
        if why is not None:
            assert was, (k, why)                       # nothing new is refused
        elif was:                                      # let through: then only its order had refused it
            assert call in vm.SEQUENCING and vm.SEQUENCING[call] in want["cells"][k]["message"], k


def test_every_refusal_names_its_entry_point_and_reason(tables):
    got, want = tables
    n = 0
    for state, call in vm.cells():
        why = got[vm.key(state, call)]
        if why is None:
            continue
        n += 1
        assert why.startswith(call + ": "), why
        for part in vm.expected_substrings(state, call):
            assert part in why, (state, call, part, why)
    assert n == 80
