"""The variants x seams matrix replayed on the built library.

tests/golden/variant_matrix.json holds, per handle state and call, whether the
library refused before its refusals moved into mdp_variants.h's table
(tools/variant_matrix.py recorded it there; the cells that would wait for
data-parallel peers were read, not run, and are not run here).  The library
refuses exactly the same cells, every refusal names its entry point and keeps
the words callers match, and a handle that was refused its whole row trains on
bit for bit like a twin that was asked nothing.
"""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from tools import variant_matrix as vm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "variant_matrix.json")) as _f:
    GOLDEN = json.load(_f)["cells"]


def _table_refusal(call, msg):
    """the message is the variant table's, not the text of a call that came out of order"""
    return not (call in vm.SEQUENCING and vm.SEQUENCING[call] in msg)


def test_executed_cells_are_refused_and_accepted_as_before():
    ran = 0
    for state, call in vm.cells():
        if (state, call) in vm.NOT_EXECUTED:
            continue
        ran += 1
        refused, msg = vm.run_cell(state, call)
        assert refused == (GOLDEN[vm.key(state, call)]["verdict"] == "refused"), (state, call, msg)
        if refused and _table_refusal(call, msg):
            assert msg.startswith(call + ": "), msg
            for part in vm.expected_substrings(state, call):
                assert part in msg, (state, call, part, msg)
    assert ran == len(GOLDEN) - len(vm.NOT_EXECUTED)


@pytest.mark.parametrize("state", vm.STATES)
def test_a_handle_refused_its_whole_row_trains_like_its_twin(state):
    eng, twin = vm.make_state(state), vm.make_state(state)
    ask = vm.Caller(eng)
    asked = 0
    for call in vm.CALLS:
        if GOLDEN.get(vm.key(state, call), {}).get("verdict") == "refused":
            refused, msg = ask(call)
            assert refused, (state, call)
            asked += 1
    assert asked >= 4                                   # (a plain handle: the four calls that came out of order)
    for r in range(3):
        vm.update(eng, r)
        vm.update(twin, r)
    a, b = vm.state_bits(eng), vm.state_bits(twin)
    assert a.keys() == b.keys()
    assert [k for k in a if a[k] != b[k]] == []
    assert eng.check_finite() == 0
