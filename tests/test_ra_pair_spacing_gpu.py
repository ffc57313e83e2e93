"""The norm handshake's tagged pairs on both sides of the size at which their
spacing changes (ra_pair_at, mdp_apply_fused.hip).

A tensor of at most MDP_RA_MAXCH / 4 = 64 chunks keeps its pairs 64 B apart in
its [MDP_RA_MAXCH][2] area, a larger one 16 B apart as before.  Observations of
50, 47 and 18 at H = 128 put one net on both sides at once: the MADDPG critics'
W1 is (115 + 15) x 128 = 16,640 parameters, 65 chunks -- the first size that
stays packed -- and their W2 128 x 128 = 16,384, 64 chunks -- the last size that
is spaced, whose last pair ends the tensor's area.  A publish and a poll that
disagreed about where a pair sits would time the handshake out (Ctl::fault = 1)
or step with another norm, so: no fault, one fused launch per net, and both
fused bodies bit for bit the step of k_reduce + k_apply, which has no handshake.
The small sizes (every S2 tensor: 1 to 18 chunks) are
tests/test_reduce_apply_lanes_gpu.py's cases.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from tests import optimizer_edges as oe  # noqa: E402
from tests.test_reduce_apply_lanes_gpu import PATHS, _case, _differing, _round  # noqa: E402

MAXCH = 256                        # MDP_RA_MAXCH (mdp_kernels.h)


def test_pairs_on_both_sides_of_the_spacing_threshold():
    B, H, dims = 64, 128, [50, 47, 18]
    c = _case("active", B, H, dims)
    runs = {path: _round(c, B, env, H, dims) for path, env in PATHS.items()}
    sizes = runs["lanes"][4][(0, 1)]                 # agent 0's critic: W1, b1, W2, b2, W3, b3
    chunks = [(n + oe.CHUNK - 1) // oe.CHUNK for n in sizes]
    print(f"agent 0 critic chunks per tensor: {chunks}")
    assert chunks[0] == MAXCH // 4 + 1 and chunks[2] == MAXCH // 4
    assert all(r[1] == 0 for r in runs.values())     # Ctl::fault
    assert runs["lanes"][2] == (6, 0, 0) and runs["lds"][2] == (6, 0, 0) and runs["unfused"][2] == (0, 6, 6)
    assert _differing(runs["lanes"][0], runs["lds"][0]) == {}
    assert _differing(runs["lanes"][0], runs["unfused"][0]) == {}
