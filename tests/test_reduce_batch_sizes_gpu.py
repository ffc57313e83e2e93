"""k_reduce (the unfused batch reduction: the data-parallel path and the
fallback when the fused optimizer grid is not co-resident) on crafted partial
gradients, at every batch size where its code takes another path.

nwg = ceil(B / 16) partial rows per net.  Lane q of an element's 8 lanes sums
partials w = q + 8 k: k < 8 (w < 64) behind guards, 8 <= k < 32 (64 <= w < 256,
the t[24] block) behind guards, then a tail loop for w >= 256
(mdp_kernels.hip k_reduce).  The partials are small integers, so every partial
sum is an integer below 2^24 in magnitude and fp32 addition is exact in any
order: the reduced gradient must equal the integer sum bit for bit, and a
dropped, duplicated or misplaced partial shows up exactly.  No tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from maddpg_amd import _lib  # noqa: E402
from maddpg_amd.engine import Engine  # noqa: E402

DIMS = [6, 5]
APRE_W, CPRE_W = 144, 212          # MDP_APRE_W, MDP_CPRE_W (mdp_kernels.h)
RA_MAXCH = 256                     # MDP_RA_MAXCH
SENTINEL = 12345.0                 # what the GRAD region holds where no reduction wrote

# below / at / above every boundary of the three partial ranges (64, 256), a
# single row, rows that fill the 8 lanes unevenly, and two tail-loop lengths
NWG = [1, 7, 8, 9, 63, 64, 65, 72, 200, 255, 256, 257, 264, 313]


def _partials(nwg, width):
    """v(w, e) = ((131 w + 7 e) % 17) - 8, as exact small integers"""
    w = np.arange(nwg, dtype=np.int64)[:, None]
    e = np.arange(width, dtype=np.int64)[None, :]
    return ((131 * w + 7 * e) % 17) - 8


def _slab_bytes(n, nwg, B, slab_c, slab_a, row_stride):
    """MDP_R_SLAB as mdp_api.cpp build_layout sizes it"""
    ra_sync = _lib.MAX_AGENTS * 2 * 8 * 128 + _lib.MAX_AGENTS * 2 * 6 * RA_MAXCH * 16   # mdp_ra_sync_bytes()
    return (n * (4 * nwg * (slab_c + slab_a) + 2 * 8 * 8 * nwg + 8 * B) + 256 + 256 + ra_sync
            + 4 * nwg * 16 * (APRE_W + CPRE_W + 2 * row_stride) + 512)


@pytest.mark.parametrize("nwg", NWG)
def test_reduce_is_the_exact_sum_of_the_partials(nwg):
    B = 16 * nwg if nwg == 1 else 16 * nwg - 5        # ragged on purpose: nwg = ceil(B / 16)
    assert (B + 15) // 16 == nwg
    eng = Engine(DIMS, batch_size=B, capacity=64)
    n = len(DIMS)
    size = {(i, net): eng.grad_view(i, net).numel() for i in range(n) for net in (0, 1)}
    # a net's tensors are contiguous and 4-padded: its size is its span in the GRAD region
    for (i, net), s in size.items():
        infos = eng.net_tensors(i, net)
        assert s == sum(((dr * dc + 3) // 4) * 4 for (_, _, _, dr, dc) in infos)
    slab_c = max(size[(i, 1)] for i in range(n))      # row strides: the widest net of each kind
    slab_a = max(size[(i, 0)] for i in range(n))
    assert size[(1, 0)] < slab_a                      # agent 1's actor is narrower than its slab row
    slab = eng.region("slab")
    assert slab.numel() * 4 == _slab_bytes(n, nwg, B, slab_c, slab_a, eng.row_stride), \
        "the SLAB region's layout changed: this test writes its rows by that layout"
    # critic slabs first, then actor slabs; n blocks of nwg rows each.  The strict
    # path reads block 0; the later blocks (throughput mode's) are poison here.
    rows_c = slab[:n * nwg * slab_c].view(n * nwg, slab_c)
    rows_a = slab[n * nwg * slab_c: n * nwg * (slab_c + slab_a)].view(n * nwg, slab_a)
    want = {}
    for rows, width, net in ((rows_c, slab_c, 1), (rows_a, slab_a, 0)):
        v = _partials(nwg, width)
        assert np.abs(v).sum(0).max() < 2 ** 24       # every partial sum is exact in fp32
        rows.fill_(float("nan"))
        rows[:nwg] = torch.from_numpy(v.astype(np.float32)).to(rows.device)
        want[net] = v.sum(0).astype(np.float32)
    grad = eng.region("grad")
    grad.fill_(SENTINEL)
    torch.cuda.synchronize()
    for i in range(n):
        for net in (1, 0):
            eng.reduce_grad(i, net)
    eng.synchronize()
    got = grad.cpu().numpy()
    written = np.zeros(got.shape, bool)
    for (i, net), s in size.items():
        off = eng.net_tensors(i, net)[0][0]
        g = got[off:off + s]
        assert g.tobytes() == want[net][:s].tobytes(), \
            (nwg, i, net, np.flatnonzero(g != want[net][:s])[:8], g[g != want[net][:s]][:8])
        written[off:off + s] = True
    assert (got[~written] == SENTINEL).all()          # nothing outside the four nets' spans
    assert written.sum() == eng.param_floats
