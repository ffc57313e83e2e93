"""The launches' dynamic-LDS sizes against the formulas they replaced.

Every lds_*_bytes function of maddpg_amd/csrc/mdp_kernels.h sums the buffer
list its kernel carves (mdp_carve.h).  tests/native/lds_carve_check prints all of
them over a grid of topologies -- 1..8 agents, the three kernel widths, narrow,
odd, mixed and LDS-envelope-edge observation widths, local_q off / on / agent 0
only, every critic group size -- and tests/golden/lds_sizes.json holds what the
hand-written closed forms before the lists returned on the same grid (the
program compiled against that mdp_kernels.h).  Every value must be equal, but
lds_critic_pre_bytes: the old formula counted 5632 bytes critic_pre_tile never
takes, and the launch's max(lds_actor_r_bytes, lds_critic_pre_bytes) must not
notice.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "native", "lds_carve_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lds_sizes.json")


@pytest.fixture(scope="module")
def sizes():
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        subprocess.run(["make", "-C", os.path.join(ROOT, "maddpg_amd", "csrc"), "lds-check"],
                       check=True, capture_output=True, timeout=300)
    if not os.path.exists(BIN):
        pytest.skip("lds_carve_check not built (no hipcc here)")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-2000:]
    with open(GOLDEN) as f:
        return json.loads(p.stdout), json.load(f)


def test_grid_is_the_golden_grid(sizes):
    got, want = sizes
    key = lambda r: (r["obs"], r["H"], r["local_q"])
    assert [key(r) for r in got] == [key(r) for r in want]
    assert len(want) == 441
    assert all(len(r["critic"]) == len(r["obs"]) for r in got)  # G = 1..n


def test_sizes_equal_the_replaced_formulas(sizes):
    got, want = sizes
    for g, w in zip(got, want):
        assert g.keys() == w.keys()
        for k in w:
            if k != "critic_pre":
                assert g[k] == w[k], (k, w["obs"], w["H"], w["local_q"])


def test_critic_pre_is_exact_and_the_launch_size_unchanged(sizes):
    got, want = sizes
    for g, w in zip(got, want):
        assert g["critic_pre"] == w["critic_pre"] - 5632, (w["obs"], w["H"], w["local_q"])
        assert max(g["actor_r"], g["critic_pre"]) == max(w["actor_r"], w["critic_pre"])
