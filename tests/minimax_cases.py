"""Fixtures shared by tests/test_minimax_oracle.py (CPU) and tests/test_minimax_gpu.py.

Trainer-only cases on injected indices and uniforms, ring L = 200.  Shapes: the
smallest that reach every path of the minimax kernels -- B = 40 is two full
16-row tiles and a ragged one, tag N = 6 at H = 128 is the tightest LDS carve
and three 16-column tiles of action gradients, act_dims [3, 5] has pad entries,
the adversary case has a DDPG agent beside MADDPG ones, H = 256 takes the
actor kernel's serial critic layer 1.
"""
import copy

import numpy as np

from maddpg_amd.envs import minimax_eps, spec
from oracle import trainer
from tests import minimax_oracle as mo
from tests import mixed_width
from tests.helpers import synthetic_trainer_case

L = 200
NETS4 = ("actor", "critic", "tgt_actor", "tgt_critic")
CASES = {
    "spread": dict(dims=spec("simple_spread").obs_dims, H=64, B=40, n_adv=0),
    "tag": dict(dims=spec("simple_tag", 6).obs_dims, H=128, B=32, n_adv=3),
    "speaker_listener": dict(dims=spec("simple_speaker_listener").obs_dims, H=64, B=24, n_adv=0, widths=[3, 5]),
    "adversary": dict(dims=spec("simple_adversary").obs_dims, H=64, B=40, n_adv=1, local_q=[True, False, False]),
    "spread_wide": dict(dims=spec("simple_spread").obs_dims, H=256, B=16, n_adv=0),
}
EPS = ("authors", "large")   # 1e-3 across the sides / 1e-5 within one; 0.3 for every pair
SEED = 31


def eps_matrix(name, kind):
    n = len(CASES[name]["dims"])
    if kind == "authors":
        return minimax_eps(n, CASES[name]["n_adv"], 1e-3, 1e-5)
    if kind == "zero":
        return np.zeros((n, n), np.float32)
    return minimax_eps(n, 0, 0.3, 0.3)


def make_case(name, kind, seed=SEED, spec=None, prepare=None):
    """the case's replay, weights and noise with ReLU-margin-clean rows for eps `kind`.
    spec: a shape outside CASES (same keys); kind may be an n x n matrix; prepare(c)
    puts a constructed state into the weights / replay before the rows are cleaned
    (tests/minimax_edges.py)"""
    kw = CASES[name] if spec is None else spec
    dims, H, B = kw["dims"], kw["H"], kw["B"]
    widths = kw.get("widths")
    if widths is None:
        c = synthetic_trainer_case(dims, B, L, seed, kw.get("local_q"), H)
        c["widths"] = [5] * len(dims)
    else:
        c = mixed_width.mixed_case(dims, widths, B, L, seed, kw.get("local_q"), H)
    c["spec"] = kw
    c["eps"] = eps_matrix(name, kind) if isinstance(kind, str) else np.asarray(kind, np.float32)
    if prepare is not None:
        prepare(c)
    c["replaced"] = mo.clean_idx(c, c["widths"], c["eps"])
    return c


def oracle_agents(c):
    return [trainer.AgentParams(**copy.deepcopy(p), local_q=c["local_q"][j], lr=c.get("lr", 1e-2))
            for j, p in enumerate(c["params"])]


def batches(c, i, idx=None):
    idx = c["idx"][i] if idx is None else idx
    return [tuple(x[idx] for x in c["data"][j]) for j in range(len(c["params"]))]


def oracle_update(ags, c, i, sign=1):
    return mo.update_batch(ags, i, batches(c, i), mixed_width.narrow(c["u_tgt"][i], c["widths"]), c["u_act"][i],
                           c["eps"][i], sign=sign)
