"""GPU: `simple_spread` with tanh-squashed Box(2) actions and an entropy
coefficient stays finite and learns.

The run and the criterion are tests/test_box_squash_learning_gpu.py's: 1,024 env
copies, 12 lockstep batches of 1,024 episodes, seeds 0 and 1; after every batch
every episode reward and every parameter is finite, and the mean of the last 4
batches lies above the mean of the first 2 by more than 2 standard errors of the
difference.  No reward level and no entropy level is asserted: nobody has
measured one.  ALPHA is the first of 0.2, 0.05, 1.0 that met the criterion on
both seeds on MI355X; DESIGN.md section 29 and profiles/box_entropy.json have the
curves of every value tried, with the mean of -log pi and of logstd per batch
beside the alpha = 0 run of the same seed.
"""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from tests.test_box_squash_learning_gpu import BATCHES, E, T, criterion  # noqa: E402

ALPHA = 0.2


def mean_logstd(r):
    """the mean logstd head entry of every agent's actor on the observations of the first E
    replay rows (the same inputs after every batch)"""
    eng = r.eng
    rows = eng.replay_rows(0, E)
    out = []
    for j in range(eng.n):
        obs_off = eng.row_layout[j][0]
        obs = rows[:, obs_off:obs_off + eng.obs_dims[j]].contiguous()
        flat = eng.actor_logits(j, obs).cpu().numpy()
        out.append(float(flat[:, 2:4].mean()))
    return out


def train(seed, alpha, batches=BATCHES):
    """per batch of E episodes: the team rewards, the per-agent mean of -log pi of the last
    actor step (None without a coefficient) and the per-agent mean logstd"""
    from maddpg_amd.runner import VecRunner
    r = VecRunner("simple_spread", E, seed=seed, episode_log_rows=4 * E, max_episode_len=T, continuous=True,
                  squash="tanh", entropy_alpha=alpha)
    rows, ent, lsd = [], [], []
    for _ in range(batches):
        for _ in range(T):
            r.step()
        r.synchronize()
        rew = r.episode_rewards(r.episodes() - E, E)
        assert np.all(np.isfinite(rew))
        assert r.eng.check_finite() == 0
        rows.append(rew[:, 0].astype(np.float64))
        ent.append([-r.eng.entropy_info(i)["logp"] for i in range(r.n)] if alpha else None)
        lsd.append(mean_logstd(r))
    return r, np.stack(rows), ent, lsd


@pytest.mark.parametrize("seed", [0, 1])
def test_simple_spread_with_an_entropy_coefficient_is_finite_and_learns(seed):
    r, rew, ent, lsd = train(seed, ALPHA)
    assert r.eng.act_kinds == ["box"] * 3 and r.eng.act_squash == ["tanh"] * 3 and r.rounds > 0
    assert r.eng.act_entropy == [float(np.float32(ALPHA))] * 3
    first, last, se = criterion(rew)
    print(f"simple_spread tanh Box(2) alpha {ALPHA} seed {seed}: curve {[round(float(x), 3) for x in rew.mean(1)]}; "
          f"first window {first:.3f}, last window {last:.3f}, s.e. of the difference {se:.4f}")
    print(f"  mean -log pi per batch (agent 0) {[round(e[0], 3) for e in ent]}")
    print(f"  mean logstd per batch (agent 0) {[round(x[0], 3) for x in lsd]}")
    assert np.all(np.isfinite(ent)) and np.all(np.isfinite(lsd))
    assert r.eng.check_finite() == 0
    assert last - first > 2.0 * se, rew.mean(1).tolist()


if __name__ == "__main__":           # python -m tests.test_box_entropy_learning_gpu OUT.json ALPHA...: the record
    res = {}
    for alpha in [float(a) for a in sys.argv[2:]]:
        for seed in (0, 1):
            _r, rew, ent, lsd = train(seed, alpha)
            first, last, se = criterion(rew)
            res[f"alpha_{alpha:g}_seed_{seed}"] = {
                "alpha": alpha, "seed": seed, "reward": [float(x) for x in rew.mean(1)], "neg_logp": ent,
                "logstd": lsd, "first": first, "last": last, "se": se, "standard_errors": (last - first) / se,
                "met": bool(last - first > 2.0 * se)}
            print(json.dumps({k: res[f"alpha_{alpha:g}_seed_{seed}"][k] for k in ("alpha", "seed", "first", "last",
                                                                                 "standard_errors", "met")}), flush=True)
            with open(sys.argv[1], "w") as fp:
                json.dump(res, fp, indent=1)
