#!/usr/bin/env python3
"""Does MADDPG with inferred policies learn as MADDPG does?  (A record, and the
learning test's fixture.)

    python tools/approx_learning.py --out profiles/approx.json --golden tests/golden/approx_learning.json

Per scenario and seed, MADDPG and --approx-policies (lambda 1e-3) are trained
from the same seed for `--batches` lockstep batches of 1,024 episodes.  Kept per
run: the curve of every agent's mean episode reward, and for the approx run the
final cross-entropy of every pair on fresh replay rows, the cross-entropy of
the true policies on the same rows, and the mean KL(policy || approximator).
The golden file is the simple_spread run of the first seed.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENARIOS = {"simple_spread": 0, "simple_adversary": 1}


def train(scenario, seed, batches, approx):
    from maddpg_amd.runner import VecRunner
    t0 = time.perf_counter()
    r = VecRunner(scenario, 1024, seed=seed, episode_log_rows=4096, num_adversaries=SCENARIOS[scenario],
                  **(dict(approx=True) if approx else {}))
    curve = []
    for _ in range(batches):
        for _ in range(25):
            r.step()
        r.synchronize()
        n = r.episodes()
        curve.append(r.episode_rewards(n - 1024, 1024).mean(0).astype(float).tolist())
    return r, curve, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, default=18)
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--scenarios", nargs="*", default=list(SCENARIOS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--golden", default=None)
    args = ap.parse_args()
    res = {"batches_of_1024_episodes": args.batches, "approx_lambda": 1e-3,
           "curve": "[batch][total, agent 0, ...] mean episode reward of the batch's 1,024 episodes"}
    for scenario in args.scenarios:
        res[scenario] = {}
        for seed in args.seeds:
            _, base, tb = train(scenario, seed, args.batches, False)
            r, curve, ta = train(scenario, seed, args.batches, True)
            q = r.eng.approx_quality()
            rec = {"maddpg": base, "approx": curve, "seconds": {"maddpg": round(tb, 2), "approx": round(ta, 2)},
                   "final_last4_total": {"maddpg": sum(b[0] for b in base[-4:]) / 4,
                                         "approx": sum(c[0] for c in curve[-4:]) / 4},
                   "pairs": {f"{i},{j}": v for (i, j), v in q["pairs"].items()},
                   "mean_ce": q["mean_ce"], "mean_ce_true": q["mean_ce_true"], "mean_kl": q["mean_kl"]}
            res[scenario][f"seed{seed}"] = rec
            print(scenario, seed, json.dumps({k: rec[k] for k in ("seconds", "final_last4_total", "mean_ce",
                                                                  "mean_ce_true", "mean_kl")}), flush=True)
            if args.golden and scenario == "simple_spread" and seed == args.seeds[0]:
                g = {"scenario": scenario, "seed": seed, "batches": args.batches, "num_envs": 1024,
                     "r0": base[0][0], "r1": sum(b[0] for b in base[-4:]) / 4,
                     "maddpg_mean_episode_reward": [b[0] for b in base],
                     "approx_mean_episode_reward": [c[0] for c in curve],
                     "approx_final": sum(c[0] for c in curve[-4:]) / 4,
                     "approx_pairs": rec["pairs"]}
                os.makedirs(os.path.dirname(os.path.abspath(args.golden)), exist_ok=True)
                with open(args.golden, "w") as f:
                    json.dump(g, f, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
