#!/usr/bin/env python3
"""Does M3DDPG do better against opponents it was not trained with?  (No bar: a record.)

    python tools/minimax_purpose.py --out profiles/minimax.json

Per scenario and seed, MADDPG and --minimax (1e-3 / 1e-5) are trained from the same
seed for `--batches` lockstep batches of 1,024 episodes, then the two checkpoints
play the 2 x 2 cross-play table (Engine.cross_play, what --evaluate --tournament
prints): rows supply the adversaries, columns the good agents; set 0 is MADDPG,
set 1 is M3DDPG.  A side "does better against the unseen opponent" when its
M3DDPG actors score higher against the MADDPG run's opponents than its MADDPG
actors do against those same opponents (adversaries: cell [1][0] against [0][0];
good agents: [0][1] against [0][0]); `unseen` in the output names every cell.

simple_adversary (1 + 2) and simple_tag (3 + 1), every agent on MADDPG critics.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENARIOS = {"simple_adversary": 1, "simple_tag": 3}


def train(scenario, seed, batches, minimax):
    from maddpg_amd.runner import VecRunner
    r = VecRunner(scenario, 1024, seed=seed, episode_log_rows=4096, num_adversaries=SCENARIOS[scenario],
                  **(dict(minimax=True) if minimax else {}))
    curve = []
    for _ in range(batches):
        for _ in range(25):
            r.step()
        r.synchronize()
        n = r.episodes()
        curve.append(r.episode_rewards(n - 1024, 1024).mean(0).astype(float).tolist())
    return r, curve


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"batches_of_1024_episodes": args.batches, "eval_episodes": args.episodes, "adv_eps": 1e-3,
           "adv_eps_s": 1e-5, "sets": ["maddpg", "m3ddpg"],
           "table": "[row set: adversaries][column set: good agents] -> mean return of the side's agents +- s.e."}
    for scenario, na in SCENARIOS.items():
        res[scenario] = {}
        for seed in args.seeds:
            runs = [train(scenario, seed, args.batches, mm) for mm in (False, True)]
            eng = runs[0][0].eng
            bank = eng.actor_bank(2)
            for k, (r, _) in enumerate(runs):
                eng.bank_write(bank, k, r.eng.state_dict())
            team = list(range(na))
            ret = eng.cross_play(bank, team, args.episodes)["returns"].cpu().numpy().astype(np.float64)
            adv = ret[..., :na].mean(-1)
            good = ret[..., na:].mean(-1)
            cell = lambda x: [[[float(x[a, b].mean()), float(x[a, b].std() / np.sqrt(x.shape[-1]))]  # noqa: E731
                               for b in range(2)] for a in range(2)]
            A, G = adv.mean(-1), good.mean(-1)
            out = {"adversaries": cell(adv), "good": cell(good),
                   "curves": {"maddpg": runs[0][1], "m3ddpg": runs[1][1]},
                   "unseen": {
                       # against the opponents of the OTHER run
                       "m3ddpg_adversaries_vs_maddpg_good": float(A[1, 0]),
                       "maddpg_adversaries_vs_m3ddpg_good": float(A[0, 1]),
                       "m3ddpg_good_vs_maddpg_adversaries": float(G[0, 1]),
                       "maddpg_good_vs_m3ddpg_adversaries": float(G[1, 0]),
                       # the same actors against the opponents they trained with
                       "maddpg_adversaries_at_home": float(A[0, 0]), "m3ddpg_adversaries_at_home": float(A[1, 1]),
                       "maddpg_good_at_home": float(G[0, 0]), "m3ddpg_good_at_home": float(G[1, 1])}}
            res[scenario][f"seed_{seed}"] = out
            print(scenario, seed, json.dumps(out["unseen"]), flush=True)
            for r, _ in runs:
                r.eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
