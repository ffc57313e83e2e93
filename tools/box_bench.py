#!/usr/bin/env python
"""Per-launch cost of a strict round with Box(2) agents against the all-Discrete
round on the same general kernels.

Two shapes: simple_spread N=3 at 64 units (1,024 envs, B=1024) and simple_tag
N=6 at 128 units (4,096 envs, B=4096).  Two variants each: `discrete` (the
scenario's Discrete(5) spaces with MDP_GENERAL_GRADS=1, so that both run the
general kernels) and `box` (--continuous-actions: every agent Box(2)).  Each
variant runs in its own process, the variants alternate per repeat, and the
figures are medians over the repeats: HIP-event times of the critic, actor and
rollout launches' own packets in eager passes after warm-up.

    python tools/box_bench.py --out profiles/box_actions_launches.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "simple_spread N=3, 64 units": dict(scenario="simple_spread", num_envs=1024, batch_size=1024, num_units=64),
    "simple_tag N=6, 128 units": dict(scenario="simple_tag", num_envs=4096, n_agents=6, scenario_adversaries=4,
                                      num_adversaries=4, batch_size=4096, num_units=128),
}
VARIANTS = ("discrete", "box")
KINDS = ("critic_grad", "actor_grad", "rollout")


def worker(name, variant, rounds, warmup):
    import torch
    from maddpg_amd.runner import VecRunner
    if not torch.cuda.is_available():
        raise SystemExit("box_bench measures on the GPU only")
    kw = dict(CONFIGS[name])
    r = VecRunner(kw.pop("scenario"), kw.pop("num_envs"), seed=0, continuous=variant == "box", **kw)
    r.prefill()
    eng = r.eng
    for _ in range(warmup):
        eng.update_round()
        eng.env_step()
    eng.synchronize()
    out = {"variant": variant, "grad_variant": [int(eng.lib.mdp_grad_variant(eng.h, i)) for i in range(r.n)]}
    for kind in KINDS:
        eng.prof_enable(kind, True)
        for _ in range(rounds):
            if kind == "rollout":
                eng.env_step()
            else:
                eng.update_round()
        ms, n = eng.prof_read(kind)
        eng.prof_enable(kind, False)
        out[kind + "_us"] = round(ms / max(n, 1) * 1e3, 3)
        out[kind + "_launches"] = n
    eng.close()
    print("BOX_BENCH " + json.dumps(out), flush=True)


def run_variant(name, variant, args):
    env = dict(os.environ)
    env.pop("MDP_LIB", None)
    env["MDP_GENERAL_GRADS"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, variant, "--rounds", str(args.rounds),
           "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
    for line in p.stdout.splitlines():
        if line.startswith("BOX_BENCH "):
            return json.loads(line[len("BOX_BENCH "):])
    raise SystemExit(f"{name} {variant}: no result (rc {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per measuring process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=2, metavar=("CONFIG", "VARIANT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.rounds, args.warmup)
    res = {"timing": "HIP events on each launch's own packet, eager passes after warm-up; each variant in its own "
                     "process, variants alternated per repeat; medians over the repeats; both variants on the general "
                     "gradient kernels (MDP_GENERAL_GRADS=1)"}
    for name in CONFIGS:
        runs = {v: [] for v in VARIANTS}
        for _ in range(args.repeats):
            for v in VARIANTS:
                runs[v].append(run_variant(name, v, args))
                print(name, json.dumps(runs[v][-1]), flush=True)
        med = {v: {k + "_us": statistics.median(x[k + "_us"] for x in runs[v]) for k in KINDS} for v in VARIANTS}
        res[name] = {"config": CONFIGS[name], "runs": runs, "median": med,
                     "box_over_discrete": {k: round(med["box"][k + "_us"] / med["discrete"][k + "_us"], 3) for k in KINDS}}
        print(name, "box / discrete:", res[name]["box_over_discrete"], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
