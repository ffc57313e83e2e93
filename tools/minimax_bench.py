#!/usr/bin/env python3
"""What M3DDPG costs: the minimax gradient launches and the whole strict round.

    python tools/minimax_bench.py --out profiles/minimax_bench.json [--parent-lib OLD/libmaddpg_hip.so]

Per configuration three variants, each in a process of its own (the library and
MDP_GENERAL_GRADS are chosen when it loads / creates the handle), alternated
`--repeats` times so a drift of the shared machine shows as spread:

  parent_general  MADDPG on the general kernels (MDP_GENERAL_GRADS=1)
  parent_shipped  MADDPG as shipped (register kernels where they apply)
  minimax         M3DDPG, the authors' rates 1e-3 / 1e-5 (general kernels)

The parent variants load --parent-lib (a build of the commit before M3DDPG) when
given, else this build's library (its uniform kernels are the same instructions).

Numbers: `critic_grad_us` / `actor_grad_us` are the mean event-timed
MDP_K_CRITIC_GRAD / MDP_K_ACTOR_GRAD launch (HIP events on the launch's own
packet, an eager pass of its own); `round_us` is a host clock around `--rounds`
replayed update rounds with a device synchronise on both sides, after warm-up
rounds.  The replay is filled to the gate by the device rollout first.  The
minimax launch adds one critic backward-to-input and one partial critic forward
to the step: each should stay under twice the parent's general launch.

configs[3]: simple_adversary, the adversary on DDPG, 4,096 envs, B=1024, 64 units
            (the adversary's launches are the parent's own: the means are over all three agents).
configs[4]: simple_tag N=6 (4 adversaries), 4,096 envs, B=4096, 128 units.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "configs[3]": dict(scenario="simple_adversary", num_envs=4096, num_adversaries=1, adv_policy="ddpg",
                       batch_size=1024, num_units=64),
    "configs[4]": dict(scenario="simple_tag", num_envs=4096, n_agents=6, scenario_adversaries=4,
                       num_adversaries=4, batch_size=4096, num_units=128),
}
VARIANTS = ("parent_general", "parent_shipped", "minimax")
KEYS = ("round_us", "critic_grad_us", "actor_grad_us")


def worker(name, variant, rounds, warmup):
    import torch
    from maddpg_amd.runner import VecRunner
    if not torch.cuda.is_available():
        raise SystemExit("minimax_bench measures on the GPU only")
    kw = dict(CONFIGS[name])
    mm = dict(minimax=True) if variant == "minimax" else {}
    r = VecRunner(kw.pop("scenario"), kw.pop("num_envs"), seed=0, **kw, **mm)
    r.prefill()
    eng = r.eng
    for _ in range(warmup):
        eng.update_round()
    eng.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        eng.update_round()
    eng.synchronize()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"variant": variant, "rounds": rounds, "round_us": round(dt / rounds * 1e6, 2)}
    for kind in ("critic_grad", "actor_grad"):
        eng.prof_enable(kind, True)
        for _ in range(max(4, rounds // 8)):
            eng.update_round()
        ms, n = eng.prof_read(kind)
        eng.prof_enable(kind, False)
        out[kind + "_us"] = round(ms / max(n, 1) * 1e3, 3)
        out[kind + "_launches"] = n
    out["grad_variant"] = [int(eng.lib.mdp_grad_variant(eng.h, i)) for i in range(r.n)]
    eng.close()
    print("MINIMAX_BENCH " + json.dumps(out), flush=True)


def run_variant(name, variant, args):
    env = dict(os.environ)
    env.pop("MDP_GENERAL_GRADS", None)
    env.pop("MDP_LIB", None)
    if variant == "parent_general":
        env["MDP_GENERAL_GRADS"] = "1"
    if variant.startswith("parent_") and args.parent_lib:
        env["MDP_LIB"] = os.path.abspath(args.parent_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, variant, "--rounds", str(args.rounds),
           "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
    for line in p.stdout.splitlines():
        if line.startswith("MINIMAX_BENCH "):
            return json.loads(line[len("MINIMAX_BENCH "):])
    raise SystemExit(f"{name} {variant}: no result (rc {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per measuring process")
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    ap.add_argument("--parent-lib", default=None, help="libmaddpg_hip.so built from the commit before M3DDPG")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=2, metavar=("CONFIG", "VARIANT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.rounds, args.warmup)
    res = {"timing": "round_us: host clock around replayed update rounds, device synchronise on both sides, after "
                     "warm-up; *_grad_us: HIP events on the launch's own packet in separate eager passes; each "
                     "variant in its own process, variants alternated per repeat; medians over the repeats",
           "parent_lib": "a build of the parent commit" if args.parent_lib else "this build (uniform kernels)"}
    for name in args.configs:
        runs = {v: [] for v in VARIANTS}
        for _ in range(args.repeats):
            for v in VARIANTS:
                runs[v].append(run_variant(name, v, args))
                print(name, json.dumps(runs[v][-1]), flush=True)
        med = {v: {k: statistics.median(x[k] for x in runs[v]) for k in KEYS} for v in VARIANTS}
        pg, mm = med["parent_general"], med["minimax"]
        res[name] = {
            "config": CONFIGS[name], "runs": runs, "median": med,
            "mm_critic_launch_over_parent_general": round(mm["critic_grad_us"] / pg["critic_grad_us"], 3),
            "mm_actor_launch_over_parent_general": round(mm["actor_grad_us"] / pg["actor_grad_us"], 3),
            "mm_launches_under_two_parent_launches": bool(mm["critic_grad_us"] < 2 * pg["critic_grad_us"] and
                                                          mm["actor_grad_us"] < 2 * pg["actor_grad_us"]),
            "mm_round_over_parent_general_round": round(mm["round_us"] / pg["round_us"], 3),
            "mm_round_over_parent_shipped_round": round(mm["round_us"] / med["parent_shipped"]["round_us"], 3),
            "general_kernels_cost_us_per_round": round(pg["round_us"] - med["parent_shipped"]["round_us"], 2),
        }
        print(name, json.dumps({k: v for k, v in res[name].items() if k != "runs"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
