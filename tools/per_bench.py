#!/usr/bin/env python3
"""What prioritized replay costs: env-steps/s and trainer-updates/s with PER off
and on, timed the way bench.py times its loop (replay prefilled to the gate,
warm-up steps, device sync on both sides of the timed steps, step graphs
replayed), plus the event times of the three PER kernels (mdp_prof_enable; that
pass runs eagerly, outside the timed loop).

    python tools/per_bench.py --out profiles/per_bench.json

configs[1]: simple_spread N=3, 1,024 envs, B=1024, 64 units.
configs[4]: simple_tag N=6 (4 adversaries), 4,096 envs, B=4096, 128 units.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "configs[1]": dict(scenario="simple_spread", num_envs=1024, batch_size=1024, num_units=64),
    "configs[4]": dict(scenario="simple_tag", num_envs=4096, n_agents=6, scenario_adversaries=4,
                       num_adversaries=4, batch_size=4096, num_units=128),
}


def measure(cfg, prioritized, steps, warmup):
    import torch
    from maddpg_amd.runner import VecRunner
    kw = dict(cfg)
    r = VecRunner(kw.pop("scenario"), kw.pop("num_envs"), seed=0, prioritized=prioritized, **kw)
    r.prefill()
    for _ in range(warmup):
        r.step()
    r.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rounds = 0
    for _ in range(steps):
        rounds += r.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    r.synchronize()
    out = {"prioritized": prioritized, "steps": steps, "update_rounds": rounds,
           "ms_per_step": round(dt / steps * 1e3, 4),
           "env_steps_per_sec": round(steps * r.num_envs / dt, 1),
           "trainer_updates_per_sec": round(rounds * r.n / dt, 1)}
    if prioritized:
        kinds = ("per_sync", "per_sample", "per_update")
        for k in kinds:
            r.eng.prof_enable(k, True)
        for _ in range(max(3, steps // 4)):
            r.step()
        out["kernels_us_per_launch"] = {}
        for k in kinds:
            ms, n = r.eng.prof_read(k)
            out["kernels_us_per_launch"][k] = {"launches": n, "mean_us": round(ms / max(n, 1) * 1e3, 3)}
            r.eng.prof_enable(k, False)
        out["per_info_agent0"] = {k: float(v) for k, v in r.eng.per_info(0).items()}
    r.eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"timing": "as bench.py: prefilled replay, warm-up, torch.cuda.synchronize() on both sides of the timed "
                     "steps, one graph replay per step; kernel times from HIP events on the launches' own packets "
                     "in a separate eager pass"}
    for name in args.configs:
        off = measure(CONFIGS[name], False, args.steps, args.warmup)
        on = measure(CONFIGS[name], True, args.steps, args.warmup)
        res[name] = {"config": CONFIGS[name], "uniform": off, "prioritized": on,
                     "per_cost_ms_per_step": round(on["ms_per_step"] - off["ms_per_step"], 4),
                     "per_cost_us_per_round": round((on["ms_per_step"] - off["ms_per_step"]) * 1e3 /
                                                    max(on["update_rounds"] / on["steps"], 1e-9), 2)}
        print(name, json.dumps(res[name]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
