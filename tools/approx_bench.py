#!/usr/bin/env python3
"""What MADDPG with inferred policies costs: its critic instantiation, the
approximator gradient launch and the whole strict round.

    python tools/approx_bench.py --out profiles/approx_bench.json [--parent-lib OLD/libmaddpg_hip.so]

Per configuration four variants, each in a process of its own (the library and
MDP_GENERAL_GRADS are chosen when it loads / creates the handle), alternated
`--repeats` times so a drift of the shared machine shows as spread:

  parent_general  MADDPG on the general kernels (MDP_GENERAL_GRADS=1), --parent-lib
  parent_shipped  MADDPG as shipped (register kernels where they apply), --parent-lib
  this_general    this build's uniform general kernels (MDP_GENERAL_GRADS=1), no option
  approx          --approx-policies (general kernels)

The parent variants load --parent-lib (a build of the commit before this
feature) when given, else this build's library.

Numbers: `critic_grad_us` / `actor_grad_us` are the mean event-timed
MDP_K_CRITIC_GRAD / MDP_K_ACTOR_GRAD launch (HIP events on the launch's own
packet, an eager pass of its own; not reported for actor_grad under approx,
where that kind also counts the approximator launches); `approx_grad_us` is the
median over `--calls` calls of a device event pair around mdp_approx_grad (all
m pairs of observer 0 in one launch; the pair of events adds its own few us);
`round_us` is a host clock around `--rounds` replayed update rounds with a
device synchronise on both sides, after warm-up rounds.  The replay is filled
to the gate by the device rollout first.  The approximator launch is m actor
steps without their critic half: it should take less than m of the parent's
general actor launches.

configs[1]: simple_spread N=3, 4,096 envs, B=1024, 64 units.
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
    "configs[1]": dict(scenario="simple_spread", num_envs=4096, batch_size=1024, num_units=64),
    "configs[4]": dict(scenario="simple_tag", num_envs=4096, n_agents=6, scenario_adversaries=4,
                       num_adversaries=4, batch_size=4096, num_units=128),
}
VARIANTS = ("parent_general", "parent_shipped", "this_general", "approx")
TAG = "APPROX_BENCH "


def worker(name, variant, rounds, warmup, calls):
    import torch
    from maddpg_amd.runner import VecRunner
    if not torch.cuda.is_available():
        raise SystemExit("approx_bench measures on the GPU only")
    kw = dict(CONFIGS[name])
    opt = dict(approx=True) if variant == "approx" else {}
    r = VecRunner(kw.pop("scenario"), kw.pop("num_envs"), seed=0, **kw, **opt)
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
    for kind in ("critic_grad",) + (() if variant == "approx" else ("actor_grad",)):
        eng.prof_enable(kind, True)
        for _ in range(max(4, rounds // 8)):
            eng.update_round()
        ms, n = eng.prof_read(kind)
        eng.prof_enable(kind, False)
        out[kind + "_us"] = round(ms / max(n, 1) * 1e3, 3)
        out[kind + "_launches"] = n
    if variant == "approx":
        idx = eng.make_index(eng.batch_size)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for _ in range(8):
            eng.approx_grad(0, idx)
        eng.synchronize()
        for a, b in ev:
            a.record(eng.stream)
            eng._c("mdp_approx_grad", 0, eng._ptr(idx))
            b.record(eng.stream)
        eng.synchronize()
        torch.cuda.synchronize()
        out["approx_grad_us"] = round(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, 3)
        out["pairs_per_launch"] = r.n - 1
        out["approx_buffer_bytes"] = int(eng.approx_buf.numel())
        slab = max(sum(dr * dc for (_o, _r, _c, dr, dc) in eng.net_tensors(j, 0)) for j in range(r.n))
        out["approx_slab_bytes_about"] = 4 * (r.n - 1) * ((eng.batch_size + 15) // 16) * slab
    out["grad_variant"] = [int(eng.lib.mdp_grad_variant(eng.h, i)) for i in range(r.n)]
    eng.close()
    print(TAG + json.dumps(out), flush=True)


def run_variant(name, variant, args):
    env = dict(os.environ)
    env.pop("MDP_GENERAL_GRADS", None)
    env.pop("MDP_LIB", None)
    if variant in ("parent_general", "this_general"):
        env["MDP_GENERAL_GRADS"] = "1"
    if variant.startswith("parent_") and args.parent_lib:
        env["MDP_LIB"] = os.path.abspath(args.parent_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, variant, "--rounds", str(args.rounds),
           "--warmup", str(args.warmup), "--calls", str(args.calls)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
    for line in p.stdout.splitlines():
        if line.startswith(TAG):
            return json.loads(line[len(TAG):])
    raise SystemExit(f"{name} {variant}: no result (rc {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per measuring process")
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    ap.add_argument("--parent-lib", default=None, help="libmaddpg_hip.so built from the commit before this feature")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=2, metavar=("CONFIG", "VARIANT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.rounds, args.warmup, args.calls)
    res = {"timing": "round_us: host clock around replayed update rounds, device synchronise on both sides, after "
                     "warm-up; critic/actor_grad_us: HIP events on the launch's own packet in separate eager passes; "
                     "approx_grad_us: median of device event pairs around mdp_approx_grad; each variant in its own "
                     "process, variants alternated per repeat; medians over the repeats, spread = [min, max]",
           "parent_lib": "a build of the parent commit" if args.parent_lib else "this build (uniform kernels)"}
    for name in args.configs:
        runs = {v: [] for v in VARIANTS}
        for _ in range(args.repeats):
            for v in VARIANTS:
                runs[v].append(run_variant(name, v, args))
                print(name, json.dumps(runs[v][-1]), flush=True)
        keys = {v: [k for k in runs[v][0] if k.endswith("_us")] for v in VARIANTS}
        med = {v: {k: statistics.median(x[k] for x in runs[v]) for k in keys[v]} for v in VARIANTS}
        spread = {v: {k: [min(x[k] for x in runs[v]), max(x[k] for x in runs[v])] for k in keys[v]} for v in VARIANTS}
        pg, tg, ax = med["parent_general"], med["this_general"], med["approx"]
        m = runs["approx"][0]["pairs_per_launch"]
        res[name] = {
            "config": CONFIGS[name], "runs": runs, "median": med, "spread": spread,
            "this_uniform_critic_over_parent_general": round(tg["critic_grad_us"] / pg["critic_grad_us"], 3),
            "approx_critic_over_parent_general": round(ax["critic_grad_us"] / pg["critic_grad_us"], 3),
            "approx_grad_us": ax["approx_grad_us"], "pairs_per_launch": m,
            "m_parent_general_actor_launches_us": round(m * pg["actor_grad_us"], 3),
            "approx_grad_under_m_actor_launches": bool(ax["approx_grad_us"] < m * pg["actor_grad_us"]),
            "approx_round_over_parent_general_round": round(ax["round_us"] / pg["round_us"], 3),
            "approx_round_over_parent_shipped_round": round(ax["round_us"] / med["parent_shipped"]["round_us"], 3),
            "approx_buffer_bytes": runs["approx"][0]["approx_buffer_bytes"],
            "approx_slab_bytes_about": runs["approx"][0]["approx_slab_bytes_about"],
        }
        print(name, json.dumps({k: v for k, v in res[name].items() if k != "runs"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
