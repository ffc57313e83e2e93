#!/usr/bin/env python
"""Per-launch cost of a strict round with entropy-regularised tanh Box(2) agents
against the same round without coefficients.

The shapes, the launches and the timing are tools/box_squash_bench.py's:
simple_spread N=3 at 64 units (1,024 envs, B=1024) and simple_tag N=6 at 128
units (4,096 envs, B=4096); HIP-event times of the critic, actor and rollout
launches' own packets in eager passes after warm-up.  Two variants, both
--continuous-actions --action-squash tanh (the general kernels): `tanh` runs
the SQ instantiations, `entropy` (--entropy-alpha 0.2) the entropy ones.  The
one-wave fold launch behind each entropy gradient launch is a launch of its
own, outside those packets: round_us, the wall time of one captured update
round (graph replays between two synchronisations), holds it.  Each variant
runs in its own process, the variants alternate per repeat, and the figures are
medians over the repeats.

    python tools/box_entropy_bench.py --out profiles/box_entropy_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.box_bench import CONFIGS, KINDS  # noqa: E402

VARIANTS = ("tanh", "entropy")
ALPHA = 0.2


def worker(name, variant, rounds, warmup):
    import torch
    from maddpg_amd.runner import VecRunner
    if not torch.cuda.is_available():
        raise SystemExit("box_entropy_bench measures on the GPU only")
    kw = dict(CONFIGS[name])
    r = VecRunner(kw.pop("scenario"), kw.pop("num_envs"), seed=0, continuous=True, squash="tanh",
                  entropy_alpha=ALPHA if variant == "entropy" else 0.0, **kw)
    r.prefill()
    eng = r.eng
    for _ in range(warmup):
        eng.update_round()
        eng.env_step()
    eng.synchronize()
    out = {"variant": variant, "act_squash": eng.act_squash, "act_entropy": eng.act_entropy,
           "grad_variant": [int(eng.lib.mdp_grad_variant(eng.h, i)) for i in range(r.n)]}
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
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        eng.update_round()
    eng.synchronize()
    out["round_us"] = round((time.perf_counter() - t0) / rounds * 1e6, 3)
    out["check_finite"] = int(eng.check_finite())
    eng.close()
    print("BOX_ENTROPY_BENCH " + json.dumps(out), flush=True)


def run_variant(name, variant, args):
    env = dict(os.environ)
    env.pop("MDP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, variant, "--rounds", str(args.rounds),
           "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
    for line in p.stdout.splitlines():
        if line.startswith("BOX_ENTROPY_BENCH "):
            return json.loads(line[len("BOX_ENTROPY_BENCH "):])
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
                     "process, variants alternated per repeat; medians over the repeats; both variants tanh Box(2) on "
                     "the general gradient kernels; round_us: wall time of one update round as graph replays, "
                     "which holds the one-wave fold launch behind each entropy gradient launch"}
    for name in CONFIGS:
        runs = {v: [] for v in VARIANTS}
        for _ in range(args.repeats):
            for v in VARIANTS:
                runs[v].append(run_variant(name, v, args))     # (raises, and so stops, if a process gave no result)
                print(name, json.dumps(runs[v][-1]), flush=True)
        med = {v: {k + "_us": statistics.median(x[k + "_us"] for x in runs[v]) for k in KINDS + ("round",)}
               for v in VARIANTS}
        res[name] = {"config": CONFIGS[name], "runs": runs, "median": med,
                     "entropy_over_tanh": {k: round(med["entropy"][k + "_us"] / med["tanh"][k + "_us"], 3)
                                           for k in KINDS + ("round",)}}
        print(name, "entropy / tanh:", res[name]["entropy_over_tanh"], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
