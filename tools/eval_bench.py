"""Policy evaluation: one launch against the two ways the parent could score 1,024 episodes.

For BASELINE configs[1] (simple_spread N=3, 64 units) and configs[4] (simple_tag
N=6, 128 units, batch 4096), 1,024 episodes of 25 steps with records, on ONE handle
with 1,024 env copies, in one session:

  evaluate      mdp_evaluate(1024, bench) -- one k_eval_episodes launch (device events)
  step_chain    25 mdp_env_step_bench launches carrying the 1,024 env copies through
                one episode (device events around the 25 launches)
  host_loop     experiments/train.py --benchmark's loop for the same episodes: per
                step the launch, the [E, n, 8] copy to the host and the Python loop
                over env copies and agents (host clock, ends synchronised)

Each figure is the median of --repeats timed windows after --warmup untimed ones.
--bench-ab FILE merges the six bench.py figures (parent / this commit, alternating)
that a session recorded, with the no-slowdown bar of DESIGN sections 11 and 12.

    python tools/eval_bench.py [--out profiles/eval_bench.json] [--bench-ab FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPISODES, STEPS = 1024, 25
CONFIGS = {
    "configs[1]": dict(scenario="simple_spread", n=3, adv=None, num_units=64, batch_size=1024),
    "configs[4]": dict(scenario="simple_tag", n=6, adv=4, num_units=128, batch_size=4096),
}


def measure(name, c, repeats, warmup):
    import torch
    from maddpg_amd import _lib
    from maddpg_amd.engine import Engine
    from maddpg_amd.envs import bench_record, spec
    sp = spec(c["scenario"], c["n"], c["adv"])
    eng = Engine(sp.obs_dims, num_units=c["num_units"], batch_size=c["batch_size"], capacity=1 << 16,
                 num_envs=EPISODES, scenario=c["scenario"], num_adversaries=sp.num_adversaries,
                 max_episode_len=STEPS, seed=1)
    eng.init_params(0)
    eng.env_reset()
    n = eng.n
    ret = torch.empty((EPISODES, n), dtype=torch.float32, device=eng.device)
    rec = torch.empty((EPISODES, n, _lib.BENCH_W), dtype=torch.float32, device=eng.device)
    info = torch.empty((EPISODES, n, _lib.BENCH_W), dtype=torch.float32, device=eng.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def timed_events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(eng.stream)
        fn()
        b.record(eng.stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e3           # us

    def one_launch():
        eng._c("mdp_evaluate", 0, EPISODES, 0, None, p(ret), p(rec))

    def chain():
        for _ in range(STEPS):
            eng._c("mdp_env_step_bench", p(info))

    def host_loop():
        t0 = time.perf_counter()
        closed = []
        for _ in range(STEPS):
            rows = eng.env_step_bench(info).cpu().numpy()
            closed.append([[bench_record(sp, rows[e, i], i) for i in range(n)] for e in range(EPISODES)])
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e6

    out = {"scenario": c["scenario"], "agents": n, "num_units": c["num_units"], "episodes": EPISODES,
           "steps_per_episode": STEPS, "repeats": repeats}
    for key, fn, ev in (("evaluate", one_launch, True), ("step_chain", chain, True), ("host_loop", host_loop, False)):
        reps = repeats if ev else max(3, repeats // 4)
        for _ in range(warmup if ev else 1):
            fn()
        eng.synchronize()
        xs = [timed_events(fn) if ev else fn() for _ in range(reps)]
        out[key + "_us"] = {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2),
                            "max": round(max(xs), 2), "windows": reps}
    e = out["evaluate_us"]["median"]
    out["step_chain_over_evaluate"] = round(out["step_chain_us"]["median"] / e, 2)
    out["host_loop_over_evaluate"] = round(out["host_loop_us"]["median"] / e, 2)
    out["episodes_per_sec_evaluate"] = round(EPISODES / e * 1e6, 1)
    eng.prof_enable("eval")
    one_launch()
    ms, launches = eng.prof_read("eval")
    out["kernel_us_packet"] = round(ms * 1e3 / max(launches, 1), 2)
    out["grid_workgroups"] = (EPISODES + 15) // 16
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/eval_bench.json")
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-ab", default=None,
                    help="JSON {'parent': [v, v, v], 'new': [v, v, v]}: bench.py values of alternating runs")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on a GPU; none is available")
    res = {"device": torch.cuda.get_device_name(0), "configs": {}}
    for name, c in CONFIGS.items():
        res["configs"][name] = measure(name, c, a.repeats, a.warmup)
    if a.bench_ab:
        ab = json.load(open(a.bench_ab))
        pm, nm = statistics.median(ab["parent"]), statistics.median(ab["new"])
        spread = max(ab["parent"]) - min(ab["parent"])
        res["bench_py"] = {"unit": "env-steps/s", "parent": ab["parent"], "new": ab["new"], "parent_median": pm,
                           "new_median": nm, "parent_spread": round(spread, 3),
                           "bar": "new median >= parent median - parent (max - min)",
                           "holds": bool(nm >= pm - spread)}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
