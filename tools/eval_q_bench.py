"""Critic evaluation: Q against the realised return in the evaluation launch, timed
against what it replaces, and the diagnostic's first measurements.

Timing, for BASELINE configs[1] (simple_spread N=3, 64 units) and configs[4]'s
topology (simple_tag N=6, 128 units), 1,024 episodes of 115 steps, 25 scored:

  evaluate_q     mdp_evaluate_q(1024, steps=115, scored=25): both launches
  parent         the device work of the host loop the parent needs for the same
                 numbers, on a handle with max_episode_len = 115: mdp_evaluate(1024)
                 for the trajectory plus one mdp_q_values launch of 1,024 rows per
                 agent and step (n x 115 launches).  A lower bound of that loop: its
                 stepping of a second engine in place of mdp_evaluate, the row
                 fetches, the twin critic and numpy's discounting are left out.

Each figure is the median of --repeats windows between two events on the handle's
stream, the two variants alternating window by window; min and max give the spread.

Measurements (`learning`): `simple` trained as tests/test_learning_gpu.py trains it
(12 lockstep batches of 1,024 env copies), MADDPG and MATD3: evaluate_q(1024) on the
freshly initialised and on the trained engine, the same ids -- mean Q, mean
return-to-go, mean and RMS gap per critic.  --bench-ab FILE merges bench.py figures
(parent / this commit, alternating) that a session recorded.

    python tools/eval_q_bench.py [--out profiles/eval_q.json] [--bench-ab FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPISODES, STEPS, SCORED = 1024, 115, 25
CONFIGS = {
    "configs[1] (simple_spread N=3, H=64)": dict(scenario="simple_spread", n=3, adv=None, num_units=64, batch_size=1024),
    "configs[4] topology (simple_tag N=6, H=128)": dict(scenario="simple_tag", n=6, adv=4, num_units=128,
                                                        batch_size=4096),
}


def stat(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2),
            "windows": len(xs)}


def timing(name, c, repeats, warmup):
    import torch
    from maddpg_amd.engine import Engine
    from maddpg_amd.envs import spec
    sp = spec(c["scenario"], c["n"], c["adv"])

    def engine(max_len):
        e = Engine(sp.obs_dims, num_units=c["num_units"], batch_size=c["batch_size"], capacity=1 << 16,
                   num_envs=EPISODES, scenario=c["scenario"], num_adversaries=sp.num_adversaries,
                   max_episode_len=max_len, seed=1)
        e.init_params(0)
        return e

    new, par = engine(SCORED), engine(STEPS)
    n = new.n
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=new.device)  # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    q, rew, g, gap = f32(EPISODES, STEPS, n, 1), f32(EPISODES, STEPS, n), f32(EPISODES, STEPS, n), f32(EPISODES, n, 1)
    ret = f32(EPISODES, n)
    x = [torch.rand((EPISODES, par._tensors[(j, 1)][0][3]), dtype=torch.float32, device=new.device) for j in range(n)]
    qv = f32(EPISODES)

    def evaluate_q():
        new._c("mdp_evaluate_q", 0, EPISODES, 0, STEPS, SCORED, None, p(q), p(rew), p(g), p(gap))

    def parent():
        par._c("mdp_evaluate", 0, EPISODES, 0, None, p(ret), None)
        for _t in range(STEPS):
            for j in range(n):
                par._c("mdp_q_values", j, 0, p(x[j]), p(qv), EPISODES)

    def window(eng, fn):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.synchronize()
        a.record(eng.stream)
        fn()
        z.record(eng.stream)
        z.synchronize()
        return a.elapsed_time(z) * 1e3

    for _ in range(warmup):
        evaluate_q()
        parent()
    # the two calls play the same trajectory: their undiscounted 115-step returns agree bit for bit
    new.synchronize()
    par.synchronize()
    s = torch.zeros_like(ret)
    for t in range(STEPS):
        s = s + rew[:, t]
    assert torch.equal(s, ret), "evaluate_q's rewards are not evaluate's"
    xs_new, xs_par = [], []
    for _ in range(repeats):
        xs_new.append(window(new, evaluate_q))
        xs_par.append(window(par, parent))
    out = {"scenario": c["scenario"], "agents": n, "num_units": c["num_units"], "episodes": EPISODES, "steps": STEPS,
           "scored": SCORED, "evaluate_q_us": stat(xs_new), "parent_evaluate_plus_q_values_us": stat(xs_par),
           "parent_q_values_launches": n * STEPS, "same_rewards_both_ways": True}
    xs_ev = [window(par, lambda: par._c("mdp_evaluate", 0, EPISODES, 0, None, p(ret), None)) for _ in range(repeats)]
    out["parent_evaluate_alone_us"] = stat(xs_ev)
    out["ratio_parent_over_evaluate_q"] = round(out["parent_evaluate_plus_q_values_us"]["median"]
                                                / out["evaluate_q_us"]["median"], 2)
    out["ratio_evaluate_q_over_evaluate_alone"] = round(out["evaluate_q_us"]["median"]
                                                        / out["parent_evaluate_alone_us"]["median"], 2)
    print(name, json.dumps(out), flush=True)
    return out


def learning(td3):
    from maddpg_amd.runner import VecRunner
    r = VecRunner("simple", 1024, seed=0, episode_log_rows=4096, td3=td3)
    out = {"algorithm": "MATD3 (policy_delay 2)" if td3 else "MADDPG", "scenario": "simple", "batches": 12,
           "num_envs": 1024, "eval_episodes": 1024}
    for tag in ("untrained", "trained"):
        if tag == "trained":
            for _ in range(12 * 25):
                r.step()
            r.synchronize()
        res = r.evaluate_q(1024)
        out["steps"], out["scored"] = res["steps"], res["scored"]
        out[tag] = {k: (v[0] if isinstance(v, list) else v) for k, v in res["summary"].items()}   # agent 0: the only one
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/eval_q.json")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bench-ab", default=None,
                    help="JSON {'parent': [v, v, v], 'new': [v, v, v]}: bench.py values of alternating runs")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_q_bench.py measures on a GPU; none is available")
    res = {"device": torch.cuda.get_device_name(0), "timing": {}, "learning": []}
    for name, c in CONFIGS.items():
        res["timing"][name] = timing(name, c, a.repeats, a.warmup)
    for td3 in (False, True):
        res["learning"].append(learning(td3))
    if a.bench_ab:
        ab = json.load(open(a.bench_ab))
        res["bench_py"] = {"unit": "env-steps/s", "parent": ab["parent"], "new": ab["new"],
                           "parent_median": statistics.median(ab["parent"]), "new_median": statistics.median(ab["new"]),
                           "inside_each_others_spread": bool(min(ab["new"]) <= max(ab["parent"])
                                                             and min(ab["parent"]) <= max(ab["new"]))}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
