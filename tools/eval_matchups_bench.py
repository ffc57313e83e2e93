"""Matchup evaluation: one launch over a cross-play table against the parent's loop.

For BASELINE configs[4]'s topology (simple_tag N=6, 128 units) and simple_tag 3+1
at 64 units: a bank of 8 actor sets, the 8 x 8 cross-play table (64 matchups, the
adversaries from the row set, the good agents from the column set), 1,024 episodes
of 25 steps with records per matchup, on ONE handle, in one session:

  matchups       mdp_evaluate_matchups(64 x 1024, bench): the one launch (its own
                 dispatch packet's begin -> end, MDP_K_EVAL) and the whole call
                 (host clock: the table's staging, the launch, the synchronise)
  parent_loop    what the parent offers for the same table, per pairing:
                 mdp_set_params of the mix (every agent's actor from host arrays)
                 + mdp_evaluate(1024, bench).  `launches`: the 64 launches alone
                 (the sum of their dispatch packets); `loop`: the whole loop (host
                 clock, ends synchronised)

Each figure is the median of --repeats timed windows after --warmup untimed ones;
min and max give the spread of the windows.  Both ways produce the same numbers
(checked here once, bit for bit).  --bench-ab FILE merges the six bench.py figures
(parent / this commit, alternating) that a session recorded.

    python tools/eval_matchups_bench.py [--out profiles/eval_matchups_bench.json] [--bench-ab FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPISODES, STEPS, SETS = 1024, 25, 8
CONFIGS = {
    "configs[4] topology (simple_tag N=6, H=128)": dict(scenario="simple_tag", n=6, adv=4, num_units=128, batch_size=4096),
    "simple_tag 3+1, H=64": dict(scenario="simple_tag", n=4, adv=3, num_units=64, batch_size=1024),
}


def stat(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2),
            "windows": len(xs)}


def measure(name, c, repeats, warmup):
    import numpy as np
    import torch
    from maddpg_amd import _lib
    from maddpg_amd.engine import Engine
    from maddpg_amd.envs import spec
    sp = spec(c["scenario"], c["n"], c["adv"])
    eng = Engine(sp.obs_dims, num_units=c["num_units"], batch_size=c["batch_size"], capacity=1 << 16,
                 num_envs=EPISODES, scenario=c["scenario"], num_adversaries=sp.num_adversaries,
                 max_episode_len=STEPS, seed=1)
    n, team = eng.n, list(range(c["adv"]))
    bank = eng.actor_bank(SETS)
    flats = []                      # [set][agent]: the host arrays the parent's loop writes with mdp_set_params
    for k in range(SETS):
        eng.init_params(k)
        eng.bank_snapshot(bank, k)
        flats.append([eng._flat_params(j, "actor", eng.get_params(j, "actor")) for j in range(n)])
    table = np.empty((SETS, SETS, n), np.int32)
    for j in range(n):
        table[:, :, j] = np.arange(SETS)[:, None] if j in team else np.arange(SETS)[None, :]
    table = np.ascontiguousarray(table.reshape(SETS * SETS, n))
    M = len(table)
    ret = torch.empty((M, EPISODES, n), dtype=torch.float32, device=eng.device)
    rec = torch.empty((M, EPISODES, n, _lib.BENCH_W), dtype=torch.float32, device=eng.device)
    ret1 = torch.empty((M, EPISODES, n), dtype=torch.float32, device=eng.device)
    rec1 = torch.empty((M, EPISODES, n, _lib.BENCH_W), dtype=torch.float32, device=eng.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    tptr = table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def one_launch():
        eng._c("mdp_evaluate_matchups", p(bank), SETS, tptr, M, 0, EPISODES, 0, None, p(ret), p(rec))

    def launches_only():
        for m in range(M):
            eng._c("mdp_evaluate", 0, EPISODES, 0, None, p(ret1[m]), p(rec1[m]))

    def parent_loop():
        for m in range(M):
            for j in range(n):
                f = flats[table[m, j]][j]
                eng._c("mdp_set_params", j, _lib.WHICH["actor"], _lib.fptr(f), f.size)
            eng._c("mdp_evaluate", 0, EPISODES, 0, None, p(ret1[m]), p(rec1[m]))

    def host_clock(fn):
        eng.synchronize()
        t0 = time.perf_counter()
        fn()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def packets(fn):
        """the sum of fn's evaluation launches' dispatch packets (us) and their count"""
        ms0, n0 = eng.prof_read("eval")
        fn()
        ms1, n1 = eng.prof_read("eval")
        return (ms1 - ms0) * 1e3, n1 - n0

    out = {"scenario": c["scenario"], "agents": n, "adversaries": c["adv"], "num_units": c["num_units"],
           "sets": SETS, "matchups": M, "episodes": EPISODES, "steps_per_episode": STEPS}
    for _ in range(warmup):
        one_launch()
    for _ in range(max(1, warmup // 3)):
        parent_loop()
    eng.synchronize()
    assert torch.equal(ret, ret1) and torch.equal(rec, rec1), "the two ways disagree"
    out["same_numbers_both_ways"] = True
    loop_windows = max(3, repeats // 4)
    out["matchups_call_us"] = stat([host_clock(one_launch) for _ in range(repeats)])
    out["parent_loop_us"] = stat([host_clock(parent_loop) for _ in range(loop_windows)])
    out["parent_launches_host_clock_us"] = stat([host_clock(launches_only) for _ in range(loop_windows)])
    eng.prof_enable("eval")
    xs = [packets(one_launch) for _ in range(repeats)]
    assert all(k == 1 for _us, k in xs)
    out["matchups_launch_us"] = stat([us for us, _k in xs])
    xs = [packets(launches_only) for _ in range(loop_windows)]
    assert all(k == M for _us, k in xs)
    out["parent_launches_us"] = stat([us for us, _k in xs])
    out["parent_launch_each_us"] = round(out["parent_launches_us"]["median"] / M, 2)
    eng.prof_enable("eval", False)
    out["launches_ratio"] = round(out["parent_launches_us"]["median"] / out["matchups_launch_us"]["median"], 2)
    out["loop_ratio"] = round(out["parent_loop_us"]["median"] / out["matchups_call_us"]["median"], 2)
    out["episodes_per_sec_matchups"] = round(M * EPISODES / out["matchups_launch_us"]["median"] * 1e6, 1)
    out["grid_workgroups"] = [(EPISODES + 15) // 16, M]
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/eval_matchups_bench.json")
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-ab", default=None,
                    help="JSON {'parent': [v, v, v], 'new': [v, v, v]}: bench.py values of alternating runs")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_matchups_bench.py measures on a GPU; none is available")
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
