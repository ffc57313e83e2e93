"""The variants x seams matrix of the C ABI, recorded from a built library.

Every handle state of STATES meets every call of CALLS on a fresh handle of
its own, so an accepted call cannot change a later cell; a cell is "refused"
(the call returned < 0, with mdp_last_error's text) or "accepted".  The cells
of NOT_EXECUTED would wait for data-parallel peers that do not exist: they are
marked accepted by reading the shim and are never run.

    python tools/variant_matrix.py tests/golden/variant_matrix.json

wrote the golden file from the commit before the variant table existed
(DESIGN.md section 25); tests/test_variant_gate.py holds the table's pure
function to it and tests/test_variant_matrix_gpu.py replays it on the library.
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the shapes of tests/test_approx_gpu.py::test_approx_refusals_leave_the_handle_training
DIMS, B, ROWS = [6, 5, 4], 40, 200
CAPACITY = ROWS + 7

STATES = ("plain", "prioritized", "MATD3", "M3DDPG", "inferred policies", "Box agent", "throughput mode",
          "plain after one update", "plain, world_size 2")
ENABLES = ("mdp_per_enable", "mdp_td3_enable", "mdp_minimax_enable", "mdp_approx_enable")
DP_CALLS = ("mdp_dp_init", "mdp_dp_xgmi_open", "mdp_dp_xgmi_connect", "mdp_dp_xgmi_probe", "mdp_dp_xgmi_enable")
PHASE_CALLS = ("mdp_critic_grad", "mdp_actor_grad", "mdp_reduce_grad", "mdp_apply_grad")
CALLS = ENABLES + ("mdp_set_act_spaces", "mdp_set_update_mode", "mdp_update_all") + DP_CALLS + PHASE_CALLS

# the state's own Engine keyword (the four variants and the Box property)
STATE_KW = {"prioritized": dict(prioritized=True), "MATD3": dict(td3=True), "M3DDPG": dict(minimax=True),
            "inferred policies": dict(approx=True),
            "Box agent": dict(act_kinds=["box", "discrete", "discrete"], act_dims=[2, 5, 5]),
            "plain, world_size 2": dict(world_size=2)}
# mdp_set_act_spaces is accepted on a fresh handle only (no parameter write, row or update before it)
NOT_FRESH = ("plain after one update",)
# a handle nothing keeps from joining: the call would go on to wait for its peers
NOT_EXECUTED = {(s, c) for s in ("plain", "plain after one update", "plain, world_size 2")
                for c in ("mdp_dp_init", "mdp_dp_xgmi_open")}
BY_READING = "accepted (by reading; not executed)"


# refusals that are not the variant table's: the call came out of order on a handle that could
# take it (the same text before and after the table; the table lets these cells go on)
SEQUENCING = {"mdp_update_all": "set throughput mode first", "mdp_dp_xgmi_connect": "call mdp_dp_xgmi_open first",
              "mdp_dp_xgmi_probe": "not connected", "mdp_dp_xgmi_enable": "not connected"}
VARIANT_STATES = {"prioritized": "prioritized replay", "MATD3": "MATD3", "M3DDPG": "M3DDPG",
                  "inferred policies": "inferred policies"}
VARIANT_OF = dict(zip(ENABLES, VARIANT_STATES.values()))


def expected_substrings(state, call):
    """what the table's refusal of `call` on a handle in `state` must say, beside the
    entry point's name (the substrings callers and tests match)"""
    if call == "mdp_set_act_spaces" or state == "Box agent":
        return ["Box action space"] + (["one GPU", "data-parallel"] if call in DP_CALLS else [])
    if call in ENABLES:
        if state in VARIANT_STATES:
            same = VARIANT_STATES[state] == VARIANT_OF[call]
            return [f"{call}: already enabled"] if same else [VARIANT_STATES[state], VARIANT_OF[call]]
        return {"throughput mode": ["strict update mode"],
                "plain after one update": ["before the handle's first update, round or train"],
                "plain, world_size 2": ["one GPU", "data-parallel"]}[state]
    if call in ("mdp_set_update_mode", "mdp_update_all"):
        return ["strict", VARIANT_STATES[state]]
    if call in DP_CALLS:
        return ["throughput mode"] if state == "throughput mode" else ["one GPU", "data-parallel", VARIANT_STATES[state]]
    return ["phase entry points", VARIANT_STATES[state]]


def cells():
    """every (state, call) of the matrix, in file order"""
    return [(s, c) for s in STATES for c in CALLS if not (c == "mdp_set_act_spaces" and s in NOT_FRESH)]


def key(state, call):
    return f"{state} | {call}"


def inputs(seed=3):
    """replay rows and one round's injected indices and uniforms, the same for every handle"""
    rng = np.random.default_rng(seed)
    n = len(DIMS)
    return dict(idx=rng.integers(0, ROWS, (n, B)).astype(np.int32),
                u_tgt=rng.uniform(0.01, 0.99, (n, n, B, 5)).astype(np.float32),
                u_act=rng.uniform(0.01, 0.99, (n, B, 5)).astype(np.float32), rows_seed=seed + 1)


def make_state(state, fresh=False):
    """an Engine in `state`; unless `fresh`, with parameters and ROWS replay rows"""
    import torch

    from maddpg_amd.engine import Engine
    eng = Engine(DIMS, batch_size=B, capacity=CAPACITY, **STATE_KW.get(state, {}))
    if state == "throughput mode":
        eng.set_update_mode("throughput")
    if fresh:
        return eng
    rows = np.random.default_rng(inputs()["rows_seed"]).standard_normal((ROWS, eng.row_stride)).astype(np.float32)
    eng.init_params(0)
    eng.add_rows(torch.from_numpy(rows))
    if state == "plain after one update":
        update(eng, 0)
    return eng


def update(eng, r):
    """round r of the injected inputs: every agent's update in turn, or one throughput round"""
    import torch
    x = inputs()
    t = torch.from_numpy
    if eng.update_mode == "throughput":
        eng.update_all(idx=t(np.roll(x["idx"], r, 1)), u_tgt=t(x["u_tgt"]), u_act=t(x["u_act"]))
        return
    for i in range(eng.n):
        eng.update(i, idx=t(np.roll(x["idx"][i], r)), u_tgt=t(x["u_tgt"][i]), u_act=t(x["u_act"][i]))


def state_bits(eng):
    """everything training writes and a checkpoint keeps, plus the sum trees, as bytes"""
    out = {k: np.ascontiguousarray(v).tobytes() for k, v in eng.state_dict().items()}
    if eng.prioritized:
        for i in range(eng.n):
            out[f"per_tree_{i}"] = np.ascontiguousarray(eng.per_tree(i)).tobytes()
    return out


class Caller:
    """valid arguments for every call of CALLS on one Engine: only the handle's state can refuse them"""

    def __init__(self, eng):
        import torch
        self.eng, lib = eng, eng.lib
        cfg = ctypes.byref(eng.cfg)
        nb = max(lib.mdp_per_bytes(cfg), lib.mdp_td3_bytes(cfg), lib.mdp_approx_bytes(cfg))
        self.buf = torch.empty(nb, dtype=torch.uint8, device=eng.device)
        self.eps = np.zeros((eng.n, eng.n), np.float32)
        self.idx = torch.from_numpy(inputs()["idx"][0]).to(eng.device)
        self.out = ctypes.create_string_buffer(64)
        self.bad = ctypes.c_int32(0)

    def __call__(self, call):
        from maddpg_amd import _lib
        eng, lib, h = self.eng, self.eng.lib, self.eng.h
        buf, nb, idx = eng._ptr(self.buf), self.buf.numel(), eng._ptr(self.idx)
        i32 = lambda *v: (ctypes.c_int32 * _lib.MAX_AGENTS)(*v)  # noqa: E731
        rc = {
            "mdp_per_enable": lambda: lib.mdp_per_enable(h, buf, nb, 0.6, 0.4, 0.001, 0.01, 1.0),
            "mdp_td3_enable": lambda: lib.mdp_td3_enable(h, buf, nb, 2),
            "mdp_minimax_enable": lambda: lib.mdp_minimax_enable(h, _lib.fptr(self.eps)),
            "mdp_approx_enable": lambda: lib.mdp_approx_enable(h, buf, nb, 1e-3),
            "mdp_set_act_spaces": lambda: lib.mdp_set_act_spaces(h, i32(1, 0, 0), i32(2, 5, 5)),
            "mdp_set_update_mode": lambda: lib.mdp_set_update_mode(h, 1),
            "mdp_update_all": lambda: lib.mdp_update_all(h, None, None, None),
            "mdp_dp_init": lambda: lib.mdp_dp_init(h, bytes(128), 2, 0),
            "mdp_dp_xgmi_open": lambda: lib.mdp_dp_xgmi_open(h, 2, 0, self.out),
            "mdp_dp_xgmi_connect": lambda: lib.mdp_dp_xgmi_connect(h, bytes(128)),
            "mdp_dp_xgmi_probe": lambda: lib.mdp_dp_xgmi_probe(h, ctypes.byref(self.bad)),
            "mdp_dp_xgmi_enable": lambda: lib.mdp_dp_xgmi_enable(h),
            "mdp_critic_grad": lambda: lib.mdp_critic_grad(h, 0, idx, None),
            "mdp_actor_grad": lambda: lib.mdp_actor_grad(h, 0, idx, None),
            "mdp_reduce_grad": lambda: lib.mdp_reduce_grad(h, 0, 1),
            "mdp_apply_grad": lambda: lib.mdp_apply_grad(h, 0, 1, 1.0),
        }[call]()
        msg = lib.mdp_last_error(h).decode() if rc < 0 else None
        eng.synchronize()
        return rc < 0, msg


def run_cell(state, call):
    """(refused, message) of `call` on a fresh handle in `state`; NOT_EXECUTED cells are not run"""
    if (state, call) in NOT_EXECUTED:
        return False, None
    eng = make_state(state, fresh=call == "mdp_set_act_spaces")
    try:
        return Caller(eng)(call)
    finally:
        eng.close()


def record():
    out = {}
    for state, call in cells():
        refused, msg = run_cell(state, call)
        verdict = "refused" if refused else (BY_READING if (state, call) in NOT_EXECUTED else "accepted")
        out[key(state, call)] = {"verdict": verdict, "message": msg}
        print(f"{key(state, call):58s} {verdict}{': ' + msg if msg else ''}", flush=True)
    return out


def main(argv):
    path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "variant_matrix.json")
    cellmap = record()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"shapes": {"obs_dims": DIMS, "batch_size": B, "capacity": CAPACITY, "rows": ROWS},
                   "states": list(STATES), "calls": list(CALLS), "cells": cellmap}, f, indent=1)
        f.write("\n")
    print(f"wrote {len(cellmap)} cells to {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
