"""CPU: the policy-evaluation entry points exist, refuse a NULL handle, and the CLI
has the evaluation flags with evaluation off by default."""
import ctypes

from maddpg_amd import _lib


def test_library_exports_the_evaluation_entry_points():
    lib = _lib.load()
    for name in ("mdp_evaluate", "mdp_eval_initial_state", "mdp_env_step_bench_u"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in _lib.header_symbols(), name
    # a NULL handle is refused (no launch, no crash); the ABI version did not move
    assert lib.mdp_evaluate(None, 0, 16, 0, None, None, None) < 0
    pos, vel, goal = (ctypes.c_float * 8)(), (ctypes.c_float * 8)(), (ctypes.c_int32 * 2)()
    assert lib.mdp_eval_initial_state(None, 0, 2, pos, vel, goal) < 0
    assert lib.mdp_env_step_bench_u(None, None, None) < 0
    assert lib.mdp_abi_version() == 5
    assert _lib.EVAL_MODE == {"sample": 0, "mean": 1} and _lib.KERNEL_EVAL == {"eval": 12}
    # the timed kinds end with the evaluation launch
    assert lib.mdp_prof_enable(None, 12, 1) < 0
    text = open(_lib.HEADER).read()
    assert "MDP_K_EVAL = 12" in text and "MDP_K_COUNT = 13" in text
    assert "MDP_EVAL_SAMPLE = 0, MDP_EVAL_MEAN = 1" in text


def test_cli_has_the_evaluation_flags_off_by_default():
    from experiments.train import parse_args
    a = parse_args([])
    assert a.evaluate is False and a.eval_episodes == 0 and a.eval_mode == "sample" and a.adv_load_dir == ""
    b = parse_args(["--evaluate", "--eval-episodes", "256", "--eval-mode", "mean", "--adv-load-dir", "/x/"])
    assert b.evaluate and b.eval_episodes == 256 and b.eval_mode == "mean" and b.adv_load_dir == "/x/"
