"""CPU: the critic-evaluation entry point is exported, typed and declared, refuses a
NULL handle and a handle whose mdp_create failed, and train.py takes --eval-q."""
import ctypes

from maddpg_amd import _lib


def test_entry_point_is_exported_and_declared():
    lib = _lib.load()
    name = "mdp_evaluate_q"
    assert hasattr(lib, name) and name in _lib.SIGNATURES and name in _lib.header_symbols()
    assert len(_lib.SIGNATURES[name][1]) == 11
    assert lib.mdp_abi_version() == _lib.ABI_VERSION == 5          # the ABI version stays
    assert _lib.KERNEL_EVAL == {"eval": 12}                       # timed under MDP_K_EVAL, no new kind


def test_null_and_failed_handles_are_refused():
    lib = _lib.load()
    args = (0, 16, 0, 12, 5, None, None, None, None, None)
    assert lib.mdp_evaluate_q(None, *args) < 0
    h, arena = ctypes.c_void_p(), ctypes.create_string_buffer(16)
    assert lib.mdp_create(None, ctypes.cast(arena, ctypes.c_void_p), 16, None, ctypes.byref(h)) < 0
    assert h.value
    try:
        assert lib.mdp_evaluate_q(h, *args) < 0
    finally:
        assert lib.mdp_destroy(h) == 0


def test_cli_flag():
    from experiments.train import eval_q_lines, parse_args
    assert parse_args([]).eval_q is False
    a = parse_args(["--evaluate", "--eval-q", "--eval-episodes", "64"])
    assert a.evaluate and a.eval_q and a.eval_episodes == 64
    s = {"q_mean": [[1.0, 2.0]], "g_mean": [[0.5, 0.5]], "gap_mean": [[0.5, 1.5]], "gap_rms": [[0.6, 1.6]],
         "steps": 115, "scored": 25, "truncation": 0.0094}
    lines = list(eval_q_lines(s))
    assert len(lines) == 1 and lines[0].startswith("eval_q agent 0: mean Q [1.0, 2.0], mean return-to-go 0.5,")
    assert "25 of 115 steps scored" in lines[0]
