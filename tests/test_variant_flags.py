"""The variant table on the Python side (maddpg_amd/variants.py).

The command lines experiments/train.py refuses are those it refused when
td3_flags, minimax_flags, approx_flags and continuous_flags each listed the
other flags by hand: every pair of variant flags, every pre-checked flag with
throughput mode or several GPUs, and TF1 checkpoints with --td3 and
--approx-policies.  (--prioritized-replay alone has no flag check of its own:
the library refuses its throughput and multi-GPU runs.)  Engine and VecRunner
make their checks from the same table before any device call.
"""
import itertools

import pytest

from experiments.train import approx_flags, continuous_flags, minimax_flags, parse_args, td3_flags
from maddpg_amd import variants

FLAGS = [r.flag for r in variants.ROWS]
PRECHECKED = [r.flag for r in variants.ROWS if r.precheck]


def _cli(argv, world=1):
    """the four checks in train()'s order; the SystemExit text, or None when all pass"""
    a = parse_args(argv)
    try:
        for check in (td3_flags, minimax_flags, approx_flags, continuous_flags):
            check(a, world)
    except SystemExit as e:
        return str(e)
    return None


def test_the_table_lists_the_five_flags():
    assert FLAGS == ["--prioritized-replay", "--td3", "--minimax", "--approx-policies", "--continuous-actions"]
    assert PRECHECKED == FLAGS[1:]
    assert [r.flag for r in variants.ROWS if r.npz_only] == ["--td3", "--approx-policies"]
    assert [r.kw for r in variants.ROWS] == ["prioritized", "td3", "minimax", "approx", "continuous"]


def test_no_flag_and_each_flag_alone_pass():
    assert _cli([]) is None
    for f in FLAGS:
        assert _cli([f]) is None, f


@pytest.mark.parametrize("a,b", list(itertools.permutations(FLAGS, 2)))
def test_every_pair_of_flags_is_refused(a, b):
    why = _cli([a, b])
    assert why in (f"{a} does not combine with {b}", f"{b} does not combine with {a}"), why


@pytest.mark.parametrize("flag", FLAGS)
def test_throughput_several_gpus_and_tf1(flag):
    checked = flag in PRECHECKED
    assert _cli([flag, "--update-mode", "throughput"]) == (f"{flag} needs --update-mode strict" if checked else None)
    assert _cli([flag, "--num-gpus", "2"]) == (f"{flag} runs on one GPU (--num-gpus 1)" if checked else None)
    assert _cli([flag], world=2) == (f"{flag} runs on one GPU (--num-gpus 1)" if checked else None)
    why = _cli([flag, "--save-format", "tf1"])
    if variants.by_flag(flag).npz_only:
        assert why.startswith(f"{flag} saves npz checkpoints only")
    else:
        assert why is None


def test_a_flag_that_is_not_given_refuses_nothing():
    a = parse_args(["--td3", "--minimax", "--update-mode", "throughput", "--num-gpus", "2"])
    approx_flags(a)
    continuous_flags(a, world=2)
    b = parse_args(["--approx-policies", "--continuous-actions"])
    td3_flags(b)
    minimax_flags(b)


def test_engine_and_runner_refuse_from_the_table_before_any_device_call():
    from maddpg_amd._lib import MdpError
    from maddpg_amd.engine import Engine
    from maddpg_amd.runner import VecRunner
    for x, y in itertools.combinations(variants.VARIANTS, 2):
        with pytest.raises(MdpError) as e:
            Engine([6, 5, 4], **{x.kw: True, y.kw: True})
        assert x.name in str(e.value) and y.name in str(e.value)
    with pytest.raises(MdpError, match="M3DDPG"):      # an eps matrix alone asks for M3DDPG
        Engine([6, 5], td3=True, minimax_eps=[[0, 1e-3], [1e-3, 0]])
    for r in variants.VARIANTS:
        with pytest.raises(MdpError, match="one GPU"):
            Engine([6, 5, 4], world_size=2, **{r.kw: True})
    for r in variants.ROWS:
        if r.precheck:
            with pytest.raises(ValueError, match=f"{r.flag} runs on one GPU"):
                VecRunner("simple_spread", 4, world_size=2, **{r.kw: True})
