"""GPU: the evaluation flags of experiments/train.py (--eval-episodes during
training, --evaluate with --adv-load-dir for cross-play)."""
import filecmp
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)


def test_training_with_evaluation_is_the_same_training(tmp_path, capsys):
    """--eval-episodes 64 changes no learning-curve pickle and no checkpoint; it adds
    one `eval:` line and one entry of <exp-name>_eval_rewards.pkl per curve point,
    scored on the same ids every time"""
    from experiments.train import parse_args, train

    def run(tag, extra):
        d = str(tmp_path / tag) + "/"
        train(parse_args(["--scenario", "simple", "--num-envs", "64", "--num-episodes", "512", "--save-rate", "128",
                          "--batch-size", "64", "--max-episode-len", "5", "--buffer-size", "4096", "--save-dir", d,
                          "--plots-dir", d,
                          "--exp-name", "t"] + extra))
        return d, capsys.readouterr().out

    d0, out0 = run("plain", [])
    d1, out1 = run("eval", ["--eval-episodes", "64"])
    for f in ("t_rewards.pkl", "t_agrewards.pkl"):
        assert filecmp.cmp(d0 + f, d1 + f, shallow=False), f
    with np.load(d0 + "maddpg_amd_state.npz") as z0, np.load(d1 + "maddpg_amd_state.npz") as z1:
        assert sorted(z0.files) == sorted(z1.files) and len(z0.files) > 8
        for k in z0.files:                        # (the .npz container itself carries timestamps)
            assert z0[k].tobytes() == z1[k].tobytes(), k
    points = len(pickle.load(open(d0 + "t_rewards.pkl", "rb")))
    assert points == 4 and "eval:" not in out0
    assert not (tmp_path / "plain" / "t_eval_rewards.pkl").exists()
    ev = pickle.load(open(d1 + "t_eval_rewards.pkl", "rb"))
    assert len(ev) == points and all(len(e) == 1 and np.isfinite(e[0]) for e in ev)
    assert sum(line.startswith("eval: ") for line in out1.splitlines()) == points
    strip = lambda out: [ln.split(", time:")[0] for ln in out.splitlines()  # noqa: E731
                         if not ln.startswith(("eval: ", "throughput: "))]
    assert strip(out0) == strip(out1)
    assert len({tuple(e) for e in ev}) > 1        # the policy moved between the points


def test_evaluate_cross_play_is_the_hand_mixed_engine(tmp_path, capsys):
    """--evaluate --adv-load-dir: the adversary of one tiny simple_adversary checkpoint
    against the good agents of another == an Engine whose parameters were mixed by hand"""
    from experiments.train import parse_args, train
    common = ["--scenario", "simple_adversary", "--num-adversaries", "1", "--adv-policy", "ddpg", "--batch-size", "64",
              "--max-episode-len", "5", "--buffer-size", "4096", "--plots-dir", str(tmp_path) + "/"]
    dirs = []
    for k in (0, 1):
        d = str(tmp_path / f"ck{k}") + "/"
        train(parse_args(common + ["--num-envs", "64", "--num-episodes", "128", "--save-rate", "64", "--seed", str(k),
                                   "--save-dir", d, "--exp-name", f"c{k}"]))
        dirs.append(d)
    capsys.readouterr()
    bdir = str(tmp_path) + "/bench/"
    r = train(parse_args(common + ["--evaluate", "--eval-episodes", "48", "--eval-mode", "mean", "--load-dir", dirs[0],
                                   "--adv-load-dir", dirs[1], "--benchmark-dir", bdir, "--exp-name", "x"]))
    out = capsys.readouterr().out
    assert r.rounds == 0 and out.count("mean return") == 3 and out.count("mean record sums") == 3
    got = pickle.load(open(bdir + "x_eval.pkl", "rb"))
    assert got["returns"].shape == (48, 3) and got["bench"].shape == (48, 3, 8) and got["mode"] == "mean"

    from maddpg_amd.runner import VecRunner
    mixed = VecRunner("simple_adversary", 1, num_adversaries=1, adv_policy="ddpg", batch_size=64, max_episode_len=5,
                      capacity=4096)
    src = [VecRunner("simple_adversary", 1, num_adversaries=1, adv_policy="ddpg", batch_size=64, max_episode_len=5,
                      capacity=4096)
           for _ in dirs]
    for s, d in zip(src, dirs):
        s.eng.load_state(d)
    for i in range(3):
        mixed.eng.set_params(i, "actor", src[1 if i == 0 else 0].eng.get_params(i, "actor"))
    want = mixed.eng.evaluate(48, mode="mean", bench=True)
    np.testing.assert_array_equal(got["returns"], want["returns"].cpu().numpy())
    np.testing.assert_array_equal(got["bench"], want["bench"].cpu().numpy())
    # and it differs from either checkpoint playing itself
    for s in src:
        assert not np.array_equal(s.eng.evaluate(48, mode="mean")["returns"].cpu().numpy(), got["returns"])
