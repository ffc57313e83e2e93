"""GPU: experiments/train.py --continuous-actions -- a short run saves, --evaluate
loads and scores it, and --eval-episodes does not change the run."""
import filecmp
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)


def test_continuous_run_saves_evaluates_and_is_unchanged_by_eval_episodes(tmp_path, capsys):
    from experiments.train import parse_args, train
    common = ["--scenario", "simple", "--continuous-actions", "--batch-size", "64", "--max-episode-len", "5",
              "--buffer-size", "4096"]

    def run(tag, extra):
        d = str(tmp_path / tag) + "/"
        r = train(parse_args(common + ["--num-envs", "64", "--num-episodes", "512", "--save-rate", "128", "--save-dir", d,
                                       "--plots-dir", d, "--exp-name", "t"] + extra))
        return d, capsys.readouterr().out, r

    d0, out0, r0 = run("plain", [])
    assert r0.eng.act_kinds == ["box"] and r0.eng.act_dims == [2] and r0.rounds > 0
    assert r0.eng.lib.mdp_grad_variant(r0.eng.h, 0) == 0 and r0.eng.check_finite() == 0
    with np.load(d0 + "maddpg_amd_state.npz") as z:
        assert z["agent_0/actor/W3"].shape == (64, 4) and z["agent_0/critic/W1"].shape == (4 + 2, 64)
    d1, out1, _r1 = run("eval", ["--eval-episodes", "64"])
    for f in ("t_rewards.pkl", "t_agrewards.pkl"):
        assert filecmp.cmp(d0 + f, d1 + f, shallow=False), f
    with np.load(d0 + "maddpg_amd_state.npz") as z0, np.load(d1 + "maddpg_amd_state.npz") as z1:
        assert sorted(z0.files) == sorted(z1.files)
        for k in z0.files:
            assert z0[k].tobytes() == z1[k].tobytes(), k
    points = len(pickle.load(open(d0 + "t_rewards.pkl", "rb")))
    assert points == 4 and "eval:" not in out0
    assert sum(line.startswith("eval: ") for line in out1.splitlines()) == points
    strip = lambda out: [ln.split(", time:")[0] for ln in out.splitlines()  # noqa: E731
                         if not ln.startswith(("eval: ", "throughput: "))]
    assert strip(out0) == strip(out1)
    # --evaluate loads the checkpoint into a Box engine and prints its score
    bdir = str(tmp_path) + "/bench/"
    r = train(parse_args(common + ["--evaluate", "--eval-episodes", "48", "--load-dir", d0, "--benchmark-dir", bdir,
                                   "--plots-dir", bdir, "--exp-name", "x"]))
    out = capsys.readouterr().out
    assert r.rounds == 0 and out.count("mean return") == 1
    got = pickle.load(open(bdir + "x_eval.pkl", "rb"))
    assert got["returns"].shape == (48, 1) and np.isfinite(got["returns"]).all()
    want = r0.eng.evaluate(48)["returns"].cpu().numpy()
    np.testing.assert_array_equal(got["returns"], want)
    # a Discrete engine refuses the Box checkpoint
    with pytest.raises((ValueError, SystemExit), match="does not match the handle's"):
        train(parse_args([a for a in common if a != "--continuous-actions"] +
                         ["--evaluate", "--eval-episodes", "48", "--load-dir", d0, "--benchmark-dir", bdir,
                          "--plots-dir", bdir, "--exp-name", "y"]))


def test_eval_q_and_tournament_with_continuous_actions(tmp_path, capsys):
    """--evaluate --eval-q on a Box checkpoint is the Engine's own evaluate_q; the
    diagonal cells of --tournament over two simple_tag Box checkpoints are their
    plain --evaluate runs"""
    from experiments.train import parse_args, train
    tiny = ["--continuous-actions", "--batch-size", "64", "--max-episode-len", "5", "--buffer-size", "4096",
            "--plots-dir", str(tmp_path) + "/"]
    short = ["--num-envs", "64", "--num-episodes", "128", "--save-rate", "64"]
    bdir = str(tmp_path) + "/bench/"
    ev = ["--evaluate", "--eval-episodes", "48", "--benchmark-dir", bdir]
    # --eval-q
    d = str(tmp_path / "q") + "/"
    train(parse_args(["--scenario", "simple"] + tiny + short + ["--save-dir", d, "--exp-name", "q"]))
    capsys.readouterr()
    r = train(parse_args(["--scenario", "simple"] + tiny + ev + ["--eval-q", "--load-dir", d, "--exp-name", "q"]))
    out = capsys.readouterr().out
    assert r.rounds == 0 and r.eng.act_kinds == ["box"]
    assert sum(ln.startswith("eval_q agent 0: ") for ln in out.splitlines()) == 1
    q = pickle.load(open(bdir + "q_eval.pkl", "rb"))["eval_q"]
    want = r.eng.evaluate_q(48)
    assert (q["scored"], q["episodes"]) == (5, 48) and np.isfinite(q["gap"]).all()
    np.testing.assert_array_equal(q["gap"], want["gap"].cpu().numpy())
    # --tournament
    tag = ["--scenario", "simple_tag", "--num-adversaries", "3"] + tiny
    dirs = []
    for k in (0, 1):
        dk = str(tmp_path / f"ck{k}") + "/"
        rk = train(parse_args(tag + short + ["--seed", str(k), "--save-dir", dk, "--exp-name", f"c{k}"]))
        assert rk.eng.act_kinds == ["box"] * 4 and rk.eng.check_finite() == 0
        dirs.append(dk)
    capsys.readouterr()
    r = train(parse_args(tag + ev + ["--tournament"] + dirs + ["--exp-name", "t"]))
    out = capsys.readouterr().out
    assert r.rounds == 0 and out.count("tournament [") == 4
    got = pickle.load(open(bdir + "t_tournament.pkl", "rb"))
    assert got["returns"].shape == (2, 2, 48, 4) and np.isfinite(got["returns"]).all()
    assert not np.array_equal(got["returns"][0, 0], got["returns"][1, 1])
    for k in (0, 1):
        train(parse_args(tag + ev + ["--load-dir", dirs[k], "--exp-name", f"p{k}"]))
        pair = pickle.load(open(bdir + f"p{k}_eval.pkl", "rb"))
        np.testing.assert_array_equal(got["returns"][k, k], pair["returns"])
