"""GPU: experiments/train.py --continuous-actions --action-squash tanh on
simple_spread -- a short run prints finite learning-curve lines and saves,
--evaluate loads and scores it; the flag alone is refused."""
import pickle
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)


def test_squashed_spread_run_saves_and_evaluates(tmp_path, capsys):
    from experiments.train import parse_args, train
    common = ["--scenario", "simple_spread", "--continuous-actions", "--action-squash", "tanh", "--batch-size", "64",
              "--max-episode-len", "5", "--buffer-size", "4096"]
    d = str(tmp_path / "run") + "/"
    r = train(parse_args(common + ["--num-envs", "64", "--num-episodes", "256", "--save-rate", "64", "--save-dir", d,
                                   "--plots-dir", d, "--exp-name", "t"]))
    out = capsys.readouterr().out
    assert r.eng.act_kinds == ["box"] * 3 and r.eng.act_squash == ["tanh"] * 3 and r.rounds > 0
    assert r.eng.check_finite() == 0
    curve = pickle.load(open(d + "t_rewards.pkl", "rb"))
    assert len(curve) == 4 and np.all(np.isfinite(curve))
    lines = [ln for ln in out.splitlines() if "mean episode reward" in ln]
    assert len(lines) == 4
    for ln in lines:
        assert "inf" not in ln and "nan" not in ln, ln
        assert np.isfinite(float(re.search(r"mean episode reward: (\S+?),", ln).group(1)))
    with np.load(d + "maddpg_amd_state.npz") as z:
        assert z["act_squash"].tolist() == [1, 1, 1] and z["agent_0/actor/W3"].shape == (64, 4)
    # --evaluate loads the checkpoint into a squashed engine and prints its score
    bdir = str(tmp_path) + "/bench/"
    ev = ["--evaluate", "--eval-episodes", "48", "--load-dir", d, "--benchmark-dir", bdir, "--plots-dir", bdir]
    r2 = train(parse_args(common + ev + ["--exp-name", "x"]))
    out = capsys.readouterr().out
    assert r2.rounds == 0 and out.count("mean return") == 3 and "inf" not in out and "nan" not in out   # one per agent
    got = pickle.load(open(bdir + "x_eval.pkl", "rb"))
    assert got["returns"].shape == (48, 3) and np.isfinite(got["returns"]).all()
    np.testing.assert_array_equal(got["returns"], r.eng.evaluate(48)["returns"].cpu().numpy())
    # without the flag the npz is refused: its actors were trained behind a tanh
    with pytest.raises((ValueError, SystemExit), match="action squash"):
        train(parse_args([a for a in common if a not in ("--action-squash", "tanh")] + ev + ["--exp-name", "y"]))


def test_action_squash_alone_is_refused(capsys):
    from experiments.train import main, parse_args, train
    with pytest.raises(SystemExit, match="--action-squash needs --continuous-actions"):
        train(parse_args(["--scenario", "simple_spread", "--action-squash", "tanh", "--num-envs", "64"]))
    with pytest.raises(SystemExit, match="--action-squash needs --continuous-actions"):
        main(["--scenario", "simple_spread", "--action-squash", "tanh", "--num-envs", "64"])
