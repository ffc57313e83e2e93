"""GPU: experiments/train.py --continuous-actions --action-squash tanh
--entropy-alpha 0.2 on simple_spread -- a short run follows every learning-curve
line with one finite entropy: line and saves the coefficients, --evaluate loads
the checkpoint; without the flag the npz is refused, and the flag alone too."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)


def test_entropy_spread_run_prints_the_entropy_line_saves_and_evaluates(tmp_path, capsys):
    from experiments.train import parse_args, train
    common = ["--scenario", "simple_spread", "--continuous-actions", "--action-squash", "tanh", "--entropy-alpha", "0.2",
              "--batch-size", "64", "--max-episode-len", "5", "--buffer-size", "4096"]
    d = str(tmp_path / "run") + "/"
    r = train(parse_args(common + ["--num-envs", "64", "--num-episodes", "256", "--save-rate", "64", "--save-dir", d,
                                   "--plots-dir", d, "--exp-name", "t"]))
    out = capsys.readouterr().out.splitlines()
    assert r.eng.act_entropy == [float(np.float32(0.2))] * 3 and r.eng.act_squash == ["tanh"] * 3 and r.rounds > 0
    assert r.eng.check_finite() == 0
    at = [k for k, ln in enumerate(out) if "mean episode reward" in ln]
    assert len(at) == 4
    for k in at:                          # each learning-curve line is followed by its entropy: line
        ln = out[k + 1]
        assert ln.startswith("entropy: episodes: ") and "alpha: 0.2" in ln, ln
        vals = [float(v) for v in re.search(r"mean -log pi: \[(.*)\]", ln).group(1).split(",")]
        assert len(vals) == 3 and np.all(np.isfinite(vals))
    assert sum(ln.startswith("entropy:") for ln in out) == 4
    with np.load(d + "maddpg_amd_state.npz") as z:
        assert z["act_entropy"].tolist() == [float(np.float32(0.2))] * 3 and z["act_squash"].tolist() == [1, 1, 1]
    bdir = str(tmp_path) + "/bench/"
    ev = ["--evaluate", "--eval-episodes", "48", "--load-dir", d, "--benchmark-dir", bdir, "--plots-dir", bdir]
    r2 = train(parse_args(common + ev + ["--exp-name", "x"]))
    out = capsys.readouterr().out
    assert r2.rounds == 0 and out.count("mean return") == 3 and "inf" not in out and "nan" not in out
    # without the flag the npz is refused: its critics estimate reward plus entropy
    with pytest.raises((ValueError, SystemExit), match="entropy coefficients"):
        train(parse_args([a for a in common if a not in ("--entropy-alpha", "0.2")] + ev + ["--exp-name", "y"]))


def test_entropy_alpha_alone_is_refused():
    from experiments.train import main, parse_args, train
    with pytest.raises(SystemExit, match="--entropy-alpha needs --continuous-actions"):
        train(parse_args(["--scenario", "simple_spread", "--entropy-alpha", "0.2", "--num-envs", "64"]))
    with pytest.raises(SystemExit, match="--entropy-alpha needs --continuous-actions"):
        main(["--scenario", "simple_spread", "--entropy-alpha", "0.2", "--num-envs", "64"])
