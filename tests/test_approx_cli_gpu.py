"""GPU: experiments/train.py --approx-policies -- the extra line per learning-curve
point, the checkpoint with the approximators, --restore and --evaluate."""
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)


def test_approx_policies_trains_saves_restores_and_evaluates(tmp_path, capsys):
    from experiments.train import parse_args, train
    d = str(tmp_path / "run") + "/"
    common = ["--scenario", "simple_spread", "--num-envs", "64", "--batch-size", "64", "--max-episode-len", "5",
              "--buffer-size", "4096", "--save-dir", d, "--plots-dir", d, "--exp-name", "a"]
    run = ["--num-episodes", "512", "--save-rate", "128"]
    train(parse_args(common + run + ["--approx-policies"]))
    out = capsys.readouterr().out
    points = len(pickle.load(open(d + "a_rewards.pkl", "rb")))
    lines = out.splitlines()
    extra = [k for k, ln in enumerate(lines) if ln.startswith("approx: ")]
    assert points == 4 and len(extra) == points
    for k in extra:                                   # each follows a learning-curve line, which is the reference's
        assert lines[k - 1].startswith("steps: ") and ", mean episode reward: " in lines[k - 1]
        assert "pairs: 6, mean cross-entropy: " in lines[k] and ", mean KL: " in lines[k]
        assert np.isfinite(float(lines[k].split("mean cross-entropy: ")[1].split(",")[0]))
    with np.load(d + "maddpg_amd_state.npz") as z:
        saved = {k: z[k] for k in z.files}
    assert "agent_0/approx_1/net/W1" in saved and "agent_2/approx_0/beta_power" in saved
    assert saved["agent_0/approx_1/beta_power"][0] < 0.9          # the approximators stepped

    # the same run without the flag prints the same lines but the extra ones (other numbers: another algorithm)
    d2 = str(tmp_path / "plain") + "/"
    train(parse_args([a if a != d else d2 for a in common] + run))
    plain = capsys.readouterr().out.splitlines()
    assert not any(ln.startswith("approx: ") for ln in plain)
    shape = lambda ls: [ln.split(":")[0] for ln in ls if not ln.startswith("approx: ")]   # noqa: E731
    assert shape(plain) == shape(lines)

    # --restore continues from the checkpoint: it loads the approximators and trains on
    train(parse_args(common + ["--num-episodes", "128", "--save-rate", "128", "--approx-policies", "--restore"]))
    out = capsys.readouterr().out
    assert "Loading previous state..." in out and out.count("approx: ") == 1
    with np.load(d + "maddpg_amd_state.npz") as z:
        assert z["agent_0/approx_1/beta_power"][0] < saved["agent_0/approx_1/beta_power"][0]
        np.savez(str(tmp_path / "keep.npz"), **{k: z[k] for k in z.files})

    # --evaluate scores the checkpoint as it scores any other: with and without the flag the same returns
    bdir = str(tmp_path) + "/bench/"
    got = []
    for tag, flag in (("e0", []), ("e1", ["--approx-policies"])):
        r = train(parse_args(common + flag + ["--evaluate", "--eval-episodes", "48", "--benchmark-dir", bdir,
                                              "--exp-name", tag]))
        assert r.rounds == 0
        got.append(pickle.load(open(bdir + tag + "_eval.pkl", "rb"))["returns"])
    assert capsys.readouterr().out.count("mean return") == 6
    assert got[0].shape == (48, 3) and np.array_equal(got[0], got[1])
    with np.load(d + "maddpg_amd_state.npz") as z, np.load(str(tmp_path / "keep.npz")) as k:
        assert all(z[n].tobytes() == k[n].tobytes() for n in k.files)     # evaluation left the checkpoint alone
