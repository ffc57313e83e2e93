"""GPU: --eval-q of experiments/train.py (with --evaluate on a saved checkpoint, and
with --eval-episodes during training, which it must leave byte for byte alone)."""
import filecmp
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

BASE = ["--scenario", "simple", "--batch-size", "64", "--max-episode-len", "5", "--buffer-size", "4096",
        "--exp-name", "t"]


def test_eval_q_in_training_and_on_the_checkpoint(tmp_path, capsys):
    """training with --eval-episodes 64 with and without --eval-q: the same prints (the
    eval_q: lines apart), pickles and checkpoint; one eval_q: line and one entry of
    t_eval_q.pkl per curve point.  Then --evaluate --eval-q on that checkpoint: the
    Engine's own evaluate_q on the loaded parameters, printed and pickled; without the
    flag the _eval.pkl has no such entry and no eval_q line is printed."""
    from experiments.train import parse_args, train

    def run(tag, extra):
        d = str(tmp_path / tag) + "/"
        train(parse_args(BASE + ["--num-envs", "64", "--num-episodes", "512", "--save-rate", "128", "--save-dir", d,
                                 "--plots-dir", d, "--eval-episodes", "64"] + extra))
        return d, capsys.readouterr().out

    d0, out0 = run("plain", [])
    d1, out1 = run("q", ["--eval-q"])
    for f in ("t_rewards.pkl", "t_agrewards.pkl", "t_eval_rewards.pkl"):
        assert filecmp.cmp(d0 + f, d1 + f, shallow=False), f
    with np.load(d0 + "maddpg_amd_state.npz") as z0, np.load(d1 + "maddpg_amd_state.npz") as z1:
        assert sorted(z0.files) == sorted(z1.files) and len(z0.files) > 8
        for k in z0.files:                        # (the .npz container itself carries timestamps)
            assert z0[k].tobytes() == z1[k].tobytes(), k
    points = len(pickle.load(open(d0 + "t_rewards.pkl", "rb")))
    assert points == 4 and "eval_q" not in out0 and not (tmp_path / "plain" / "t_eval_q.pkl").exists()
    strip = lambda out: [ln.split(", time:")[0] for ln in out.splitlines()  # noqa: E731
                         if not ln.startswith(("eval_q: ", "throughput: "))]
    assert strip(out0) == strip(out1)
    assert sum(ln.startswith("eval_q: ") for ln in out1.splitlines()) == points
    curve = pickle.load(open(d1 + "t_eval_q.pkl", "rb"))
    assert len(curve) == points and [c["train_episodes"] for c in curve] == [128, 256, 384, 512]
    assert all(c["scored"] == 5 and c["steps"] == 95 and np.isfinite(c["gap_rms"][0][0]) for c in curve)
    assert len({c["gap_mean"][0][0] for c in curve}) > 1            # the critic moved between the points

    # --evaluate on the checkpoint
    outs = {}
    for tag, extra in (("e0", []), ("e1", ["--eval-q"])):
        b = str(tmp_path / tag) + "/"
        r = train(parse_args(BASE + ["--evaluate", "--eval-episodes", "48", "--load-dir", d1, "--benchmark-dir", b,
                                     "--plots-dir", b] + extra))
        outs[tag] = (capsys.readouterr().out, pickle.load(open(b + "t_eval.pkl", "rb")), r)
    assert outs["e0"][0].splitlines() == [ln for ln in outs["e1"][0].splitlines() if not ln.startswith("eval_q ")]
    assert "eval_q" not in outs["e0"][0] and "eval_q" not in outs["e0"][1]
    out, got, r = outs["e1"]
    assert r.rounds == 0 and sum(ln.startswith("eval_q agent 0: ") for ln in out.splitlines()) == 1
    np.testing.assert_array_equal(got["returns"], outs["e0"][1]["returns"])
    want = r.eng.evaluate_q(48)
    q = got["eval_q"]
    assert (q["steps"], q["scored"], q["episodes"]) == (95, 5, 48)
    np.testing.assert_array_equal(q["gap"], want["gap"].cpu().numpy())
    for k in ("q_mean", "g_mean", "gap_mean", "gap_rms", "truncation"):
        assert q[k] == want["summary"][k], k
