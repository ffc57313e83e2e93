"""GPU: experiments/train.py --evaluate --tournament DIR [DIR ...] (the K x K
cross-play table in one Engine.evaluate_matchups call)."""
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)


def test_tournament_cells_are_the_pairwise_evaluate_runs(tmp_path, capsys):
    """two tiny simple_tag checkpoints A, B: cell (a, b) of --tournament A B == the
    --evaluate --load-dir b --adv-load-dir a run (the first --num-adversaries
    agents from a, the rest from b): per-episode returns and means, exactly"""
    from experiments.train import parse_args, train
    common = ["--scenario", "simple_tag", "--num-adversaries", "3", "--batch-size", "64", "--max-episode-len", "5",
              "--buffer-size", "4096", "--plots-dir", str(tmp_path) + "/"]
    dirs = []
    for k in (0, 1):
        d = str(tmp_path / f"ck{k}") + "/"
        train(parse_args(common + ["--num-envs", "64", "--num-episodes", "128", "--save-rate", "64", "--seed", str(k),
                                   "--save-dir", d, "--exp-name", f"c{k}"]))
        dirs.append(d)
    capsys.readouterr()
    bdir = str(tmp_path) + "/bench/"
    ev = ["--evaluate", "--eval-episodes", "48", "--benchmark-dir", bdir]
    r = train(parse_args(common + ev + ["--tournament"] + dirs + ["--exp-name", "t"]))
    out = capsys.readouterr().out
    assert r.rounds == 0 and out.count("tournament [") == 4 and "Loading previous state" not in out
    got = pickle.load(open(bdir + "t_tournament.pkl", "rb"))
    assert got["checkpoints"] == dirs and got["team"] == [0, 1, 2] and got["episodes"] == 48
    assert got["returns"].shape == (2, 2, 48, 4) and got["mean"].shape == got["sem"].shape == (2, 2, 4)
    assert got["side"].shape == (2, 2, 2, 2)
    for a in (0, 1):
        for b in (0, 1):
            train(parse_args(common + ev + ["--load-dir", dirs[b], "--adv-load-dir", dirs[a], "--exp-name", f"p{a}{b}"]))
            pair = pickle.load(open(bdir + f"p{a}{b}_eval.pkl", "rb"))
            np.testing.assert_array_equal(got["returns"][a, b], pair["returns"])
            r64 = np.ascontiguousarray(pair["returns"], np.float64)
            np.testing.assert_array_equal(got["mean"][a, b], r64.mean(0))
            np.testing.assert_allclose(got["mean"][a, b], pair["summary"]["mean"], rtol=1e-13)
            np.testing.assert_array_equal(got["side"][a, b, 0, 0], r64[:, :3].mean(1).mean())
            np.testing.assert_array_equal(got["side"][a, b, 1, 0], r64[:, 3:].mean(1).mean())
            assert np.all(np.isfinite(got["sem"][a, b])) and np.any(got["sem"][a, b] > 0)
    # the checkpoints differ (in 5 steps the adversaries rarely reach the good agent, so the columns tell)
    assert not np.array_equal(got["returns"][:, 0], got["returns"][:, 1])

    # another team: agent 3 from the row checkpoint is the transposed pairing of the default team
    train(parse_args(common + ev + ["--tournament"] + dirs + ["--tournament-team", "3", "--exp-name", "g"]))
    flip = pickle.load(open(bdir + "g_tournament.pkl", "rb"))
    assert flip["team"] == [3]
    np.testing.assert_array_equal(flip["returns"], got["returns"].transpose(1, 0, 2, 3))


@pytest.mark.parametrize("extra,why", [
    (["--tournament", "/x/", "/y/"], "--tournament needs --evaluate"),
    (["--evaluate", "--tournament", "/x/", "/y/", "--adv-load-dir", "/z/"], "--adv-load-dir"),
    (["--evaluate", "--tournament", "/x/", "/y/", "--num-adversaries", "0"], "team is empty"),
    (["--evaluate", "--tournament", "/x/", "/y/", "--tournament-team", "0,1,2,3"], "every agent"),
])
def test_refused_flag_combinations_exit_with_their_message(extra, why, tmp_path):
    from experiments.train import parse_args, train
    args = ["--scenario", "simple_tag", "--batch-size", "64", "--max-episode-len", "5", "--buffer-size", "4096",
            "--benchmark-dir", str(tmp_path) + "/"]
    if "--num-adversaries" not in extra:
        args += ["--num-adversaries", "3"]
    with pytest.raises(SystemExit) as e:
        train(parse_args(args + extra))
    assert why in str(e.value.code) and e.value.code != 0
    assert not list(tmp_path.iterdir())
