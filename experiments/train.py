"""MADDPG training on MI355X -- drop-in for the reference's ``experiments/train.py``.

Same flags, defaults and console lines as ``experiments/train.py:11-189``.
The loop runs on the device (``maddpg_amd.runner.VecRunner``): E copies of the
MPE scenario step per launch, experience goes straight into the device
replay, and every agent's ``update()`` runs in the reference's order at the
reference cadence (one round per 100 transitions; with E=1 -- the default --
this is exactly the reference loop).  Extra flags: ``--num-envs``, ``--seed``,
``--num-agents``/``--scenario-adversaries`` (scenario size), ``--train-every``,
``--evaluate`` / ``--eval-episodes`` / ``--eval-mode`` / ``--adv-load-dir``
(device-side policy evaluation on fixed episode ids; it leaves training untouched),
``--eval-q`` (with either: the critics' Q against the realised discounted return),
``--evaluate --tournament DIR [DIR ...]`` / ``--tournament-team`` (the cross-play
table of several checkpoints in one launch).

Episode accounting follows the reference exactly: ``len(episode_rewards)`` is
the number of finished episodes + 1 (a new 0 entry is appended at every reset,
``train.py:127-133``), the progress line is printed when that length is a
multiple of ``--save-rate`` and averages the last ``--save-rate`` entries
(including the fresh 0), and training stops once it exceeds
``--num-episodes``.  Every env copy terminates at ``--max-episode-len`` steps
(MPE scenarios have no done callback), so the episode count is known on the
host without a device sync.

    python experiments/train.py --scenario simple_spread --num-envs 1024 --exp-name spread
    python experiments/train.py --scenario simple_spread --num-envs 4096 --num-gpus 8
    torchrun --nproc-per-node 8 experiments/train.py --scenario simple_spread --num-envs 4096
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    parser = argparse.ArgumentParser("Reinforcement Learning experiments for multiagent environments")
    # Environment
    parser.add_argument("--scenario", type=str, default="simple", help="name of the scenario script")
    parser.add_argument("--max-episode-len", type=int, default=25, help="maximum episode length")
    parser.add_argument("--num-episodes", type=int, default=60000, help="number of episodes")
    parser.add_argument("--num-adversaries", type=int, default=0, help="number of adversaries")
    parser.add_argument("--good-policy", type=str, default="maddpg", help="policy for good agents")
    parser.add_argument("--adv-policy", type=str, default="maddpg", help="policy of adversaries")
    # Core training parameters
    parser.add_argument("--lr", type=float, default=1e-2, help="learning rate for Adam optimizer")
    parser.add_argument("--gamma", type=float, default=0.95, help="discount factor")
    parser.add_argument("--batch-size", type=int, default=1024, help="number of episodes to optimize at the same time")
    parser.add_argument("--num-units", type=int, default=64, help="number of units in the mlp")
    # Checkpointing
    parser.add_argument("--exp-name", type=str, default=None, help="name of the experiment")
    parser.add_argument("--save-dir", type=str, default="/tmp/policy/", help="directory in which training state and model should be saved")
    parser.add_argument("--save-rate", type=int, default=1000, help="save model once every time this many episodes are completed")
    parser.add_argument("--load-dir", type=str, default="", help="directory in which training state and model are loaded")
    # Evaluation
    parser.add_argument("--restore", action="store_true", default=False)
    parser.add_argument("--display", action="store_true", default=False)
    parser.add_argument("--benchmark", action="store_true", default=False)
    parser.add_argument("--benchmark-iters", type=int, default=100000, help="number of iterations run for benchmarking")
    parser.add_argument("--benchmark-dir", type=str, default="./benchmark_files/", help="directory where benchmark data is saved")
    parser.add_argument("--plots-dir", type=str, default="./learning_curves/", help="directory where plot data is saved")
    # MI355X build extensions
    parser.add_argument("--num-envs", type=int, default=1, help="env copies stepped together per GPU")
    parser.add_argument("--seed", type=int, default=0, help="seed of weights, index stream and device RNG")
    parser.add_argument("--num-agents", type=int, default=None, help="scenario agent count override")
    parser.add_argument("--scenario-adversaries", type=int, default=None, help="adversaries in the scenario world")
    parser.add_argument("--train-every", type=int, default=100, help="transitions per update round (maddpg.py:164)")
    parser.add_argument("--display-frames", type=int, default=100,
                        help="--display: steps rendered to PNG frames (no window on a GPU box)")
    parser.add_argument("--save-format", choices=["npz", "tf1"], default="npz",
                        help="checkpoint format: npz, or tf1 (a tf.train.Saver checkpoint with the reference's "
                             "variable names; --load-dir reads either)")
    # the reference's hard-coded constants, as flags with its values
    parser.add_argument("--tau", type=float, default=1e-2, help="Polyak rate of the target nets (maddpg.py:21)")
    parser.add_argument("--grad-clip", type=float, default=0.5, help="per-tensor clip_by_norm (maddpg.py:130,142)")
    parser.add_argument("--actor-reg", type=float, default=1e-3, help="actor logits regulariser (maddpg.py:56)")
    parser.add_argument("--buffer-size", type=int, default=int(1e6), help="replay capacity (maddpg.py:147)")
    parser.add_argument("--check-nan", action="store_true", default=False,
                        help="debug: after every training step check every parameter, Adam slot and update stat "
                             "for NaN / Inf and stop with 'Nan detected' (the reference's _Function(check_nan), "
                             "tf_util.py:322,366-368)")
    parser.add_argument("--num-gpus", type=int, default=None,
                        help="start one rank per GPU from this command (torchrun child, 127.0.0.1 rendezvous); "
                             "under torchrun it must equal WORLD_SIZE (default: torchrun's world, else 1)")
    parser.add_argument("--update-mode", choices=["strict", "throughput"], default="strict",
                        help="strict: the reference's update order; throughput: every agent's gradients from "
                             "the round-start parameters, then every optimizer step (SURVEY 8e, single GPU)")
    parser.add_argument("--prioritized-replay", action="store_true", default=False,
                        help="device-side prioritized experience replay (the reference's "
                             "prioritized_replay_buffer.py; one sum tree per agent, strict mode, one GPU)")
    parser.add_argument("--per-alpha", type=float, default=0.6, help="priority exponent (prioritized_replay_buffer.py:149)")
    parser.add_argument("--per-beta0", type=float, default=0.4, help="initial importance-sampling exponent (:150)")
    parser.add_argument("--per-beta-inc", type=float, default=0.001, help="beta increment per sample call (:151)")
    parser.add_argument("--per-eps", type=float, default=0.01, help="added to |TD error| before the clip (:148)")
    parser.add_argument("--td3", action="store_true", default=False,
                        help="MATD3: twin critics per agent, the TD target from the smaller target critic, the "
                             "policy and the target nets updated every --policy-delay-th critic step (strict "
                             "mode, one GPU, npz checkpoints; not with --prioritized-replay)")
    parser.add_argument("--policy-delay", type=int, default=2,
                        help="--td3: critic steps per policy / target update, 1..8 (1: twin critics without delay)")
    parser.add_argument("--minimax", action="store_true", default=False,
                        help="M3DDPG: in the critic target and the actor loss the other agents' actions move one "
                             "normalised gradient step against this agent's Q (strict mode, one GPU; not with "
                             "--td3 or --prioritized-replay)")
    parser.add_argument("--adv-eps", type=float, default=1e-3,
                        help="--minimax: perturbation rate for agents on the other side of --num-adversaries")
    parser.add_argument("--adv-eps-s", type=float, default=1e-5,
                        help="--minimax: perturbation rate for agents on the same side")
    parser.add_argument("--approx-policies", action="store_true", default=False,
                        help="MADDPG with inferred policies: every agent learns approximators of the other agents' "
                             "policies from replay and builds its TD target from them (strict mode, one GPU, npz "
                             "checkpoints; not with --td3, --minimax or --prioritized-replay)")
    parser.add_argument("--continuous-actions", action="store_true", default=False,
                        help="Box action spaces: every agent that moves and does not speak gets a Box(2) space and a "
                             "diagonal-Gaussian policy, its action the force itself (strict mode, one GPU; not with "
                             "--prioritized-replay, --td3, --minimax or --approx-policies)")
    parser.add_argument("--action-squash", choices=("none", "tanh"), default="none",
                        help="--continuous-actions: tanh puts every Box agent's sample through tanh, an action "
                             "inside [-1, 1] (the force a * accel is then bounded, as a Discrete(5) agent's is). "
                             "npz checkpoints record it; with a TF1 bundle give the flag again on restore")
    parser.add_argument("--entropy-alpha", type=float, default=0.0,
                        help="--continuous-actions: every Box agent's entropy coefficient (soft MADDPG: the agent "
                             "maximises its reward plus alpha times its own policy's entropy; fixed). 0: none. Each "
                             "learning-curve line is then followed by an entropy: line, the per-agent mean of -log pi. "
                             "npz checkpoints record it; with a TF1 bundle give the flag again on restore")
    parser.add_argument("--approx-lambda", type=float, default=1e-3,
                        help="--approx-policies: weight of the approximators' entropy regulariser")
    # device-side policy evaluation (whole episodes in one launch; training state untouched)
    parser.add_argument("--evaluate", action="store_true", default=False,
                        help="load as --benchmark does and score the policies on evaluation episodes 0 .. "
                             "--eval-episodes - 1 (1024 when that flag is 0); nothing trains")
    parser.add_argument("--eval-episodes", type=int, default=0,
                        help="training: score these many fixed evaluation episodes at every learning-curve point "
                             "(0: off); --evaluate: episodes to score")
    parser.add_argument("--eval-mode", choices=["sample", "mean"], default="sample",
                        help="sample: the policies act as in training (Gumbel-softmax); mean: softmax of the "
                             "logits without noise")
    parser.add_argument("--eval-q", action="store_true", default=False,
                        help="--evaluate, or training with --eval-episodes: also score the critics -- Q against the "
                             "discounted return the policies then collect on the same ids (mean and RMS gap per "
                             "agent and critic)")
    parser.add_argument("--adv-load-dir", type=str, default="",
                        help="--evaluate: take the first --num-adversaries agents from this checkpoint and the rest "
                             "from --load-dir (cross-play)")
    parser.add_argument("--tournament", type=str, nargs="+", default=[], metavar="DIR",
                        help="--evaluate: the K x K cross-play table of these checkpoints (each as --load-dir takes "
                             "it) in one launch: the row checkpoint supplies the agents of --tournament-team, the "
                             "column checkpoint the rest")
    parser.add_argument("--tournament-team", type=str, default="",
                        help="--tournament: comma-separated agent indices the row checkpoint supplies "
                             "(default: the first --num-adversaries agents)")
    return parser.parse_args(argv)


class LearningCurve:
    """The reference's episode bookkeeping (train.py:123-133, 164-189) for E env
    copies that terminate together.

    ``len(episode_rewards)`` is finished episodes + 1 (a fresh 0 entry is
    appended at every reset).  The reference, whose episodes end one at a
    time, checks ``len % save_rate == 0`` after each reset and stops once the
    length exceeds ``num_episodes``; E simultaneous terminations step the
    length by E, so every multiple of ``save_rate`` crossed -- up to the
    length the reference stops at, num_episodes + 1 -- gives one print and one
    curve point, each the mean of the last ``save_rate`` entries at that length
    (save_rate - 1 finished episodes, in env order, plus the fresh 0).
    ``read(first, count)`` returns finished episodes [first, first + count) as
    [count, 1 + n] rows (total, per agent).
    """

    def __init__(self, save_rate, num_episodes, n):
        self.save_rate, self.num_episodes, self.n = save_rate, num_episodes, n
        self.finished = 0
        self.final_ep_rewards, self.final_ep_ag_rewards = [], []

    @property
    def length(self):
        return self.finished + 1

    @property
    def done(self):
        return self.length > self.num_episodes

    def finish(self, count, read):
        """`count` episodes ended; returns [(length, mean reward, per-agent means)]
        for every save_rate multiple crossed (read=None: count only, no points)."""
        before = self.length
        self.finished += count
        last = min(self.length, self.num_episodes + 1)
        sr = self.save_rate
        marks = list(range((before // sr + 1) * sr, last + 1, sr))
        if not marks or read is None:
            return []
        lo = marks[0] - sr                       # first finished episode any window needs
        span = marks[-1] - 1 - lo
        log = read(lo, span) if span > 0 else np.zeros((0, 1 + self.n), np.float32)
        out = []
        for mk in marks:
            w = log[mk - sr - lo: mk - 1 - lo]   # episodes [mk - sr, mk - 1) + the fresh 0
            mean_ep = float(np.sum(w[:, 0], dtype=np.float64) / sr)
            mean_ag = [float(np.sum(w[:, 1 + j], dtype=np.float64) / sr) for j in range(self.n)]
            self.final_ep_rewards.append(mean_ep)
            self.final_ep_ag_rewards.extend(mean_ag)
            out.append((mk, mean_ep, mean_ag))
        return out


def benchmark(arglist, runner, exp_name, rank):
    """--benchmark (train.py:139-148): run the loaded policies, record every
    agent's scenario benchmark_data() each step, no training.  The reference
    keeps ``agent_info`` = one entry per episode, each ``[[info_n['n'] per
    step]]``; a reset appends the new entry BEFORE the step's info is stored,
    so an episode's terminal-step record opens the next entry, and the dump
    (once train_step > --benchmark-iters at a terminal step) drops the last
    entry.  With E env copies every copy keeps its own episode stream; the
    pickle lists episodes in (episode, env copy) order.  E=1 is the reference
    structure exactly."""
    from maddpg_amd.envs import bench_record
    eng, sp, n = runner.eng, runner.spec, runner.n
    E, L = arglist.num_envs, arglist.max_episode_len
    if sp.name == "simple":
        raise AttributeError("'Scenario' object has no attribute 'benchmark_data' (scenario simple)")
    if sp.name == "simple_speaker_listener":
        raise NameError("simple_speaker_listener: upstream's benchmark_data names an undefined variable "
                        "(it raises on its first call); --benchmark has nothing to record")
    open_eps = [[[]] for _ in range(E)]
    closed = []
    train_step = 0
    vec_steps = 0
    while True:
        info = eng.env_step_bench().cpu().numpy()        # [E, n, BENCH_W]
        vec_steps += 1
        train_step += E
        terminal = vec_steps % L == 0
        if terminal:
            closed.extend(open_eps)
            open_eps = [[[]] for _ in range(E)]
        for e in range(E):
            open_eps[e][0].append([bench_record(sp, info[e, i], i) for i in range(n)])
        if train_step > arglist.benchmark_iters and terminal:
            if rank == 0:
                file_name = arglist.benchmark_dir + exp_name + '.pkl'
                print('Finished benchmarking, now saving...', flush=True)
                os.makedirs(os.path.dirname(file_name) or ".", exist_ok=True)
                with open(file_name, 'wb') as fp:
                    pickle.dump(closed, fp)
            break
    runner.synchronize()
    return runner


def scenario_has_records(sp):
    return sp.name not in ("simple", "simple_speaker_listener")


def eval_q_summary(res):
    """what --eval-q keeps of Engine.evaluate_q: the summary, the window and the per-episode gaps"""
    return {"steps": res["steps"], "scored": res["scored"], "episodes": int(res["gap"].shape[0]),
            "gap": res["gap"].cpu().numpy(), **res["summary"]}


def eval_q_lines(s):
    """one line per agent: per critic the mean Q and mean return-to-go over the
    scored steps, the mean gap and its RMS over the episodes"""
    for i in range(len(s["q_mean"])):
        yield ("eval_q agent {}: mean Q {}, mean return-to-go {}, mean gap {}, rms gap {} ({} of {} steps scored, "
               "truncation {:.4f})".format(i, s["q_mean"][i], s["g_mean"][i][0], s["gap_mean"][i], s["gap_rms"][i],
                                           s["scored"], s["steps"], s["truncation"]))


def evaluate(arglist, runner, exp_name, rank):
    """--evaluate: the loaded policies play evaluation episodes [0, M) on the
    device (Engine.evaluate), M = --eval-episodes or 1024.  Prints every agent's
    mean return with its standard error and, where the scenario has
    benchmark_data, the per-episode means of the record sums; pickles returns,
    records and summary to <benchmark-dir><exp-name>_eval.pkl."""
    eng, sp, n = runner.eng, runner.spec, runner.n
    M = arglist.eval_episodes if arglist.eval_episodes > 0 else 1024
    res = eng.evaluate(M, 0, mode=arglist.eval_mode, bench=scenario_has_records(sp))
    ret = res["returns"].cpu().numpy()
    rec = None if res["bench"] is None else res["bench"].cpu().numpy()
    out = {"scenario": sp.name, "mode": arglist.eval_mode, "episodes": M, "first_episode": 0,
           "returns": ret, "bench": rec, "summary": res["summary"]}
    if rank == 0:
        for i in range(n):
            sem = res["summary"]["std"][i] / np.sqrt(M)
            print("eval agent {}: mean return {} +- {} over {} episodes".format(i, res["summary"]["mean"][i], sem, M),
                  flush=True)
        if rec is not None:
            mean_rec = rec.mean(axis=0, dtype=np.float64)
            out["bench_mean"] = mean_rec
            for i in range(n):
                print("eval agent {}: mean record sums per episode {}".format(i, mean_rec[i].tolist()), flush=True)
        if arglist.eval_q:
            out["eval_q"] = eval_q_summary(runner.evaluate_q(M, first_episode=0, mode=arglist.eval_mode))
            for line in eval_q_lines(out["eval_q"]):
                print(line, flush=True)
        file_name = arglist.benchmark_dir + exp_name + '_eval.pkl'
        os.makedirs(os.path.dirname(file_name) or ".", exist_ok=True)
        with open(file_name, 'wb') as fp:
            pickle.dump(out, fp)
    runner.synchronize()
    return runner


def tournament_flags(arglist):
    """--tournament's flag combinations, refused before anything is built"""
    if arglist.tournament and not arglist.evaluate:
        raise SystemExit("--tournament needs --evaluate")
    if arglist.tournament and arglist.adv_load_dir:
        raise SystemExit("--tournament and --adv-load-dir exclude each other (the tournament's rows are the "
                         "adversary checkpoints)")


def tournament_team(arglist, n):
    """the agents the row checkpoint supplies: --tournament-team, or the first
    --num-adversaries agents; an empty or full team is no cross-play"""
    tournament_flags(arglist)
    if arglist.tournament_team:
        try:
            team = sorted({int(x) for x in arglist.tournament_team.split(",")})
        except ValueError:
            raise SystemExit("--tournament-team: comma-separated agent indices, got {!r}".format(arglist.tournament_team))
    else:
        team = list(range(min(n, arglist.num_adversaries)))
    if any(not 0 <= a < n for a in team):
        raise SystemExit("--tournament-team {}: agent out of range for {} agents".format(team, n))
    if not team:
        raise SystemExit("--tournament: the team is empty (give --tournament-team or --num-adversaries)")
    if len(team) == n:
        raise SystemExit("--tournament: the team holds every agent, the column checkpoint would supply none")
    return team


def tournament(arglist, runner, exp_name, rank):
    """--evaluate --tournament DIR [DIR ...]: every checkpoint's team against every
    checkpoint's other agents on evaluation episodes [0, M) in one
    Engine.evaluate_matchups call.  Prints the K x K table of the team's and the
    others' mean return (the mean over the side's agents) with standard errors;
    pickles the table, the per-episode returns and the checkpoint names to
    <benchmark-dir><exp-name>_tournament.pkl."""
    eng, sp, n = runner.eng, runner.spec, runner.n
    team = tournament_team(arglist, n)
    others = [j for j in range(n) if j not in team]
    names = list(arglist.tournament)
    K = len(names)
    M = arglist.eval_episodes if arglist.eval_episodes > 0 else 1024
    bank = eng.actor_bank(K)
    for k, d in enumerate(names):
        eng.bank_write(bank, k, d)
    res = eng.cross_play(bank, team, M, 0, mode=arglist.eval_mode)
    ret = res["returns"].cpu().numpy()                     # [K, K, M, n]
    mean, sem = np.empty((K, K, n)), np.empty((K, K, n))
    side = np.empty((K, K, 2, 2))                          # [row, column, team / others, mean / standard error]
    for a in range(K):
        for b in range(K):
            r64 = np.ascontiguousarray(ret[a, b], np.float64)
            mean[a, b], sem[a, b] = r64.mean(0), r64.std(0) / np.sqrt(M)
            for q, ags in enumerate((team, others)):
                s = r64[:, ags].mean(1)
                side[a, b, q] = s.mean(), s.std() / np.sqrt(M)
    out = {"scenario": sp.name, "mode": arglist.eval_mode, "episodes": M, "first_episode": 0, "checkpoints": names,
           "team": team, "table": res["table"], "returns": ret, "mean": mean, "sem": sem, "side": side}
    if rank == 0:
        print("tournament: rows supply agents {}, columns agents {}; {} episodes".format(team, others, M), flush=True)
        for k, d in enumerate(names):
            print("tournament checkpoint {}: {}".format(k, d), flush=True)
        for a in range(K):
            for b in range(K):
                print("tournament [{}][{}]: team mean return {} +- {}, others {} +- {}".format(
                    a, b, side[a, b, 0, 0], side[a, b, 0, 1], side[a, b, 1, 0], side[a, b, 1, 1]), flush=True)
        file_name = arglist.benchmark_dir + exp_name + '_tournament.pkl'
        os.makedirs(os.path.dirname(file_name) or ".", exist_ok=True)
        with open(file_name, 'wb') as fp:
            pickle.dump(out, fp)
    runner.synchronize()
    return runner


def display(arglist, runner, exp_name, rank):
    """--display (train.py:150-154): the loaded policies act, nothing trains,
    every step is rendered.  Headless: env copy 0 is rasterised to
    <plots-dir><exp-name>_display/frame_NNNNN.png (+ positions.npz) for
    --display-frames steps (the reference loops until interrupted)."""
    from maddpg_amd.render import FrameWriter
    out = FrameWriter(os.path.join(arglist.plots_dir, exp_name + "_display"), runner.spec)
    for _ in range(arglist.display_frames):
        runner.rollout()                                   # action_n, env.step, reset at terminal
        if rank == 0:
            st = runner.eng.env_state()
            out.add(st["pos"][0], st["goal"][0])
    if rank == 0:
        print(f"Rendered {out.close()} frames to {out.dir}", flush=True)
    runner.synchronize()
    return runner


def train(arglist):
    import torch

    from maddpg_amd.parallel import init_process_group_from_env
    from maddpg_amd.runner import VecRunner

    tournament_flags(arglist)
    exp_name = arglist.exp_name if arglist.exp_name is not None else arglist.scenario
    world, rank, local = init_process_group_from_env()
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    from maddpg_amd._lib import MdpError
    from maddpg_amd.common.tf_util import per_kwargs
    per = per_kwargs(arglist)
    td3_flags(arglist, world)
    minimax_flags(arglist, world)
    approx_flags(arglist, world)
    continuous_flags(arglist, world)
    try:
        runner = _make_runner(arglist, VecRunner, world, rank, per)
    except MdpError as e:      # e.g. prioritized replay with throughput mode or several GPUs
        if not (per or arglist.td3 or arglist.minimax or arglist.approx_policies or arglist.continuous_actions):
            raise
        raise SystemExit(str(e))
    return _train(arglist, runner, exp_name, world, rank)


def _combination(flag, arglist, world):
    """each variant flag (maddpg_amd/variants.py) runs alone, in strict mode, on one
    GPU: refuse the combinations the library has no variant for before anything is built"""
    from maddpg_amd.variants import flag_refusal
    why = flag_refusal(flag, arglist, world)
    if why:
        raise SystemExit(why)


def td3_flags(arglist, world=1):
    """--td3 is MATD3, with npz checkpoints"""
    if not getattr(arglist, "td3", False):
        return
    if not 1 <= arglist.policy_delay <= 8:
        raise SystemExit("--policy-delay must be in 1..8")
    _combination("--td3", arglist, world)


def continuous_flags(arglist, world=1):
    """--continuous-actions is Box spaces; --action-squash is a setting of theirs"""
    if getattr(arglist, "action_squash", "none") != "none" and not getattr(arglist, "continuous_actions", False):
        raise SystemExit("--action-squash needs --continuous-actions")
    alpha = getattr(arglist, "entropy_alpha", 0.0) or 0.0
    if not (alpha >= 0 and alpha != float("inf")):
        raise SystemExit("--entropy-alpha must be finite and >= 0")
    if alpha and not getattr(arglist, "continuous_actions", False):
        raise SystemExit("--entropy-alpha needs --continuous-actions")
    _combination("--continuous-actions", arglist, world)


def minimax_flags(arglist, world=1):
    """--minimax is M3DDPG"""
    if not getattr(arglist, "minimax", False):
        return
    for name in ("adv_eps", "adv_eps_s"):
        v = getattr(arglist, name)
        if not (v >= 0 and v != float("inf")):
            raise SystemExit(f"--{name.replace('_', '-')} must be finite and >= 0")
    _combination("--minimax", arglist, world)


def approx_flags(arglist, world=1):
    """--approx-policies is MADDPG with inferred policies, with npz checkpoints"""
    if not getattr(arglist, "approx_policies", False):
        return
    lam = arglist.approx_lambda
    if not (lam >= 0 and lam != float("inf")):
        raise SystemExit("--approx-lambda must be finite and >= 0")
    _combination("--approx-policies", arglist, world)


def _make_runner(arglist, VecRunner, world, rank, per):
    from maddpg_amd.common.tf_util import approx_kwargs, minimax_kwargs, td3_kwargs
    runner = VecRunner(arglist.scenario, arglist.num_envs, n_agents=arglist.num_agents,
                       scenario_adversaries=arglist.scenario_adversaries,
                       num_adversaries=arglist.num_adversaries, good_policy=arglist.good_policy,
                       adv_policy=arglist.adv_policy, batch_size=arglist.batch_size,
                       num_units=arglist.num_units, lr=arglist.lr, gamma=arglist.gamma,
                       max_episode_len=arglist.max_episode_len, seed=arglist.seed,
                       train_every=arglist.train_every, world_size=world, rank=rank,
                       tau=arglist.tau, grad_clip=arglist.grad_clip, actor_reg=arglist.actor_reg,
                       capacity=arglist.buffer_size,
                       # the learning-curve windows of one terminal step span <= save_rate + E episodes
                       episode_log_rows=max(4096, 4 * arglist.num_envs, arglist.save_rate + 2 * arglist.num_envs),
                       continuous=getattr(arglist, "continuous_actions", False),
                       squash=getattr(arglist, "action_squash", "none"),
                       entropy_alpha=getattr(arglist, "entropy_alpha", 0.0),
                       **per, **td3_kwargs(arglist), **minimax_kwargs(arglist), **approx_kwargs(arglist))
    if arglist.update_mode != "strict":
        runner.eng.set_update_mode(arglist.update_mode)
    return runner


def _train(arglist, runner, exp_name, world, rank):
    n = runner.n
    num_adversaries = min(n, arglist.num_adversaries)
    say = (lambda *a: print(*a, flush=True)) if rank == 0 else (lambda *a: None)
    say('Using good policy {} and adv policy {}'.format(arglist.good_policy, arglist.adv_policy))

    if arglist.tournament:     # the checkpoints go into a bank; the handle's own parameters are never played
        return tournament(arglist, runner, exp_name, rank)
    if arglist.load_dir == "":
        arglist.load_dir = arglist.save_dir
    if arglist.restore or arglist.benchmark or arglist.display or arglist.evaluate:   # train.py:92-96
        say('Loading previous state...')
        runner.eng.load_state(arglist.load_dir)
    if arglist.evaluate:
        if arglist.adv_load_dir:     # cross-play: the adversaries of another checkpoint
            runner.eng.load_state(arglist.adv_load_dir, agents=range(num_adversaries))
        return evaluate(arglist, runner, exp_name, rank)
    if arglist.benchmark:
        return benchmark(arglist, runner, exp_name, rank)
    if arglist.display:
        return display(arglist, runner, exp_name, rank)

    E, L = arglist.num_envs, arglist.max_episode_len
    curve = LearningCurve(arglist.save_rate, arglist.num_episodes, n)
    eval_curve = []      # --eval-episodes: per curve point, every agent's mean return on the fixed ids
    eval_q_curve = []    # --eval-q: per curve point, the critics' summary on the same ids
    t_start = time.time()
    t_run = time.perf_counter()
    vec_steps = 0
    say('Starting iterations...')
    from maddpg_amd.common.tf_util import check_nan
    # one episode of every env copy (L vector steps, the steps without a round
    # included) as one graph replay; --check-nan looks after every step
    group = L if (L <= 64 and not arglist.check_nan) else 1
    while True:
        if group > 1:
            runner.steps(group)
            vec_steps += group
        else:
            if runner.step() and arglist.check_nan:
                check_nan(runner.eng)
            vec_steps += 1
            if vec_steps % L:
                continue
        # every env copy just terminated (train.py:116,127): E new episodes
        steps = vec_steps * E
        points = curve.finish(E, runner.episode_rewards if rank == 0 else None)
        if points and rank == 0:
            runner.eng.save_state(arglist.save_dir, arglist.save_format)
        for length, mean_ep, mean_ag in points:
            if rank != 0:
                break
            if num_adversaries == 0:
                print("steps: {}, episodes: {}, mean episode reward: {}, time: {}".format(
                    steps, length, mean_ep, round(time.time() - t_start, 3)), flush=True)
            else:
                print("steps: {}, episodes: {}, mean episode reward: {}, agent episode reward: {}, time: {}".format(
                    steps, length, mean_ep, mean_ag, round(time.time() - t_start, 3)), flush=True)
            if getattr(arglist, "entropy_alpha", 0.0):
                # per agent the mean of -log pi over its last actor step's batch (0: no coefficient)
                ent = [-runner.eng.entropy_info(i)["logp"] if a else 0.0
                       for i, a in enumerate(runner.eng.act_entropy)]
                print("entropy: episodes: {}, alpha: {}, mean -log pi: {}".format(
                    length, arglist.entropy_alpha, ent), flush=True)
            if arglist.approx_policies:
                # the approximators' fit on a fresh draw of replay rows (the training index stream stays put)
                aq = runner.eng.approx_quality()
                print("approx: episodes: {}, pairs: {}, mean cross-entropy: {}, mean KL: {}".format(
                    length, len(aq["pairs"]), aq["mean_ce"], aq["mean_kl"]), flush=True)
            t_start = time.time()
        if arglist.eval_episodes > 0 and rank == 0:
            # the same ids every time: checkpoints compared on identical start states
            ev = runner.evaluate(arglist.eval_episodes, 0, mode=arglist.eval_mode)["summary"] if points else None
            for length, _, _ in points:
                eval_curve.append(ev["mean"])
                print("eval: episodes: {}, eval episodes: {}, mean return: {}, std: {}".format(
                    length, arglist.eval_episodes, ev["mean"], ev["std"]), flush=True)
            if arglist.eval_q and points:
                eq = eval_q_summary(runner.evaluate_q(arglist.eval_episodes, first_episode=0, mode=arglist.eval_mode))
                del eq["gap"]
                for length, _, _ in points:
                    eval_q_curve.append(dict(eq, train_episodes=length))
                    print("eval_q: episodes: {}, eval episodes: {}, mean Q: {}, mean return-to-go: {}, mean gap: {}, "
                          "rms gap: {}".format(length, arglist.eval_episodes, eq["q_mean"],
                                               [g[0] for g in eq["g_mean"]], eq["gap_mean"], eq["gap_rms"]), flush=True)
        if curve.done:
            if rank == 0:
                os.makedirs(arglist.plots_dir, exist_ok=True)
                if arglist.eval_episodes > 0:
                    with open(arglist.plots_dir + exp_name + '_eval_rewards.pkl', 'wb') as fp:
                        pickle.dump(eval_curve, fp)
                    if arglist.eval_q:
                        with open(arglist.plots_dir + exp_name + '_eval_q.pkl', 'wb') as fp:
                            pickle.dump(eval_q_curve, fp)
                with open(arglist.plots_dir + exp_name + '_rewards.pkl', 'wb') as fp:
                    pickle.dump(curve.final_ep_rewards, fp)
                with open(arglist.plots_dir + exp_name + '_agrewards.pkl', 'wb') as fp:
                    pickle.dump(curve.final_ep_ag_rewards, fp)
            say('...Finished total of {} episodes.'.format(curve.length))
            break
    runner.synchronize()
    # SURVEY 5's counters beside the reference's prints: env-steps/s (transitions
    # of every env copy on every rank) and trainer-updates/s over the whole run
    el = time.perf_counter() - t_run
    runner.throughput = {"env_steps_per_sec": vec_steps * E * world / el,
                         "trainer_updates_per_sec": runner.rounds * n / el, "seconds": el}
    say('throughput: {:.1f} env-steps/s, {:.1f} trainer-updates/s over {:.2f} s'.format(
        runner.throughput["env_steps_per_sec"], runner.throughput["trainer_updates_per_sec"], el))
    return runner


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    arglist = parse_args(argv)
    td3_flags(arglist)
    minimax_flags(arglist)
    approx_flags(arglist)
    continuous_flags(arglist)
    if arglist.num_gpus is not None:
        from maddpg_amd.launch import rank_launch_plan, run_ranks
        plan = rank_launch_plan(arglist.num_gpus, os.environ, os.path.abspath(__file__), argv,
                                who="train.py")
        if plan is not None:          # N > 1 without torchrun: N rank processes, this one only waits
            return run_ranks(plan)
    train(arglist)
    return 0


if __name__ == '__main__':
    sys.exit(main())
