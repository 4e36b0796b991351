"""GPU checks of the reward family (include/go1reward.h, libgo1reward.so): the compiled kernels on the synthetic buffers of the emulator
test against the model of tests/reward_ref.py, the family against the step kernel itself through the environment (the running
episode_sums before and after every step), `auxiliary_rewards` on the real environment, the sweep end to end, and the cost.

Figures of a run on an MI355X (profiles/reward_metrics_parity.txt holds the table): standing and scripted trot, 3840 measured env-steps each, no
reset, no teleport; for every one of the 19 terms fp32(episode_sums before + term) is episode_sums after bit for bit; total equals rew_buf
(the bound is 4 ulps of the sum of the |r_k|)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import reward_ref as R
from test_gpu_response_trace import DEVICE, StandStill, make_env, report
from test_reward_metrics import (REPO, SHAPES, STEPS, TROT_RESET_CAP, TROT_WINDOW, check_two_runs, two_runs, ulp32)
from util import make_sim

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


# ---- 9. the compiled kernels on the synthetic buffers ---------------------------------------------------------------------------------------
def gpu_sim(n):
    cfg, S, meta, B = make_sim("train", n)
    return cfg, S, meta, B.clone_to(DEVICE)


def gpu_family(S, meta, B):
    import go1reward_host as G
    return G.Go1Reward(S, B, meta["reward_names"])


@pytest.mark.parametrize("N", SHAPES)
def test_reward_kernels_against_the_model(N):
    """the emulator test's script on the device: an environment's rows do not depend on its workgroup, the bookkeeping and both group
    tables are the model's bit for bit, and every term meets the fp64 model by the parity gate's rule"""
    from test_reward_metrics import GRAVITY, WARMUP, check_against_fp64
    rng = np.random.default_rng(900 + N)
    index, runs = two_runs(rng, gpu_sim, N, gpu_family)
    check_two_runs(index, runs)
    S, posts, group, per_step = runs[0][:4]
    model = R.State(S, posts[0], WARMUP)
    for post, step in zip(posts[1:], per_step):
        view = R.step_view(post, model.snap)
        model.accumulate(post, GRAVITY)
        live = (model.last_valid != 0) & np.isfinite(post["torques"]).all(axis=0)
        if live.any():
            check_against_fp64(S, view, GRAVITY, step["last_raw"], step["last_scaled"], live, f"N={N}")


# ---- 10. against the step kernel itself, through the environment ------------------------------------------------------------------------------
def compare_with_episode_sums(env, actions, tag, between=None):
    """step the armed environment through `actions`, copying episode_sums before and after every step.  For every measured env-step and
    term k: |last_scaled[k] - (S_after - S_before)| <= ulp(max(|S_before|, |S_after|)) + 4 ulp(|last_scaled[k]|) (what the running
    sum's own rounding can hide, plus the parity gate's floor), and total equals rew_buf within 4 ulps of sum |r_k|.  Returns
    {"ulps": (K + 1,) per term the largest deviation as a share of that bound, and for total the largest deviation in ulps of sum |r_k|,
    "inexact": (K,) env-steps where fp32(S_before + last_scaled[k]) is not S_after bit for bit, "measured", "reset", "teleported", "steps"}"""
    B = env.buffers
    K, N = len(env.reward_names), env.num_envs
    worst, inexact = np.zeros(K + 1), np.zeros(K, np.int64)
    measured = reset_steps = 0
    for step, action in enumerate(actions):
        if between is not None:
            between(step)
        before = B.episode_sums.cpu().numpy().copy()
        env.step(action)
        after = B.episode_sums.cpu().numpy()
        scaled, valid = env.last_reward_terms()
        assert scaled.shape == (K + 4, N) and scaled.data_ptr() == env._reward.state["last_scaled"].data_ptr()          # views, no copy
        scaled, valid = scaled.cpu().numpy(), valid.cpu().numpy() != 0
        reset = B.reset_buf.cpu().numpy() != 0
        assert np.array_equal(~valid, reset), (tag, step)                    # skipped: exactly the env-steps with reset_buf set
        reset_steps += int(reset.sum())
        measured += int(valid.sum())
        if not valid.any():
            continue
        r = scaled[:K][:, valid].astype(f64)
        delta = after[:K][:, valid].astype(f64) - before[:K][:, valid]
        dev = np.abs(r - delta)
        hidden = ulp32(np.maximum(np.abs(before[:K][:, valid]), np.abs(after[:K][:, valid])))
        allowed = hidden + 4.0 * ulp32(r)
        assert (dev <= allowed).all(), (tag, step, env.reward_names[int(np.argmax((dev - allowed).max(axis=1)))], float((dev / allowed).max()))
        worst[:K] = np.maximum(worst[:K], (dev / allowed).max(axis=1))
        inexact += ((before[:K][:, valid] + scaled[:K][:, valid]).astype(f32) != after[:K][:, valid]).sum(axis=1)
        rew = B.rew_buf.cpu().numpy()[valid].astype(f64)
        floor = ulp32(np.abs(r).sum(axis=0))
        tdev = np.abs(scaled[K + 3][valid] - rew)
        assert (tdev <= 4.0 * floor).all(), (tag, step, "total", float((tdev / floor).max()))
        worst[K] = max(worst[K], float((tdev / floor).max()))
    res = env._reward
    return dict(ulps=worst, inexact=inexact, measured=measured, reset=reset_steps, steps=len(actions),
                teleported=int(res.state["teleported"].sum().item()))


def test_rewards_against_the_step_kernel():
    """64 environments, the train configuration on the plane.  Standing still after the settle window of the standing scenario
    (test_trunk_metrics: set down at rest, 50 steps), then the scripted trot with pauses for TROT_WINDOW steps.  The table of the
    largest deviations goes to profiles/reward_metrics_parity.txt."""
    from test_foot_metrics import standing_env
    from test_trunk_metrics import STANDING_WARMUP, set_down, trot_with_pauses
    N = 64
    group = torch.zeros(N, dtype=torch.int32)
    env = standing_env(N, DEVICE)
    env.reset()
    set_down(env)
    zero = torch.zeros(N, 12, device=DEVICE)
    for _ in range(STANDING_WARMUP):
        env.step(zero)
    assert not hasattr(env, "reward_functions")
    env.start_reward_metrics(group)
    assert not hasattr(env, "reward_functions")                              # armed, but no step accumulated yet
    stand = compare_with_episode_sums(env, [zero] * 60, "stand")
    assert len(env.reward_functions) == len(env.reward_names)
    env.stop_reward_metrics()
    res = env.read_reward_metrics()
    assert stand["reset"] == 0 and stand["teleported"] == 0 and stand["measured"] == N * 60 and res["groups"].tolist() == [[N, N * 60, 0, 0]]
    assert abs(sum(abs(v[0]) for v in res["share"].values()) - 1.0) < 1e-12 and res["total"][0, 0] == N * 60
    assert env.sim_config.only_positive_rewards_ji22_style and 0.0 <= res["total"][0, 1] <= res["positive"][0, 1]      # pos * exp(neg / sigma), neg <= 0

    env = make_env(N, "plane", 20.0, seed=4)
    env.reset()
    env.start_reward_metrics(group)
    trot = compare_with_episode_sums(env, [trot_with_pauses(step, N).to(DEVICE) for step in range(TROT_WINDOW)], "trot")
    assert trot["reset"] <= TROT_RESET_CAP * N * TROT_WINDOW and trot["teleported"] == 0 and trot["measured"] + trot["reset"] == N * TROT_WINDOW
    names = list(env.reward_names) + ["total"]
    lines = ["The reward family against the step kernel, one MI355X, 64 environments, the train configuration on the plane.  MEASURED.",
             "Per term, over the measured env-steps: the largest |last_scaled[k] - (episode_sums after - before)| as a share of its bound,",
             "ulp(max(|before|, |after|)) + 4 ulp(|last_scaled[k]|) (the first part is what the running sum's own rounding can hide), and the",
             "number of env-steps where fp32(before + last_scaled[k]) is not `after` bit for bit: 0 means the family's term is the step",
             "kernel's, bit for bit, on every measured env-step.  total: the largest |total - rew_buf| in ulps of the sum of the |r_k|",
             "(bound: 4).", "",
             f"standing still: {stand['steps']} steps, {stand['measured']} env-steps measured, {stand['reset']} reset, {stand['teleported']} teleported",
             f"scripted trot:  {trot['steps']} steps, {trot['measured']} env-steps measured, {trot['reset']} reset, {trot['teleported']} teleported", "",
             f"{'term':<34}{'stand: / bound':>16}{'not exact':>12}{'trot: / bound':>16}{'not exact':>12}"]
    for k, name in enumerate(names):
        exact = (f"{stand['inexact'][k]:>12}", f"{trot['inexact'][k]:>12}") if k < len(names) - 1 else (f"{'(ulps)':>12}", f"{'(ulps)':>12}")
        lines.append(f"{name:<34}{stand['ulps'][k]:>16.3f}{exact[0]}{trot['ulps'][k]:>16.3f}{exact[1]}")
    report("reward_metrics_parity.txt", "\n".join(lines))
    assert stand["inexact"].sum() == 0 and trot["inexact"].sum() == 0, (stand["inexact"].tolist(), trot["inexact"].tolist())
    assert stand["ulps"][-1] == 0.0 and trot["ulps"][-1] == 0.0              # and total is rew_buf: the running sums are formed as the step kernel forms them


# ---- 11. auxiliary_rewards on the real environment -------------------------------------------------------------------------------------------
def test_auxiliary_rewards_on_the_environment():
    from go1_gym_learn.eval_metrics.metrics import METRICS_FNS
    from test_trunk_metrics import trot_with_pauses
    N = 64
    env = make_env(N, "plane", 20.0, seed=4)
    env.reset()
    aux = METRICS_FNS["auxiliary_rewards"]
    with pytest.raises(NotImplementedError, match="the rewards are computed by the step kernel"):
        aux(env, None, None)
    current = torch.cuda.current_device()
    env.start_reward_metrics(torch.zeros(N, dtype=torch.int32))
    # the handle's device block lives on the buffers' device, and arming leaves the current device as it was
    assert env._reward.device_index == env.buffers.device.index == env.sim_device_id and torch.cuda.current_device() == current
    for step in range(5):
        env.step(trot_with_pauses(step, N).to(DEVICE))
    got = aux(env, None, None)
    scaled, valid = env.last_reward_terms()
    first = env.reward_names[0]
    assert list(got) == [first] and got[first].shape == (N,) and valid.all()
    assert got[first].numpy().tobytes() == scaled[0].cpu().numpy().tobytes()  # the reference's quirk: the first term only
    again = aux(env, None, None)                                             # last-step values: called twice, the same
    assert again[first].numpy().tobytes() == got[first].numpy().tobytes()
    fns = env.reward_functions
    assert len(fns) == len(env.reward_names) and all(f().shape == (N,) and f().is_cuda for f in fns)
    table = torch.stack([f() for f in fns]).cpu().numpy() * np.array([env.reward_scales[n] for n in env.reward_names], f32)[:, None]
    assert table.astype(f32).tobytes() == scaled[:len(fns)].cpu().numpy().tobytes()
    with pytest.raises(RuntimeError, match="refused while rewards is armed"):
        env.load_state(env.save_state())
    # a reset from the host between two steps: the family takes its snapshot again, and the next steps still meet the rule
    ids = torch.tensor([3, 17, 40], device=DEVICE)

    def between(step):
        if step == 1:
            env.reset_idx(ids)
    out = compare_with_episode_sums(env, [trot_with_pauses(5 + step, N).to(DEVICE) for step in range(4)], "after reset_idx", between)
    assert out["inexact"].sum() == 0 and out["measured"] + out["reset"] == 4 * N
    dof_acc = env.reward_names.index("dof_acc")
    env.reset_idx(ids)
    env.step(torch.zeros(N, 12, device=DEVICE))
    raw = env.reward_functions[dof_acc]().cpu().numpy()
    qd = env.buffers.dof_vel.cpu().numpy().astype(f64)
    want = ((qd / f64(f32(env.dt))) ** 2).sum(axis=0)                          # against a last_dof_vel of 0
    measured = env.last_reward_terms()[1].cpu().numpy() != 0
    assert measured[ids.cpu().numpy()].any()
    for e in ids.tolist():
        assert not measured[e] or abs(raw[e] - want[e]) <= 1e-5 * want[e] + 1e-6, (e, raw[e], want[e])
    env.stop_reward_metrics()
    assert not hasattr(env, "reward_functions")
    with pytest.raises(NotImplementedError, match="the rewards are computed by the step kernel"):
        aux(env, None, None)
    env.load_state(env.save_state())                                         # no longer refused


# ---- 12. the sweep end to end -------------------------------------------------------------------------------------------------------------------
class FreshPolicy:
    """a freshly initialised ActorCritic of the sizes the first observation shows"""

    def __init__(self):
        self.net = None

    def act_inference(self, obs, policy_info={}):
        if self.net is None:
            from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
            torch.manual_seed(3)
            h = obs["obs_history"]
            self.net = ActorCritic(0, obs["privileged_obs"].shape[1], h.shape[1], 12).to(h.device).eval()
        return self.net.act_inference(obs)


def test_reward_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sweep
    N, WINDOW = 64, 30
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--rewards", "--vx", "0.5", "1.0", "--envs", str(N), "--steps", str(WINDOW),
                               "--warmup-steps", "0", "--seed", "5", "--presets", "static_medium", "--terrain", "plane"])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_rewards(a, FreshPolicy(), dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits]))
    stem = str(tmp_path / "eval" / "static_medium")
    js = json.load(open(stem + "_rewards.json"))
    md = open(stem + "_rewards.md").read()
    print(md)
    assert open(stem + "_rewards.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(stem + "_rewards.png") > 5000
    K = len(js["names"])
    assert [c["vx"] for c in js["cells"]] == [0.5, 1.0] and K >= 10 and len(md.splitlines()) >= 2 + 2 + K + 8
    groups = np.array(js["reward_groups"])
    assert groups[:, 0].tolist() == [N / 2] * 2 and (groups[:, 1:].sum(axis=1) == groups[:, 0] * WINDOW).all()      # measured + reset + teleported
    assert (groups[:, 1] > 0).all()
    nan = lambda x: np.nan if x is None else x
    for g in range(2):
        shares = np.array([nan(js["share"][n][g]) for n in js["names"]])
        assert abs(np.abs(shares).sum() - 1.0) < 1e-9
        means = np.array([nan(js["terms"][n][g][1]) for n in js["names"]])
        assert abs(means.sum() - js["sum"][g][1]) <= 1e-6 * np.abs(means).sum() and js["terms"]["tracking_lin_vel"][g][1] > 0 > js["terms"]["torques"][g][1]
        assert abs(js["positive"][g][1] + js["negative"][g][1] - js["sum"][g][1]) <= 1e-6 * np.abs(means).sum()
        assert abs(js["forgiven"][g] - (js["total"][g][1] - js["sum"][g][1])) < 1e-15
        assert 0.0 <= js["total"][g][1] <= js["positive"][g][1] + 1e-15                        # the train configuration's ji22 rule: pos * exp(neg / sigma)
        assert all(js["terms"][n][g][0] == groups[g, 1] for n in js["names"])                # every term counts every measured env-step


# ---- 13. the cost -------------------------------------------------------------------------------------------------------------------------------
def test_reward_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS_, REPS = 1024, 150, 2
    env = make_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def window(armed):
        if armed:
            env.start_reward_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS_):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_reward_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS_

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_reward_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["groups"][:, 1:].sum() == ENVS * STEPS_
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    K = len(env.reward_names)
    names = ["nothing armed", "rewards armed", "read"]
    lines = [f"Cost of the reward measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS_} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  rewards armed: the same loop after start_reward_metrics(): one go1reward_accumulate launch more",
              f"per step (4 x {ENVS} lanes: the {K} active terms with the step kernel's own functions, {K + 4} accumulator rows per environment) and",
              "the host's evaluation of the step's gravity vector; its cost is the difference of the two columns.  read: read_reward_metrics()",
              f"(go1reward_reduce over 16 groups: 16 x {K + 4} table rows and 16 count rows, and the device-to-host copies of the two tables and the",
              "per-environment state), events around the call."]
    report("reward_metrics_cost.txt", "\n".join(lines))
