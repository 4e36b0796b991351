"""GPU checks of the behaviour table: libgo1eval's behaviour kernel against the fp64 model of tests/behaviour_ref.py on recorded
rollouts, with the fp32 host definitions (BEHAVIOUR_FNS evaluated by torch, StrideTracker in fp32) as the yardstick for its
arithmetic; the reduction's determinism and accuracy; the simulation's and the first table's indifference to the second; the
behaviour sweep end to end against a host pass; and the recorded cost of a sweep step.

Reports: with GO1_EVAL_REPORT_DIR set, the parity tables and the cost table are also written there
(behaviour_metrics_parity_<terrain>.txt, behaviour_metrics_cost.txt); they are always printed."""
import math
import os
import types

import numpy as np
import pytest
import torch

import behaviour_ref as R
import eval_ref as E

pytestmark = pytest.mark.gpu
SLACK = 1e-6                   # the slack of tests/test_gpu_eval_metrics.py's yardstick: d_kernel <= 2 d_reference + 1e-6
DEVICE = "cuda:0"


def report(name, text):
    print("\n" + text)
    d = os.environ.get("GO1_EVAL_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "w") as f:
            f.write(text + "\n")


def make_env(N, terrain, episode_length_s, seed=0):
    """the recipe of tests/test_gpu_eval_metrics.py::make_env"""
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    c = apply_train_config(make_cfg(), num_envs=N)
    t = c.terrain
    if terrain == "plane":
        t.mesh_type = "plane"
    else:                                   # the train config's tile grid with rough slopes, stairs and obstacles, and the height scan
        t.mesh_type = terrain
        t.terrain_proportions, t.curriculum, t.center_robots = [0.1, 0.1, 0.35, 0.25, 0.2], True, False
        t.num_rows, t.num_cols, t.terrain_length, t.terrain_width, t.border_size = 4, 4, 8.0, 8.0, 5.0
        t.min_init_terrain_level, t.max_init_terrain_level = 0, 3
        t.measure_heights = True
    c.env.episode_length_s = episode_length_s
    torch.manual_seed(seed)
    np.random.seed(seed)
    return VelocityTrackingEasyEnv(sim_device=DEVICE, headless=True, cfg=c)


def to_numpy(snap):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in snap.items()}


def host_env(snap, cfg):
    """an environment object with the [N, k] views BEHAVIOUR_FNS read, over a snapshot's SoA tensors"""
    N = snap["commands"].shape[1]
    env = types.SimpleNamespace(cfg=cfg, feet_indices=torch.tensor([4, 8, 12, 16], device=snap["commands"].device))
    env.commands = snap["commands"].t()[:, :cfg.commands.num_commands]
    env.root_states = snap["root_states"].t()
    env.measured_heights = snap["measured_heights"].t() if snap["measured_heights"] is not None else 0
    env.contact_forces = snap["contact_forces"].view(17, 3, N).permute(2, 0, 1)
    env.foot_positions = snap["foot_positions"].view(4, 3, N).permute(2, 0, 1)
    env.foot_velocities = snap["foot_velocities"].view(4, 3, N).permute(2, 0, 1)
    for k in ("desired_contact_states", "foot_indices", "last_actions", "last_last_actions"):
        setattr(env, k, snap[k].t())
    return env


def host_values(env):
    """(7, N) fp64 of the fp32 host definitions"""
    from go1_gym_learn.eval_metrics.behaviour import BEHAVIOUR_FNS
    return np.stack([fn(env, None, None).double().numpy() for fn in BEHAVIOUR_FNS.values()])


def fold_host_step(ref, tracker, values, snap, warmup_steps):
    """one step of the host pass into the accumulators `ref`: the per-step values as they are, the stride values from the fp32
    StrideTracker, in the kernel's order"""
    live = ~(np.asarray(snap["reset_buf"]).astype(bool) | (np.asarray(snap["episode_length_buf"]).astype(np.int64) <= warmup_steps))
    for m in R.PER_STEP:
        ref._fold(m, live, values[m])
    for e, f, freq, duty, swing in tracker.step(R.contacts(snap).T, R.foot_heights(snap).T, np.asarray(snap["commands"]).T, live):
        one = np.zeros(ref.N, bool)
        one[e] = True
        for m, v in ((R.FREQ, freq), (R.DUTY, duty), (R.SWING, swing)):
            ref._fold(m, one, np.full(ref.N, np.float64(v)))


def kernel_state(bh):
    torch.cuda.synchronize()
    st = R.State(bh.num_envs)
    for k in ("count", "nonfinite"):
        setattr(st, k, bh.acc[k].cpu().numpy().view(np.uint32).astype(np.int64))
    for k in ("sum", "sumsq", "min", "max"):
        setattr(st, k, bh.acc[k].cpu().numpy().astype(np.float64))
    for k in ("prev_contact", "stride_steps", "stance_steps"):
        setattr(st, k, bh.stride[k].cpu().numpy().astype(np.int64))
    st.swing_peak = bh.stride["swing_peak"].cpu().numpy().astype(np.float64)
    return st


def distance(x, ref):
    """largest distance over the environments, relative to the largest magnitude of the quantity over the environments"""
    scale = np.abs(ref).max()
    return float(np.abs(x - ref).max() / scale) if scale > 0 else float(np.abs(x - ref).max())


def distances(acc, model):
    """per metric: the largest of the distances of the per-environment sums, sums of squares and means from the fp64 model"""
    out = []
    for m in range(R.M):
        has = model.count[m] > 0
        n = np.maximum(model.count[m], 1)
        mean_a, mean_m = np.where(has, acc.sum[m] / n, 0.0), np.where(has, model.sum[m] / n, 0.0)
        out.append(max(distance(acc.sum[m], model.sum[m]), distance(acc.sumsq[m], model.sumsq[m]), distance(mean_a, mean_m)))
    return out


def check_against_model(kernel, model, reference, title, report_name):
    """counts, stride state and contact_match equal; the kernel's arithmetic within 2 x the host definition's own distance + 1e-6.
    The table of both distances is reported before anything about it is asserted."""
    for k in ("count", "nonfinite", "prev_contact", "stride_steps", "stance_steps", "swing_peak"):
        assert np.array_equal(getattr(kernel, k), getattr(model, k)), k
    assert np.array_equal(reference.count, model.count) and np.array_equal(reference.nonfinite, model.nonfinite)
    for k in ("sum", "sumsq", "min", "max"):
        assert np.array_equal(getattr(kernel, k)[0], getattr(model, k)[0]), ("contact_match", k)
    d_k, d_ref = distances(kernel, model), distances(reference, model)
    lines = [title, f"{'metric':<20}{'kernel vs fp64':>16}{'host fp32 vs fp64':>20}{'bound 2 d_ref + 1e-6':>22}"]
    for m, name in enumerate(R.METRICS):
        lines.append(f"{name:<20}{d_k[m]:>16.3e}{d_ref[m]:>20.3e}{2 * d_ref[m] + SLACK:>22.3e}")
    report(report_name, "\n".join(lines))
    for m, name in enumerate(R.METRICS):
        assert d_k[m] <= 2 * d_ref[m] + SLACK, (name, d_k[m], d_ref[m])


# ---- 1. the kernel against the model on recorded rollouts -------------------------------------------------------------------------------
N1, STEPS1, WARMUP1 = 192, 150, 5
ACTION_SCALE1, EPISODE_S1 = 2.0, 1.0          # the regime of tests/test_gpu_eval_metrics.py: robots fall, the others time out after 1 s
ZERO_HZ1 = slice(0, 8)                        # environments whose copy of the commanded step frequency is zeroed on every seventh step


def rollout1(terrain):
    """the kernel runs on a COPY of the buffers it reads, refreshed from the simulator's after every step, so that a 0 Hz command
    (a non-finite raibert_heuristic) can be put into the copy without touching anything the simulator owns"""
    import go1eval_host
    env = make_env(N1, terrain, EPISODE_S1, seed=4)
    assert bool(env.sim_config.measure_heights) == (terrain != "plane")
    group = (torch.arange(N1) % 5 - 1).to(torch.int32)                   # four groups and every fifth environment not evaluated
    staged = types.SimpleNamespace(device=env.buffers.device, **{k: getattr(env.buffers, k).clone() for k in R.INPUTS})
    bh = go1eval_host.Go1Behaviour(env.sim_config, staged, env.dt)
    bh.arm(group, WARMUP1)
    g = torch.Generator(device=env.device).manual_seed(11)
    snaps, events = [], dict(terminated=0, timed_out=0)
    for k in range(STEPS1):
        env.step(ACTION_SCALE1 * torch.randn(N1, 12, device=env.device, generator=g))
        for name in R.INPUTS:
            getattr(staged, name).copy_(getattr(env.buffers, name))
        if k % 7 == 3:
            staged.commands[4, ZERO_HZ1] = 0.0
        s = {name: getattr(staged, name).clone() for name in R.INPUTS}
        if not env.sim_config.measure_heights:
            s["measured_heights"] = None
        s["time_out_buf"] = env.buffers.time_out_buf.clone()
        snaps.append(s)
        bh.accumulate()
    return env, bh, group.numpy(), snaps


def replay(env, snaps):
    from go1_gym_learn.eval_metrics.behaviour import StrideTracker
    S = env.sim_config
    model, reference = R.State(N1), R.State(N1)
    tracker = StrideTracker(N1, env.dt, dtype=np.float32)
    terminated = timed_out = 0
    for s in snaps:
        n = to_numpy(s)
        reset, tout = n["reset_buf"].astype(bool), n.pop("time_out_buf").astype(bool)
        terminated, timed_out = terminated + int((reset & ~tout).sum()), timed_out + int((reset & tout).sum())
        R.accumulate_snapshot(model, n, WARMUP1, env.dt, int(S.num_commands), float(S.base_height_target))
        fold_host_step(reference, tracker, host_values(host_env({k: v for k, v in s.items() if k != "time_out_buf"}, env.cfg)), n, WARMUP1)
    return model, reference, terminated, timed_out


def assert_eventful(model, terminated, timed_out):
    assert model.completed_strides >= 1000, model.completed_strides
    assert terminated >= 1 and timed_out >= 1, "no termination / no time-out in the rollout"
    assert model.excluded > terminated + timed_out, "no warm-up exclusion in the rollout"
    assert model.double_touchdowns >= 1 and model.discarded_strides >= 1
    assert model.nonfinite[R.METRICS.index("raibert_heuristic")].sum() > 0
    return (f"completed strides {model.completed_strides}, discarded {model.discarded_strides}, double touchdowns {model.double_touchdowns}, "
            f"terminations {terminated}, time-outs {timed_out}, warm-up exclusions {model.excluded - terminated - timed_out}, "
            f"non-finite raibert_heuristic {int(model.nonfinite[4].sum())}")


@pytest.fixture(scope="module")
def plane_run():
    return rollout1("plane")


def test_behaviour_kernel_against_the_model_on_the_plane(plane_run):
    env, bh, group, snaps = plane_run
    model, reference, terminated, timed_out = replay(env, snaps)
    events = assert_eventful(model, terminated, timed_out)
    check_against_model(kernel_state(bh), model, reference, f"plane, {N1} environments, {STEPS1} steps, warm-up {WARMUP1}: {events}",
                        "behaviour_metrics_parity_plane.txt")


def test_behaviour_kernel_against_the_model_on_a_height_field():
    env, bh, group, snaps = rollout1("heightfield")
    model, reference, terminated, timed_out = replay(env, snaps)
    events = assert_eventful(model, terminated, timed_out)
    check_against_model(kernel_state(bh), model, reference,
                        f"height field with the 187-point scan, {N1} environments, {STEPS1} steps, warm-up {WARMUP1}: {events}",
                        "behaviour_metrics_parity_heightfield.txt")


# ---- 2. the reduction -----------------------------------------------------------------------------------------------------------------------
def test_behaviour_reduction_is_reproducible_and_within_the_summation_bound(plane_run):
    import go1eval_host as G
    env, bh, group, snaps = plane_run
    first = bh.reduce().cpu().numpy().copy()
    second = bh.reduce().cpu().numpy().copy()
    assert first.shape == (4, R.M, 6) and first.tobytes() == second.tobytes()
    res = bh.results()
    assert list(res) == G.BEHAVIOUR_NAMES and res["duty_factor_err"].tobytes() == first[:, R.DUTY, :].tobytes()
    st = kernel_state(bh)
    assert np.array_equal(first, R.reduce(st, group, 4), equal_nan=True)             # (the model's fixed order is the kernel's)
    # against math.fsum: the textbook bound of any fp64 summation order, (k - 1) u sum|x| for k terms, over the count
    checked = 0
    for g in range(4):
        members = np.nonzero(group == g)[0]
        for m in range(R.M):
            x = [float(st.sum[m][e]) for e in members if st.count[m][e] > 0]
            n = int(st.count[m][members].sum())
            assert first[g, m, 0] == n and n > 0
            bound = (len(x) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in x) / n
            assert abs(first[g, m, 1] - math.fsum(x) / n) <= bound, (g, R.METRICS[m], first[g, m, 1], math.fsum(x) / n, bound)
            checked += 1
    assert checked == 4 * R.M


# ---- 3. neither the simulation nor the first table notices -----------------------------------------------------------------------------------
def test_behaviour_table_leaves_the_simulation_and_the_ten_metrics_bit_identical():
    import go1eval_host as G
    N, STEPS = 64, 30
    unarmed, ten, both = [make_env(N, "plane", 1.0, seed=3) for _ in range(3)]
    groups = torch.arange(N) % 2
    ten.start_metrics(groups, warmup_steps=3)
    both.start_metrics(groups, warmup_steps=3, behaviour=True)
    assert unarmed._behaviour is None and ten._behaviour is None and both._behaviour is not None and both._behaviour.armed
    g = torch.Generator(device=unarmed.device).manual_seed(2)
    for k in range(STEPS):
        a = 1.0 * torch.randn(N, 12, device=unarmed.device, generator=g)
        for e in (unarmed, ten, both):
            e.step(a)
    torch.cuda.synchronize()
    checked = 0
    for name, t in unarmed.buffers.tensors.items():
        if t is None:
            continue
        o = both.buffers.tensors[name]
        if name == "episode_log":
            # the one buffer the step kernel sums with fp32 atomics across environments: its last bits depend on the order the
            # wavefronts arrive in, metrics or none (tests/test_gpu_eval_metrics.py treats it the same way)
            log0, log1 = t.cpu().numpy(), o.cpu().numpy()
            assert log0[-1] == log1[-1] and np.allclose(log0, log1, rtol=1e-5, atol=1e-6), name
            continue
        assert t.cpu().numpy().tobytes() == o.cpu().numpy().tobytes(), name
        checked += 1
    assert checked > 30
    for e in (ten, both):
        e.stop_metrics()
    plain, full = ten.read_metrics(), both.read_metrics()
    assert list(plain) == G.METRIC_NAMES + ["groups"]                                  # the keys of a measurement without the second table
    assert list(full) == G.METRIC_NAMES + ["groups", "behaviour"] and list(full["behaviour"]) == G.BEHAVIOUR_NAMES
    for k in plain:
        assert plain[k].tobytes() == full[k].tobytes(), k
    assert full["groups"][:, 1].tolist() == [32.0 * STEPS] * 2
    per_step = full["behaviour"]["contact_match"][:, 0]
    assert (per_step > 0).all() and (per_step == full["lin_vel_x"][:, 0]).all()        # the same steps count for both tables
    assert np.isfinite(full["behaviour"]["orientation_err"][:, 1:5]).all() and (full["behaviour"]["contact_match"][:, 4] <= 1.0).all()
    both.step(a)                                                                       # disarmed: nothing is folded any more
    assert both.read_metrics()["behaviour"]["contact_match"].tobytes() == full["behaviour"]["contact_match"].tobytes()
    both.start_metrics(groups, warmup_steps=3)                                         # a new measurement without the second table reads none
    both.step(a)
    assert list(both.read_metrics()) == G.METRIC_NAMES + ["groups"]


# ---- 4. the behaviour sweep end to end, and what it costs ----------------------------------------------------------------------------------
def fresh_policy(num_envs):
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
    from scripts.train_config import apply_train_config
    c = apply_train_config(make_cfg(), num_envs=num_envs).env
    torch.manual_seed(0)
    return ActorCritic(c.num_observations, c.num_privileged_obs, c.num_observations * c.num_observation_history, c.num_actions).to(DEVICE).eval()


def live_snapshot(base):
    B = base.buffers
    s = {k: getattr(B, k) for k in R.INPUTS if k != "measured_heights"}
    s["measured_heights"] = B.measured_heights if base.sim_config.measure_heights else None
    return s


def host_pass_step(base, tracker, warmup_steps):
    """what a host-side evaluation does after a step: the seven definitions (each ends in a device-to-host copy) and the stride
    tracker on the host's copies of the contacts, the foot heights and the commands"""
    from go1_gym_learn.eval_metrics.behaviour import BEHAVIOUR_FNS, foot_contacts
    values = [fn(base, None, None) for fn in BEHAVIOUR_FNS.values()]
    live = ~(base.reset_buf.bool() | (base.episode_length_buf <= warmup_steps))
    events = tracker.step(foot_contacts(base).cpu().numpy(), base.foot_positions[:, :, 2].cpu().numpy(), base.commands.cpu().numpy(),
                          live.cpu().numpy())
    return values, events


def test_behaviour_sweep_end_to_end():
    from go1_gym_learn.eval_metrics import behaviour as BH
    from go1_gym_learn.eval_metrics import sweep
    N, STEPS, W, SEED, PRESET = 256, 60, 5, 5, "static_medium"
    axes = dict(frequency=[2, 4], footswing_height=[0.05, 0.15])
    policy = fresh_policy(N)
    res = BH.run_behaviour_sweep(policy, PRESET, axes, num_envs=N, steps=STEPS, warmup_steps=W, seed=SEED)
    assert res["cells"] == BH.behaviour_cells(axes) and len(res["cells"]) == 4
    assert res["groups"][:, 0].tolist() == [64.0] * 4 and res["groups"][:, 1].tolist() == [64.0 * STEPS] * 4
    assert sorted(res["behaviour"]) == sorted(R.METRICS) and sorted(res["metrics"]) == sorted(E.METRICS)
    # the same seeded rollout again: the host definitions and the stride tracker after every step, and the fp64 model
    env, _ = sweep.build_eval_env(PRESET, N, SEED)
    obs, group, commands = BH.prepare(env, res["cells"])
    base = env.env
    assert commands[:, 4].tolist() == [2.0, 2.0, 4.0, 4.0] * 64 and torch.allclose(commands[:4, 9], torch.tensor([0.05, 0.15, 0.05, 0.15], device=DEVICE))
    S = base.sim_config
    model, reference = R.State(N), R.State(N)
    tracker = BH.StrideTracker(N, base.dt, dtype=np.float32)
    with torch.inference_mode():
        for _ in range(STEPS):
            obs = sweep.policy_step(env, policy, obs, commands)
            n = to_numpy(live_snapshot(base))
            R.accumulate_snapshot(model, n, W, base.dt, int(S.num_commands), float(S.base_height_target))
            fold_host_step(reference, tracker, np.stack([fn(base, None, None).double().numpy() for fn in BH.BEHAVIOUR_FNS.values()]), n, W)
    assert sweep.commands_held(env, commands)
    assert model.completed_strides > 0, "no stride completed in the sweep: the stride rows below would show nothing"
    gnp = group.cpu().numpy()
    t_model, t_ref = R.reduce(model, gnp, 4), R.reduce(reference, gnp, 4)
    table = np.stack([res["behaviour"][n] for n in R.METRICS], axis=1)
    assert np.array_equal(table[:, :, 0], t_model[:, :, 0]) and np.array_equal(table[:, :, 5], t_model[:, :, 5])     # counts, non-finite
    assert np.array_equal(t_ref[:, :, 0], t_model[:, :, 0])
    assert np.array_equal(table[:, 0], t_model[:, 0])                                                               # contact_match
    lines = [f"behaviour sweep {PRESET}: group means, kernel vs fp64 | host pass vs fp64"]
    for m, name in enumerate(R.METRICS):
        d_k, d_ref = distance(table[:, m, 1], t_model[:, m, 1]), distance(t_ref[:, m, 1], t_model[:, m, 1])
        lines.append(f"{name:<20}{d_k:>12.3e}{d_ref:>12.3e}")
        assert d_k <= 2 * d_ref + SLACK, (name, d_k, d_ref)
    print("\n" + "\n".join(lines))
    print("\n" + BH.behaviour_markdown_table(res))


def test_behaviour_cost_is_recorded():
    """no time is asserted: the four configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    from go1_gym_learn.eval_metrics import behaviour as BH
    from go1_gym_learn.eval_metrics import sweep
    N, STEPS, W, SEED, PRESET, REPS = 1024, 150, 10, 5, "static_medium", 2
    cells = BH.behaviour_cells(dict(frequency=[2, 4], footswing_height=[0.05, 0.15]))
    policy = fresh_policy(N)
    env, _ = sweep.build_eval_env(PRESET, N, SEED)
    obs, group, commands = BH.prepare(env, cells)
    base = env.env
    tracker = BH.StrideTracker(N, base.dt, dtype=np.float32)

    def timed(steps, hook=lambda: None):
        nonlocal obs
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.inference_mode():
            a.record()
            for _ in range(steps):
                obs = sweep.policy_step(env, policy, obs, commands)
                hook()
            b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / steps

    def armed(steps, behaviour):
        base.start_metrics(group, warmup_steps=W, behaviour=behaviour)
        t = timed(steps)
        base.stop_metrics()
        return t
    configurations = [("nothing armed", timed), ("ten metrics", lambda steps: armed(steps, False)), ("both tables", lambda steps: armed(steps, True)),
                      ("host pass", lambda steps: timed(steps, lambda: host_pass_step(base, tracker, W)))]
    for _, run in configurations:               # warm: every kernel and every host path once, outside the timed windows
        run(10)
    rows = [[run(STEPS) for _, run in configurations] for _ in range(REPS)]
    assert all(t > 0 for row in rows for t in row)
    lines = [f"Cost of a behaviour-sweep step, one MI355X, {N} environments, {PRESET}, 2 x 2 command cells, {STEPS} steps per window, device events",
             "around the step loop (commands written, policy inference, env.step, metrics), warm, the four configurations in alternation.",
             "MEASURED; microseconds per step.", "", f"{'rep':>4}" + "".join(f"{name:>16}" for name, _ in configurations)]
    lines += [f"{r + 1:>4}" + "".join(f"{t:>16.1f}" for t in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: no metrics.  ten metrics: start_metrics(), one go1eval_accumulate launch per step.  both tables:",
              "start_metrics(behaviour=True), go1eval_accumulate and go1eval_behaviour_accumulate per step; no host read in either.",
              "host pass: the seven BEHAVIOUR_FNS and the StrideTracker called on the host after every step (nine device-to-host copies)."]
    report("behaviour_metrics_cost.txt", "\n".join(lines))
