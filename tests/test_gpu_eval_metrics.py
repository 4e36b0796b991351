"""GPU checks of the policy-evaluation feature: libgo1eval's accumulate kernel against the fp64 model of tests/eval_ref.py on
recorded rollouts, with the reference's own fp32 expressions (METRICS_FNS evaluated by torch) as the yardstick for its
arithmetic; the group reduction's determinism and accuracy; the simulation's indifference to armed metrics; the sweep end to
end; and smoke()'s stale-binary guard for the fourth library.

Reports: with GO1_EVAL_REPORT_DIR set, the parity table and the sweep's per-step cost are also written there
(eval_metrics_parity_<terrain>.txt, eval_sweep_cost.txt: the sources of profiles/eval_metrics_parity.txt and
profiles/eval_sweep_cost.txt); they are always printed."""
import hashlib
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import eval_ref as E

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SELECTIONS = ("lin_vel_x", "ang_vel_yaw", "max_torques", "termination")      # no arithmetic: minima and maxima equal the model's
SLACK = 1e-6
DEVICE = "cuda:0"


def report(name, text):
    print("\n" + text)
    d = os.environ.get("GO1_EVAL_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "w") as f:
            f.write(text + "\n")


def make_env(N, terrain, episode_length_s, seed=0):
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


def snapshot(env):
    """clones of the SoA buffers go1eval_accumulate reads"""
    B = env.buffers
    s = {k: getattr(B, k).clone() for k in E.INPUTS if k != "measured_heights"}
    s["measured_heights"] = B.measured_heights.clone() if env.sim_config.measure_heights else None
    return s


def to_numpy(snap):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in snap.items()}


def reference_values(snap):
    """(M, N) fp64 of the reference's fp32 expressions: METRICS_FNS on the snapshot's [N, k] views, evaluated by torch on the device"""
    from go1_gym_learn.eval_metrics.metrics import METRICS_FNS, SCALAR_METRICS
    env = types.SimpleNamespace(default_body_mass=4.801)
    for k in ("base_lin_vel", "base_ang_vel", "commands", "root_states", "torques", "dof_vel"):
        setattr(env, k, snap[k].t())
    env.payloads, env.reset_buf = snap["payloads"], snap["reset_buf"].bool()
    env.measured_heights = snap["measured_heights"].t() if snap["measured_heights"] is not None else 0
    return np.stack([METRICS_FNS[n](env, None, None).double().numpy() for n in SCALAR_METRICS])


def kernel_accumulators(ev):
    torch.cuda.synchronize()
    acc = E.Accumulators(ev.num_envs)
    for k in ("count", "nonfinite"):
        setattr(acc, k, ev.acc[k].cpu().numpy().view(np.uint32).astype(np.int64))
    for k in ("sum", "sumsq", "min", "max"):
        setattr(acc, k, ev.acc[k].cpu().numpy().astype(np.float64))
    for k in ("steps", "episodes_terminated", "episodes_timed_out"):
        setattr(acc, k, ev.per_env[k].cpu().numpy().view(np.uint32).astype(np.int64))
    return acc


def distance(x, ref):
    """largest distance over the environments, relative to the largest magnitude of the quantity over the environments"""
    scale = np.abs(ref).max()
    return float(np.abs(x - ref).max() / scale) if scale > 0 else float(np.abs(x - ref).max())


def distances(acc, model):
    """per metric: the largest of the distances of the per-environment sums, sums of squares and means from the fp64 model"""
    out = []
    for m in range(E.M):
        has = model.count[m] > 0
        n = np.maximum(model.count[m], 1)
        mean_a, mean_m = np.where(has, acc.sum[m] / n, 0.0), np.where(has, model.sum[m] / n, 0.0)
        out.append(max(distance(acc.sum[m], model.sum[m]), distance(acc.sumsq[m], model.sumsq[m]), distance(mean_a, mean_m)))
    return out


def check_against_model(kernel, model, reference, title):
    """counts and selections equal; the kernel's arithmetic within 2 x the reference expression's own distance + 1e-6"""
    for k in ("count", "nonfinite", "steps", "episodes_terminated", "episodes_timed_out"):
        assert np.array_equal(getattr(kernel, k), getattr(model, k)), k
    for name in SELECTIONS:
        m = E.METRICS.index(name)
        assert np.array_equal(kernel.min[m], model.min[m]) and np.array_equal(kernel.max[m], model.max[m]), name
    d_k, d_ref = distances(kernel, model), distances(reference, model)
    lines = [title, f"{'metric':<20}{'kernel vs fp64':>16}{'torch fp32 vs fp64':>20}{'bound 2 d_ref + 1e-6':>22}"]
    for m, name in enumerate(E.METRICS):
        lines.append(f"{name:<20}{d_k[m]:>16.3e}{d_ref[m]:>20.3e}{2 * d_ref[m] + SLACK:>22.3e}")
    text = "\n".join(lines)
    for m, name in enumerate(E.METRICS):
        assert d_k[m] <= 2 * d_ref[m] + SLACK, (name, d_k[m], d_ref[m])
    return text


# ---- 6. the accumulate kernel against the model ---------------------------------------------------------------------------------------
N6, STEPS6, WARMUP6 = 512, 300, 5
# actions of scale 2 throw some robots over within an episode of 1 s (51 steps), the others time out: counted with the oracle-backed
# environment of tests/fake_sim.py (64 environments, 120 steps: 66 / 93 terminations and 126 / 108 time-outs on plane / height field)
ACTION_SCALE6, EPISODE_S6 = 2.0, 1.0


STILL6 = slice(0, 16)          # environments whose copy of base_lin_vel is zeroed on every seventh step


def rollout6(terrain):
    """The kernel runs on a COPY of the buffers it reads (a second set of tensors, refreshed from the simulator's after every
    step), so that robots standing still (a simulated robot never has exactly zero speed) can be put into the copy
    without touching anything the simulator owns."""
    import go1eval_host
    env = make_env(N6, terrain, EPISODE_S6, seed=4)
    assert bool(env.sim_config.measure_heights) == (terrain != "plane")
    group = (torch.arange(N6) % 5 - 1).to(torch.int32)                   # four groups and every fifth environment not evaluated
    staged = types.SimpleNamespace(device=env.buffers.device, **{k: getattr(env.buffers, k).clone() for k in E.INPUTS})
    ev = go1eval_host.Go1Eval(env.sim_config, staged)
    ev.arm(group, WARMUP6)
    g = torch.Generator(device=env.device).manual_seed(11)
    snaps = []
    for k in range(STEPS6):
        env.step(ACTION_SCALE6 * torch.randn(N6, 12, device=env.device, generator=g))
        for name in E.INPUTS:
            getattr(staged, name).copy_(getattr(env.buffers, name))
        if k % 7 == 3:
            staged.base_lin_vel[0:2, STILL6] = 0.0
        s = {name: getattr(staged, name).clone() for name in E.INPUTS}
        if not env.sim_config.measure_heights:
            s["measured_heights"] = None
        snaps.append(s)
        ev.accumulate()
    return env, ev, group.numpy(), snaps


@pytest.fixture(scope="module")
def plane_run():
    return rollout6("plane")


def replay(snaps):
    model, reference = E.Accumulators(N6), E.Accumulators(N6)
    for s in snaps:
        n = to_numpy(s)
        E.accumulate_snapshot(model, n, WARMUP6)
        E.accumulate(reference, reference_values(s), n["reset_buf"], n["time_out_buf"], n["episode_length_buf"], WARMUP6)
    return model, reference


def assert_eventful(model):
    cot = E.METRICS.index("CoT")
    assert model.episodes_terminated.sum() > 0 and model.episodes_timed_out.sum() > 0, "no termination / no time-out in the rollout"
    assert model.warmup_excluded > 0 and model.nonfinite[cot].sum() > 0, "no warm-up exclusion / no non-finite CoT in the rollout"
    return (f"terminations {int(model.episodes_terminated.sum())}, time-outs {int(model.episodes_timed_out.sum())}, warm-up exclusions "
            f"{model.warmup_excluded}, non-finite CoT {int(model.nonfinite[cot].sum())}")


def test_kernel_against_the_model_on_the_plane(plane_run):
    env, ev, group, snaps = plane_run
    model, reference = replay(snaps)
    events = assert_eventful(model)
    text = check_against_model(kernel_accumulators(ev), model, reference,
                               f"plane, {N6} environments, {STEPS6} steps, warm-up {WARMUP6}: {events}")
    report("eval_metrics_parity_plane.txt", text)


def test_kernel_against_the_model_on_a_height_field():
    env, ev, group, snaps = rollout6("heightfield")
    model, reference = replay(snaps)
    events = assert_eventful(model)
    text = check_against_model(kernel_accumulators(ev), model, reference,
                               f"height field with the 187-point scan, {N6} environments, {STEPS6} steps, warm-up {WARMUP6}: {events}")
    report("eval_metrics_parity_heightfield.txt", text)


# ---- 7. the reduction ---------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys, hashlib, types
sys.path[:0] = [{pkg!r}]
import numpy as np, torch
import go1eval_host as G
z = np.load({path!r})
N = int(z["group"].shape[0])
S = types.SimpleNamespace(num_envs=N, measure_heights=0)
B = types.SimpleNamespace(device=torch.device("cuda:0"))
for k in G._INPUTS:
    setattr(B, k, torch.zeros(1, device="cuda:0"))
ev = G.Go1Eval(S, B)
ev.arm(torch.from_numpy(z["group"]), 0)
for k in G._ACCUMULATORS:
    ev.acc[k].copy_(torch.from_numpy(z[k]))
for k in G._PER_ENV:
    ev.per_env[k].copy_(torch.from_numpy(z[k]))
print("TABLE", hashlib.sha256(ev.reduce().cpu().numpy().tobytes()).hexdigest())
"""


def test_reduction_is_reproducible_and_within_the_summation_bound(plane_run, tmp_path):
    env, ev, group, snaps = plane_run
    first = ev.reduce().cpu().numpy().copy()
    second = ev.reduce().cpu().numpy().copy()
    assert first.tobytes() == second.tobytes()
    res = ev.results()
    assert sorted(res) == sorted(E.METRICS + ["groups"]) and res["CoT"].tobytes() == first[:, E.METRICS.index("CoT"), :].tobytes()
    # two fresh processes, the same accumulators: the same bits
    path = str(tmp_path / "acc.npz")
    np.savez(path, group=group, **{k: v.cpu().numpy() for k, v in list(ev.acc.items()) + list(ev.per_env.items())})
    code = _CHILD.format(pkg=os.path.join(REPO, "walk-these-ways_amd"), path=path)
    digests = []
    for _ in range(2):
        out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, timeout=300).stdout
        digests.append([ln.split()[1] for ln in out.splitlines() if ln.startswith("TABLE")][0])
    assert digests[0] == digests[1] == hashlib.sha256(first.tobytes()).hexdigest()
    # against math.fsum: the textbook bound of any fp64 summation order, (k - 1) u sum|x| for k terms, over the count
    acc = kernel_accumulators(ev)
    assert np.array_equal(first, E.reduce(acc, group, 4), equal_nan=True)          # (the model's fixed order is the kernel's)
    checked = 0
    for g in range(4):
        members = np.nonzero(group == g)[0]
        assert first[g, E.M, 0] == len(members) and first[g, E.M, 1] == STEPS6 * len(members)
        assert first[g, E.M, 2] == acc.episodes_terminated[members].sum() and first[g, E.M, 3] == acc.episodes_timed_out[members].sum()
        assert first[g, E.M, 4] == (acc.episodes_terminated[members] > 0).sum() / len(members)
        for m in range(E.M):
            x = [float(acc.sum[m][e]) for e in members if acc.count[m][e] > 0]
            n = int(acc.count[m][members].sum())
            assert first[g, m, 0] == n and n > 0
            bound = (len(x) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in x) / n
            assert abs(first[g, m, 1] - math.fsum(x) / n) <= bound, (g, E.METRICS[m], first[g, m, 1], math.fsum(x) / n, bound)
            checked += 1
    assert checked == 4 * E.M


# ---- 8. the simulation does not notice -----------------------------------------------------------------------------------------------
def test_metrics_leave_the_simulation_bit_identical():
    N = 64
    envs = [make_env(N, "plane", 1.0, seed=3) for _ in range(2)]
    assert "go1eval_host" not in sys.modules or envs[0]._metrics is None
    envs[1].start_metrics(torch.arange(N) % 2, warmup_steps=3)
    envs[1].start_recording()                                      # the recorder armed at the same time
    g = torch.Generator(device=envs[0].device).manual_seed(2)
    frames = []
    for k in range(200):
        a = 1.0 * torch.randn(N, 12, device=envs[0].device, generator=g)
        for e in envs:
            e.step(a)
        if k % 25 == 24 and not frames:
            frames = envs[1].get_complete_frames()
    torch.cuda.synchronize()
    assert envs[0]._metrics is None and envs[1]._metrics is not None and envs[1]._metrics.armed
    checked = 0
    for name, t in envs[0].buffers.tensors.items():
        if t is None:
            continue
        o = envs[1].buffers.tensors[name]
        if name == "episode_log":
            # the one buffer the step kernel sums with fp32 atomics across environments (go1_maps.h: the Runner's episode statistics): its
            # last bits depend on the order the wavefronts arrive in, metrics or none.  The episode count is exact, the sums agree to
            # the rounding of an fp32 sum in another order
            log0, log1 = t.cpu().numpy(), o.cpu().numpy()
            assert log0[-1] == log1[-1] and np.allclose(log0, log1, rtol=1e-5, atol=1e-6), name
            continue
        assert t.cpu().numpy().tobytes() == o.cpu().numpy().tobytes(), name
        checked += 1
    assert checked > 30
    envs[1].stop_metrics()
    res = envs[1].read_metrics()
    assert res["groups"][:, 0].tolist() == [32.0, 32.0] and res["groups"][:, 1].tolist() == [6400.0, 6400.0]
    assert (res["lin_vel_x"][:, 0] > 0).all() and np.isfinite(res["lin_vel_x"][:, 1:5]).all()
    envs[1].step(a)                                                # disarmed: nothing is folded any more
    assert envs[1].read_metrics()["groups"][:, 1].tolist() == [6400.0, 6400.0]
    assert len(frames) > 0 and frames[0].shape == (240, 360, 4)    # and the recorder recorded an episode of env 0 meanwhile


# ---- 9. the sweep end to end -------------------------------------------------------------------------------------------------------------
def test_sweep_end_to_end():
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym_learn.eval_metrics import sweep
    from go1_gym_learn.eval_metrics.metrics import METRICS_FNS, SCALAR_METRICS
    from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
    from scripts.train_config import apply_train_config
    N, STEPS, W, SEED = 1024, 150, 10, 5
    grid = dict(vx=[0.5, 1.5], yaw=[0.0, 0.5], gait=[sweep.GAITS["trotting"], sweep.GAITS["pacing"]])
    c = apply_train_config(make_cfg(), num_envs=N).env
    torch.manual_seed(0)
    policy = ActorCritic(c.num_observations, c.num_privileged_obs, c.num_observations * c.num_observation_history, c.num_actions).to(DEVICE).eval()
    spread, cost = {}, []
    for preset in ("static_medium", "rand_large"):
        res = sweep.run_sweep(policy, preset, grid, num_envs=N, steps=STEPS, warmup_steps=W, seed=SEED)
        assert len(res["cells"]) == 8 and res["groups"][:, 0].tolist() == [128.0] * 8 and res["groups"][:, 1].tolist() == [128.0 * STEPS] * 8
        # second pass over the same seeds: the reference's functions on the host after every step, and the fp64 model
        env, _ = sweep.build_eval_env(preset, N, SEED)
        obs, group, commands = sweep.prepare(env, res["cells"])
        base = env.env
        spread[preset] = float(base.payloads.std())
        model, reference = E.Accumulators(N), E.Accumulators(N)
        with torch.inference_mode():
            for _ in range(STEPS):
                obs = sweep.policy_step(env, policy, obs, commands)
                vals = np.stack([METRICS_FNS[n](base, policy, obs).double().numpy() for n in SCALAR_METRICS])
                s = to_numpy(snapshot(base))
                E.accumulate_snapshot(model, s, W)
                E.accumulate(reference, vals, s["reset_buf"], s["time_out_buf"], s["episode_length_buf"], W)
        # robots fell and were respawned with commands drawn by the reset; every environment still carries its cell's commands
        # (those the last step reset get theirs back before the next step)
        assert model.episodes_terminated.sum() > 0, "no fall in the sweep: the check below would show nothing"
        assert sweep.commands_held(env, commands)
        last_reset = base.reset_buf.bool()
        assert torch.equal(base.commands[~last_reset], commands[~last_reset]) and int((~last_reset).sum()) > N // 2
        t_model, t_ref = E.reduce(model, group.cpu().numpy(), 8), E.reduce(reference, group.cpu().numpy(), 8)
        assert t_model[:, E.M, 2].sum() == model.episodes_terminated.sum() == res["groups"][:, 2].sum()
        table = np.concatenate([np.stack([res["metrics"][n] for n in E.METRICS], axis=1),
                                np.pad(res["groups"], ((0, 0), (0, 1)))[:, None, :]], axis=1)
        assert np.array_equal(table[:, :, 0], t_model[:, :, 0]) and np.array_equal(table[:, :, 5], t_model[:, :, 5])     # counts, non-finite
        assert np.array_equal(table[:, E.M], t_model[:, E.M], equal_nan=True)
        lines = [f"sweep {preset}: group means, kernel vs fp64 | host functions vs fp64"]
        for m, name in enumerate(E.METRICS):
            for col in (1, 2):                                        # mean, std
                d_k, d_ref = distance(table[:, m, col], t_model[:, m, col]), distance(t_ref[:, m, col], t_model[:, m, col])
                if col == 1:
                    lines.append(f"{name:<20}{d_k:>12.3e}{d_ref:>12.3e}")
                assert d_k <= 2 * d_ref + SLACK, (preset, name, col, d_k, d_ref)
            if name in SELECTIONS:
                assert np.array_equal(table[:, m, 3:5], t_model[:, m, 3:5]), name
        print("\n" + "\n".join(lines))

        # cost of a step: device events around the loop, warm (the passes above ran every kernel); no time is asserted
        def timed(hook):
            nonlocal obs
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.inference_mode():
                a.record()
                for _ in range(STEPS):
                    obs = sweep.policy_step(env, policy, obs, commands)
                    hook()
                b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * 1000.0 / STEPS
        row = [preset]
        for rep in range(2):
            row.append(timed(lambda: None))
            base.start_metrics(group, warmup_steps=W)
            row.append(timed(lambda: None))
            base.stop_metrics()
            row.append(timed(lambda: [METRICS_FNS[n](base, policy, obs) for n in SCALAR_METRICS]))
        cost.append(row)
    # the preset reached the device: rand_large draws payloads from [-1.5, 4], static_medium from [0, 0.01]
    assert spread["rand_large"] > 10 * spread["static_medium"] and spread["rand_large"] > 1.0, spread
    lines = [f"Cost of a sweep step, one MI355X, {N} environments, 2 x 2 x 2 command grid, {STEPS} steps per window, device events around the",
             "step loop (commands written, policy inference, env.step, metrics), warm, two alternated repetitions.  MEASURED; microseconds per step.",
             "", f"{'preset':<16}{'rep':>4}{'no metrics':>14}{'kernel':>14}{'host functions':>18}"]
    for row in cost:
        for rep in range(2):
            lines.append(f"{row[0]:<16}{rep + 1:>4}{row[1 + 3 * rep]:>14.1f}{row[2 + 3 * rep]:>14.1f}{row[3 + 3 * rep]:>18.1f}")
    lines += ["", "no metrics: nothing armed.  kernel: start_metrics() armed, one go1eval_accumulate launch per step, no host read.",
              "host functions: the ten scalar METRICS_FNS called after every step (each ends in a device-to-host copy)."]
    report("eval_sweep_cost.txt", "\n".join(lines))


# ---- 10. smoke() with the fourth library --------------------------------------------------------------------------------------------------
def test_smoke_guards_the_eval_library(monkeypatch):
    import __graft_entry__ as g
    g.smoke()
    monkeypatch.setattr(g, "EVAL_FLAGS", g.EVAL_FLAGS + ["-DSTALE"])        # the sources' hash no longer matches the built library's stamp
    with pytest.raises(AssertionError, match="libgo1eval.so is stale"):
        g.smoke()
