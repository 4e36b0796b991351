"""GPU checks of the trace and the step response: go1eval_trace_record against the simulator's buffers and the two tables' models
on real rollouts (plane and height field, all environments and a subset), go1eval_response / go1eval_response_reduce against the
model of tests/response_ref.py bit for bit on uploaded synthetic traces, the full ring, the simulation's and the two tables'
indifference to an armed trace, the response sweep end to end against a host pass, and the recorded cost of a traced step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (response_trace_cost.txt: the source of
profiles/response_trace_cost.txt); it is always printed."""
import os
import types

import numpy as np
import pytest
import torch

import response_ref as P

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


def snapshot(env):
    """clones of the SoA buffers go1eval_trace_record reads"""
    B = env.buffers
    s = {k: getattr(B, k).clone() for k in P.INPUTS if k != "measured_heights"}
    s["measured_heights"] = B.measured_heights.clone() if env.sim_config.measure_heights else None
    return s


def to_numpy(snap):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in snap.items()}


def reference_values(snap):
    """{channel: (N,) fp64} of the reference's fp32 expressions for base_height and power_consumption: METRICS_FNS on the
    snapshot's [N, k] views, evaluated by torch on the device (tests/test_gpu_eval_metrics.py::reference_values)"""
    from go1_gym_learn.eval_metrics.metrics import METRICS_FNS
    env = types.SimpleNamespace(default_body_mass=4.801)
    for k in ("base_lin_vel", "base_ang_vel", "commands", "root_states", "torques", "dof_vel"):
        setattr(env, k, snap[k].t())
    env.measured_heights = snap["measured_heights"].t() if snap["measured_heights"] is not None else 0
    return {P.BASE_HEIGHT: METRICS_FNS["base_height"](env, None, None).double().numpy(),
            P.POWER: METRICS_FNS["power_consumption"](env, None, None).double().numpy()}


def distance(x, ref):
    """largest distance over the rows and environments, relative to the largest magnitude of the quantity (the two tables' tests)"""
    scale = np.abs(ref).max()
    return float(np.abs(x - ref).max() / scale) if scale > 0 else float(np.abs(x - ref).max())


def stack(trace):
    """(rows, 24, K) from a read_trace() result"""
    return np.stack([trace[name] for name in P.CHANNELS], axis=1)


SUBSET = [0, 199, 64, 63, 7]
COPIES = [0, 1, 2, 6, 7, 8, 9, P.RESET] + list(range(12, 24))        # channels that are one buffer element each (channel 9: one fp32 add)


def traced_rollout(N, terrain, steps, subset, seed=6):
    """zero actions; one trace of every environment, and one of `subset` from a second environment built with the same seed"""
    full, part = make_env(N, terrain, 20.0, seed), make_env(N, terrain, 20.0, seed)
    assert bool(full.sim_config.measure_heights) == (terrain != "plane")
    full.start_trace(capacity=steps)
    part.start_trace(subset, capacity=steps)
    snaps = []
    zero = torch.zeros(N, 12, device=DEVICE)
    for _ in range(steps):
        full.step(zero)
        part.step(zero)
        snaps.append(snapshot(full))                                     # the buffers after the step, read on the host below
    full.stop_trace()
    part.stop_trace()
    return full, snaps, full.read_trace(), part.read_trace()


def check_trace_against_the_buffers(env, snaps, trace, part, subset, title):
    N, steps = env.num_envs, len(snaps)
    assert trace["rows"] == part["rows"] == steps and not trace["truncated"] and not part["truncated"]
    assert trace["env_ids"].tolist() == list(range(N)) and part["env_ids"].tolist() == subset
    got = stack(trace)
    assert got.shape == (steps, 24, N) and got.dtype == np.float32
    target = float(env.sim_config.base_height_target)
    model = np.stack([P.trace_row(to_numpy(s), None, target, rounded=False) for s in snaps])         # fp64
    exact = np.stack([P.trace_row(to_numpy(s), None, target) for s in snaps])                        # the header's roundings
    for c in COPIES + [P.CONTACT_MATCH, P.MAX_TORQUES]:                  # equal to the buffers / to the model: no arithmetic to round
        assert got[:, c].tobytes() == exact[:, c].tobytes(), P.CHANNELS[c]
        assert np.array_equal(got[:, c].astype(np.float64), model[:, c]) or c == 9, P.CHANNELS[c]
    assert got[:, 0].tobytes() == np.stack([s["base_lin_vel"][0].cpu().numpy() for s in snaps]).tobytes()
    assert got[:, 23].tobytes() == np.stack([s["dof_pos"][11].cpu().numpy() for s in snaps]).tobytes()
    assert np.abs(got[:, 12:24]).max() > 0.1 and np.abs(got[:, P.POWER]).max() > 0 and len(np.unique(got[:, P.CONTACT_MATCH])) >= 2
    # base_height and power_consumption: the kernel's distance from the fp64 model within twice the reference expression's own + 1e-6
    ref = {c: np.stack([reference_values(s)[c] for s in snaps]) for c in (P.BASE_HEIGHT, P.POWER)}
    lines = [title, f"{'channel':<20}{'kernel vs fp64':>16}{'torch fp32 vs fp64':>20}{'bound 2 d_ref + 1e-6':>22}"]
    worst = {}
    for c in (P.BASE_HEIGHT, P.POWER):
        worst[c] = (distance(got[:, c].astype(np.float64), model[:, c]), distance(ref[c], model[:, c]))
        lines.append(f"{P.CHANNELS[c]:<20}{worst[c][0]:>16.3e}{worst[c][1]:>20.3e}{2 * worst[c][1] + SLACK:>22.3e}")
    print("\n" + "\n".join(lines))
    for c, (d_k, d_ref) in worst.items():
        assert d_k <= 2 * d_ref + SLACK, (P.CHANNELS[c], d_k, d_ref)
    # the subset trace: the matching columns of the full one
    sub = stack(part)
    assert sub.shape == (steps, 24, len(subset)) and sub.tobytes() == np.ascontiguousarray(got[:, :, subset]).tobytes()


def test_trace_against_the_buffers_on_the_plane():
    env, snaps, trace, part = traced_rollout(200, "plane", 40, SUBSET)
    check_trace_against_the_buffers(env, snaps, trace, part, SUBSET, "trace on the plane, 200 environments, 40 steps, zero actions")


def test_trace_against_the_buffers_on_a_height_field():
    subset = [0, 95, 64, 63, 7]
    env, snaps, trace, part = traced_rollout(96, "heightfield", 20, subset)
    assert snaps[0]["measured_heights"] is not None and snaps[0]["measured_heights"].shape[0] > 1
    check_trace_against_the_buffers(env, snaps, trace, part, subset, "trace on a height field with the height scan, 96 environments, 20 steps")


# ---- the analysis on uploaded traces -----------------------------------------------------------------------------------------------------
def uploaded_trace(trace):
    """a Go1Trace that holds `trace` (rows, 24, K) as if it had recorded it: the analysis is a pure function of the trace"""
    import go1eval_host as G
    rows, _, K = trace.shape
    S = types.SimpleNamespace(num_envs=K, measure_heights=0, base_height_target=0.3)
    B = types.SimpleNamespace(device=torch.device(DEVICE), **{k: torch.zeros(1, device=DEVICE) for k in G._TRACE_INPUTS})
    tr = G.Go1Trace(S, B)
    tr.arm(None, capacity=rows)
    tr.trace.copy_(torch.from_numpy(trace))
    tr.rows = rows
    return tr


def test_response_and_reduce_equal_the_model_bit_for_bit():
    K, rows, s0, pre, w, hold, tail, groups, band, dt = 300, 80, 30, 20, 17, 10, 10, 3, 0.1, 0.02
    rng = np.random.default_rng(23)
    trace, kind = P.synthetic_traces(rng, K, rows, s0, pre)
    group = rng.integers(-1, groups + 1, K).astype(np.int32)
    group[group == groups] = -1                                           # (Go1Trace sizes the table by the largest id)
    names = ["lin_vel_x", "ang_vel_yaw", "base_height", "contact_match", "lin_vel_y"]
    signals = {n: (y, r, target, scale) for n, (y, r, target, scale) in zip(names, P.SIGNALS)}
    tr = uploaded_trace(trace)
    first = tr.response(signals, s0, pre, w, band, hold, tail, dt, group)
    second = tr.response(signals, s0, pre, w, band, hold, tail, dt, group)
    want_values, want_status = P.response(trace, P.SIGNALS, s0, pre, w, band, hold, tail, dt)
    want_table = P.response_reduce(want_values, want_status, group, groups)
    assert np.array_equal(first["status"], want_status) and {0, 1, 2} <= set(want_status.tolist())
    assert (want_status[kind == 5] == 1).all() and (want_status[kind == 7] == 2).all()
    for s, name in enumerate(names):
        for m, metric in enumerate(P.VALUES):
            v = first["values"][name][metric]
            assert v.dtype == np.float32 and np.array_equal(np.isnan(v), np.isnan(want_values[s, m])), (name, metric)
            assert v.tobytes() == want_values[s, m].tobytes(), (name, metric)
            assert first[name][metric].tobytes() == want_table[:, s * P.V + m].tobytes(), (name, metric)
            assert second[name][metric].tobytes() == first[name][metric].tobytes() and second["values"][name][metric].tobytes() == v.tobytes()
    assert first["groups"].tobytes() == np.ascontiguousarray(want_table[:, -1, :4]).tobytes() == second["groups"].tobytes()
    ok = want_status == 0
    assert np.isfinite(first["values"]["lin_vel_x"]["rise_time"][ok]).sum() > 50 and (first["values"]["lin_vel_x"]["overshoot"][ok] > 0.05).sum() > 5
    assert (first["groups"][:, 1:4].sum(axis=1) == first["groups"][:, 0]).all() and first["groups"][:, 0].sum() == (group >= 0).sum()


# ---- the ring, and what an armed trace leaves alone ---------------------------------------------------------------------------------------------
def test_full_ring_records_nothing_more():
    N = 16
    env = make_env(N, "plane", 20.0, seed=1)
    env.start_trace(capacity=10)
    zero = torch.zeros(N, 12, device=DEVICE)
    for _ in range(10):
        env.step(zero)
    assert env._trace.rows == 10 and not env._trace.truncated
    before = env._trace.trace.clone()
    for _ in range(2):
        env.step(zero)
    torch.cuda.synchronize()
    assert env._trace.rows == 10 and env._trace.truncated
    assert torch.equal(before, env._trace.trace)
    out = env.read_trace()
    assert out["rows"] == 10 and out["truncated"] and out["lin_vel_x"].shape == (10, N)
    assert out["dof_pos_3"].tobytes() == before[:, 15].cpu().numpy().tobytes()
    env.start_trace(capacity=3)                                          # a new trace starts empty
    assert env._trace.rows == 0 and not env._trace.truncated and env._trace.trace.shape == (3, 24, N)


def test_trace_leaves_the_simulation_and_both_tables_bit_identical():
    N, STEPS = 128, 30
    plain, traced = [make_env(N, "plane", 1.0, seed=3) for _ in range(2)]
    groups = torch.arange(N) % 2
    for e in (plain, traced):
        e.start_metrics(groups, warmup_steps=3, behaviour=True)
    traced.start_trace(capacity=STEPS)
    assert plain._trace is None and traced._trace.armed
    g = torch.Generator(device=DEVICE).manual_seed(2)
    for _ in range(STEPS):
        a = 1.0 * torch.randn(N, 12, device=DEVICE, generator=g)
        for e in (plain, traced):
            e.step(a)
    torch.cuda.synchronize()
    for name in ("obs_buf", "rew_buf", "reset_buf"):
        assert getattr(plain, name).cpu().numpy().tobytes() == getattr(traced, name).cpu().numpy().tobytes(), name
    for e in (plain, traced):
        e.stop_metrics()
    a, b = plain.read_metrics(), traced.read_metrics()
    assert sorted(a) == sorted(b) and "behaviour" in a
    for k in a:
        if k == "behaviour":
            for m in a[k]:
                assert a[k][m].tobytes() == b[k][m].tobytes(), m
        else:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert a["groups"][:, 1].tolist() == [64.0 * STEPS] * 2
    out = traced.read_trace()
    assert out["rows"] == STEPS and out["reset"].sum() > 0                 # episodes of 1 s under random actions: resets were traced
    assert out["reset"][-1].tobytes() == traced.reset_buf.float().cpu().numpy().tobytes()


# ---- the response sweep end to end, and what a traced step costs -------------------------------------------------------------------------------
class StandStill:
    """the scripted policy: zero actions (a robot that stands on its default pose)"""

    def act_inference(self, obs, policy_info={}):
        h = obs["obs_history"]
        return torch.zeros(h.shape[0], 12, device=h.device)


def test_response_sweep_end_to_end():
    from go1_gym_learn.eval_metrics import response
    N, PRESET = 256, "static_medium"                                       # base_set() switches the pushes off for every preset
    res = response.run_response_sweep(StandStill(), PRESET, "lin_vel_x", 0.0, [0.5, 1.0], num_envs=N, settle_steps=50, pre=20, window=60,
                                      seed=5, terrain="plane", trace_envs=list(range(N)))
    assert res["signals"] == ["lin_vel_x", "contact_match"] and res["smooth"] == 17 and res["cells"] == [0.5, 1.0]
    trace = res["trace"]
    assert trace["rows"] == 80 and not trace["truncated"]
    held = res["status"] == 0
    assert (trace["cmd_lin_vel_x"][:20, held] == 0.0).all() and (trace["cmd_lin_vel_x"][20:, held] == np.tile(np.float32([0.5, 1.0]), N // 2)[held]).all()
    # a host pass of the trace through the model: the same values, statuses and table
    signals = [(tuple(response.RESPONSE_SIGNALS[n]) + (0.0, 0.0))[:4] for n in res["signals"]]
    want_values, want_status = P.response(stack(trace), signals, 20, 20, 17, 0.1, 10, 25, res["dt"])
    group = np.arange(N) % 2
    want_table = P.response_reduce(want_values, want_status, group, 2)
    assert np.array_equal(res["status"], want_status)
    for s, name in enumerate(res["signals"]):
        for m, metric in enumerate(P.VALUES):
            assert res["values"][name][metric].tobytes() == want_values[s, m].tobytes(), (name, metric)
            assert res["response"][name][metric].tobytes() == want_table[:, s * P.V + m].tobytes(), (name, metric)
    assert res["groups"].tobytes() == np.ascontiguousarray(want_table[:, -1, :4]).tobytes()
    assert res["groups"][:, 0].tolist() == [128.0, 128.0] and (res["groups"][:, 1:4].sum(axis=1) == 128.0).all()
    print("\n" + "\n\n".join(response.response_markdown_table(res, s) for s in res["signals"]))
    # a condition of the test, not a measurement: a robot that stands still does not fall, so most environments are analysed
    assert (res["groups"][:, 1] >= 64.0).all(), res["groups"]
    ok = res["status"] == 0
    assert (res["values"]["contact_match"]["overshoot"][ok] == 0).all()


def test_trace_cost_is_recorded():
    """no time is asserted: the three configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    from go1_gym_learn.eval_metrics import response, sweep
    N, STEPS, SEED, PRESET, REPS = 1024, 150, 5, "static_medium", 2
    env, _ = sweep.build_eval_env(PRESET, N, SEED)
    base = env.env
    env.reset()
    commands = response.switch_commands("lin_vel_x", [0.5, 1.0], base.commands.shape[1], base.device)[torch.arange(N, device=base.device) % 2]
    base.commands[:] = commands
    obs = env.get_observations()
    policy = StandStill()

    def timed(steps):
        nonlocal obs
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.inference_mode():
            a.record()
            for _ in range(steps):
                obs = sweep.policy_step(env, policy, obs, commands)
            b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / steps

    def traced(steps, env_ids):
        base.start_trace(env_ids, capacity=steps)
        t = timed(steps)
        base.stop_trace()
        assert base._trace.rows == steps and not base._trace.truncated
        return t
    configurations = [("nothing armed", timed), ("trace of all", lambda steps: traced(steps, None)),
                      ("trace of 8", lambda steps: traced(steps, list(range(0, N, N // 8))))]
    for _, run in configurations:               # warm: every kernel and every allocation size once, outside the timed windows
        run(STEPS)
    rows = [[run(STEPS) for _, run in configurations] for _ in range(REPS)]
    assert all(t > 0 for row in rows for t in row)
    lines = [f"Cost of a traced step, one MI355X, {N} environments, {PRESET}, a scripted policy of zero actions, {STEPS} steps per window, device",
             "events around the step loop (commands written, env.step, trace), warm, the three configurations in alternation.",
             "MEASURED; microseconds per step.", "", f"{'rep':>4}" + "".join(f"{name:>16}" for name, _ in configurations)]
    lines += [f"{r + 1:>4}" + "".join(f"{t:>16.1f}" for t in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: no trace, no metrics.  trace of all: start_trace(), one go1eval_trace_record launch per step over the 1024",
              "environments (24 channels, 98 KB per row).  trace of 8: start_trace([0, 128, ...]), the same launch over 8 environments.",
              "No host read in any of the three."]
    report("response_trace_cost.txt", "\n".join(lines))
