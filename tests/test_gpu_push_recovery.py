"""GPU checks of the push and the disturbance recovery: go1eval_push on random attitudes against the fp64 model of
tests/recovery_ref.py within its derived bound and bit-identical everywhere else, the simulation's indifference to pushes of
other environments, to an all-zero table and to the loaded family, go1eval_recovery / go1eval_recovery_reduce against the model
bit for bit on uploaded synthetic traces, the push sweep end to end against a host pass of its own trace, and the recorded cost.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (push_recovery_cost.txt: the source of
profiles/push_recovery_cost.txt); it is always printed."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import recovery_ref as P
from test_gpu_response_trace import DEVICE, StandStill, make_env, report, stack, uploaded_trace

pytestmark = pytest.mark.gpu
N, SUBSET = 70, [69, 0, 64, 63, 7]              # one full wavefront plus a tail of six; an unordered subset across both
ROWS, PRE, W, HOLD, BAND, DT = 40, 8, 5, 5, 0.1, 0.02


def same_bits(a, b):
    """bit for bit, on the device: -0.0 is not +0.0 and a NaN equals itself"""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


# ---- 1. the push kernel --------------------------------------------------------------------------------------------------------------
def random_state(rng):
    """(13, N) fp32 root_states with random unit quaternions; some velocities are -0.0"""
    before = rng.standard_normal((13, N)).astype(np.float32)
    q = rng.standard_normal((4, N))
    before[3:7] = q / np.linalg.norm(q, axis=0)
    before[7, ::3] = -0.0
    return before


def check_push(got, before, table, ids):
    """Rows 7, 8, 9 and 12 of the pushed environments against the fp64 model within 16 * 2^-24 * |push| + 2^-24 * |new value| per
    element: at most a dozen fp32 roundings on terms bounded by the push's norm, plus the final add (P.push_bound; not tuned).
    The heading divides by the planar length n of the forward axis, so the count of roundings holds while n is not small: under
    the SIMT emulator 20000 random attitudes stay below 0.83 of the bound for n >= 0.05 (a nose within 3 degrees of the
    vertical is the exception); the attitudes used here are asserted to lie in that range.  Every other element is bit-identical."""
    want, written = P.push(before, table, ids)
    x, y, z, w = before[3:7].astype(np.float64)
    assert np.hypot(1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z))[written].min() >= 0.05
    touched = np.zeros((13, N), bool)
    touched[np.ix_(P.PUSHED_ROWS, np.nonzero(written)[0])] = True
    assert got[~touched].tobytes() == before[~touched].tobytes()
    worst = 0.0
    for k, e in enumerate(range(N) if ids is None else ids):
        if 0 <= e < N and written[e]:
            for r in P.PUSHED_ROWS:
                d, bound = abs(float(got[r, e]) - want[r, e]), P.push_bound(table[k], want[r, e])
                worst = max(worst, d / bound)
                assert d <= bound, (k, e, r, float(got[r, e]), want[r, e], bound)
    return written, worst


def launch_push(before, table, ids):
    """go1eval_push itself on device copies (ids outside [0, N) reach the kernel this way; Go1Push refuses them on the host)"""
    import go1eval_host as G
    lib = G.load_library()
    root = torch.from_numpy(before.copy()).to(DEVICE)
    soa = torch.from_numpy(np.ascontiguousarray(table.T)).to(DEVICE)
    env_ids = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=DEVICE)
    cfg, buf = G.Go1PushConfig(), G.Go1PushBuffers()
    cfg.num_envs, cfg.num_pushed = N, table.shape[0]
    buf.root_states, buf.push, buf.env_ids = root.data_ptr(), soa.data_ptr(), None if ids is None else env_ids.data_ptr()
    assert lib.go1eval_push(ctypes.byref(cfg), ctypes.byref(buf), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return root.cpu().numpy()


@pytest.mark.parametrize("ids", [None, SUBSET, [69, 70, 3, -1, 64]])
def test_push_kernel_against_the_fp64_model(ids):
    rng = np.random.default_rng(41)
    before = random_state(rng)
    K = N if ids is None else len(ids)
    table = rng.uniform(-1.5, 1.5, (K, 4)).astype(np.float32)
    table[1::4] = 0.0                                                            # all-zero rows write nothing
    table[2, 1:] = 0.0                                                           # one value is enough to be written
    got = launch_push(before, table, ids)
    written, worst = check_push(got, before, table, ids)
    print(f"\ngo1eval_push, ids={ids}: {int(written.sum())} environments written, worst error / bound = {worst:.3f}")
    valid = [(k, e) for k, e in enumerate(range(N) if ids is None else ids) if 0 <= e < N]
    assert [bool(written[e]) for k, e in valid] == [bool(table[k].any()) for k, e in valid] and written.sum() >= 3
    quiet = ~written & (before[7] == 0)
    assert quiet.any() and np.signbit(got[7, quiet]).all()                        # -0.0 stays -0.0 where nothing is pushed


def test_go1push_on_the_device():
    """the host class: the table transposed and uploaded, ids as given, two launches of one table add twice"""
    import go1eval_host as G
    rng = np.random.default_rng(43)
    before = random_state(rng)
    B = types.SimpleNamespace(device=torch.device(DEVICE), root_states=torch.from_numpy(before.copy()).to(DEVICE))
    push = G.Go1Push(types.SimpleNamespace(num_envs=N), B)
    table = rng.uniform(-1.0, 1.0, (5, 4)).astype(np.float32)
    table[3] = 0.0
    push.load(table, SUBSET)
    push.launch()
    torch.cuda.synchronize()
    once = B.root_states.cpu().numpy()
    written, _ = check_push(once, before, table, SUBSET)
    assert sorted(np.nonzero(written)[0].tolist()) == [0, 7, 64, 69]
    push.launch()
    torch.cuda.synchronize()
    check_push(B.root_states.cpu().numpy(), once, table, SUBSET)
    with pytest.raises(ValueError):
        push.load(table, [69, 0, 64, 70, 7])


# ---- 2. the simulation ------------------------------------------------------------------------------------------------------------------
PER_ENV_FIRST = ("obs_buf", "privileged_obs_buf", "obs_history")          # [N][k]; every other per-environment buffer is [...][N]


def per_env_buffers(env):
    """{name: (tensor, axis of the environments)} of the simulator's state buffers that hold one slice per environment"""
    out = {}
    for name, t in env.buffers.tensors.items():
        if not isinstance(t, torch.Tensor) or name.startswith("curriculum"):
            continue
        if name in PER_ENV_FIRST:
            out[name] = (t, 0)
        elif t.shape[-1] == N:
            out[name] = (t, t.dim() - 1)
    return out


def test_pushes_leave_the_other_environments_and_a_zero_table_leaves_everything_bit_identical():
    import go1eval_host as G
    STEPS, AT = 30, 10
    pushed = [3] + list(range(64, 70))
    plain, shoved, zero = [make_env(N, "plane", 20.0, seed=4) for _ in range(3)]
    groups = torch.arange(N) % 2
    for e in (plain, zero):
        e.start_metrics(groups, warmup_steps=3, behaviour=True)
    for e in (plain, shoved, zero):
        e.start_trace(capacity=STEPS)
    zero._push = G.Go1Push(zero.sim_config, zero.buffers)                  # the family loaded, not yet used
    assert plain._push is None and shoved._push is None
    table = np.zeros((len(pushed), 4), np.float32)
    table[:, 0], table[:, 1], table[:, 3] = 0.5, 1.0, 0.25
    table[2] = 0.0                                                         # environment 65: named, not pushed
    keep = torch.tensor([e for e in range(N) if e not in pushed or e == 65], device=DEVICE)
    hit = torch.tensor([e for e in pushed if e != 65], device=DEVICE)
    action = torch.zeros(N, 12, device=DEVICE)
    names = per_env_buffers(plain)
    assert len(names) > 40 and {"root_states", "dof_pos", "obs_buf", "obs_history", "commands", "episode_length_buf", "lag_buffer"} <= set(names)
    for step in range(STEPS):
        if step == AT:
            before = shoved.buffers.root_states.clone()
            shoved.push_robots(table, pushed)
            zero.push_robots(np.zeros((N, 4), np.float32))
            after = shoved.buffers.root_states
            assert same_bits(before.index_select(1, keep), after.index_select(1, keep))
            assert not torch.equal(before[7:9].index_select(1, hit), after[7:9].index_select(1, hit))
            assert same_bits(before[:7], after[:7]) and same_bits(before[10:12], after[10:12])
        for e in (plain, shoved, zero):
            e.step(action)
        for name, (t, axis) in names.items():
            other = shoved.buffers.tensors[name]
            assert same_bits(t.index_select(axis, keep), other.index_select(axis, keep)), (step, name)
            assert same_bits(t, zero.buffers.tensors[name]), (step, name)
        if step == AT:                                                      # the push is simulated: the pushed robots moved
            assert not torch.equal(plain.buffers.base_lin_vel.index_select(1, hit), shoved.buffers.base_lin_vel.index_select(1, hit))
    # the zero table: the global buffers as well.  episode_log is no state: the step kernel adds the finished episodes' sums to it with
    # fp32 atomicAdd, so its last bits depend on the order in which the resetting environments arrive, in two identical runs too
    for name, t in plain.buffers.tensors.items():
        if isinstance(t, torch.Tensor) and name != "episode_log":
            assert same_bits(t, zero.buffers.tensors[name]), name
    assert torch.allclose(plain.buffers.episode_log, zero.buffers.episode_log, rtol=1e-5, atol=1e-6)
    for e in (plain, shoved, zero):
        e.stop_trace()
    for e in (plain, zero):
        e.stop_metrics()
    a, b = plain.read_metrics(), zero.read_metrics()
    assert sorted(a) == sorted(b) and "behaviour" in a
    for k in a:
        for m, x in (a[k].items() if k == "behaviour" else [(k, a[k])]):
            y = b[k][m] if k == "behaviour" else b[k]
            assert x.tobytes() == y.tobytes(), (k, m)
    ta, tb, tc = stack(plain.read_trace()), stack(shoved.read_trace()), stack(zero.read_trace())
    assert ta.shape == (STEPS, 24, N) and ta.tobytes() == tc.tobytes()
    cols = keep.cpu().numpy()
    assert np.ascontiguousarray(ta[:, :, cols]).tobytes() == np.ascontiguousarray(tb[:, :, cols]).tobytes()
    moved = hit.cpu().numpy()
    assert np.array_equal(ta[:AT, :, moved], tb[:AT, :, moved]) and (ta[AT, P.VY, moved] != tb[AT, P.VY, moved]).all()


# ---- 3. the analysis on uploaded traces ---------------------------------------------------------------------------------------------------
def test_recovery_and_reduce_equal_the_model_bit_for_bit():
    K, p0, groups = N, 12, 3
    rng = np.random.default_rng(47)
    trace, kind = P.synthetic_traces(rng, K, ROWS, p0, PRE)
    group = rng.integers(-1, groups, K).astype(np.int32)
    group[group == 1] = 0                                                  # three groups, the middle one empty
    group[-1] = 2
    tr = uploaded_trace(trace)
    first = tr.recovery(p0, PRE, W, BAND, HOLD, DT, group)
    second = tr.recovery(p0, PRE, W, BAND, HOLD, DT, group)
    want_values, want_status = P.recovery(trace, p0, PRE, W, BAND, HOLD, DT)
    want_table = P.recovery_reduce(want_values, want_status, group, groups)
    assert np.array_equal(first["status"], want_status) and set(want_status.tolist()) == {0, 1, 2, 3}
    assert (want_status[kind == 5] == 1).all() and (want_status[kind == 6] == 3).all() and (want_status[kind == 7] == 2).all()
    for m, metric in enumerate(P.VALUES):
        v = first["values"][metric]
        assert v.dtype == np.float32 and np.array_equal(np.isnan(v), np.isnan(want_values[m])), metric
        assert v.tobytes() == want_values[m].tobytes(), metric
        assert first[metric].tobytes() == want_table[:, m].tobytes(), metric
        assert second[metric].tobytes() == first[metric].tobytes() and second["values"][metric].tobytes() == v.tobytes()
    assert first["groups"].tobytes() == np.ascontiguousarray(want_table[:, -1, :5]).tobytes() == second["groups"].tobytes()
    assert first["groups"][1].tolist() == [0.0] * 5 and np.isnan(first["peak_vel_err"][1, 1:5]).all()
    assert (first["groups"][:, 1:5].sum(axis=1) == first["groups"][:, 0]).all() and first["groups"][:, 0].sum() == (group >= 0).sum()
    ok = want_status == 0
    assert ok.sum() >= 20 and (first["values"]["recovered"][ok] == 1).any() and (first["values"]["recovered"][ok] == 0).any()
    # the reduction's sums against math.fsum: the textbook bound of any fp64 summation order, (k - 1) u sum|x| for k terms, over the
    # count; the two divisions (the kernel's and this one's) round once each: 2 u |mean|
    checked = 0
    for g in (0, 2):
        members = np.nonzero(group == g)[0]
        for m, metric in enumerate(P.VALUES):
            x = [float(want_values[m, e]) for e in members if np.isfinite(want_values[m, e])]
            row = first[metric][g]
            assert row[0] == len(x) and row[5] == len(members) - len(x)
            if x:
                mean = math.fsum(x) / len(x)
                bound = (len(x) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in x) / len(x) + 2.0 ** -52 * abs(mean)
                assert abs(row[1] - mean) <= bound, (g, metric, row[1], mean, bound)
                assert row[3] == min(x) and row[4] == max(x)
                checked += 1
    assert checked >= 14


# ---- 4. the push sweep end to end ---------------------------------------------------------------------------------------------------------------
def test_push_sweep_end_to_end():
    from go1_gym_learn.eval_metrics import recovery
    res = recovery.run_push_sweep(StandStill(), "static_medium", (0, 1.0), (0, 90), num_envs=N, settle_steps=10, pre=PRE, window=30,
                                  smooth=W, band=BAND, hold=HOLD, seed=5, terrain="plane", trace_envs=list(range(N)))     # raises unless commands_held
    assert res["cells"] == [(0.0, 0.0), (0.0, 90.0), (1.0, 0.0), (1.0, 90.0)] and res["smooth"] == W
    trace = res["trace"]
    assert trace["rows"] == PRE + 30 and not trace["truncated"]
    # a host pass of the sweep's own trace through the model: the same values, statuses and table
    want_values, want_status = P.recovery(stack(trace), PRE, PRE, W, BAND, HOLD, res["dt"])
    group = np.arange(N) % 4
    want_table = P.recovery_reduce(want_values, want_status, group, 4)
    assert np.array_equal(res["status"], want_status)
    for m, metric in enumerate(P.VALUES):
        assert res["values"][metric].tobytes() == want_values[m].tobytes(), metric
        assert res["recovery"][metric].tobytes() == want_table[:, m].tobytes(), metric
    assert res["groups"].tobytes() == np.ascontiguousarray(want_table[:, -1, :5]).tobytes()
    assert res["groups"][:, 0].tolist() == [18.0, 18.0, 17.0, 17.0] and res["groups"][:, 0].sum() == N
    assert (res["groups"][:, 1:5].sum(axis=1) == res["groups"][:, 0]).all()
    print("\n" + recovery.recovery_markdown_table(res))
    # the push reached the robots of the pushed cells and only them: the first row after it differs from the control cells'
    # by about the pushed speed (cells 2 and 3), in the trace's body-frame velocities
    held = res["status"] != 2
    assert held.all()
    jump = np.hypot(trace["lin_vel_x"][PRE] - trace["lin_vel_x"][PRE - 1], trace["lin_vel_y"][PRE] - trace["lin_vel_y"][PRE - 1])
    print(f"planar velocity change over the push step: control cells {jump[group < 2].max():.3f} m/s at most, pushed cells {jump[group >= 2].min():.3f} m/s at least")


# ---- 5. the cost -------------------------------------------------------------------------------------------------------------------------------
def test_push_and_recovery_cost_is_recorded():
    """no time is asserted: the configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    from go1_gym_learn.eval_metrics import recovery, response, sweep
    ENVS, STEPS, SEED, PRESET, REPS = 1024, 150, 5, "static_medium", 2
    env, _ = sweep.build_eval_env(PRESET, ENVS, SEED)
    base = env.env
    env.reset()
    commands = sweep.command_table([response.BASE_CELL], base.commands.shape[1], base.device).repeat(ENVS, 1)
    base.commands[:] = commands
    obs = env.get_observations()
    policy = StandStill()
    table = recovery.push_table(recovery.push_cells([0, 0.5, 1.0], [0, 90, 180, 270]), ENVS)
    group = torch.arange(ENVS, dtype=torch.int32) % 12

    def window(push_at):
        nonlocal obs
        base.start_trace(capacity=STEPS)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        obs = sweep.rollout(env, policy, obs, STEPS if push_at is None else push_at, commands)
        if push_at is not None:
            base.push_robots(table)
            obs = sweep.rollout(env, policy, obs, STEPS - push_at, commands)
        b.record()
        torch.cuda.synchronize()
        base.stop_trace()
        assert base._trace.rows == STEPS and not base._trace.truncated
        return a.elapsed_time(b) * 1000.0 / STEPS

    def analysis(_):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = base.trace_recovery(push_row=25, pre=25, smooth=17, band=0.1, hold=10, groups=group)
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS
        return a.elapsed_time(b) * 1000.0
    configurations = [("traced", lambda: window(None)), ("traced, one push", lambda: window(25)), ("analysis", lambda: analysis(None))]
    for _, run in configurations:               # warm: every kernel and every allocation size once, outside the timed windows
        run()
    rows = [[run() for _, run in configurations] for _ in range(REPS)]
    assert all(t > 0 for row in rows for t in row)
    lines = [f"Cost of a push and of the recovery analysis, one MI355X, {ENVS} environments, {PRESET}, a scripted policy of zero actions, {STEPS} steps",
             "per window, device events around the step loop (commands written, env.step, trace), warm, the configurations in alternation.",
             "MEASURED; microseconds per step for the two windows, microseconds per call for the analysis.", "",
             f"{'rep':>4}" + "".join(f"{name:>20}" for name, _ in configurations)]
    lines += [f"{r + 1:>4}" + "".join(f"{t:>20.1f}" for t in row) for r, row in enumerate(rows)]
    lines += ["", "traced: start_trace() of all environments, one go1eval_trace_record launch per step.  traced, one push: the same window with",
              f"one push_robots() of all {ENVS} environments after step 25 (the table checked on the host, uploaded, one go1eval_push launch); its",
              f"cost is the difference of the two columns times {STEPS}.  analysis: trace_recovery() of the {STEPS}-row trace (go1eval_recovery,",
              "go1eval_recovery_reduce over 12 groups, one device-to-host copy of table, values and statuses), events around the call."]
    report("push_recovery_cost.txt", "\n".join(lines))
