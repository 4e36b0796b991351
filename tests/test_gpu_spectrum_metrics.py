"""GPU checks of the spectrum family (include/go1spectrum.h, libgo1spectrum.so): the scripted buffers of the emulator test through the
compiled kernels against the model of tests/spectrum_ref.py bit for bit, the real environment under a scripted trot with the model
replayed on the buffers read back after every step, the simulation's indifference to an armed measurement, the refusal of a restore
while armed, and the recorded cost of an armed step, of one fold and of one read.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (spectrum_metrics_cost.txt: the source of
profiles/spectrum_metrics_cost.txt); it is always printed."""
import ctypes

import numpy as np
import pytest
import torch

import spectrum_ref as T
from test_gpu_response_trace import DEVICE, make_env, report
from test_gpu_terrain_metrics import same_bits
from test_spectrum_metrics import DT, SHAPES, bits, check_against_the_model, drive, same_as_the_model, spectrum_groups, spectrum_on

pytestmark = pytest.mark.gpu


# ---- 1. the compiled kernels on the scripted buffers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,W,taper", SHAPES)
def test_spectrum_kernels_equal_the_model_bit_for_bit(N, W, taper):
    groups = 3
    rng = np.random.default_rng(1200 + N + W)                            # the emulator test's script
    cfg = T.config(W, warmup_steps=T.SCRIPT_WARMUP, taper_name=taper, dt=DT)
    snaps, kind = T.scripted_steps(rng, N, W)
    group = spectrum_groups(rng, N, groups)
    sm, B = spectrum_on(DEVICE, N)
    res, acc = drive(sm, B, cfg, snaps, group, groups)
    check_against_the_model(res, acc, sm.ring.cpu().numpy(), cfg, snaps, kind, group, groups, N)
    again = sm.read()                                                    # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ("groups", "psd", "psd_sum", "psd_segments", "env_psd_sum", "env_psd_segments", "valid", "steps", "resets",
                                                        "segments", "segments_dropped"))
    assert all(bits(again["metrics"][m]) == bits(res["metrics"][m]) for m in T.METRICS)
    before = sm.ring.clone()
    assert sm.lib.go1spectrum_record(ctypes.byref(sm.cfg), ctypes.byref(sm.buf), W, sm._stream()) == -7 and torch.equal(sm.ring, before)
    with pytest.raises(RuntimeError, match="go1spectrum_fold failed: -12"):
        sm.cfg.high_bin = 0
        sm.fold()
    assert bits(sm.read()["env_psd_sum"]) == bits(res["env_psd_sum"])    # the refused fold wrote nothing


# ---- 2. the real environment ------------------------------------------------------------------------------------------------------------------
def snapshot(env):
    """host copies of the buffers go1spectrum_record reads, as they stand after a step"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in T.INPUTS}


def test_spectrum_through_the_environment():
    """2 W + 3 steps of the foot family's trot script, 64 environments, W = 16: the simulation is bit-identical with the measurement
    armed and not armed (the family only reads); the kernels' accumulators, ring, state, density sums and tables equal the model
    replayed on the buffers read back after every step, bit for bit; every environment that did not reset folded two segments; a step
    after the stop launches nothing; and an armed family refuses a restore."""
    from test_foot_metrics import trot_action
    N, GROUPS, W = 64, 3, 16
    STEPS = 2 * W + 3
    plain, env = make_env(N, "plane", 20.0, seed=4), make_env(N, "plane", 20.0, seed=4)
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    for e in (plain, env):
        e.reset()
    env.start_spectrum_metrics(group, warmup_steps=0, segment_steps=W, high_freq=10.0)
    assert plain._spectrum is None
    snaps = []
    for step in range(STEPS):
        action = trot_action(step, N).to(DEVICE)
        for e in (plain, env):
            e.step(action)
        snaps.append(snapshot(env))
    # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
    for name, t in plain.buffers.tensors.items():
        if isinstance(t, torch.Tensor) and name != "episode_log":
            assert same_bits(t, env.buffers.tensors[name]), name
    env.stop_spectrum_metrics()
    res = env.read_spectrum_metrics()
    sm = env._spectrum
    c = sm.cfg
    cfg = T.config(W, warmup_steps=0, high_freq=10.0, dt=float(env.dt))
    assert (c.num_envs, c.warmup_steps, c.num_groups, c.segment_steps, c.high_bin) == (N, 0, GROUPS, W, cfg.high_bin) and bits(np.float32(c.bin_width)) == bits(cfg.bin_width)
    assert sm.calls == STEPS and all(bits(sm.tables[k]) == bits(cfg.tables[k]) for k in T.TABLES)
    st, folds = T.run(cfg, snaps, N)
    assert len(folds) == 2
    acc = {k: t.cpu().numpy() for k, t in sm.acc.items()}
    same_as_the_model(res, acc, sm.ring.cpu().numpy(), st, group.numpy(), GROUPS)
    quiet = st.resets == 0
    assert quiet.any() and (res["segments"].view(np.uint32)[quiet] == 2).all() and (res["segments_dropped"][quiet] == 0).all()
    assert res["steps"].tolist() == [STEPS] * N and (res["groups"][:, 3] + res["groups"][:, 4] == 2 * res["groups"][:, 0]).all()
    # the script moves every joint of a robot that did not reset: a power above 0 and a peak in every action, torque and joint-speed row
    power = np.stack([acc["min"][s * 5] for s in range(36)])[:, quiet]
    print(f"\nMI355X: resets {int(st.resets.sum())}; environments with two segments {int(quiet.sum())}; smallest segment power of an action, torque or joint speed "
          f"{power.min():.3g}; peak frequencies of the thigh actions {sorted(set(np.round(acc['max'][[s * 5 + 1 for s in (1, 4, 7, 10)]][:, quiet].ravel(), 3).tolist()))} Hz")
    assert (power[[1, 2, 4, 5, 7, 8, 10, 11]] > 0).all()                  # the scripted thigh and calf actions themselves
    env.step(torch.zeros(N, 12, device=DEVICE))                          # disarmed: no further launch
    assert env.read_spectrum_metrics()["steps"].tolist() == [STEPS] * N
    with pytest.raises(RuntimeError, match="spectrum"):                  # an armed family refuses a restore
        env.start_spectrum_metrics(group, segment_steps=W)
        env.load_state(env.save_state())
    env.stop_spectrum_metrics()


# ---- 3. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_spectrum_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = make_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0, out

    def window(armed):
        if armed:
            env.start_spectrum_metrics(group, warmup_steps=0)            # the default segment: 100 steps, so one fold per window
        us, _ = timed(lambda: [env.step(action) for _ in range(STEPS)])
        if armed:
            env.stop_spectrum_metrics()
        return us / STEPS

    def fold():
        """one fold more of what the ring holds after the window (a closed segment's tail and the open one's head): the full transform
        of every environment whose open segment is valid"""
        valid = int(env._spectrum.state["valid"].sum())
        us, _ = timed(env._spectrum.fold)
        return us, valid

    def read():
        us, res = timed(env.read_spectrum_metrics)
        assert res["groups"][:, 0].sum() == ENVS and res["steps"].tolist() == [STEPS] * ENVS
        return us
    window(False), window(True), fold(), read()                          # warm: every kernel and every allocation size once
    rows, valid = [], []
    for _ in range(REPS):
        off, on = window(False), window(True)
        one, n = fold()
        rows.append([off, on, one, read()])
        valid.append(n)
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "spectrum armed", "one fold", "read"]
    lines = [f"Cost of the spectrum measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the fold and the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  spectrum armed: the same loop after start_spectrum_metrics() with the default segment of 100",
              "steps: one go1spectrum_record launch more per step (40 x 1024 threads) and one go1spectrum_fold in the window, averaged over its",
              "150 steps.  one fold: go1spectrum_fold alone (40 x 16 wavefronts, 51 bins x 100 samples each), events around the call, on the",
              f"ring as the window left it; environments whose segment was valid and so transformed: {valid} of {ENVS}.  read:",
              "read_spectrum_metrics() (go1spectrum_reduce over 16 groups: 16 x 201 table rows and 16 x 40 x 52 density sums, and the",
              "device-to-host copies of the tables, the per-environment density sums and the state arrays), events around the call."]
    report("spectrum_metrics_cost.txt", "\n".join(lines))
