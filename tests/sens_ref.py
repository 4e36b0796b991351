"""TEST INFRASTRUCTURE: numpy model of libgo1sens's kernels, written from the text of include/go1sens.h (the nine parameters and where
the simulator keeps them, the bin of a value, the values in force carried from launch to launch, the parameter thread's six steps, the
pair thread, the clear and the snapshot, the folding rule, the `value` rows, the group row, the curves, the counts and the pair map).
Every value is formed in np.float32 in the header's operation order and summed in float64, so accumulators, state and the four result
tables are compared with the kernels' bit for bit.  The metric-row reduction is joint_ref.py's (eval_ref.py's fixed order, vectorised
over the rows); the per-bin order (the foot profile's) is restated here."""
import types

import numpy as np

import eval_ref as E
from joint_ref import _combine_rows

PARAMETERS = ["friction", "restitution", "payload", "com_x", "com_y", "com_z", "motor_strength", "Kp_factor", "Kd_factor"]
QUANTITIES = ["steps", "measured", "falls", "timeouts", "reward_sum", "lin_err_sum", "yaw_err_sum", "power_sum"]
COUNTS = ["unbinned", "redraws", "bad"]
PAIR_QUANTITIES = ["steps", "falls", "measured", "lin_err_sum"]
GROUP_FIELDS = ["envs", "launches"]
P, BINS, SIDE, CELLS = len(PARAMETERS), 16, 8, 64
ROWS = P + 1
STEP_INPUTS = ["reset_buf", "time_out_buf", "episode_length_buf", "rew_buf", "base_lin_vel", "base_ang_vel", "commands", "torques", "dof_vel"]
PARAMETER_INPUTS = ["friction_coeffs", "restitutions", "payloads", "com_displacements", "motor_strengths", "Kp_factors", "Kd_factors"]
INPUTS = STEP_INPUTS + PARAMETER_INPUTS
STATE = ["cur", "pair_cur", "steps", "measured", "falls", "timeouts", "reward_sum", "lin_err_sum", "yaw_err_sum", "power_sum", "unbinned", "redraws", "bad",
         "launches", "pair_steps", "pair_falls", "pair_measured", "pair_lin_err_sum"]
# parameter -> (buffer, row)
SOURCE = [("friction_coeffs", None), ("restitutions", None), ("payloads", None), ("com_displacements", 0), ("com_displacements", 1), ("com_displacements", 2),
          ("motor_strengths", 0), ("Kp_factors", 0), ("Kd_factors", 0)]
f32 = np.float32


def config(ranges, warmup_steps=0, pair=None):
    """what Go1SensConfig says for {name: (lo, hi)} and a pair of names: active, lo and scale = 16 / (hi - lo), computed in fp64 and
    rounded to fp32 once"""
    active = np.array([name in ranges for name in PARAMETERS])
    lo = np.array([ranges[name][0] if name in ranges else 0.0 for name in PARAMETERS]).astype(f32)
    scale = np.array([BINS / (ranges[name][1] - ranges[name][0]) if name in ranges else 0.0 for name in PARAMETERS]).astype(f32)
    a, b = (PARAMETERS.index(pair[0]), PARAMETERS.index(pair[1])) if pair else (-1, -1)
    return types.SimpleNamespace(warmup_steps=warmup_steps, active=active, lo=lo, scale=scale, pair_a=a, pair_b=b, ranges=dict(ranges), pair=pair)


def now(snap, p):
    """the simulator's value of parameter p at this moment, (N,) np.float32"""
    name, row = SOURCE[p]
    v = snap[name] if row is None else snap[name][row]
    assert v.dtype == f32
    return v


def bin_of(v, lo, scale):
    """(the bins of the np.float32 vector v, -1 where it has none)"""
    assert v.dtype == f32 and lo.dtype == f32 and scale.dtype == f32
    with np.errstate(all="ignore"):
        t = (v - lo) * scale
        t = np.fmin(np.fmax(t, f32(0.0)), f32(BINS - 1))
    assert t.dtype == f32
    return np.where(np.isfinite(v), np.where(np.isfinite(v), t, 0).astype(np.int64), -1)


class State:
    """the accumulators and the state after go1sens_clear on the buffers `snap`, in the kernel's own number formats"""

    def __init__(self, N, cfg, snap):
        self.N = N
        self.count, self.nonfinite = np.zeros((P, N), np.uint32), np.zeros((P, N), np.uint32)
        self.sum, self.sumsq = np.zeros((P, N)), np.zeros((P, N))
        self.min, self.max = np.full((P, N), np.inf, f32), np.full((P, N), -np.inf, f32)
        self.steps, self.measured, self.falls, self.timeouts = (np.zeros((P, BINS, N), np.uint32) for _ in range(4))
        self.reward_sum, self.lin_err_sum, self.yaw_err_sum, self.power_sum = (np.zeros((P, BINS, N)) for _ in range(4))
        self.unbinned, self.redraws, self.bad = (np.zeros((P, N), np.uint32) for _ in range(3))
        self.launches = np.zeros(N, np.uint32)
        self.pair_steps, self.pair_falls, self.pair_measured = (np.zeros((CELLS, N), np.uint32) for _ in range(3))
        self.pair_lin_err_sum = np.zeros((CELLS, N))
        self.cur, self.pair_cur = np.zeros((P, N), f32), np.zeros((2, N), f32)
        snapshot(self, cfg, snap)

    def fold(self, row, live, v):
        """fold the np.float32 vector v into `row` for the environments `live`"""
        assert v.dtype == f32
        fin = np.isfinite(v)
        self.nonfinite[row] += (live & ~fin).astype(np.uint32)
        ok = live & fin
        self.count[row] += ok.astype(np.uint32)
        v64 = v.astype(np.float64)
        with np.errstate(all="ignore"):
            np.add(self.sum[row], v64, out=self.sum[row], where=ok)
            np.add(self.sumsq[row], v64 * v64, out=self.sumsq[row], where=ok)
            np.fmin(self.min[row], v, out=self.min[row], where=ok)
            np.fmax(self.max[row], v, out=self.max[row], where=ok)

    def arrays(self):
        return {k: getattr(self, k) for k in ["count", "sum", "sumsq", "min", "max", "nonfinite"] + STATE}


def clear(N, cfg, snap):
    """go1sens_clear"""
    return State(N, cfg, snap)


def snapshot(st, cfg, snap):
    """go1sens_snapshot: cur and pair_cur from the buffers, nothing else"""
    st.cur = np.stack([now(snap, p) for p in range(P)]).astype(f32)
    if cfg.pair_a >= 0 and cfg.pair_b >= 0:
        st.pair_cur = np.stack([now(snap, cfg.pair_a), now(snap, cfg.pair_b)]).astype(f32)
    else:
        st.pair_cur = np.zeros((2, st.N), f32)


def outcomes(snap):
    """(lin_err, yaw_err, power, all three finite) of the step, np.float32 each"""
    with np.errstate(all="ignore"):
        ex, ey = snap["base_lin_vel"][0] - snap["commands"][0], snap["base_lin_vel"][1] - snap["commands"][1]
        lin = np.sqrt(ex * ex + ey * ey)
        yaw = np.abs(snap["base_ang_vel"][2] - snap["commands"][2])
        carry = np.zeros(lin.shape[0])
        for j in range(12):
            product = snap["torques"][j] * snap["dof_vel"][j]
            assert product.dtype == f32
            carry = carry + product.astype(np.float64)
        power = carry.astype(f32)
    assert lin.dtype == yaw.dtype == power.dtype == f32
    return lin, yaw, power, np.isfinite(lin) & np.isfinite(yaw) & np.isfinite(power)


def _add(words, row, where, amount=1):
    """words[row[e], e] += amount[e] for the environments `where`; row may be a bin per environment"""
    e = np.nonzero(where)[0]
    r = row[e] if isinstance(row, np.ndarray) else row
    words[r, e] += amount[e] if isinstance(amount, np.ndarray) else amount


def accumulate(st, cfg, snap):
    """one go1sens_accumulate launch on the SoA buffers `snap` (np.float32 / uint8 / int32 arrays).  Returns what the step did, for the
    tests that look at single steps: {"bin": (9, N) the bin charged (-1: none or inactive), "fall", "timeout": (N,), "measured": (N,)
    the step entered the outcome sums of a binned value, "redrawn": (9, N)}"""
    N = st.N
    r = snap["rew_buf"]
    assert r.dtype == f32
    reset = snap["reset_buf"] != 0
    timed = snap["time_out_buf"] != 0
    live = ~reset & (snap["episode_length_buf"] > cfg.warmup_steps)
    lin, yaw, power, fine = outcomes(snap)
    good_reward = np.isfinite(r)
    did = dict(bin=np.full((P, N), -1, np.int64), fall=reset & ~timed, timeout=reset & timed, measured=live & fine, redrawn=np.zeros((P, N), bool))
    for p in range(P):
        if not cfg.active[p]:
            continue
        v = st.cur[p].copy()
        b = bin_of(v, cfg.lo[p], cfg.scale[p])
        did["bin"][p] = b
        st.fold(p, np.ones(N, bool), v)                                                   # 1
        binned = b >= 0
        st.unbinned[p] += (~binned).astype(np.uint32)                                     # 2
        safe = np.where(binned, b, 0)
        _add(st.steps[p], safe, binned)                                                   # 3
        _add(st.reward_sum[p], safe, binned & good_reward, r.astype(np.float64))
        st.bad[p] += (binned & ~good_reward).astype(np.uint32)
        _add(st.timeouts[p], safe, binned & reset & timed)                                # 4
        _add(st.falls[p], safe, binned & reset & ~timed)
        ok = binned & live & fine                                                         # 5
        _add(st.measured[p], safe, ok)
        _add(st.lin_err_sum[p], safe, ok, lin.astype(np.float64))
        _add(st.yaw_err_sum[p], safe, ok, yaw.astype(np.float64))
        _add(st.power_sum[p], safe, ok, power.astype(np.float64))
        st.bad[p] += (binned & live & ~fine).astype(np.uint32)
        w = now(snap, p)                                                                  # 6
        changed = w.view(np.uint32) != v.view(np.uint32)
        did["redrawn"][p] = changed
        st.redraws[p] += changed.astype(np.uint32)
        st.cur[p] = w
    st.launches += 1                                                                      # the pair thread
    if cfg.pair_a >= 0 and cfg.pair_b >= 0:
        a, b = cfg.pair_a, cfg.pair_b
        ba, bb = bin_of(st.pair_cur[0], cfg.lo[a], cfg.scale[a]), bin_of(st.pair_cur[1], cfg.lo[b], cfg.scale[b])
        has = (ba >= 0) & (bb >= 0)
        cell = np.where(has, SIDE * (ba >> 1) + (bb >> 1), 0)
        _add(st.pair_steps, cell, has)
        _add(st.pair_falls, cell, has & reset & ~timed)
        ok = has & live & fine
        _add(st.pair_measured, cell, ok)
        _add(st.pair_lin_err_sum, cell, ok, lin.astype(np.float64))
        st.pair_cur = np.stack([now(snap, a), now(snap, b)]).astype(f32)
    return did


def _bin_sums(words, members):
    """(F, 16) from words (F, 16, N): slice k adds the members e = k, k + 16, ... in ascending order; then slice k takes k + 8, + 4, + 2, + 1"""
    slices = E.REDUCE_THREADS // BINS
    partial = np.zeros((slices,) + words.shape[:2])
    for e in members:
        partial[e % slices] += words[:, :, e]
    k = slices // 2
    while k > 0:
        partial[:k] += partial[k:2 * k]
        k //= 2
    return partial[0]


def reduce(st, group, num_groups):
    """((G, 10, 6) result table, (G, 9, 8, 16) curves, (G, 9, 3) counts, (G, 4, 64) pair map) of go1sens_reduce, fp64"""
    group = np.asarray(group)
    out = np.zeros((num_groups, ROWS, len(E.FIELDS)))
    curves = np.zeros((num_groups, P, len(QUANTITIES), BINS))
    counts = np.zeros((num_groups, P, len(COUNTS)))
    pair = np.zeros((num_groups, len(PAIR_QUANTITIES), CELLS))
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    words = np.stack([getattr(st, q).astype(np.float64) for q in QUANTITIES], axis=1)                  # (9, 8, 16, N)
    pair_words = np.stack([getattr(st, "pair_" + q).astype(np.float64) for q in PAIR_QUANTITIES])       # (4, 64, N)
    for g in range(num_groups):
        members = [int(e) for e in np.nonzero(group == g)[0]]
        n = _combine_rows(st.count.astype(np.float64), members, np.add, 0.0)
        nf = _combine_rows(st.nonfinite.astype(np.float64), members, np.add, 0.0)
        S, Q = _combine_rows(st.sum, members, np.add, 0.0), _combine_rows(st.sumsq, members, np.add, 0.0)
        low, high = _combine_rows(lows, members, np.fmin, np.inf), _combine_rows(highs, members, np.fmax, -np.inf)
        some = n > 0
        with np.errstate(all="ignore"):
            mean = S / n
            var = Q / n - mean * mean
            rows = np.stack([n, mean, np.sqrt(np.fmax(var, 0.0)), low, high, nf], axis=1)
        rows[~some, 1:5] = np.nan
        out[g, :P] = rows
        out[g, P, :2] = _combine_rows(np.stack([np.ones(st.N), st.launches.astype(np.float64)]), members, np.add, 0.0)
        for p in range(P):
            curves[g, p] = _bin_sums(words[p], members)
            counts[g, p] = _combine_rows(np.stack([getattr(st, c)[p].astype(np.float64) for c in COUNTS]), members, np.add, 0.0)
        for part in range(CELLS // BINS):
            pair[g, :, part * BINS:(part + 1) * BINS] = _bin_sums(pair_words[:, part * BINS:(part + 1) * BINS], members)
    return out, curves, counts, pair


def run(cfg, first, snaps, N, outside=None):
    """(the state after a clear on the buffers `first` and a launch on each of `snaps`, what every launch did); outside = {launch index:
    parameter buffers}: a go1sens_snapshot on those buffers in front of that launch"""
    st, did = clear(N, cfg, first), []
    for k, s in enumerate(snaps):
        if outside and k in outside:
            snapshot(st, cfg, outside[k])
        did.append(accumulate(st, cfg, s))
    return st, did


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP, SCRIPT_COMMANDS = 12, 2, 15
SCRIPT_RANGES = dict(friction=(0.05, 4.5), restitution=(0.0, 1.0), payload=(-1.0, 3.0), com_x=(-0.1, 0.1), com_z=(-0.1, 0.1), motor_strength=(-0.99, 0.9),
                     Kd_factor=(0.5, 1.5))                                 # com_y and Kp_factor stay inactive
SCRIPT_PAIR = ("friction", "motor_strength")
KINDS = ["steady", "redrawn", "falls", "times_out", "nonfinite_value", "outside", "nan_velocity", "random"]
SCRIPT_SNAPSHOT = 7                    # a go1sens_snapshot stands in front of this launch, on buffers changed from outside


def script_config(pair=True):
    return config(SCRIPT_RANGES, warmup_steps=SCRIPT_WARMUP, pair=SCRIPT_PAIR if pair else None)


def _draw(rng, N):
    """the seven parameter buffers, drawn inside the script's ranges (the inactive ones too)"""
    u = lambda lo, hi, *lead: rng.uniform(lo, hi, (*lead, N)).astype(f32)
    strength = u(-0.99, 0.9)
    return dict(friction_coeffs=u(0.05, 4.5), restitutions=u(0.0, 1.0), payloads=u(-1.0, 3.0), com_displacements=u(-0.1, 0.1, 3),
                motor_strengths=np.tile(strength, (12, 1)), Kp_factors=np.tile(u(0.8, 1.3), (12, 1)), Kd_factors=np.tile(u(0.5, 1.5), (12, 1)))


def scripted_steps(rng, N, steps=SCRIPT_STEPS, pair=True):
    """(config, the buffers at the clear, `steps` snapshots of the buffers after a step, {SCRIPT_SNAPSHOT: the parameter buffers a
    go1sens_snapshot takes in front of that launch}, the kind of every environment).  The kinds: "steady" never resets and no step
    changes its parameters; "redrawn" falls on launch 4 with every parameter re-drawn on that very step (the fall belongs to the OLD
    bins: the buffers of launch 4 hold the new values); "falls" falls on launches 5 and 9 with its motor parameters re-drawn by the
    reset itself; "times_out" resets with time_out_buf on launch 6; "nonfinite_value" carries a NaN friction
    and an infinite payload from launch 2 to launch 5; "outside" carries values below and above the ranges; "nan_velocity" has a NaN
    velocity on launch 8, a NaN torque on launch 9 and infinite and NaN rewards on launches 4 and 10; "random" resets with probability
    0.15 (half of them time-outs) and is re-drawn with probability 0.2.  Before launch SCRIPT_SNAPSHOT the motor parameters of the
    "steady" kind change from outside and a go1sens_snapshot follows (the caller's part): no re-draw is counted for them.  time_out_buf
    carries noise on the steps without a reset: nothing reads it there."""
    cfg = script_config(pair)
    kind = rng.integers(0, len(KINDS), N)
    kind[:min(N, len(KINDS))] = np.arange(len(KINDS))[:N]
    steady, redrawn, falls, times_out, odd_value, outside, odd_velocity, random_ = (kind == k for k in range(len(KINDS)))
    params = _draw(rng, N)
    params["friction_coeffs"][outside] = f32(-0.5)
    params["payloads"][outside] = f32(7.0)
    params["com_displacements"][0, outside] = f32(0.1)                       # the upper edge itself: the last bin
    first = {k: v.copy() for k, v in params.items()}
    outside = {}
    age = rng.integers(0, 6, N).astype(np.int32)
    snaps = []
    for t in range(steps):
        reset = redrawn & (t == 4) | falls & ((t == 5) | (t == 9)) | times_out & (t == 6) | random_ & (rng.random(N) < 0.15)
        timed = np.where(reset, rng.random(N) < 0.5, rng.random(N) < 0.2)
        timed = np.where(times_out, True, np.where(redrawn | falls, False, timed))
        age = np.where(reset, 0, age + 1).astype(np.int32)
        r = (0.02 * rng.standard_normal(N) + 0.01).astype(f32)
        fresh = _draw(rng, N)
        if t == SCRIPT_SNAPSHOT:                                             # from outside, between two launches
            for k in ("motor_strengths", "Kp_factors", "Kd_factors"):
                params[k] = np.where(steady, _draw(rng, N)[k], params[k]).astype(f32)
            outside[t] = {k: v.copy() for k, v in params.items()}
        again = redrawn & (t == 4) | random_ & (rng.random(N) < 0.2)
        motors = falls & reset
        for k in params:
            params[k] = np.where(again | (motors & (k in ("motor_strengths", "Kp_factors", "Kd_factors"))), fresh[k], params[k]).astype(f32)
        if t == 1:
            params["friction_coeffs"][odd_value], params["payloads"][odd_value] = np.nan, np.inf
        if t == 4:
            params["friction_coeffs"][odd_value], params["payloads"][odd_value] = f32(1.0), f32(0.5)
        s = dict(reset_buf=np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8), time_out_buf=timed.astype(np.uint8), episode_length_buf=age.copy(),
                 rew_buf=r, base_lin_vel=rng.standard_normal((3, N)).astype(f32), base_ang_vel=rng.standard_normal((3, N)).astype(f32),
                 commands=rng.standard_normal((SCRIPT_COMMANDS, N)).astype(f32), torques=(5.0 * rng.standard_normal((12, N))).astype(f32),
                 dof_vel=(3.0 * rng.standard_normal((12, N))).astype(f32), **{k: v.copy() for k, v in params.items()})
        if t == 8:
            s["base_lin_vel"][0, odd_velocity] = np.nan
        if t == 9:
            s["torques"][7, odd_velocity] = np.nan
        if t == 4:
            s["rew_buf"][odd_velocity] = np.inf
        if t == 10:
            s["rew_buf"][odd_velocity] = np.nan
        snaps.append(s)
    return cfg, first, snaps, outside, kind
