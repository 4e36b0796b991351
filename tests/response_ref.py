"""TEST INFRASTRUCTURE: numpy model of libgo1eval's trace and step-response kernels, written from the text of include/go1eval.h
(the 24 channels, the status rules, the smoothed signal, the seven values, the group table).  The header fixes where a value is
rounded to fp32 and where a sum is carried in fp64, and the model rounds exactly there, so the kernels' outputs are compared
with it bit for bit.  The step values of channels 3, 5 and 10 are eval_ref.py's and channel 4 is behaviour_ref.py's contact
rule; the group reduction is eval_ref.py's fixed combination order."""
import numpy as np

import behaviour_ref as R
import eval_ref as E

CHANNELS = ["lin_vel_x", "lin_vel_y", "ang_vel_yaw", "base_height", "contact_match", "power_consumption", "cmd_lin_vel_x", "cmd_lin_vel_y",
            "cmd_ang_vel_yaw", "cmd_base_height", "max_torques", "reset"] + [f"dof_pos_{j}" for j in range(12)]
C = len(CHANNELS)
BASE_HEIGHT, CONTACT_MATCH, POWER, MAX_TORQUES, RESET = 3, 4, 5, 10, 11
VALUES = ["reached", "rise_time", "overshoot", "settled", "settling_time", "steady_state_err", "iae"]
V = len(VALUES)
GROUP_FIELDS = ["envs", "ok", "reset", "not_held"]
# the buffers go1eval_trace_record reads (SoA, [k][N]); measured_heights may be absent (None)
INPUTS = ["base_lin_vel", "base_ang_vel", "commands", "root_states", "measured_heights", "contact_forces", "desired_contact_states",
          "torques", "dof_vel", "dof_pos", "reset_buf"]
f32, f64 = np.float32, np.float64


def step_values(snap):
    """(base_height, contact_match, power_consumption, max_torques), each (N,) fp64, every operation in fp64: the two tables'
    models' values of the step (eval_ref.metric_values, behaviour_ref.contacts)"""
    s = dict(snap)
    s.setdefault("payloads", np.zeros(np.asarray(snap["root_states"]).shape[1]))
    v = E.metric_values(s)
    desired = np.asarray(snap["desired_contact_states"], f64)
    match = 0.25 * (R.contacts(snap) == (desired > 0.5)).sum(axis=0)
    return v[E.METRICS.index("base_height")], match, v[E.METRICS.index("power_consumption")], v[E.METRICS.index("max_torques")]


def rounded_step_values(snap):
    """the same four with the header's roundings (fp32 terms, an fp64 carry in ascending order, rounded to fp32 once): what the
    kernel's bits are"""
    z = np.asarray(snap["root_states"], f32)[2]
    if snap.get("measured_heights") is None:
        height = z
    else:
        h = np.asarray(snap["measured_heights"], f32)
        s = np.zeros(z.shape[0], f64)
        for p in range(h.shape[0]):
            s += (z - h[p]).astype(f64)
        height = s.astype(f32) / f32(h.shape[0])
    tq, qd = np.asarray(snap["torques"], f32), np.asarray(snap["dof_vel"], f32)
    power = np.zeros(z.shape[0], f64)
    for j in range(12):
        power += (tq[j] * qd[j]).astype(f64)
    _, match, _, tmax = step_values(snap)
    return height, match.astype(f32), power.astype(f32), tmax.astype(f32)


def trace_row(snap, env_ids, base_height_target, rounded=True):
    """(24, K): one go1eval_trace_record launch.  env_ids None: every environment.  rounded=True: fp32, the kernel's bits;
    False: fp64 with channels 3, 4, 5 and 10 from step_values (the yardstick of the kernel's arithmetic)"""
    N = np.asarray(snap["root_states"]).shape[1]
    ids = np.arange(N) if env_ids is None else np.asarray(env_ids, np.int64)
    T = f32 if rounded else f64
    full = np.zeros((C, N), T)
    vel, ang, cmd = (np.asarray(snap[k], T) for k in ("base_lin_vel", "base_ang_vel", "commands"))
    full[0], full[1], full[2] = vel[0], vel[1], ang[2]
    full[BASE_HEIGHT], full[CONTACT_MATCH], full[POWER], full[MAX_TORQUES] = rounded_step_values(snap) if rounded else step_values(snap)
    full[6:9] = cmd[0:3]
    full[9] = cmd[3] + T(f32(base_height_target))
    full[RESET] = np.asarray(snap["reset_buf"]) != 0
    full[12:24] = np.asarray(snap["dof_pos"], T)
    out = np.full((C, ids.size), np.nan, T)
    ok = (ids >= 0) & (ids < N)
    out[:, ok] = full[:, ids[ok]]
    return out


def window_ok(rows, switch_row, pre, smooth, hold, tail, band, dt):
    """the conditions go1eval_response checks before it launches"""
    return bool(1 <= smooth <= pre + 1 and pre <= switch_row < rows and hold >= 1 and tail >= 1 and max(hold, tail) <= rows - switch_row
                and dt > 0 and band > 0)


def response(trace, signals, switch_row, pre, smooth, band, hold, tail, dt):
    """one go1eval_response launch.  trace: (rows, 24, K) fp32; signals: [(y_channel, r_channel or None, fixed_target, fixed_scale)].
    Returns values (S, 7, K) fp32 and status (K,) int32."""
    trace = np.asarray(trace, f32)
    end, _, K = trace.shape
    s0, w = switch_row, smooth
    assert window_ok(end, s0, pre, w, hold, tail, band, dt)
    dt, band = f32(dt), f32(band)
    fell = (trace[s0 - pre:end, RESET] != 0).any(axis=0)                                          # rule 1
    moved = np.zeros(K, bool)
    targets = []
    for y, r, target, scale in signals:
        if r is None or r < 0:
            r1 = np.full(K, f32(target))
            targets.append((r1, r1))
            continue
        ch = trace[:, r]
        r1 = ch[s0]
        r0 = ch[s0 - 1] if s0 > 0 else r1
        moved |= (ch[s0:end] != r1).any(axis=0) | (ch[s0 - pre:s0] != r0).any(axis=0)
        targets.append((r1, r0))
    status = np.where(fell, 1, np.where(moved, 2, 0)).astype(np.int32)
    values = np.full((len(signals), V, K), np.nan, f32)
    with np.errstate(all="ignore"):
        for s, (y, r, target, scale) in enumerate(signals):
            r1, r0 = targets[s]                                                                   # rule 2
            D = np.full(K, f32(scale)) if f32(scale) > 0 else np.abs(r1 - r0)
            dead = (status != 0) | (D < f32(1e-6))
            sgn = np.where(r1 >= r0, f32(1), f32(-1))
            near, inside = f32(0.1) * D, band * D
            ych = trace[:, y]
            t_r, t_s = np.full(K, -1), np.full(K, s0)
            over = np.zeros(K, f32)
            tail_sum, abs_sum = np.zeros(K, f64), np.zeros(K, f64)
            for t in range(s0, end):
                acc = np.zeros(K, f64)                                                            # rule 3
                for u in range(t - w + 1, t + 1):
                    acc += ych[u].astype(f64)
                err = (acc / f64(w)).astype(f32) - r1
                t_r = np.where((t_r < 0) & (np.abs(err) <= near), t, t_r)                         # rule 4
                over = np.fmax(over, sgn * err / D)
                t_s = np.where(np.abs(err) > inside, t + 1, t_s)
                raw = ych[t] - r1
                abs_sum += np.abs(raw).astype(f64)
                if t >= end - tail:
                    tail_sum += raw.astype(f64)
            reached, settled = t_r >= 0, t_s <= end - hold
            v = values[s]
            v[0] = reached
            v[1] = np.where(reached, (t_r - s0 + 1).astype(f32) * dt, f32(np.nan))
            v[2] = over
            v[3] = settled
            v[4] = np.where(settled, (t_s - s0 + 1).astype(f32) * dt, f32(np.nan))
            v[5] = (tail_sum / f64(tail)).astype(f32)
            v[6] = (f64(dt) * abs_sum).astype(f32)
            v[:, dead] = np.nan
    return values, status


def response_reduce(values, status, group, num_groups):
    """(G, S * 7 + 1, 6) fp64 result table of go1eval_response_reduce: per row the metric row of eval_ref.reduce over accumulators
    that folded the one value, and the group's own row"""
    values, status, group = np.asarray(values, f32), np.asarray(status), np.asarray(group)
    S, _, K = values.shape
    flat = values.reshape(S * V, K).astype(f64)
    add = lambda a, b: a + b
    out = np.zeros((num_groups, S * V + 1, len(E.FIELDS)))
    for g in range(num_groups):
        members = [int(e) for e in np.nonzero(group == g)[0]]
        for m in range(S * V):
            v = flat[m]
            fin = np.isfinite(v)
            n = E._combine(fin.astype(f64), members, add, 0.0)
            nf = E._combine((~fin).astype(f64), members, add, 0.0)
            if n > 0:
                total = E._combine(np.where(fin, v, 0.0), members, add, 0.0)
                squares = E._combine(np.where(fin, v * v, 0.0), members, add, 0.0)
                mean = total / n
                counted = [e for e in members if fin[e]]
                out[g, m] = [n, mean, np.sqrt(max(squares / n - mean * mean, 0.0)), min(v[e] for e in counted), max(v[e] for e in counted), nf]
            else:
                out[g, m] = [0.0, np.nan, np.nan, np.nan, np.nan, nf]
        out[g, S * V] = [float(len(members))] + [float(sum(1 for e in members if status[e] == k)) for k in (0, 1, 2)] + [0.0, 0.0]
    return out


def synthetic_traces(rng, K, rows, s0, pre):
    """TEST DATA.  K traces (rows, 24, K) that mix the hand-computable cases at random: first-order and overshooting responses up and down with noise, responses
    that stall short, late excursions, no step at all, resets inside and just outside the window, commands that move"""
    t = np.zeros((rows, C, K), np.float32)
    t[:] = rng.standard_normal((rows, C, K)).astype(np.float32) * 0.01
    t[:, RESET] = 0.0
    kind = rng.integers(0, 9, K)
    for k in range(K):
        r0, r1 = rng.choice([0.0, 0.5, 1.0, 1.5], 2, replace=False)
        if kind[k] == 4:
            r1 = r0                                                             # no step
        i = np.arange(rows - s0)
        tau = rng.uniform(1.0, 4.0)
        y = r0 + (r1 - r0) * (1.0 - np.exp(-(i + 1) / tau))
        if kind[k] == 1:
            y += (r1 - r0) * 0.6 * np.exp(-i / 10.0) * np.sin(i / 4.0)           # overshoots
        if kind[k] == 2:
            y = r0 + (r1 - r0) * 0.8 * (1.0 - np.exp(-(i + 1) / tau))           # stalls short
        if kind[k] == 3:
            y[-int(rng.integers(1, 12))] += 0.5 * (r1 - r0)                      # leaves the band late
        noise = 0.005 * rng.standard_normal(rows)
        for c, (lo, hi) in enumerate([(r0, r1), (0.3 * r0, 0.3 * r1), (-r0, -r1), (0.3 + 0.05 * r0, 0.3 + 0.05 * r1)]):
            scale = (hi - lo) / (r1 - r0) if r1 != r0 else 0.0
            t[:s0, c, k] = lo + noise[:s0] * abs(scale)
            t[s0:, c, k] = lo + (y - r0) * scale + noise[s0:] * abs(scale)
            t[:s0, 6 + c, k], t[s0:, 6 + c, k] = lo, hi
        t[:, 4, k] = np.round(4 * np.clip(0.5 + 0.5 * (1 - np.exp(-np.arange(rows) / 8.0)) + 0.2 * rng.standard_normal(rows), 0, 1)) / 4
        if kind[k] == 5:
            t[int(rng.integers(s0 - pre, rows)), RESET, k] = 1.0              # reset inside the window
        if kind[k] == 6 and s0 - pre >= 1:
            t[s0 - pre - 1, RESET, k] = 1.0                                   # just outside
        if kind[k] == 7:
            t[int(rng.integers(s0 + 1, rows)):, 6 + int(rng.integers(0, 4)), k] += 0.25      # the command moves
        if kind[k] == 8:
            t[:, :, k] = np.nan                                                 # an id outside the simulator
    return t, kind


SIGNALS = [(0, 6, 0.0, 0.0), (2, 8, 0.0, 0.0), (3, 9, 0.0, 0.0), (4, None, 1.0, 1.0), (1, 7, 0.0, 0.5)]
