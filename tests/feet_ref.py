"""TEST INFRASTRUCTURE: numpy model of libgo1feet's kernels, written from the text of include/go1feet.h (the twelve values per foot,
the stance state and its events, the GRF profile, the folding rules, the metric rows, the group row and the profile table).  Every
value is formed in np.float32 in the header's operation order and summed in float64, so accumulators, state, profile and the three
result tables are compared with the kernels' bit for bit.  The metric-row reduction is joint_ref.py's (eval_ref.py's fixed order,
vectorised over the rows); the profile's own order is restated here."""
import types

import numpy as np

import eval_ref as E
from joint_ref import _combine_rows

METRICS = ["contact", "force_normal", "force_tangent", "friction_use", "force_excess", "impact_vel_sq", "touchdown_speed", "touchdown_force",
           "stance_peak_force", "stance_impulse", "stance_slip", "stance_time"]
(CONTACT, FORCE_NORMAL, FORCE_TANGENT, FRICTION_USE, FORCE_EXCESS, IMPACT_VEL_SQ, TOUCHDOWN_SPEED, TOUCHDOWN_FORCE, STANCE_PEAK_FORCE,
 STANCE_IMPULSE, STANCE_SLIP, STANCE_TIME) = range(12)
M, FEET, BINS = len(METRICS), 4, 16
ROWS = FEET * M + 1
GROUP_FIELDS = ["envs", "steps", "resets"]
# the buffers go1feet_accumulate reads (SoA, [k][N])
INPUTS = ["contact_forces", "foot_velocities", "prev_foot_velocities", "foot_indices", "friction_coeffs", "reset_buf", "episode_length_buf"]
STATE = ["prev_contact", "stance_valid", "stance_steps", "stance_peak", "stance_impulse", "stance_slip", "steps", "resets", "profile_sum",
         "profile_count"]
AIR, GROUND, UNKNOWN = 0, 1, 2
f32 = np.float32


def config(dt=0.02, terrain_friction=1.0, max_contact_force=100.0, warmup_steps=0):
    """what Go1FeetConfig says"""
    return types.SimpleNamespace(dt=dt, terrain_friction=terrain_friction, max_contact_force=max_contact_force, warmup_steps=warmup_steps)


def foot_inputs(snap, f):
    """fx, fy, fz, vx, vy, pvz, ph of foot f: np.float32 vectors over the environments"""
    body = 12 * (f + 1)
    return (snap["contact_forces"][body], snap["contact_forces"][body + 1], snap["contact_forces"][body + 2], snap["foot_velocities"][3 * f],
            snap["foot_velocities"][3 * f + 1], snap["prev_foot_velocities"][3 * f + 2], snap["foot_indices"][f])


def phase_bin(ph):
    """the profile bin of the finite np.float32 values ph: clamped as a float, then converted"""
    with np.errstate(over="ignore"):
        b = np.floor(ph * f32(BINS))
    assert b.dtype == f32
    b = np.where(b > f32(BINS - 1), f32(BINS - 1), np.where(b > f32(0.0), b, f32(0.0)))
    return b.astype(np.int64)


def step_values(cfg, fx, fy, fz, vx, vy, pvz, mu):
    """(contact (bool), s, {the six per-step rows and the two touchdown rows: np.float32 vectors}) for np.float32 vectors"""
    assert all(a.dtype == f32 for a in (fx, fy, fz, vx, vy, pvz, mu))
    zero, one = f32(0.0), f32(1.0)
    with np.errstate(all="ignore"):
        c = fz > f32(1.0)
        hh = fx * fx + fy * fy
        fn, ft, s = np.sqrt(hh + fz * fz), np.sqrt(hh), np.sqrt(vx * vx + vy * vy)
        d = fn - f32(cfg.max_contact_force)
        excess = np.where(np.isnan(d), d, np.where(d > zero, d, zero))
        m = np.where(pvz < f32(-100.0), f32(-100.0), np.where(pvz > zero, zero, pvz))
        values = dict(contact=np.where(c, one, zero), force_normal=fz, force_tangent=ft, friction_use=ft / (mu * fz), force_excess=excess,
                      impact_vel_sq=np.where(fn > one, m * m, zero), touchdown_speed=np.where(pvz < zero, -pvz, zero), touchdown_force=fz)
    assert all(v.dtype == f32 for v in values.values()) and s.dtype == f32
    return c, s, values


class State:
    """the accumulators and the state after go1feet_clear, in the kernel's own number formats"""

    def __init__(self, N):
        self.N = N
        R = FEET * M
        self.count, self.nonfinite = np.zeros((R, N), np.uint32), np.zeros((R, N), np.uint32)
        self.sum, self.sumsq = np.zeros((R, N)), np.zeros((R, N))
        self.min, self.max = np.full((R, N), np.inf, f32), np.full((R, N), -np.inf, f32)
        self.prev_contact, self.stance_valid = np.full((FEET, N), UNKNOWN, np.uint8), np.zeros((FEET, N), np.uint8)
        self.stance_steps = np.zeros((FEET, N), np.int32)
        self.stance_peak, self.stance_impulse, self.stance_slip = (np.zeros((FEET, N), f32) for _ in range(3))
        self.steps, self.resets = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
        self.profile_sum, self.profile_count = np.zeros((FEET, BINS, N)), np.zeros((FEET, BINS, N), np.uint32)

    def fold(self, row, live, v):
        """fold the np.float32 vector v into `row` for the environments `live`"""
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


def accumulate(st, cfg, snap):
    """one go1feet_accumulate launch on the SoA buffers `snap` (np.float32 / uint8 / int32 arrays)"""
    reset = snap["reset_buf"] != 0
    st.steps += 1                                                                        # 1
    st.resets += reset.astype(np.uint32)
    live = ~reset & (snap["episode_length_buf"] > cfg.warmup_steps)                      # 2, 3
    dt = f32(cfg.dt)
    mu = f32(0.5) * (snap["friction_coeffs"] + f32(cfg.terrain_friction))
    env = np.arange(st.N)
    for f in range(FEET):
        fx, fy, fz, vx, vy, pvz, ph = foot_inputs(snap, f)
        c, s, values = step_values(cfg, fx, fy, fz, vx, vy, pvz, mu)
        prev, valid = st.prev_contact[f].copy(), st.stance_valid[f] != 0
        row = f * M
        st.fold(row + CONTACT, live, values["contact"])                                  # 4: the per-step rows
        for name in ("force_normal", "force_tangent", "friction_use"):
            st.fold(row + METRICS.index(name), live & c, values[name])
        st.fold(row + FORCE_EXCESS, live, values["force_excess"])
        st.fold(row + IMPACT_VEL_SQ, live, values["impact_vel_sq"])
        touchdown = live & c & (prev == AIR)
        further = live & c & (prev == GROUND) & valid
        liftoff = live & ~c & (prev == GROUND) & valid
        st.fold(row + TOUCHDOWN_SPEED, touchdown, values["touchdown_speed"])
        st.fold(row + TOUCHDOWN_FORCE, touchdown, values["touchdown_force"])
        st.fold(row + STANCE_PEAK_FORCE, liftoff, st.stance_peak[f])
        st.fold(row + STANCE_IMPULSE, liftoff, st.stance_impulse[f])
        st.fold(row + STANCE_SLIP, liftoff, st.stance_slip[f])
        st.fold(row + STANCE_TIME, liftoff, st.stance_steps[f].astype(f32) * dt)
        sample = live & np.isfinite(ph) & np.isfinite(fz)                                # the profile
        b = phase_bin(np.where(sample, ph, f32(0.0)))
        st.profile_sum[f, b[sample], env[sample]] += fz[sample].astype(np.float64)
        st.profile_count[f, b[sample], env[sample]] += 1
        with np.errstate(all="ignore"):                                                  # the state
            load, slide = fz * dt, s * dt
            st.stance_steps[f] = np.where(touchdown, 1, np.where(further, st.stance_steps[f] + 1, st.stance_steps[f])).astype(np.int32)
            st.stance_peak[f] = np.where(touchdown, fz, np.where(further, np.fmax(st.stance_peak[f], fz), st.stance_peak[f]))
            st.stance_impulse[f] = np.where(touchdown, load, np.where(further, st.stance_impulse[f] + load, st.stance_impulse[f]))
            st.stance_slip[f] = np.where(touchdown, slide, np.where(further, st.stance_slip[f] + slide, st.stance_slip[f]))
        assert st.stance_impulse.dtype == f32 and st.stance_slip.dtype == f32 and st.stance_peak.dtype == f32
        st.stance_valid[f] = np.where(live, np.where(c, np.where(touchdown, 1, st.stance_valid[f]), 0), 0).astype(np.uint8)
        st.prev_contact[f] = np.where(live, np.where(c, GROUND, AIR), UNKNOWN).astype(np.uint8)
    return st


def reduce(st, group, num_groups):
    """((G, 4 * 12 + 1, 6) fp64 result table, (G, 4, 16, 2) fp64 profile table) of go1feet_reduce"""
    group = np.asarray(group)
    out = np.zeros((num_groups, ROWS, len(E.FIELDS)))
    profile = np.zeros((num_groups, FEET, BINS, 2))
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    slices = E.REDUCE_THREADS // BINS
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
        out[g, :FEET * M] = rows
        per_env = np.stack([np.ones(st.N), st.steps.astype(np.float64), st.resets.astype(np.float64)])
        out[g, FEET * M, :3] = _combine_rows(per_env, members, np.add, 0.0)
        # the profile: slice k adds the members e = k, k + 16, ... in ascending order; then slice k takes k + 8, + 4, + 2, + 1
        partial = np.zeros((slices, FEET, BINS, 2))
        for e in members:
            partial[e % slices, :, :, 0] += st.profile_sum[:, :, e]
            partial[e % slices, :, :, 1] += st.profile_count[:, :, e].astype(np.float64)
        k = slices // 2
        while k > 0:
            partial[:k] += partial[k:2 * k]
            k //= 2
        profile[g] = partial[0]
    return out, profile


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP = 12, 2
KINDS = ["trot", "resets", "heavy", "slides", "nonfinite", "stands", "frictionless"]
# on the ground (1) or in the air (0) per script step; foot f starts the pattern at step f, so every foot has its own events
PATTERN = [1, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 0]


def script_config():
    return config(dt=0.02, terrain_friction=0.7, max_contact_force=100.0, warmup_steps=SCRIPT_WARMUP)


def scripted_steps(rng, N, steps=SCRIPT_STEPS):
    """`steps` snapshots of the input buffers for N environments and the kind of every environment: feet that trot through PATTERN
    (touchdowns, stances of one to three steps, lift-offs; the phase advances with the step); environments that reset on the first
    step, mid-script and twice in a row (episode_length_buf starts again, so the warm-up applies again); heavy ones (forces beyond
    max_contact_force, downward speeds beyond -100); ones that slide on one ulp either side of the contact threshold; ones that carry
    +-inf and NaN in each input; ones that stand on all four feet throughout; ones without friction of their own on a ground with
    some, and with phases outside [0, 1).  Returns (config, snapshots, kind)."""
    cfg = script_config()
    kind = rng.integers(0, len(KINDS), N)
    kind[:min(N, len(KINDS))] = np.arange(len(KINDS))[:N]
    bad = np.array([np.inf, -np.inf, np.nan], f32)
    one = f32(1.0)
    edge = np.array([one, np.nextafter(one, f32(2)), np.nextafter(one, f32(0)), 0.0, -0.0, -5.0, 30.0], f32)
    phases = np.array([0.0, 0.0625, 0.9999999, 1.0, -0.1, 1e30, -1e30, 0.5], f32)
    age = np.zeros(N, np.int32)
    mu = rng.uniform(0.1, 3.0, N).astype(f32)
    mu[kind == 6] = 0.0
    snaps = []
    for t in range(steps):
        s = dict(contact_forces=(3.0 * rng.standard_normal((51, N))).astype(f32), foot_velocities=(0.5 * rng.standard_normal((12, N))).astype(f32),
                 prev_foot_velocities=(1.5 * rng.standard_normal((12, N))).astype(f32), foot_indices=rng.random((4, N)).astype(f32),
                 friction_coeffs=mu.copy())
        for f in range(FEET):
            z = 12 * (f + 1) + 2
            down = PATTERN[(t + f) % len(PATTERN)] == 1
            load = rng.uniform(20.0, 90.0, N).astype(f32) if down else rng.uniform(-0.5, 0.9, N).astype(f32)
            s["contact_forces"][z] = load
            s["foot_indices"][f] = f32(((t + 3 * f) % 12) / 12.0) + (rng.random(N) * 0.01).astype(f32)
            k = t * FEET + f                                                # every (step, foot) another value
            s["contact_forces"][z, kind == 2] = load[kind == 2] * f32(4.0)
            s["contact_forces"][z - 1, kind == 2] = f32(150.0)
            s["prev_foot_velocities"][3 * f + 2, kind == 2] = f32((-250.0, -100.0, 3.0, -0.5)[k % 4])
            s["contact_forces"][z, kind == 3] = edge[(k * 3) % len(edge)]
            s["contact_forces"][z, kind == 5] = f32(30.0) + f32(k % 5)
            which = ("contact_forces", "foot_velocities", "prev_foot_velocities", "foot_indices")[k % 4]
            rows = dict(contact_forces=z - (k // 4) % 3, foot_velocities=3 * f + (k // 4) % 2, prev_foot_velocities=3 * f + 2, foot_indices=f)
            if (k // 2) % 2 == 0:                                           # half of the (step, foot) pairs carry one bad value
                s[which][rows[which], kind == 4] = bad[(k // 4) % 3]
            s["foot_indices"][f, kind == 6] = phases[k % len(phases)]
        reset = (kind == 1) & np.isin(t, (0, 5, 8, 9)) | (rng.random(N) < 0.03)
        s["reset_buf"] = np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8)
        age = np.where(reset, 0, age + 1).astype(np.int32)
        s["episode_length_buf"] = age.copy()
        snaps.append(s)
    return cfg, snaps, kind


def run(cfg, snaps, N):
    st = State(N)
    for s in snaps:
        accumulate(st, cfg, s)
    return st
