"""TEST INFRASTRUCTURE: numpy model of libgo1gait's kernels, written from the text of include/go1gait.h (the fifteen rows, the contact
and touchdown rule, the reference stride of FL with its chatter and its length limit, the touchdown phases against the gait clocks, the
two kinds of histogram, the folding rule, the metric rows, the group row and the histogram table).  Every value is formed in np.float32
in the header's operation order and summed in float64, so accumulators, state, histograms and both result tables are compared with the
kernels' bit for bit.  The metric-row reduction is joint_ref.py's (eval_ref.py's fixed order, vectorised over the rows); the histograms'
own order (the foot profile's) is restated here."""
import types

import numpy as np

import eval_ref as E
from joint_ref import _combine_rows

FEET = ["FL", "FR", "RL", "RR"]
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
METRICS = [f"sync_{FEET[i]}_{FEET[j]}" for i, j in PAIRS] + [f"phase_err_{f}" for f in FEET[1:]] + [f"phase_abs_err_{f}" for f in FEET[1:]] + \
          [f"touchdowns_{f}" for f in FEET[1:]]
SYNC, PHASE_ERR, PHASE_ABS_ERR, TOUCHDOWNS = 0, 6, 9, 12                    # the first row of each kind; + k for foot k + 1
M, BINS, HISTS = len(METRICS), 16, 4
ROWS = M + 1
GROUP_FIELDS = ["envs", "steps", "resets", "strides", "strides_dropped"]
# the buffers go1gait_accumulate reads (SoA, [k][N])
INPUTS = ["contact_forces", "foot_indices", "reset_buf", "episode_length_buf"]
STATE = ["prev_contact", "ref_steps", "last_td", "td_count", "steps", "resets", "strides", "strides_dropped", "support_hist", "phase_hist"]
AIR, GROUND, UNKNOWN = 0, 1, 2
f32 = np.float32


def config(warmup_steps=0, min_stride_steps=1, max_stride_steps=100):
    """what Go1GaitConfig says"""
    return types.SimpleNamespace(warmup_steps=warmup_steps, min_stride_steps=min_stride_steps, max_stride_steps=max_stride_steps)


def raw_phase_bin(p):
    """floorf(p * 16 + 0.5) of the np.float32 values p, before the wrap: 0 .. 16"""
    b = np.floor(p * f32(16.0) + f32(0.5))
    assert b.dtype == f32
    return b


def phase_bin(p):
    """the histogram bin of the np.float32 phases p: a value outside [1, 15] becomes 0 as a float, then converted"""
    b = raw_phase_bin(p)
    return np.where((b >= f32(1.0)) & (b <= f32(BINS - 1)), b, f32(0.0)).astype(np.int64)


class State:
    """the accumulators and the state after go1gait_clear, in the kernel's own number formats"""

    def __init__(self, N):
        self.N = N
        self.count, self.nonfinite = np.zeros((M, N), np.uint32), np.zeros((M, N), np.uint32)
        self.sum, self.sumsq = np.zeros((M, N)), np.zeros((M, N))
        self.min, self.max = np.full((M, N), np.inf, f32), np.full((M, N), -np.inf, f32)
        self.prev_contact = np.full((4, N), UNKNOWN, np.uint8)
        self.ref_steps = np.full(N, -1, np.int32)
        self.last_td, self.td_count = np.full((3, N), -1, np.int32), np.zeros((3, N), np.int32)
        self.steps, self.resets, self.strides, self.strides_dropped = (np.zeros(N, np.uint32) for _ in range(4))
        self.support_hist, self.phase_hist = np.zeros((BINS, N), np.uint32), np.zeros((3, BINS, N), np.uint32)

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


def accumulate(st, cfg, snap):
    """one go1gait_accumulate launch on the SoA buffers `snap` (np.float32 / uint8 / int32 arrays).  Returns what the step did, per
    environment, for the tests that look at single steps: {"live", "contact" (4, N), "closed", "length", "chatter", "dropped", "opened",
    "opening_touchdown", "wrapped", "several", "none", "bad_clock"}"""
    N = st.N
    zero, one = f32(0.0), f32(1.0)
    env = np.arange(N)
    reset = snap["reset_buf"] != 0
    st.steps += 1                                                                        # 1
    st.resets += reset.astype(np.uint32)
    live = ~reset & (snap["episode_length_buf"] > cfg.warmup_steps)                      # 2
    st.prev_contact[:, ~live] = UNKNOWN
    st.ref_steps[~live] = -1
    fz = np.stack([snap["contact_forces"][12 * (f + 1) + 2] for f in range(4)])          # 3
    with np.errstate(invalid="ignore"):
        c = fz > f32(1.0)
    for k, (i, j) in enumerate(PAIRS):
        st.fold(SYNC + k, live, np.where(c[i] == c[j], one, zero))
    mask = sum(c[f].astype(np.int64) << f for f in range(4))
    st.support_hist[mask[live], env[live]] += 1
    td = c & (st.prev_contact == AIR) & live                                             # 4
    ref = st.ref_steps.copy()                                                            # 5
    going = live & (ref >= 0)
    ref[going] += 1
    dropped = going & (ref > cfg.max_stride_steps)
    ref[dropped] = -1
    st.strides_dropped += dropped.astype(np.uint32)
    closed = td[0] & (ref >= cfg.min_stride_steps)                                       # 6
    chatter = td[0] & ~closed & (ref >= 0)
    opened = td[0] & (ref < 0)
    length = np.where(closed, ref, 1).astype(f32)
    fi = snap["foot_indices"]
    wrapped, several, none, bad_clock = (np.zeros(N, bool) for _ in range(4))
    for k in range(3):
        count = st.td_count[k]
        st.fold(TOUCHDOWNS + k, closed, count.astype(f32))
        has = closed & (count >= 1)
        with np.errstate(all="ignore"):
            p = st.last_td[k].astype(f32) / length
            d = fi[0] - fi[k + 1]
            cmd = d - np.floor(d)
            err = p - cmd
            err = err - np.floor(err + f32(0.5))
        assert p.dtype == f32 and err.dtype == f32
        st.fold(PHASE_ERR + k, has, err)
        st.fold(PHASE_ABS_ERR + k, has, np.abs(err))
        safe = np.where(has, p, zero)
        st.phase_hist[k, phase_bin(safe)[has], env[has]] += 1
        wrapped |= has & (raw_phase_bin(safe) == f32(16.0))
        several |= closed & (count >= 2)
        none |= closed & (count == 0)
        bad_clock |= has & ~np.isfinite(err)
    st.strides += closed.astype(np.uint32)
    fresh = closed | opened
    ref[fresh] = 0
    st.ref_steps = ref.astype(np.int32)
    opening_touchdown = np.zeros(N, bool)
    for k in range(3):                                                                   # 7
        hit = td[k + 1] & (ref >= 0)
        st.last_td[k] = np.where(fresh, np.where(hit, 0, -1), np.where(hit, ref, st.last_td[k])).astype(np.int32)
        st.td_count[k] = np.where(fresh, np.where(hit, 1, 0), np.where(hit, st.td_count[k] + 1, st.td_count[k])).astype(np.int32)
        opening_touchdown |= fresh & hit
    st.prev_contact = np.where(live, np.where(c, GROUND, AIR), UNKNOWN).astype(np.uint8)   # 8
    return dict(live=live, contact=c, closed=closed, length=np.where(closed, length.astype(np.int64), 0), chatter=chatter, dropped=dropped,
                opened=opened, opening_touchdown=opening_touchdown, wrapped=wrapped, several=several, none=none, bad_clock=bad_clock)


def reduce(st, group, num_groups):
    """((G, 15 + 1, 6) fp64 result table, (G, 4, 16) fp64 histogram table) of go1gait_reduce"""
    group = np.asarray(group)
    out = np.zeros((num_groups, ROWS, len(E.FIELDS)))
    hist = np.zeros((num_groups, HISTS, BINS))
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    slices = E.REDUCE_THREADS // BINS
    words = np.concatenate([st.support_hist[None], st.phase_hist]).astype(np.float64)    # (4, 16, N): histogram 0 is the support pattern
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
        out[g, :M] = rows
        per_env = np.stack([np.ones(st.N)] + [getattr(st, k).astype(np.float64) for k in ("steps", "resets", "strides", "strides_dropped")])
        out[g, M, :5] = _combine_rows(per_env, members, np.add, 0.0)
        # a histogram: slice k adds the members e = k, k + 16, ... in ascending order; then slice k takes k + 8, + 4, + 2, + 1
        partial = np.zeros((slices, HISTS, BINS))
        for e in members:
            partial[e % slices] += words[:, :, e]
        k = slices // 2
        while k > 0:
            partial[:k] += partial[k:2 * k]
            k //= 2
        hist[g] = partial[0]
    return out, hist


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP, SCRIPT_MIN_STRIDE, SCRIPT_MAX_STRIDE = 96, 2, 3, 40
KINDS = ["trots", "resets", "chatters", "slow", "nonfinite", "stands", "threshold"]
TROT_PERIOD, CHATTER_PERIOD = 10, 12
# the slow kind, by step: FL touches down at 3, at 35 (a stride of 32 steps: RR's touchdown at its step 31 is phase 31/32, bin 16 -> 0), at
# 80 (45 steps later: the stride outgrew 40 steps at step 76 and was dropped; this touchdown opens one) and at 90 (a stride of 10 steps)
SLOW_FL, SLOW_RR = (3, 4, 5, 35, 36, 37, 80, 81, 82, 90, 91), (34,)


def script_config():
    return config(warmup_steps=SCRIPT_WARMUP, min_stride_steps=SCRIPT_MIN_STRIDE, max_stride_steps=SCRIPT_MAX_STRIDE)


def _on_ground(kind, t, f):
    """whether foot f of an environment of `kind` is on the ground at script step t (the threshold kind has forces of its own)"""
    if kind in (0, 1, 4):                                                    # a trot of ten steps: FL + RR, then FR + RL
        return (t + (TROT_PERIOD // 2) * (f in (1, 2))) % TROT_PERIOD < TROT_PERIOD // 2
    if kind == 2:
        # FL and RR touch down at phase 0 and again at phase 2 (chatter inside min_stride_steps = 3; RR's first is on the opening step);
        # FR touches down four times a stride; RL never leaves the ground: no touchdown at all
        phase = t % CHATTER_PERIOD
        return (phase in (0, 2, 3, 4, 5), phase in (1, 4, 7, 10), True, phase in (0, 2, 3, 4, 5))[f]
    if kind == 3:                                                            # FR stays in the air, RL on the ground: neither touches down
        return (t in SLOW_FL, False, True, t in SLOW_RR)[f]
    return True                                                              # stands


def scripted_steps(rng, N, steps=SCRIPT_STEPS):
    """`steps` snapshots of the input buffers for N environments and the kind of every environment: ones that trot with gait clocks
    that match (strides of ten steps close one after the other; RR touches down on every opening step); ones that trot and reset on
    the first step, mid-script and twice in a row (episode_length_buf starts again, so the warm-up applies again); ones whose FL and RR
    chatter two steps after a touchdown, whose FR touches down four times a stride and whose RL never does; slow ones with a stride
    of 32 steps (a touchdown at phase 31 / 32: bin 16 -> 0), one that outgrows max_stride_steps and is dropped, and one of ten; ones
    that trot with +-inf and NaN in the forces and in the gait clocks (on closing steps too); ones that stand throughout; ones whose
    feet carry one ulp either side of the contact threshold.  Returns (config, snapshots, kind)."""
    cfg = script_config()
    kind = rng.integers(0, len(KINDS), N)
    kind[:min(N, len(KINDS))] = np.arange(len(KINDS))[:N]
    bad = np.array([np.inf, -np.inf, np.nan], f32)
    one = f32(1.0)
    edge = np.array([one, np.nextafter(one, f32(2)), np.nextafter(one, f32(0)), 0.0, -0.0, -5.0, 30.0], f32)
    age = np.zeros(N, np.int32)
    snaps = []
    for t in range(steps):
        s = dict(contact_forces=(3.0 * rng.standard_normal((51, N))).astype(f32), foot_indices=rng.random((4, N)).astype(f32))
        for f in range(4):
            z = 12 * (f + 1) + 2
            down = np.array([_on_ground(int(k), t, f) for k in kind])
            s["contact_forces"][z] = np.where(down, rng.uniform(20.0, 90.0, N), rng.uniform(-0.5, 0.9, N)).astype(f32)
            trotting = np.isin(kind, (0, 1, 4))                              # the clocks of the trot: FR and RL half a cycle from FL and RR
            clock = f32(((t + (TROT_PERIOD // 2) * (f in (1, 2))) % TROT_PERIOD) / TROT_PERIOD) + (rng.random(N) * 0.01).astype(f32)
            s["foot_indices"][f, trotting] = clock[trotting]
            s["contact_forces"][z, kind == 6] = edge[((t * 4 + f) * 3) % len(edge)]
        odd = kind == 4
        if t % 2 == 0:                                                       # every closing step (a multiple of ten) among them
            s["foot_indices"][(t // 2) % 4, odd] = bad[(t // 2) % 3]
        if t % 7 == 3:
            s["contact_forces"][12 * ((t // 7) % 4 + 1) + 2, odd] = bad[(t // 7) % 3]
        reset = (kind == 1) & np.isin(t, (0, 23, 24, 50)) | np.isin(kind, (0, 1, 6)) & (rng.random(N) < 0.01)
        s["reset_buf"] = np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8)
        age = np.where(reset, 0, age + 1).astype(np.int32)
        s["episode_length_buf"] = age.copy()
        snaps.append(s)
    return cfg, snaps, kind


def run(cfg, snaps, N):
    """(the state after the snapshots, what every step did)"""
    st, did = State(N), []
    for s in snaps:
        did.append(accumulate(st, cfg, s))
    return st, did
