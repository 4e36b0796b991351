"""TEST INFRASTRUCTURE: numpy model of libgo1spectrum's kernels, written from the text of include/go1spectrum.h (the forty signals, the
ring and the segment's validity, the mean, the direct DFT with k outer and t inner, the one-sided density, the total, the peak, the five
rows, the density sum, the folding rule, the metric rows, the group row and the two density tables).  Every value is formed in np.float32
in the header's operation order and summed in float64 where the header says so, so accumulators, state, density sums and the result
tables are compared with the kernels' bit for bit.  The tables (taper, twiddles, scale, frequencies) are formed here as the header writes
them: in fp64, rounded once to fp32.  The metric-row reduction is joint_ref.py's (eval_ref.py's fixed order, vectorised over the rows)."""
import types

import numpy as np

import eval_ref as E
from joint_ref import _combine_rows

S, NUM = 40, 5
ROWS = S * NUM
TABLE_ROWS = ROWS + 1
METRICS = ["power", "peak_freq", "peak_share", "high_share", "centroid"]
POWER, PEAK_FREQ, PEAK_SHARE, HIGH_SHARE, CENTROID = range(5)
GROUP_FIELDS = ["envs", "steps", "resets", "segments", "segments_dropped"]
# the buffers go1spectrum_record reads (SoA, [k][N]), the host's tables, and the state arrays
INPUTS = ["actions", "torques", "dof_vel", "base_ang_vel", "base_lin_vel", "reset_buf", "episode_length_buf"]
TABLES = ["tw_re", "tw_im", "scale", "freq"]
STATE = ["ring", "valid", "steps", "resets", "segments", "segments_dropped", "psd_sum", "psd_segments"]
SHAPES_OF_INPUTS = dict(actions=12, torques=12, dof_vel=12, base_ang_vel=3, base_lin_vel=3)
f32 = np.float32


def taper(W, name="hann"):
    """w[t] in fp64: periodic Hann or boxcar"""
    assert name in ("hann", "boxcar")
    t = np.arange(W, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * t / W) if name == "hann" else np.ones(W)


def tables(W, dt, name="hann"):
    """the four tables of the header as fp32 arrays; the angle 2 pi k t / W is taken at (k t) mod W, which is the same angle"""
    F, fs = W // 2 + 1, 1.0 / dt
    w = taper(W, name)
    k, t = np.arange(F, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    angle = 2.0 * np.pi * ((k * t) % W).astype(np.float64) / W
    scale = np.full(F, 2.0 / (fs * (w * w).sum()))
    scale[0] *= 0.5
    scale[F - 1] *= 0.5
    return dict(tw_re=(w * np.cos(angle)).astype(f32), tw_im=(-w * np.sin(angle)).astype(f32), scale=scale.astype(f32),
                freq=(np.arange(F, dtype=np.float64) * fs / W).astype(f32))


def config(segment_steps=100, warmup_steps=0, high_freq=10.0, taper_name="hann", dt=0.02, high_bin=None):
    """what Go1SpectrumConfig says, and the tables that go with it"""
    W = int(segment_steps)
    assert W % 2 == 0 and 8 <= W <= 128
    tb = tables(W, dt, taper_name)
    if high_bin is None:
        high_bin = int(np.nonzero(tb["freq"].astype(np.float64) >= high_freq)[0][0])
    return types.SimpleNamespace(warmup_steps=warmup_steps, segment_steps=W, bins=W // 2 + 1, high_bin=high_bin, bin_width=f32(1.0 / dt / W), dt=dt,
                                 taper=taper_name, high_freq=high_freq, tables=tb)


def signals(snap):
    """the forty signals of a step, (40, N) fp32"""
    return np.concatenate([snap["actions"], snap["torques"], snap["dof_vel"], snap["base_ang_vel"], snap["base_lin_vel"][2:3]]).astype(f32, copy=False)


class State:
    """the accumulators and the state after go1spectrum_clear, in the kernel's own number formats (the ring starts at 0 here; the clear
    leaves it as it is and nothing reads a word of it before it is written)"""

    def __init__(self, N, W):
        self.N, self.W, self.F = N, W, W // 2 + 1
        self.count, self.nonfinite = np.zeros((ROWS, N), np.uint32), np.zeros((ROWS, N), np.uint32)
        self.sum, self.sumsq = np.zeros((ROWS, N)), np.zeros((ROWS, N))
        self.min, self.max = np.full((ROWS, N), np.inf, f32), np.full((ROWS, N), -np.inf, f32)
        self.ring = np.zeros((W, S, N), f32)
        self.valid = np.zeros(N, np.uint8)
        self.steps, self.resets, self.segments, self.segments_dropped = (np.zeros(N, np.uint32) for _ in range(4))
        self.psd_sum, self.psd_segments = np.zeros((S, self.F, N)), np.zeros((S, N), np.uint32)
        self.calls = 0

    def fold(self, m, live, v):
        """fold the (40, N) np.float32 values v into row m of every signal (accumulator rows m, 5 + m, ...) where `live`"""
        assert v.dtype == f32 and v.shape == (S, self.N)
        fin = np.isfinite(v)
        ok = live & fin
        self.nonfinite[m::NUM] += (live & ~fin).astype(np.uint32)
        self.count[m::NUM] += ok.astype(np.uint32)
        v64 = v.astype(np.float64)
        with np.errstate(all="ignore"):
            np.add(self.sum[m::NUM], v64, out=self.sum[m::NUM], where=ok)
            np.add(self.sumsq[m::NUM], v64 * v64, out=self.sumsq[m::NUM], where=ok)
            np.fmin(self.min[m::NUM], v, out=self.min[m::NUM], where=ok)
            np.fmax(self.max[m::NUM], v, out=self.max[m::NUM], where=ok)

    def arrays(self):
        return {k: getattr(self, k) for k in ["count", "sum", "sumsq", "min", "max", "nonfinite"] + STATE}


def record(st, cfg, snap, slot):
    """one go1spectrum_record launch"""
    assert 0 <= slot < cfg.segment_steps
    st.ring[slot] = signals(snap)
    reset = snap["reset_buf"] != 0
    st.steps += 1
    st.resets += reset.astype(np.uint32)
    live = ~reset & (snap["episode_length_buf"] > cfg.warmup_steps)
    st.valid = (live if slot == 0 else (st.valid != 0) & live).astype(np.uint8)
    return live


def transform(x, cfg):
    """steps 1 to 3 of the fold on the samples x (W, ...) fp32: {"mean", "y", "re", "im", "P" (F, ...), "total", "kp", "best"}, every
    operation an fp32 operation in the header's order"""
    W, F = cfg.segment_steps, cfg.bins
    tb = cfg.tables
    assert x.dtype == f32 and x.shape[0] == W
    tail = (1,) * (x.ndim - 1)
    with np.errstate(all="ignore"):
        total = np.zeros(x.shape[1:], f32)
        for t in range(W):
            total = total + x[t]
        mean = total / f32(W)
        y = x - mean
        re, im = np.zeros((F,) + x.shape[1:], f32), np.zeros((F,) + x.shape[1:], f32)
        for t in range(W):                                                   # every k at once: per k the additions are in ascending t
            re = re + y[t] * tb["tw_re"][:, t].reshape((F,) + tail)
            im = im + y[t] * tb["tw_im"][:, t].reshape((F,) + tail)
        P = (re * re + im * im) * tb["scale"].reshape((F,) + tail)
        assert y.dtype == f32 and re.dtype == f32 and P.dtype == f32
        total = np.zeros(x.shape[1:], f32)
        for k in range(1, F):
            total = total + P[k]
        kp, best = np.ones(x.shape[1:], np.int64), P[1].copy()
        for k in range(2, F):
            wins = P[k] > best                                               # a NaN never wins
            kp, best = np.where(wins, k, kp), np.where(wins, P[k], best)
    return dict(mean=mean, y=y, re=re, im=im, P=P, total=total, kp=kp, best=best)


def fold(st, cfg):
    """one go1spectrum_fold launch.  Returns what it did: the transform of every (signal, environment) and "valid", "rows" (5, 40, N)"""
    W, F, N = cfg.segment_steps, cfg.bins, st.N
    tb = cfg.tables
    ok = st.valid != 0
    st.segments_dropped += (~ok).astype(np.uint32)
    st.segments += ok.astype(np.uint32)
    d = transform(st.ring, cfg)
    P, total = d["P"], d["total"]
    finite = np.isfinite(total)
    with np.errstate(all="ignore"):
        good = finite & (total > f32(0.0))
        nan = np.full(total.shape, np.nan, f32)
        power = total * cfg.bin_width
        peak_freq = np.where(good, tb["freq"][d["kp"]], nan)
        peak_share = np.where(good, d["best"] / total, nan)
        high = np.zeros(total.shape, f32)
        for k in range(cfg.high_bin, F):
            high = high + P[k]
        cen = np.zeros(total.shape, f32)
        for k in range(1, F):
            cen = cen + tb["freq"][k] * P[k]
        high_share, centroid = np.where(good, high / total, nan), np.where(good, cen / total, nan)
    rows = [power, peak_freq, peak_share, high_share, centroid]
    live = np.broadcast_to(ok, (S, N))
    for m, v in enumerate(rows):
        st.fold(m, live, v.astype(f32, copy=False))
    enters = live & finite
    with np.errstate(all="ignore"):
        np.add(st.psd_sum, np.moveaxis(P, 0, 1).astype(np.float64), out=st.psd_sum, where=enters[:, None, :])
    st.psd_segments += enters.astype(np.uint32)
    d.update(valid=ok, rows=np.stack(rows), enters=enters)
    return d


def accumulate(st, cfg, snap):
    """what the host's accumulate() does with a step: the record of slot = calls mod W, and after slot W - 1 the fold (None otherwise)"""
    slot = st.calls % cfg.segment_steps
    record(st, cfg, snap, slot)
    st.calls += 1
    return fold(st, cfg) if slot == cfg.segment_steps - 1 else None


def run(cfg, snaps, N):
    """(the state after the snapshots, what every fold did)"""
    st, folds = State(N, cfg.segment_steps), []
    for s in snaps:
        d = accumulate(st, cfg, s)
        if d is not None:
            folds.append(d)
    return st, folds


def reduce(st, group, num_groups):
    """((G, 200 + 1, 6) fp64 result table, (G, 40, F) density sums, (G, 40) segment counts) of go1spectrum_reduce"""
    group = np.asarray(group)
    out = np.zeros((num_groups, TABLE_ROWS, len(E.FIELDS)))
    psd, counts = np.zeros((num_groups, S, st.F)), np.zeros((num_groups, S))
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    for g in range(num_groups):
        members = [int(e) for e in np.nonzero(group == g)[0]]
        n = _combine_rows(st.count.astype(np.float64), members, np.add, 0.0)
        nf = _combine_rows(st.nonfinite.astype(np.float64), members, np.add, 0.0)
        sums, squares = _combine_rows(st.sum, members, np.add, 0.0), _combine_rows(st.sumsq, members, np.add, 0.0)
        low, high = _combine_rows(lows, members, np.fmin, np.inf), _combine_rows(highs, members, np.fmax, -np.inf)
        some = n > 0
        with np.errstate(all="ignore"):
            mean = sums / n
            var = squares / n - mean * mean
            rows = np.stack([n, mean, np.sqrt(np.fmax(var, 0.0)), low, high, nf], axis=1)
        rows[~some, 1:5] = np.nan
        out[g, :ROWS] = rows
        per_env = np.stack([np.ones(st.N)] + [getattr(st, k).astype(np.float64) for k in ("steps", "resets", "segments", "segments_dropped")])
        out[g, ROWS, :5] = _combine_rows(per_env, members, np.add, 0.0)
        with np.errstate(all="ignore"):
            psd[g] = _combine_rows(st.psd_sum.reshape(S * st.F, st.N), members, np.add, 0.0).reshape(S, st.F)
        counts[g] = _combine_rows(st.psd_segments.astype(np.float64), members, np.add, 0.0)
    return out, psd, counts


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_WARMUP, START_AGE = 2, 50
KINDS = ["walks", "sines", "resets", "late_reset", "nonfinite", "constant", "huge", "tie"]
WALKS, SINES, RESETS, LATE_RESET, NONFINITE, CONSTANT, HUGE, TIE = range(len(KINDS))
# the nonfinite kind: (signal, step within segment 1, value): one sample each
BAD_SAMPLES = [(5, 3, np.nan), (17, 4, np.inf), (30, 5, -np.inf)]


def sine_bin(s, W):
    """the bin of signal s's on-bin sine: in [2, W / 2 - 2], differing by signal as far as the window has room"""
    return 2 + s % (W // 2 - 3)


def constant_value(s):
    """the constant of signal s: a multiple of 1 / 4, so that the fp32 sum of W of them and its quotient by W are exact"""
    return f32((s - 20) * 0.25)


def script_steps(W):
    return 3 * W + 2


def scripted_steps(rng, N, W):
    """3 W + 2 snapshots of the input buffers for N environments and the kind of every environment: one clean segment, one that the
    kinds spoil, one clean again, and two steps of a segment that is never closed.  Kinds: random walks in every signal; an on-bin sine
    sin(2 pi k0 t / W) in every signal throughout, k0 = sine_bin(s, W); resets on the first step of the second segment, in its middle and
    on the step after that (episode_length_buf starts again, so with a warm-up of 2 the steps after a reset are dead without being
    resets); a reset on the last step of the second segment, whose warm-up spoils the third segment too; one NaN, one +inf and one -inf,
    each in a single sample of a single signal of the second segment (BAD_SAMPLES); constant signals throughout; samples of +-1e20 in the
    second segment, whose densities overflow; and in the second segment the pair of impulses x[0] = 2, x[W / 2] = -2, whose odd bins have
    exactly equal power.  Returns (snapshots, kind)."""
    steps = script_steps(W)
    kind = rng.integers(0, len(KINDS), N)
    kind[:min(N, len(KINDS))] = np.arange(len(KINDS))[:N]
    walk = np.cumsum((0.1 * rng.standard_normal((steps, S, N))).astype(f32), axis=0, dtype=f32)
    t = np.arange(steps, dtype=np.float64)
    k0 = np.array([sine_bin(s, W) for s in range(S)], np.float64)
    sine = np.sin(2.0 * np.pi * ((k0[None, :] * t[:, None]) % W) / W).astype(f32)                 # (steps, S)
    x = walk.copy()
    x[:, :, kind == SINES] = sine[:, :, None]
    x[:, :, kind == CONSTANT] = np.array([constant_value(s) for s in range(S)], f32)[None, :, None]
    second = slice(W, 2 * W)
    for s, at, value in BAD_SAMPLES:
        x[W + at, s, kind == NONFINITE] = value
    huge = kind == HUGE
    first_sign = np.where(rng.random((1, S, int(huge.sum()))) < 0.5, f32(1e20), f32(-1e20))   # +-1e20 in alternation: never a constant
    x[second, :, huge] = first_sign * np.where(np.arange(W) % 2 == 0, f32(1.0), f32(-1.0))[:, None, None]
    tie = np.zeros((W, S), f32)
    tie[0], tie[W // 2] = 2.0, -2.0
    x[second, :, kind == TIE] = tie[:, :, None]
    resets = {RESETS: (W, W + W // 2, W + W // 2 + 1), LATE_RESET: (2 * W - 1,)}
    age = np.full(N, START_AGE, np.int32)
    snaps = []
    for step in range(steps):
        reset = np.zeros(N, bool)
        for k, at in resets.items():
            reset |= (kind == k) & (step in at)
        age = np.where(reset, 0, age + 1).astype(np.int32)
        lin = (3.0 * rng.standard_normal((3, N))).astype(f32)                # rows 0 and 1 are read by nobody
        lin[2] = x[step, 39]
        snaps.append(dict(actions=x[step, 0:12].copy(), torques=x[step, 12:24].copy(), dof_vel=x[step, 24:36].copy(), base_ang_vel=x[step, 36:39].copy(),
                          base_lin_vel=lin, reset_buf=np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8), episode_length_buf=age.copy()))
    return snaps, kind
