"""CPU checks of the push and the disturbance recovery (include/go1eval.h, fourth kernel family): the ctypes mirrors against the
header, argument and window refusals without a GPU, the model of tests/recovery_ref.py on hand-computable pushes and traces,
go1eval.hip itself under the SIMT emulator against that model (analysis and reduction bit for bit, the push within its derived
bound), the environment hooks where there is no GPU, the host classes, and the sweep's host pieces."""
import ctypes
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import recovery_ref as P
from test_response_trace import C_TYPES, HEADER, REPO, eval_emu, bits, enum_order, struct_fields

NAN = float("nan")
f32 = np.float32


# ---- 1. the mirrors against the header ---------------------------------------------------------------------------------------------
def test_push_and_recovery_mirrors_match_the_header():
    import go1eval_host as G
    src = open(HEADER).read()
    for macro, value in (("NUM_PUSH", G.NUM_PUSH), ("NUM_RECOVERY", G.NUM_RECOVERY), ("NUM_TRACE", 24)):
        assert f"#define GO1EVAL_{macro} {value}" in src
    for struct in (G.Go1PushConfig, G.Go1RecoveryConfig):
        want = struct_fields(src, struct.__name__)
        assert [f for f, _ in want] == [f for f, _ in struct._fields_], struct.__name__
        for (field, ctext), (_, ctype) in zip(want, struct._fields_):
            assert ctype is C_TYPES[ctext], (struct.__name__, field)
    for struct in (G.Go1PushBuffers, G.Go1RecoveryBuffers):
        want = struct_fields(src, struct.__name__)
        assert [f for f, _ in want] == [f for f, _ in struct._fields_], struct.__name__
        assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in struct._fields_)
    assert enum_order(src, "Go1PushRow", "GO1PUSH_") == G.PUSH_ROWS == P.PUSH_ROWS and len(P.PUSH_ROWS) == G.NUM_PUSH
    assert enum_order(src, "Go1RecoveryMetric", "GO1RECOVERY_") == G.RECOVERY_METRICS == P.VALUES and len(P.VALUES) == G.NUM_RECOVERY == 8
    assert enum_order(src, "Go1RecoveryStatus", "GO1RECOVERY_S_") == G.RECOVERY_STATUS == P.STATUS
    assert enum_order(src, "Go1RecoveryGroupField", "GO1RECOVERY_G_") == G.RECOVERY_GROUP_FIELDS == P.GROUP_FIELDS
    assert set(G.EXPORTED_SYMBOLS) >= {"go1eval_push", "go1eval_recovery", "go1eval_recovery_reduce"}
    ch = G.TRACE_CHANNELS.index
    assert (P.VX, P.VY, P.WZ, P.HEIGHT, P.CMD_VX, P.CMD_VY, P.CMD_WZ, P.RESET) == tuple(
        ch(n) for n in ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "base_height", "cmd_lin_vel_x", "cmd_lin_vel_y", "cmd_ang_vel_yaw", "reset"))
    # the existing layouts are as they were
    assert ctypes.sizeof(G.Go1ResponseConfig) == 11 * 4 + G.MAX_SIGNALS * 16 and ctypes.sizeof(G.Go1TraceConfig) == 20


# ---- 2. argument and window refusals without a GPU -----------------------------------------------------------------------------------
ROWS, P0, PRE, W, HOLD, DT, BAND = 40, 10, 8, 5, 5, 0.02, 0.1


def _recovery_cfg(G, **over):
    c = G.Go1RecoveryConfig()
    c.num_traced, c.rows, c.push_row, c.pre, c.smooth, c.hold, c.band, c.dt, c.num_groups = 4, ROWS, P0, PRE, W, HOLD, BAND, DT, 1
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_push_and_recovery_arguments_are_checked_before_any_launch():
    import __graft_entry__ as g
    import go1eval_host as G
    g.build_eval_hip()
    lib = G.load_library()
    ref = ctypes.byref
    cfg, buf = G.Go1PushConfig(), G.Go1PushBuffers()
    assert lib.go1eval_push(None, None, None) == -1
    assert lib.go1eval_push(ref(cfg), ref(buf), None) == -1                     # num_envs = 0
    cfg.num_envs = 8
    assert lib.go1eval_push(ref(cfg), ref(buf), None) == -2                     # nobody is pushed
    cfg.num_pushed = 5
    assert lib.go1eval_push(ref(cfg), ref(buf), None) == -2                     # no root_states, no table
    anything = np.zeros(13 * 8, np.float32)
    buf.root_states = anything.ctypes.data
    assert lib.go1eval_push(ref(cfg), ref(buf), None) == -2                     # no table
    buf.push = anything.ctypes.data
    assert lib.go1eval_push(ref(cfg), ref(buf), None) == -8                     # a subset without its ids
    assert not anything.any()

    rbuf = G.Go1RecoveryBuffers()
    for fn in (lib.go1eval_recovery, lib.go1eval_recovery_reduce):
        assert fn(None, None, None) == -1
        assert fn(ref(_recovery_cfg(G, num_traced=0)), ref(rbuf), None) == -1
        assert fn(ref(_recovery_cfg(G)), ref(rbuf), None) == -2                 # no outputs
    rbuf.values = rbuf.status = anything.ctypes.data
    assert lib.go1eval_recovery(ref(_recovery_cfg(G)), ref(rbuf), None) == -3   # no trace
    assert lib.go1eval_recovery_reduce(ref(_recovery_cfg(G)), ref(rbuf), None) == -5      # no group, no table
    rbuf.group = rbuf.results = anything.ctypes.data
    assert lib.go1eval_recovery_reduce(ref(_recovery_cfg(G, num_groups=0)), ref(rbuf), None) == -5
    rbuf.trace = anything.ctypes.data
    refused = [dict(pre=11), dict(pre=0, smooth=1), dict(push_row=40), dict(push_row=7), dict(smooth=0), dict(smooth=10), dict(hold=0),
               dict(hold=31), dict(dt=0.0), dict(band=-0.1), dict(band=NAN)]
    # p0 - pre < 0, no baseline row, p0 >= rows, p0 - pre < 0, w < 1, w > pre + 1, hold < 1, hold > rows - p0, ...
    for over in refused:
        assert lib.go1eval_recovery(ref(_recovery_cfg(G, **over)), ref(rbuf), None) == -11, over
        assert not P.window_ok(*[over.get(k, d) for k, d in (("rows", ROWS), ("push_row", P0), ("pre", PRE), ("smooth", W), ("hold", HOLD),
                                                             ("band", BAND), ("dt", DT))]), over
    assert P.window_ok(ROWS, P0, PRE, W, HOLD, BAND, DT) and P.window_ok(ROWS, P0, PRE, PRE + 1, ROWS - P0, 0.0, DT) and P.window_ok(9, 8, 8, 9, 1, 0.0, DT)
    assert not anything.any()


# ---- 3. the push model by hand -----------------------------------------------------------------------------------------------------
def roots(quats):
    """(13, N) root_states at rest with the attitudes `quats` (xyzw)"""
    r = np.zeros((13, len(quats)))
    r[3:7] = np.array(quats).T
    return r


IDENTITY = (0.0, 0.0, 0.0, 1.0)
YAW90 = (0.0, 0.0, math.sin(math.pi / 4), math.cos(math.pi / 4))
PITCH30 = (0.0, math.sin(math.pi / 12), 0.0, math.cos(math.pi / 12))


def test_push_model_in_the_heading_frame():
    r = roots([IDENTITY, YAW90, PITCH30])
    r[7:13] = 0.125
    new, written = P.push(r, [[1.0, 0.5, 0.25, -0.5], [1.0, 0.0, 0.0, 0.0], [0.6, 0.8, 0.0, 0.0]])
    assert written.all()
    assert new[[7, 8, 9, 12], 0].tolist() == [1.125, 0.625, 0.375, -0.375]          # identity attitude: forward is +x, left is +y
    assert abs(new[7, 1] - 0.125) < 1e-15 and abs(new[8, 1] - 1.125) < 1e-15        # yawed by 90 degrees: a forward push arrives as +y
    # pitched down by 30 degrees: the forward axis dips, the heading is still +x, and the planar push keeps its commanded speed
    assert np.allclose(P.heading(np.array([PITCH30]).T), ([1.0], [0.0]), atol=1e-15)
    assert abs(np.hypot(new[7, 2] - 0.125, new[8, 2] - 0.125) - 1.0) < 1e-15 and new[9, 2] == 0.125
    assert np.array_equal(new[[0, 1, 2, 3, 4, 5, 6, 10, 11]], r[[0, 1, 2, 3, 4, 5, 6, 10, 11]])
    up = (0.0, -math.sin(math.pi / 4), 0.0, math.cos(math.pi / 4))                  # the nose points straight up: no heading, (1, 0) by rule
    assert [float(h[0]) for h in P.heading(np.array([up]).T)] == [1.0, 0.0]


def test_push_model_zero_rows_subsets_and_ids_out_of_range():
    r = roots([IDENTITY] * 6)
    r[7] = -0.0
    new, written = P.push(r, np.zeros((6, 4)))
    assert not written.any() and np.signbit(new[7]).all() and bits(new) == bits(r)     # a zero row: -0.0 stays -0.0
    new, written = P.push(r, [[0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0], [3.0, 0.0, 0.0, 0.0]],
                          env_ids=[5, 0, 3, 6, -1])                                 # an unordered subset; ids 6 and -1 are skipped
    assert written.tolist() == [True, False, False, False, False, True]
    assert new[12, 5] == 1.0 and new[7, 0] == 1.0 and np.signbit(new[7, 1:5]).all() and new[7, 1:].tolist() == [0.0] * 5
    assert not np.signbit(new[7, 5])                                                # written: -0.0 + 0.0 is +0.0, which is why a zero row is not
    assert P.push_bound([3.0, 4.0, 0.0, 0.0], 2.0) == (16 * 5.0 + 2.0) * 2.0 ** -24


# ---- 4. the analysis model by hand ------------------------------------------------------------------------------------------------
def one_trace(bump=(), offset=0.0, rows=ROWS, p0=P0, channel=P.VX):
    """(rows, 24, 1): commands (1, 0, 0), lin_vel_x = 1 + offset, base height 0.5; `bump` is added to `channel` from row p0 on"""
    t = np.zeros((rows, P.C, 1), np.float32)
    t[:, P.CMD_VX, 0] = 1.0
    t[:, P.VX, 0] = 1.0 + offset
    t[:, P.HEIGHT, 0] = 0.5
    t[p0:p0 + len(bump), channel, 0] += np.asarray(bump, np.float32)
    return t


def analyse(trace, p0=P0, pre=PRE, smooth=1, band=BAND, hold=HOLD):
    values, status = P.recovery(trace, p0, pre, smooth, band, hold, DT)
    return dict(zip(P.VALUES, values[:, 0].tolist())), int(status[0])


TRIANGLE = [0.25, 0.5, 0.75, 1.0, 0.75, 0.5, 0.25]              # height 1, seven rows: every figure below is a dyadic number


def test_model_constant_trace():
    for offset in (0.0, 0.125):
        v, status = analyse(one_trace(offset=offset), smooth=W)
        assert status == 0
        assert v == dict(fell=0.0, peak_vel_err=0.0, peak_time=float(f32(1) * f32(DT)), recovered=1.0, recovery_time=0.0, height_drop=0.0,
                         yaw_rate_dev=0.0, iae_excess=0.0)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_model_triangular_bump(sign):
    """a bump of height 1 over seven rows on a steady tracking offset of 1/8: the offset is the baseline and drops out"""
    t = one_trace([sign * b for b in TRIANGLE], offset=sign * 0.125)
    v, status = analyse(t)
    assert status == 0 and v["fell"] == 0.0
    assert v["peak_vel_err"] == 1.0 and v["peak_time"] == f32(4) * f32(DT)              # the fourth row after the push
    assert v["recovered"] == 1.0 and v["recovery_time"] == f32(7) * f32(DT)             # the seventh row is the last outside 0.1 m/s
    assert v["iae_excess"] == f32(np.float64(f32(DT)) * 4.0) and v["height_drop"] == 0.0 and v["yaw_rate_dev"] == 0.0
    # a box filter of four rows: the mean of (.5, .75, 1, .75) = .75 comes first, (.75, 1, .75, .5) ties it one row later
    v, _ = analyse(t, smooth=4)
    assert v["peak_vel_err"] == 0.75 and v["peak_time"] == f32(5) * f32(DT)
    assert v["recovery_time"] == f32(9) * f32(DT)                                       # (.5, .25, 0, 0) / 4 is the last mean above 0.1
    assert v["iae_excess"] == f32(np.float64(f32(DT)) * 4.0)                            # raw, not smoothed
    # the same bump sideways is the same planar error
    v, _ = analyse(one_trace([sign * b for b in TRIANGLE], channel=P.VY))
    assert v["peak_vel_err"] == 1.0 and v["recovery_time"] == f32(7) * f32(DT)


def test_model_height_drop_and_yaw_rate_deviation():
    t = one_trace([0.0, 0.0, -0.25, -0.125], channel=P.HEIGHT)
    t[P0 + 1, P.WZ, 0], t[P0 + 2, P.WZ, 0] = 0.5, -0.75
    v, status = analyse(t)
    assert status == 0 and v["height_drop"] == 0.25 and v["yaw_rate_dev"] == 0.75 and v["peak_vel_err"] == 0.0 and v["recovery_time"] == 0.0
    v, _ = analyse(t, smooth=2)
    assert v["height_drop"] == 0.1875 and v["yaw_rate_dev"] == 0.375                    # means of (-.25, -.125) and of (-.75, 0)
    t[:, P.WZ, 0] += 0.25                                                              # a steady yaw-rate offset is the baseline
    assert analyse(t)[0]["yaw_rate_dev"] == 0.75


def test_model_status_rules():
    bump = one_trace(TRIANGLE)
    t = bump.copy()
    t[P0 - PRE - 1, P.RESET, 0] = 1.0                                                   # the row before the window: ignored
    v, status = analyse(t)
    assert status == 0 and v["peak_vel_err"] == 1.0
    t = bump.copy()
    t[P0 - 1, P.RESET, 0] = 1.0                                                         # the last baseline row
    v, status = analyse(t)
    assert status == 1 and all(np.isnan(x) for x in v.values())
    t = bump.copy()
    t[P0 + 3, P.RESET, 0] = 1.0                                                         # fell: the reset's row carries its own command draw
    t[P0 + 3, P.CMD_VX:P.CMD_WZ + 1, 0] = [0.3, -0.2, 0.7]
    v, status = analyse(t)
    assert status == 3 and v["fell"] == 1.0 and all(np.isnan(x) for k, x in v.items() if k != "fell")
    t[P0 - PRE, P.RESET, 0] = 1.0                                                       # a spoiled baseline outranks the fall
    assert analyse(t)[1] == 1
    for row, ch in ((P0 + 3, P.CMD_VX), (P0 - 2, P.CMD_VY), (ROWS - 1, P.CMD_WZ)):
        t = bump.copy()
        t[row, ch, 0] += 0.25                                                           # a command change alone
        v, status = analyse(t)
        assert status == 2 and all(np.isnan(x) for x in v.values()), (row, ch)
    t = bump.copy()
    t[P0 - PRE - 1, P.CMD_VX, 0] = 0.25                                                 # outside the window: held
    t[:, 9, 0] = np.arange(ROWS)                                                       # the height command is not looked at
    assert analyse(t)[1] == 0
    t[:, :, 0] = NAN                                                                   # the trace of an id outside the simulator
    assert analyse(t)[1] == 1


def test_model_leaves_the_band_inside_the_hold_rows():
    last = ROWS - P0 - 1
    v, _ = analyse(one_trace([0.0] * (last - HOLD) + [0.5]))                            # the row before the hold rows: recovered at the first of them
    assert v["recovered"] == 1.0 and v["recovery_time"] == f32(last - HOLD + 1) * f32(DT) and v["peak_vel_err"] == 0.5
    v, status = analyse(one_trace([0.0] * (last - HOLD + 1) + [0.5]))                   # inside the hold rows
    assert status == 0 and v["recovered"] == 0.0 and np.isnan(v["recovery_time"]) and v["peak_vel_err"] == 0.5 and v["fell"] == 0.0
    v, _ = analyse(one_trace([0.5] * (last + 1)))                                       # never comes back
    assert v["recovered"] == 0.0 and np.isnan(v["recovery_time"]) and v["peak_time"] == f32(1) * f32(DT)
    v, _ = analyse(one_trace([0.0625] * (last + 1)))                                    # never leaves the band: time 0
    assert v["recovered"] == 1.0 and v["recovery_time"] == 0.0 and v["peak_vel_err"] == 0.0625


def test_model_group_table():
    values = np.full((P.V, 7), np.nan, np.float32)
    values[:, 0], values[:, 1], values[:, 5] = 1.0, 3.0, 100.0
    values[0, 2] = 1.0
    status = np.array([0, 0, 3, 2, 1, 0, 3])
    table = P.recovery_reduce(values, status, np.array([0, 0, 0, 0, 0, -1, 1]), 3)
    assert table.shape == (3, 9, 6)
    assert table[0, 1].tolist() == [2.0, 2.0, 1.0, 1.0, 3.0, 3.0] and table[0, 0].tolist()[:2] == [3.0, 5.0 / 3.0] and table[0, 0, 5] == 2.0
    assert table[0, 8].tolist() == [5.0, 2.0, 1.0, 1.0, 1.0, 0.0]
    assert table[1, 8].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] and table[1, 1, 0] == 0.0 and np.isnan(table[1, 1, 1:5]).all() and table[1, 1, 5] == 1.0
    assert table[2, 8].tolist() == [0.0] * 6


# ---- 5. go1eval.hip under the SIMT emulator against the model -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import go1eval_host as G
    return G.load_library(eval_emu())


def unit_quaternions(rng, n):
    q = rng.standard_normal((4, n))
    return q / np.linalg.norm(q, axis=0)


def check_push(root, before, table, ids, N):
    """the kernel's root_states against the fp64 model of the fp32 state it started from: the pushed elements within push_bound,
    everything else bit-identical"""
    want, written = P.push(before, table, ids)
    id_list = list(range(N)) if ids is None else list(ids)
    touched = np.zeros((13, N), bool)
    touched[np.ix_(P.PUSHED_ROWS, np.nonzero(written)[0])] = True
    assert bits(root[~touched]) == bits(before[~touched])
    worst = 0.0
    for k, e in enumerate(id_list):
        if 0 <= e < N and written[e]:
            for r in P.PUSHED_ROWS:
                bound = P.push_bound(table[k], want[r, e])
                worst = max(worst, abs(float(root[r, e]) - want[r, e]) / bound)
                assert abs(float(root[r, e]) - want[r, e]) <= bound, (k, e, r, float(root[r, e]), want[r, e], bound)
    return written, worst


@pytest.mark.parametrize("ids", [None, [69, 0, 64, 63, 7], [69, 70, 3, -1, 64]])
def test_emulated_push_follows_the_model(emu, ids):
    import go1eval_host as G
    N = 70
    rng = np.random.default_rng(5)
    before = rng.standard_normal((13, N)).astype(np.float32)
    before[3:7] = unit_quaternions(rng, N)
    before[7, ::3] = -0.0
    K = N if ids is None else len(ids)
    table = rng.uniform(-1.5, 1.5, (K, 4)).astype(np.float32)
    table[1::4] = 0.0                                                            # all-zero rows write nothing
    table[2, 1:] = 0.0                                                           # one value is enough to be written
    root = before.copy()
    cfg, buf = G.Go1PushConfig(), G.Go1PushBuffers()
    cfg.num_envs, cfg.num_pushed = N, K
    env_ids = None if ids is None else np.array(ids, np.int32)
    soa = np.ascontiguousarray(table.T)
    buf.root_states, buf.push, buf.env_ids = root.ctypes.data, soa.ctypes.data, None if ids is None else env_ids.ctypes.data
    assert emu.go1eval_push(ctypes.byref(cfg), ctypes.byref(buf), None) == 0
    written, worst = check_push(root, before, table, ids, N)
    print(f"\npush under the emulator, ids={ids}: worst error / bound = {worst:.3f}")
    valid = [(k, e) for k, e in enumerate(range(N) if ids is None else ids) if 0 <= e < N]
    assert [bool(written[e]) for k, e in valid] == [bool(table[k].any()) for k, e in valid] and written.sum() >= 3
    assert np.signbit(root[7, ~written][before[7, ~written] == 0]).all()


def run_emulated_recovery(emu, trace, p0, pre, w, band, hold, dt, group, groups):
    import go1eval_host as G
    rows, _, K = trace.shape
    c = G.Go1RecoveryConfig()
    c.num_traced, c.rows, c.push_row, c.pre, c.smooth, c.hold, c.band, c.dt, c.num_groups = K, rows, p0, pre, w, hold, band, dt, groups
    values, status = np.full((P.V, K), -3.0, np.float32), np.full(K, -3, np.int32)
    table = np.full((groups, P.V + 1, 6), -3.0)
    b = G.Go1RecoveryBuffers()
    b.trace, b.values, b.status, b.group, b.results = (a.ctypes.data for a in (trace, values, status, group, table))
    assert emu.go1eval_recovery(ctypes.byref(c), ctypes.byref(b), None) == 0
    assert emu.go1eval_recovery_reduce(ctypes.byref(c), ctypes.byref(b), None) == 0
    return values, status, table


@pytest.mark.parametrize("w", [1, 5])
def test_emulated_recovery_and_reduce_follow_the_model(emu, w):
    K, rows, p0, pre, hold, groups = 300, 40, 12, 8, 5, 3
    rng = np.random.default_rng(31 + w)
    trace, kind = P.synthetic_traces(rng, K, rows, p0, pre)
    group = rng.integers(-1, groups + 1, K).astype(np.int32)                     # includes -1 and an id outside the table
    group[group == 1] = 2                                                        # and an empty group
    values, status, table = run_emulated_recovery(emu, trace, p0, pre, w, BAND, hold, DT, group, groups)
    want_values, want_status = P.recovery(trace, p0, pre, w, BAND, hold, DT)
    assert np.array_equal(status, want_status) and set(status.tolist()) == {0, 1, 2, 3}
    assert (status[kind == 5] == 1).all() and (status[kind == 9] == 1).all() and (status[kind == 6] == 3).all() and (status[kind == 7] == 2).all()
    assert (status[np.isin(kind, (0, 1, 2, 3, 4, 8))] == 0).all()
    assert np.array_equal(np.isnan(values), np.isnan(want_values)) and bits(values) == bits(want_values)
    v = dict(zip(P.VALUES, values))
    ok = status == 0
    assert np.isfinite(values[:, ok]).sum() == 7 * ok.sum() + (v["recovered"][ok] == 1).sum()       # only recovery_time may be NaN
    assert (v["fell"][status == 3] == 1).all() and np.isnan(values[1:, status == 3]).all() and np.isnan(values[:, np.isin(status, (1, 2))]).all()
    assert (v["recovered"][ok & (kind == 2)] == 0).all() and (v["recovered"][ok & (kind == 3)] == 0).all() and (v["recovered"][ok & (kind == 0)] == 1).all()
    assert (v["recovery_time"][ok & (kind == 0)] == 0).all() and (v["peak_vel_err"][ok & (kind == 1)] > 0.1).all()
    assert (v["recovery_time"][ok & (kind == 1)] > 0).any() and (v["height_drop"][ok & (kind == 1)] > 0.01).all() and (v["yaw_rate_dev"][ok & (kind == 1)] > 0.05).all()
    want_table = P.recovery_reduce(want_values, want_status, group, groups)
    assert np.array_equal(np.isnan(table), np.isnan(want_table)) and bits(table) == bits(want_table)
    assert table[:, -1, 0].sum() == np.isin(group, range(groups)).sum() and (table[:, -1, 1:5].sum(axis=1) == table[:, -1, 0]).all()
    assert table[1, -1].tolist() == [0.0] * 6 and np.isnan(table[1, :-1, 1:5]).all()


# ---- 6. the environment hooks without a GPU ---------------------------------------------------------------------------------------------------
def test_push_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    monkeypatch.delitem(sys.modules, "go1eval_host", raising=False)
    cfg = apply_train_config(make_cfg(), num_envs=16)
    cfg.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=cfg)
    for _ in range(3):
        env.step(torch.zeros(16, 12))
    assert "go1eval_host" not in sys.modules and env._push is None           # an environment that never pushes never imports the library
    recovery = lambda: env.trace_recovery(8, 8, 5, 0.1, 5, torch.zeros(16, dtype=torch.int32))
    for call in (lambda: env.push_robots(np.zeros((16, 4), np.float32)), lambda: env.push_robots(torch.ones(2, 4), [0, 3]), recovery):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert "go1eval_host" not in sys.modules and env._push is None
    env.step(torch.zeros(16, 12))                                             # and stepping goes on


# ---- 7. the host classes ---------------------------------------------------------------------------------------------------------------------
def test_go1push_checks_its_table_on_the_host():
    """Go1Push's host logic with the launch stubbed out: table and ids are refused before anything is copied or launched"""
    import go1eval_host as G
    calls = []
    lib = types.SimpleNamespace(go1eval_push=lambda cfg, buf, stream: calls.append(1) or 0)
    N = 8
    B = types.SimpleNamespace(device=torch.device("cpu"), root_states=torch.zeros(13, N))
    push = G.Go1Push(types.SimpleNamespace(num_envs=N), B, lib=lib)
    push._stream = lambda: None
    ok = np.ones((3, 4), np.float32)
    bad = [(ok, [0, 8, 1]), (ok, [0, -1, 1]), (ok, [2, 5, 2]), (ok, [0, 1]), (ok, None), (np.ones((3, 3)), [0, 1, 2]), (np.ones(4), [0]),
           (np.zeros((0, 4)), []), (np.array([[1.0, NAN, 0.0, 0.0]] * 3), [0, 1, 2]), (np.array([[1.0, np.inf, 0.0, 0.0]] * 8), None)]
    for table, ids in bad:
        with pytest.raises(ValueError):
            push.load(table, ids)
    with pytest.raises(AssertionError):
        push.launch()
    assert push.table is None and not calls
    push.load(torch.arange(12.0).reshape(3, 4), torch.tensor([5, 0, 7]))
    assert push.table.shape == (4, 3) and push.table[:, 1].tolist() == [4.0, 5.0, 6.0, 7.0] and push.env_ids.tolist() == [5, 0, 7]
    assert push.cfg.num_pushed == 3 and push.buf.env_ids == push.ids.data_ptr() and push.buf.root_states == B.root_states.data_ptr()
    push.launch()
    push.load(np.zeros((N, 4)))
    assert push.cfg.num_pushed == N and push.buf.env_ids is None
    push.launch()
    assert len(calls) == 2


def test_host_classes_through_the_emulated_library(emu):
    """Go1Push and Go1Trace.recovery end to end on CPU tensors, their launches served by the emulated kernels"""
    import go1eval_host as G
    rng = np.random.default_rng(11)
    N, ids = 70, [69, 0, 64, 63, 7]
    before = rng.standard_normal((13, N)).astype(np.float32)
    before[3:7] = unit_quaternions(rng, N)
    B = types.SimpleNamespace(device=torch.device("cpu"), root_states=torch.from_numpy(before.copy()),
                              **{k: torch.zeros(1) for k in G._TRACE_INPUTS if k != "root_states"})
    S = types.SimpleNamespace(num_envs=N, measure_heights=0, base_height_target=0.3)
    push = G.Go1Push(S, B, lib=emu)
    push._stream = lambda: None
    table = rng.uniform(-1.0, 1.0, (5, 4)).astype(np.float32)
    table[3] = 0.0
    push.load(table, ids)
    push.launch()
    written, _ = check_push(B.root_states.numpy(), before, table, ids, N)
    assert sorted(np.nonzero(written)[0].tolist()) == [0, 7, 64, 69]
    # the analysis of an uploaded trace
    K, rows, p0, pre, w, hold, groups = 70, 40, 8, 8, 5, 5, 3
    trace, _ = P.synthetic_traces(rng, K, rows, p0, pre)
    tr = G.Go1Trace(S, B, lib=emu)
    tr._stream = lambda: None
    tr.arm(None, capacity=rows)
    tr.trace.copy_(torch.from_numpy(trace))
    tr.rows = rows
    group = rng.integers(-1, groups, K).astype(np.int32)
    group[group == 1] = 0
    res = tr.recovery(p0, pre, w, BAND, hold, DT, group)
    want_values, want_status = P.recovery(trace, p0, pre, w, BAND, hold, DT)
    want_table = P.recovery_reduce(want_values, want_status, group, groups)
    assert list(res) == P.VALUES + ["groups", "values", "status"] and np.array_equal(res["status"], want_status)
    for m, metric in enumerate(P.VALUES):
        assert bits(res["values"][metric]) == bits(want_values[m]) and bits(res[metric]) == bits(want_table[:, m]), metric
    assert bits(res["groups"]) == bits(want_table[:, -1, :5]) and res["groups"][:, 0].sum() == (group >= 0).sum()
    with pytest.raises(RuntimeError, match="go1eval_recovery failed: -11"):
        tr.recovery(p0, pre, pre + 2, BAND, hold, DT, group)


# ---- 8. the sweep's host pieces and the tool -----------------------------------------------------------------------------------------------------
def test_push_cells_table_and_report():
    from go1_gym_learn.eval_metrics import recovery
    cells = recovery.push_cells([0, 1.0], [0, 90])
    assert cells == [(0.0, 0.0), (0.0, 90.0), (1.0, 0.0), (1.0, 90.0)]
    table = recovery.push_table(cells, 70)
    assert table.shape == (70, 4) and table.dtype == np.float32
    assert table[:6].tolist() == [[0.0] * 4, [0.0] * 4, [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0] * 4, [0.0] * 4]
    assert not np.signbit(table).any()
    back = recovery.push_table(recovery.push_cells([2.0], [180, 270, 45]), 3)
    assert back[0].tolist() == [-2.0, 0.0, 0.0, 0.0] and back[1].tolist() == [0.0, -2.0, 0.0, 0.0] and np.allclose(back[2, :2], 2.0 ** 0.5)
    metric = lambda mean: np.array([[8.0, mean, 0.5, 0.0, 1.0, 0.0], [0.0, NAN, NAN, NAN, NAN, 4.0]])
    res = dict(preset="static_medium", cells=[(0.0, 0.0), (1.0, 90.0)], recovery={m: metric(0.25) for m in P.VALUES},
               groups=np.array([[8.0, 8.0, 0.0, 0.0, 0.0], [8.0, 0.0, 1.0, 1.0, 6.0]]), status=np.array([0] * 8 + [1, 2] + [3] * 6), values={},
               num_envs=16, settle_steps=50, pre=20, window=60, smooth=17, band=0.1, hold=10, dt=0.02, seed=1)
    md = recovery.recovery_markdown_table(res).splitlines()
    assert len(md) == 4 and md[0].startswith("| push [m/s] | direction [deg] | ok / fell / baseline reset / not held | fall rate | peak velocity error")
    assert md[2] == "| 0 | 0 | 8 / 0 / 0 / 0 | 0.000 | 0.25 ± 0.5 | 0.25 ± 0.5 | 0.250 |" and md[3] == "| 1 | 90 | 0 / 6 / 1 / 1 | 1.000 | – | – | – |"
    js = json.loads(json.dumps(recovery.recovery_to_json(res)))
    assert js["cells"][1] == dict(magnitude=1.0, direction_deg=90.0) and js["status_counts"] == [8, 1, 1, 6] and js["recovery"]["peak_vel_err"][0][1] == 0.25
    assert js["group_fields"] == P.GROUP_FIELDS


def test_tool_accepts_a_push_grid():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--push", "--magnitude", "0", "0.5", "1", "--direction", "0", "90", "--trace-envs", "0", "5"])
    assert a.push and a.magnitude == [0.0, 0.5, 1.0] and a.direction == [0.0, 90.0] and a.trace_envs == [0, 5] and not a.response
    for bad in (["--magnitude", "1"], ["--direction", "0"], ["--push"], ["--push", "--magnitude", "1"], ["--push", "--direction", "0"],
                ["--push", "--magnitude", "-1", "--direction", "0"], ["--push", "--magnitude", "1", "--direction", "0", "--behaviour"],
                ["--push", "--magnitude", "1", "--direction", "0", "--response", "--switch", "vx", "0.5", "1.0"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(["--checkpoint", "c", "--out", "o"] + bad)
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", "o"])
    assert not a.push and a.magnitude is None and a.direction is None


def test_tool_writes_the_push_report(tmp_path, monkeypatch, capsys):
    """run_push with the sweep itself stubbed out: the JSON, the appended Markdown table and the traced environments' file"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import recovery, response
    metric = np.array([[8.0, 0.25, 0.5, 0.0, 1.0, 0.0]] * 2)
    rows = 6
    trace = {name: np.zeros((rows, 1), np.float32) for name in P_CHANNELS()}
    trace.update(env_ids=np.array([1], np.int32), rows=rows, truncated=False)
    seen = {}

    def sweep_stub(policy, preset, magnitudes, directions, **kw):
        seen.update(kw, preset=preset, magnitudes=magnitudes, directions=directions)
        return dict(preset=preset, cells=recovery.push_cells(magnitudes, directions), recovery={m: metric for m in P.VALUES},
                    groups=np.array([[8.0, 8.0, 0.0, 0.0, 0.0]] * 2), status=np.zeros(16, np.int32), values={}, num_envs=16, settle_steps=100,
                    pre=25, window=150, smooth=17, band=0.1, hold=10, dt=0.02, seed=1, trace=trace)
    monkeypatch.setattr(recovery, "run_push_sweep", sweep_stub)
    monkeypatch.setattr(response, "plot_trace", lambda trace, env, path, dt=0.02: open(path, "wb").write(b"png"))
    (tmp_path / "eval").mkdir()
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", str(tmp_path), "--presets", "static_medium", "--push", "--magnitude", "0", "1", "--direction", "90",
                               "--envs", "16", "--trace-envs", "1"])
    eval_sweep.run_push(a, None)
    assert seen["magnitudes"] == [0.0, 1.0] and seen["directions"] == [90.0] and seen["num_envs"] == 16 and seen["trace_envs"] == [1]
    js = json.load(open(tmp_path / "eval" / "static_medium_push.json"))
    assert js["cells"] == [dict(magnitude=0.0, direction_deg=90.0), dict(magnitude=1.0, direction_deg=90.0)] and js["status_counts"] == [16, 0, 0, 0]
    md = (tmp_path / "eval" / "static_medium_push.md").read_text()
    assert "| 1 | 90 | 8 / 0 / 0 / 0 | 0.000 | 0.25 ± 0.5 | 0.25 ± 0.5 | 0.250 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_push_trace_env1.png").read_bytes() == b"png"
    assert np.load(tmp_path / "eval" / "static_medium_push_trace.npz")["env_ids"].tolist() == [1]


def P_CHANNELS():
    import go1eval_host as G
    return G.TRACE_CHANNELS
