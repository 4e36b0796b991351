"""CPU checks of the trace and the step response (include/go1eval.h, third kernel family): the ctypes mirrors against the header,
argument validation without a GPU, the model of tests/response_ref.py on hand-computable responses, go1eval.hip itself under the
SIMT emulator against that model bit for bit, the environment hooks where there is no GPU, and the sweep's host pieces."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import response_ref as P
from test_eval_metrics import eval_emu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(REPO, "include", "go1eval.h")
NAN = float("nan")
f32 = np.float32


# ---- 1. the mirrors against the header ---------------------------------------------------------------------------------------------
C_TYPES = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}


def struct_fields(src, name):
    """[(field, C type text)] of `typedef struct name { ... } name;`"""
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(.*?)(\w+)(\[\w+\])?", decl)
            out.append((m.group(2), (m.group(1).strip() + (m.group(3) or "")).replace(" *", "*")))
    return out


def enum_order(src, name, prefix):
    body = src[src.index(f"enum {name}"):src.index("};", src.index(f"enum {name}"))]
    return [n.lower() for n, _ in sorted(re.findall(prefix + r"(\w+) = (\d+)", body), key=lambda p: int(p[1]))]


def test_trace_and_response_mirrors_match_the_header():
    import go1eval_host as G
    src = open(HEADER).read()
    for macro, value in (("NUM_TRACE", G.NUM_TRACE), ("NUM_RESPONSE", G.NUM_RESPONSE), ("MAX_SIGNALS", G.MAX_SIGNALS)):
        assert f"#define GO1EVAL_{macro} {value}" in src
    for struct in (G.Go1TraceConfig, G.Go1ResponseSignal, G.Go1ResponseConfig):
        want = struct_fields(src, struct.__name__)
        assert [f for f, _ in want] == [f for f, _ in struct._fields_], struct.__name__
        for (field, ctext), (_, ctype) in zip(want, struct._fields_):
            if ctext == "Go1ResponseSignal[GO1EVAL_MAX_SIGNALS]":
                assert ctype._type_ is G.Go1ResponseSignal and ctype._length_ == G.MAX_SIGNALS
            else:
                assert ctype is C_TYPES[ctext], (struct.__name__, field)
    for struct in (G.Go1TraceBuffers, G.Go1ResponseBuffers):
        want = struct_fields(src, struct.__name__)
        assert [f for f, _ in want] == [f for f, _ in struct._fields_], struct.__name__
        assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in struct._fields_)
    assert G.Go1TraceBuffers._fields_[-2:] == [("env_ids", ctypes.c_void_p), ("trace", ctypes.c_void_p)]
    assert enum_order(src, "Go1TraceChannel", "GO1TRACE_") == G.TRACE_CHANNELS == P.CHANNELS and len(P.CHANNELS) == G.NUM_TRACE == 24
    assert enum_order(src, "Go1ResponseMetric", "GO1RESPONSE_") == G.RESPONSE_METRICS == P.VALUES and len(P.VALUES) == G.NUM_RESPONSE
    assert enum_order(src, "Go1ResponseGroupField", "GO1RESPONSE_G_") == G.RESPONSE_GROUP_FIELDS == P.GROUP_FIELDS
    assert G._TRACE_INPUTS == P.INPUTS
    from go1_gym_learn.eval_metrics.response import RESPONSE_SIGNALS
    ch = G.TRACE_CHANNELS.index
    assert RESPONSE_SIGNALS == {"lin_vel_x": (ch("lin_vel_x"), ch("cmd_lin_vel_x")), "lin_vel_y": (ch("lin_vel_y"), ch("cmd_lin_vel_y")),
                                "ang_vel_yaw": (ch("ang_vel_yaw"), ch("cmd_ang_vel_yaw")), "base_height": (ch("base_height"), ch("cmd_base_height")),
                                "contact_match": (ch("contact_match"), None, 1.0, 1.0)}


# ---- 2. argument validation without a GPU ---------------------------------------------------------------------------------------------
def _response_cfg(G, **over):
    c = G.Go1ResponseConfig()
    c.num_traced, c.rows, c.switch_row, c.pre, c.smooth, c.hold, c.tail, c.band, c.dt, c.num_signals, c.num_groups = 4, 40, 10, 5, 3, 5, 5, 0.1, 0.02, 1, 1
    c.signal[0].y_channel, c.signal[0].r_channel = 0, 6
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_trace_and_response_arguments_are_checked_before_any_launch():
    import __graft_entry__ as g
    import go1eval_host as G
    g.build_eval_hip()
    lib = G.load_library()
    ref = ctypes.byref
    cfg, buf = G.Go1TraceConfig(), G.Go1TraceBuffers()
    assert lib.go1eval_trace_record(None, None, 0, None) == -1
    assert lib.go1eval_trace_record(ref(cfg), ref(buf), 0, None) == -1          # num_envs = 0
    cfg.num_envs, cfg.num_traced, cfg.capacity = 8, 8, 6
    assert lib.go1eval_trace_record(ref(cfg), ref(buf), 0, None) == -2          # no trace buffer
    anything = np.zeros(64, np.float32)
    buf.trace = anything.ctypes.data
    assert lib.go1eval_trace_record(ref(cfg), ref(buf), 0, None) == -3          # no inputs
    for n in G._TRACE_INPUTS:
        setattr(buf, n, anything.ctypes.data)
    assert lib.go1eval_trace_record(ref(cfg), ref(buf), 0, None) == -4          # a height scan of no points
    buf.measured_heights = None
    assert lib.go1eval_trace_record(ref(cfg), ref(buf), 6, None) == -7          # row = capacity
    assert lib.go1eval_trace_record(ref(cfg), ref(buf), -1, None) == -7
    cfg.num_traced = 5
    assert lib.go1eval_trace_record(ref(cfg), ref(buf), 0, None) == -8          # a subset without its ids
    assert not anything.any()

    rbuf = G.Go1ResponseBuffers()
    for fn in (lib.go1eval_response, lib.go1eval_response_reduce):
        assert fn(None, None, None) == -1
        assert fn(ref(_response_cfg(G, num_traced=0)), ref(rbuf), None) == -1
        assert fn(ref(_response_cfg(G)), ref(rbuf), None) == -2                 # no outputs
    rbuf.values = rbuf.status = anything.ctypes.data
    assert lib.go1eval_response(ref(_response_cfg(G)), ref(rbuf), None) == -3   # no trace
    assert lib.go1eval_response_reduce(ref(_response_cfg(G)), ref(rbuf), None) == -5      # no group, no table
    rbuf.trace = anything.ctypes.data
    refused = [dict(smooth=7), dict(smooth=0), dict(switch_row=4), dict(switch_row=40), dict(hold=31), dict(tail=31), dict(hold=0), dict(tail=0),
               dict(dt=0.0), dict(band=0.0)]             # w > pre + 1, w < 1, s0 < pre, s0 >= rows, hold / tail > rows - s0, ...
    for over in refused:
        assert lib.go1eval_response(ref(_response_cfg(G, **over)), ref(rbuf), None) == -9, over
        assert not P.window_ok(*[over.get(k, d) for k, d in (("rows", 40), ("switch_row", 10), ("pre", 5), ("smooth", 3), ("hold", 5), ("tail", 5),
                                                             ("band", 0.1), ("dt", 0.02))]), over
    assert P.window_ok(40, 10, 5, 3, 5, 5, 0.1, 0.02)
    for field, value in (("y_channel", 24), ("r_channel", 24), ("y_channel", -1)):
        c = _response_cfg(G)
        setattr(c.signal[0], field, value)
        assert lib.go1eval_response(ref(c), ref(rbuf), None) == -10, (field, value)
    for n in (0, 9):
        assert lib.go1eval_response(ref(_response_cfg(G, num_signals=n)), ref(rbuf), None) == -10
    assert not anything.any()


# ---- 3. the model by hand ---------------------------------------------------------------------------------------------------------------
ROWS, S0, PRE, HOLD, TAIL, DT, BAND = 40, 10, 5, 5, 5, 0.02, 0.1
VX = [(0, 6, 0.0, 0.0)]


def one_trace(y_after, r0=0.5, r1=1.5, y_before=None, rows=ROWS, s0=S0):
    """(rows, 24, 1): channel 0 = y (r0 before s0 unless given, y_after(t - s0) from s0 on), channel 6 = the command"""
    t = np.zeros((rows, P.C, 1), np.float32)
    t[:s0, 0, 0] = r0 if y_before is None else y_before
    t[s0:, 0, 0] = [y_after(i) for i in range(rows - s0)]
    t[:s0, 6, 0], t[s0:, 6, 0] = r0, r1
    return t


def analyse(trace, signals=VX, s0=S0, pre=PRE, smooth=1, band=BAND, hold=HOLD, tail=TAIL):
    values, status = P.response(trace, signals, s0, pre, smooth, band, hold, tail, DT)
    return dict(zip(P.VALUES, values[0, :, 0].tolist())), int(status[0])


def first_order(r0, r1):
    """the error halves every row down to 2^-16 of the step, where it stays: every value is exact in fp32"""
    return lambda i: r0 + (r1 - r0) * (1.0 - 2.0 ** -min(i + 1, 16))


@pytest.mark.parametrize("r0,r1", [(0.5, 1.5), (1.5, 0.5)])
def test_model_first_order_response_up_and_down(r0, r1):
    """|e| = D 2^-min(i + 1, 16): 1/2, 1/4, 1/8, 1/16 <= 0.1 at the fourth row.  Every figure is a dyadic number: exact in fp32, and the
    downward step gives the same numbers as the upward one, with the sign of the error reversed"""
    v, status = analyse(one_trace(first_order(r0, r1), r0, r1))
    assert status == 0
    assert v["reached"] == 1.0 and v["rise_time"] == f32(4) * f32(DT)
    assert v["overshoot"] == 0.0
    # the band is 0.1 D as well: the last row outside it is the third, so the settle row is the fourth
    assert v["settled"] == 1.0 and v["settling_time"] == f32(4) * f32(DT)
    sign = 1.0 if r1 > r0 else -1.0
    assert v["steady_state_err"] == -sign * 2.0 ** -16
    assert v["iae"] == f32(np.float64(f32(DT)) * sum(2.0 ** -min(i + 1, 16) for i in range(ROWS - S0)))


@pytest.mark.parametrize("r0,r1", [(0.5, 1.5), (1.5, 0.5)])
def test_model_overshoot_and_settle_row(r0, r1):
    """rows 0, 1 on the way (0.5, 1.0 of the step), rows 2..4 at 1.25 of it, then on the target"""
    shape = [0.5, 1.0, 1.25, 1.25, 1.25]
    v, status = analyse(one_trace(lambda i: r0 + (r1 - r0) * (shape[i] if i < 5 else 1.0), r0, r1))
    assert status == 0 and v["overshoot"] == 0.25
    assert v["reached"] == 1.0 and v["rise_time"] == f32(2) * f32(DT)          # row 1 is on the target
    assert v["settled"] == 1.0 and v["settling_time"] == f32(6) * f32(DT)      # row 4 is the last outside the band, row 5 the settle row
    assert v["steady_state_err"] == 0.0
    assert v["iae"] == f32(np.float64(f32(DT)) * (0.5 + 3 * 0.25))


def test_model_never_within_ten_percent():
    v, status = analyse(one_trace(lambda i: 0.5 + 0.75, 0.5, 1.5))             # stays 25 % short
    assert status == 0 and v["reached"] == 0.0 and np.isnan(v["rise_time"])
    assert v["settled"] == 0.0 and np.isnan(v["settling_time"]) and v["overshoot"] == 0.0
    assert v["steady_state_err"] == -0.25 and v["iae"] == f32(np.float64(f32(DT)) * 0.25 * (ROWS - S0))


def test_model_leaves_the_band_inside_the_hold_rows():
    last = ROWS - S0 - 1
    on_target = lambda i: 1.5
    v, _ = analyse(one_trace(lambda i: 1.75 if i == last - HOLD else 1.5))      # the row before the hold rows: settles at the first of them
    assert v["settled"] == 1.0 and v["settling_time"] == f32(last - HOLD + 2) * f32(DT)
    v, _ = analyse(one_trace(lambda i: 1.75 if i == last - HOLD + 1 else 1.5))  # inside the hold rows
    assert v["settled"] == 0.0 and np.isnan(v["settling_time"]) and v["reached"] == 1.0 and v["overshoot"] == 0.25
    v, _ = analyse(one_trace(on_target))
    assert v["settled"] == 1.0 and v["settling_time"] == f32(1) * f32(DT) and v["rise_time"] == f32(1) * f32(DT)


def test_model_no_step_gives_nan_and_a_fixed_scale_gives_values():
    v, status = analyse(one_trace(lambda i: 1.0, 1.0, 1.0))
    assert status == 0 and all(np.isnan(x) for x in v.values())
    t = one_trace(lambda i: 0.75, 1.0, 1.0)
    t[:, 4, 0] = t[:, 0, 0]
    v, status = analyse(t, signals=[(4, None, 1.0, 1.0)])                       # contact_match's form: target 1, scale 1
    assert status == 0 and v["reached"] == 0.0 and v["overshoot"] == 0.0 and v["steady_state_err"] == -0.25


def test_model_status_rules():
    t = one_trace(first_order(0.5, 1.5))
    t[S0 + 7, P.RESET, 0] = 1.0
    v, status = analyse(t)
    assert status == 1 and all(np.isnan(x) for x in v.values())
    t = one_trace(first_order(0.5, 1.5))
    t[S0 - PRE, P.RESET, 0] = 1.0                                              # the first row of the window
    assert analyse(t)[1] == 1
    t = one_trace(first_order(0.5, 1.5))
    t[S0 - PRE - 1, P.RESET, 0] = 1.0                                          # the row before it
    v, status = analyse(t)
    assert status == 0 and v["rise_time"] == f32(4) * f32(DT)
    t = one_trace(first_order(0.5, 1.5))
    t[S0 + 3:, 6, 0] = 1.25                                                    # the command changes again
    v, status = analyse(t)
    assert status == 2 and all(np.isnan(x) for x in v.values())
    t = one_trace(first_order(0.5, 1.5))
    t[S0 - 2, 6, 0] = 0.25                                                     # the command was not held before the switch
    assert analyse(t)[1] == 2
    t[S0 - 2, 6, 0], t[S0 - PRE - 1, 6, 0] = 0.5, 0.25                         # outside the window: held
    assert analyse(t)[1] == 0
    t[S0 + 1, P.RESET, 0] = 1.0                                                # a reset outranks a command that moved
    t[S0 + 3:, 6, 0] = 1.25
    assert analyse(t)[1] == 1


def test_model_box_filter_against_a_hand_sum():
    """w = 4 on a ramp 0, 0.25, ... after the switch from 0 to 1: ys(s0 + i) = mean of the last four rows"""
    y = lambda i: min(0.25 * i, 1.0)                                            # 0, .25, .5, .75, 1, 1, ...
    v, status = analyse(one_trace(y, 0.0, 1.0), smooth=4)
    ys = [sum(([0.0] * 3 + [y(j) for j in range(ROWS - S0)])[i:i + 4]) / 4 for i in range(ROWS - S0)]
    assert ys[:8] == [0.0, 0.0625, 0.1875, 0.375, 0.625, 0.8125, 0.9375, 1.0]
    assert status == 0 and v["rise_time"] == f32(7) * f32(DT)                   # 0.9375 is the first within 0.1: row 6
    assert v["settling_time"] == f32(7) * f32(DT) and v["overshoot"] == 0.0
    assert v["iae"] == f32(np.float64(f32(DT)) * (1.0 + 0.75 + 0.5 + 0.25))     # raw, not smoothed
    with pytest.raises(AssertionError):
        analyse(one_trace(y, 0.0, 1.0), smooth=PRE + 2)


def test_model_group_table():
    values = np.full((1, P.V, 6), np.nan, np.float32)
    values[0, :, 0], values[0, :, 1], values[0, :, 4] = 1.0, 3.0, 100.0
    status = np.array([0, 0, 1, 2, 0, 1])
    table = P.response_reduce(values, status, np.array([0, 0, 0, 0, -1, 1]), 3)
    assert table.shape == (3, 8, 6)
    assert table[0, 2].tolist() == [2.0, 2.0, 1.0, 1.0, 3.0, 2.0] and table[0, 7].tolist() == [4.0, 2.0, 1.0, 1.0, 0.0, 0.0]
    assert table[1, 7].tolist() == [1.0, 0.0, 1.0, 0.0, 0.0, 0.0] and table[1, 0, 0] == 0.0 and np.isnan(table[1, 0, 1:5]).all() and table[1, 0, 5] == 1.0
    assert table[2, 7].tolist() == [0.0] * 6


# ---- 4. go1eval.hip under the SIMT emulator against the model ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import go1eval_host as G
    lib = ctypes.CDLL(eval_emu())
    lib.go1eval_trace_record.argtypes = [ctypes.POINTER(G.Go1TraceConfig), ctypes.POINTER(G.Go1TraceBuffers), ctypes.c_int32, ctypes.c_void_p]
    return lib


def random_snapshot(rng, N, points):
    s = dict(base_lin_vel=rng.standard_normal((3, N)), base_ang_vel=rng.standard_normal((3, N)), commands=rng.standard_normal((15, N)),
             root_states=rng.standard_normal((13, N)), measured_heights=None if points == 0 else 0.1 * rng.standard_normal((points, N)),
             contact_forces=3.0 * rng.standard_normal((51, N)), desired_contact_states=rng.random((4, N)),
             torques=20 * rng.standard_normal((12, N)), dof_vel=8 * rng.standard_normal((12, N)), dof_pos=rng.standard_normal((12, N)))
    s = {k: (None if v is None else v.astype(np.float32)) for k, v in s.items()}
    s["reset_buf"] = (rng.random(N) < 0.2).astype(np.uint8) * rng.integers(1, 3, N).astype(np.uint8)
    return s


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("N,ids,points,capacity,calls", [(130, [0, 129, 64, 7, 63], 17, 6, 8), (70, None, 0, 4, 4)])
def test_emulated_trace_follows_the_model(emu, N, ids, points, capacity, calls):
    import go1eval_host as G
    rng = np.random.default_rng(3 + N)
    K = N if ids is None else len(ids)
    env_ids = None if ids is None else np.array(ids, np.int32)
    trace = np.full((capacity, P.C, K), -7.0, np.float32)
    cfg, buf = G.Go1TraceConfig(), G.Go1TraceBuffers()
    cfg.num_envs, cfg.num_traced, cfg.capacity, cfg.num_height_points, cfg.base_height_target = N, K, capacity, points, 0.3
    buf.trace = trace.ctypes.data
    buf.env_ids = None if env_ids is None else env_ids.ctypes.data
    want = trace.copy()
    for row in range(calls):
        s = random_snapshot(rng, N, points)
        for k, a in s.items():
            setattr(buf, k, None if a is None else a.ctypes.data)
        rc = emu.go1eval_trace_record(ctypes.byref(cfg), ctypes.byref(buf), row, None)
        if row < capacity:
            assert rc == 0
            want[row] = P.trace_row(s, ids, 0.3)
            # the header's roundings against the two tables' fp64 step values: a few fp32 roundings of the largest term
            exact = P.trace_row(s, ids, 0.3, rounded=False)
            assert np.allclose(want[row], exact, rtol=0, atol=2e-6 * max(1.0, np.abs(exact).max()))
            assert bits(want[row, [P.CONTACT_MATCH, P.MAX_TORQUES]]) == bits(exact[[P.CONTACT_MATCH, P.MAX_TORQUES]].astype(np.float32))
        else:
            assert rc == -7                                                     # refused: the trace stays as it is
        assert bits(trace) == bits(want), row
    assert set(np.unique(trace[:, P.RESET])) == {0.0, 1.0} and set(np.unique(trace[:, P.CONTACT_MATCH])) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    assert len(np.unique(trace[:, P.CONTACT_MATCH])) >= 4


def test_emulated_trace_writes_nan_for_an_id_outside_the_simulator(emu):
    import go1eval_host as G
    N, ids = 70, [3, 70, -1, 69]
    rng = np.random.default_rng(1)
    env_ids = np.array(ids, np.int32)
    trace = np.zeros((2, P.C, 4), np.float32)
    cfg, buf = G.Go1TraceConfig(), G.Go1TraceBuffers()
    cfg.num_envs, cfg.num_traced, cfg.capacity, cfg.base_height_target = N, 4, 2, 0.3
    s = random_snapshot(rng, N, 0)
    for k, a in s.items():
        setattr(buf, k, None if a is None else a.ctypes.data)
    buf.trace, buf.env_ids = trace.ctypes.data, env_ids.ctypes.data
    assert emu.go1eval_trace_record(ctypes.byref(cfg), ctypes.byref(buf), 1, None) == 0
    want = P.trace_row(s, ids, 0.3)
    assert np.isnan(want[:, 1:3]).all() and np.isfinite(want[:, [0, 3]]).all()
    assert bits(trace[1]) == bits(want) and not trace[0].any()


def run_emulated_response(emu, trace, signals, s0, pre, w, band, hold, tail, dt, group, G_):
    import go1eval_host as G
    rows, _, K = trace.shape
    c = G.Go1ResponseConfig()
    G.response_signals(c, {str(i): s for i, s in enumerate(signals)})
    c.num_traced, c.rows, c.switch_row, c.pre, c.smooth, c.hold, c.tail, c.band, c.dt, c.num_groups = K, rows, s0, pre, w, hold, tail, band, dt, G_
    S = len(signals)
    values, status = np.full((S, P.V, K), -3.0, np.float32), np.full(K, -3, np.int32)
    table = np.full((G_, S * P.V + 1, 6), -3.0)
    b = G.Go1ResponseBuffers()
    b.trace, b.values, b.status, b.group, b.results = (a.ctypes.data for a in (trace, values, status, group, table))
    assert emu.go1eval_response(ctypes.byref(c), ctypes.byref(b), None) == 0
    assert emu.go1eval_response_reduce(ctypes.byref(c), ctypes.byref(b), None) == 0
    return values, status, table


@pytest.mark.parametrize("w", [1, 4])
def test_emulated_response_and_reduce_follow_the_model(emu, w):
    K, rows, s0, pre, hold, tail, groups = 300, 40, 12, 6, 5, 6, 3
    rng = np.random.default_rng(17 + w)
    trace, kind = P.synthetic_traces(rng, K, rows, s0, pre)
    group = rng.integers(-1, groups + 1, K).astype(np.int32)                     # includes -1 and an id outside the table
    values, status, table = run_emulated_response(emu, trace, P.SIGNALS, s0, pre, w, BAND, hold, tail, DT, group, groups)
    want_values, want_status = P.response(trace, P.SIGNALS, s0, pre, w, BAND, hold, tail, DT)
    assert np.array_equal(status, want_status) and {0, 1, 2} <= set(status.tolist())
    assert (status[kind == 5] == 1).all() and (status[kind == 8] == 1).all() and (status[kind == 7] == 2).all() and (status[kind == 6] == 0).all()
    assert np.array_equal(np.isnan(values), np.isnan(want_values)) and bits(values) == bits(want_values)
    first = dict(zip(P.VALUES, values[0]))
    ok = status == 0
    assert np.isnan(first["rise_time"][ok & (kind == 4)]).all() and np.isnan(values[:, :, ~ok]).all()
    assert (first["reached"][ok & (kind == 2)] == 0).all() and (first["reached"][ok & (kind == 0)] == 1).all()
    assert (first["overshoot"][ok & (kind == 1)] > 0.05).all() and (first["settled"][ok] == 0).any() and (first["settled"][ok] == 1).any()
    assert (values[3, P.VALUES.index("overshoot")][ok] == 0).all()              # contact_match never passes its target
    assert np.isfinite(values[4][:, ok & (kind == 4)]).all()                    # a fixed scale gives values where the command does not move
    want_table = P.response_reduce(want_values, want_status, group, groups)
    assert np.array_equal(np.isnan(table), np.isnan(want_table)) and bits(table) == bits(want_table)
    assert table[:, -1, 0].sum() == (np.isin(group, range(groups))).sum() and (table[:, -1, 1:4].sum(axis=1) == table[:, -1, 0]).all()


# ---- 5. the environment hooks without a GPU --------------------------------------------------------------------------------------------------
def test_trace_hooks_on_cpu_buffers(monkeypatch):
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
    assert "go1eval_host" not in sys.modules and env._trace is None      # an environment that never armed a trace never imports the library
    response = lambda: env.trace_response({"lin_vel_x": (0, 6)}, 5, 5, 1, 0.1, 5, 5, torch.zeros(16, dtype=torch.int32))
    for call in (env.start_trace, lambda: env.start_trace([0, 3], capacity=10), env.stop_trace, env.read_trace, response):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert "go1eval_host" not in sys.modules
    env.step(torch.zeros(16, 12))                                         # and stepping goes on


def test_trace_ring_and_ids_on_the_host():
    """Go1Trace's host logic with the launch stubbed out: ids are checked before anything is allocated, a full ring records nothing"""
    import types
    import go1eval_host as G
    calls = []
    lib = types.SimpleNamespace(go1eval_trace_record=lambda cfg, buf, row, stream: calls.append(row) or 0)
    N = 8
    B = types.SimpleNamespace(device=torch.device("cpu"), **{n: torch.zeros(13, N) for n in G._TRACE_INPUTS})
    S = types.SimpleNamespace(num_envs=N, measure_heights=0, base_height_target=0.3)
    tr = G.Go1Trace(S, B, lib=lib)
    tr._stream = lambda: None
    assert tr.trace is None
    for bad in ([0, 8], [-1], [2, 5, 2], []):
        with pytest.raises(ValueError):
            tr.arm(bad, capacity=4)
    assert tr.trace is None and not tr.armed
    tr.arm([5, 0, 7], capacity=3)
    assert tr.trace.shape == (3, 24, 3) and tr.buf.measured_heights is None and tr.cfg.num_traced == 3
    for _ in range(5):
        tr.record()
    assert calls == [0, 1, 2] and tr.rows == 3 and tr.truncated
    out = tr.read()
    assert out["env_ids"].tolist() == [5, 0, 7] and out["rows"] == 3 and out["truncated"] and out["dof_pos_11"].shape == (3, 3)
    tr.arm(None, capacity=2)
    assert tr.cfg.num_traced == N and tr.buf.env_ids is None and tr.rows == 0 and not tr.truncated


def test_go1trace_through_the_emulated_library():
    """the host class end to end on CPU tensors, its launches served by the emulated kernels: record / read against the model's
    rows, and response() (one packed output buffer, one copy) against the model's values, statuses and table"""
    import types
    import go1eval_host as G
    lib = G.load_library(eval_emu())
    rng = np.random.default_rng(9)
    N, points, ids = 70, 5, [69, 0, 33]
    first = random_snapshot(rng, N, points)
    B = types.SimpleNamespace(device=torch.device("cpu"), **{k: torch.from_numpy(v.copy()) for k, v in first.items()})
    S = types.SimpleNamespace(num_envs=N, measure_heights=1, base_height_target=0.3)
    tr = G.Go1Trace(S, B, lib=lib)
    tr._stream = lambda: None
    tr.arm(ids, capacity=4)
    want = []
    for step in range(5):
        snap = first if step == 0 else random_snapshot(rng, N, points)
        for k, v in snap.items():
            getattr(B, k).copy_(torch.from_numpy(v))
        tr.record()
        want.append(P.trace_row(snap, ids, 0.3))
    out = tr.read()
    assert out["rows"] == 4 and out["truncated"] and out["env_ids"].tolist() == ids
    assert bits(np.stack([out[n] for n in P.CHANNELS], axis=1)) == bits(np.stack(want[:4]))
    # the analysis of an uploaded trace
    K, rows, s0, pre, w, hold, tail, groups = 70, 40, 12, 6, 5, 5, 6, 2
    trace, _ = P.synthetic_traces(rng, K, rows, s0, pre)
    tr.arm(None, capacity=rows)
    tr.trace.copy_(torch.from_numpy(trace))
    tr.rows = rows
    group = rng.integers(-1, groups, K).astype(np.int32)
    names = ["lin_vel_x", "ang_vel_yaw", "base_height", "contact_match", "lin_vel_y"]
    res = tr.response(dict(zip(names, P.SIGNALS)), s0, pre, w, BAND, hold, tail, DT, group)
    want_values, want_status = P.response(trace, P.SIGNALS, s0, pre, w, BAND, hold, tail, DT)
    want_table = P.response_reduce(want_values, want_status, group, groups)
    assert list(res) == names + ["groups", "values", "status"] and np.array_equal(res["status"], want_status)
    for s, name in enumerate(names):
        for m, metric in enumerate(P.VALUES):
            assert bits(res["values"][name][metric]) == bits(want_values[s, m]) and bits(res[name][metric]) == bits(want_table[:, s * P.V + m])
    assert bits(res["groups"]) == bits(want_table[:, -1, :4])


# ---- 6. the sweep's host pieces and the tool -------------------------------------------------------------------------------------------------------
def test_switch_commands_signals_and_tables():
    from go1_gym_learn.eval_metrics import response, sweep
    cmd = response.switch_commands("lin_vel_x", [0.0, 0.5, 1.0], 15, "cpu")
    base = sweep.command_table([response.BASE_CELL], 15, "cpu")
    assert cmd[:, 0].tolist() == [0.0, 0.5, 1.0] and torch.equal(cmd[:, 1:], base[:, 1:].repeat(3, 1))
    assert torch.equal(response.switch_commands("vx", [0.5], 15, "cpu"), cmd[1:2])
    gait = response.switch_commands("gait", ["trotting", "pacing"], 15, "cpu")
    assert gait[:, 5:8].tolist() == [list(sweep.GAITS["trotting"]), list(sweep.GAITS["pacing"])] and gait[:, 0].tolist() == [1.0, 1.0]
    with pytest.raises(KeyError):
        response.switch_commands("nothing", [1.0], 15, "cpu")
    assert response.default_signals("lin_vel_x") == response.default_signals("vx") == ["lin_vel_x", "contact_match"]
    assert response.default_signals("body_height") == ["base_height", "contact_match"] and response.default_signals("gait") == ["contact_match"]
    assert response.stride_rows(cmd, 0.02) == 17
    metric = lambda mean: np.array([[8.0, mean, 0.5, 0.0, 1.0, 0.0], [0.0, NAN, NAN, NAN, NAN, 4.0]])
    res = dict(preset="static_medium", command="lin_vel_x", from_value=0.0, cells=[0.5, 1.0], signals=["lin_vel_x", "contact_match"],
               response={s: {m: metric(0.25) for m in P.VALUES} for s in ("lin_vel_x", "contact_match")},
               groups=np.array([[8.0, 8.0, 0.0, 0.0], [8.0, 4.0, 3.0, 1.0]]), status=np.array([0] * 12 + [1] * 3 + [2]), values={},
               num_envs=16, settle_steps=50, pre=20, window=60, smooth=17, band=0.1, hold=10, tail=25, dt=0.02, seed=1)
    md = response.response_markdown_table(res).splitlines()
    assert len(md) == 4 and md[0].startswith("| lin_vel_x | signal | ok / fell / not held | reached | settled | rise time")
    assert "| 0.0 → 0.5 | lin_vel_x | 8 / 0 / 0 | 0.250 | 0.250 | 0.25 ± 0.5 |" in md[2] and "| 4 / 3 / 1 | – | – | – |" in md[3]
    import json
    js = json.loads(json.dumps(response.response_to_json(res)))
    assert js["cells"] == [0.5, 1.0] and js["status_counts"] == [12, 3, 1] and js["response"]["contact_match"]["iae"][0][1] == 0.25


def test_tool_accepts_a_response_switch():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--response", "--switch", "lin_vel_x", "0.5", "1.0", "1.5"])
    assert a.response and eval_sweep.response_switch(a) == ("lin_vel_x", 0.5, [1.0, 1.5]) and a.trace_envs is None
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--response", "--switch", "gait", "trotting", "pacing", "--trace-envs", "0", "5"])
    assert eval_sweep.response_switch(a) == ("gait", "trotting", ["pacing"]) and a.trace_envs == [0, 5]
    for bad in (["--switch", "lin_vel_x", "0.5", "1.0"], ["--trace-envs", "0"], ["--response"], ["--response", "--switch", "lin_vel_x", "0.5"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(["--checkpoint", "c", "--out", "o"] + bad)
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", "o"])
    assert not a.response and a.switch is None


def test_plot_trace_writes_a_png(tmp_path):
    pytest.importorskip("matplotlib")
    from go1_gym_learn.eval_metrics import response
    rows = 30
    trace = {name: np.random.default_rng(0).standard_normal((rows, 2)).astype(np.float32) for name in P.CHANNELS}
    trace.update(env_ids=np.array([4, 9], np.int32), rows=rows, truncated=False)
    path = tmp_path / "trace_env9.png"
    response.plot_trace(trace, 9, str(path))
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) > 2000
    sub = response.select_envs(trace, [9])
    assert sub["env_ids"].tolist() == [9] and np.array_equal(sub["lin_vel_x"][:, 0], trace["lin_vel_x"][:, 1]) and sub["rows"] == rows
    with pytest.raises(ValueError):
        response.plot_trace(trace, 5, str(path))
