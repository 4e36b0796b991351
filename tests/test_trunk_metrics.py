"""CPU checks of the trunk family (include/go1trunk.h, libgo1trunk.so): the ctypes mirrors and the exported symbols against the header,
the build's source lists and stamp, the refusals without a GPU, the host-side definition against the reference's three reward terms,
the model of tests/trunk_ref.py on hand-computable cases, go1trunk.hip itself under the SIMT emulator against that model bit for bit
(accumulators, state, histogram and both result tables), the environment hooks where there is no GPU, the two scenarios of the GPU
tests through the fp64 oracle, and the sweep's host pieces."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import trunk_ref as T
from test_eval_return_codes import Call, cfg, each, nobody, null
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from util import build_emu

HEADER = os.path.join(REPO, "include", "go1trunk.h")
SOURCE = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1trunk.hip")
TABLES = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1_tables.h")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]


# ---- 1. mirrors, symbols, sources, stamp ---------------------------------------------------------------------------------------------------
def test_trunk_mirrors_match_the_header():
    import go1trunk_host as G
    src = open(HEADER).read()
    for macro, value in (("GO1TRUNK_NUM", G.NUM_TRUNK_METRICS), ("GO1TRUNK_TILT_BINS", G.TILT_BINS), ("GO1TRUNK_NUM_FIELDS", 6),
                         ("GO1TRUNK_REDUCE_THREADS", 256), ("GO1TRUNK_CONTACT_FORCE", G.CONTACT_FORCE)):
        assert re.search(rf"#define {macro} {value}\n", src), macro
    assert (G.NUM_TRUNK_METRICS, G.TILT_BINS) == (17, 16) == (T.M, T.BINS)
    want = struct_fields(src, "Go1TrunkConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1TrunkConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "segment_steps", "dt", "tilt_limit"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1TrunkConfig._fields_):
        assert ctype is C_TYPES[ctext], field
    assert ctypes.sizeof(G.Go1TrunkConfig) == 24
    want = struct_fields(src, "Go1TrunkBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1TrunkBuffers._fields_] == T.INPUTS + ACCUMULATORS + T.STATE + ["group", "results", "hist_results"]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1TrunkBuffers._fields_)
    types_ = dict(want)
    assert types_["prev_valid"] == types_["seg_valid"] == "uint8_t*" and types_["seg_steps"] == "int32_t*" and types_["seg_anchor"] == "float*"
    assert types_["hist_results"] == types_["results"] == "double*" and types_["tilt_hist"] == types_["segments_dropped"] == "uint32_t*"
    assert G._TRUNK_INPUTS == T.INPUTS and G._TRUNK_STATE == T.STATE == list(G.Go1Trunk.STATE)
    assert enum_order(src, "Go1TrunkMetric", "GO1TRUNK_") == G.TRUNK_NAMES == T.METRICS and len(T.METRICS) == G.NUM_TRUNK_METRICS
    assert enum_order(src, "Go1TrunkGroupField", "GO1TRUNK_G_") == G.TRUNK_GROUP_FIELDS == T.GROUP_FIELDS
    import go1eval_host as E
    assert enum_order(src, "Go1TrunkField", "GO1TRUNK_F_") == E.FIELD_NAMES
    assert issubclass(G.Go1Trunk, E._Table) and G.Go1Trunk.ROWS == 17 and G.Go1Trunk.TABLE_ROWS == 18
    edges = G.tilt_edges()
    assert edges.shape == (17,) and edges[:16].tolist() == [k / 32 for k in range(16)] and edges[15] == 0.46875 and edges[16] == INF
    from go1_gym_learn.eval_metrics import trunk
    assert trunk.TRUNK_METRICS == G.TRUNK_NAMES and set(trunk.TRUNK_TERMS[:6]) < set(G.TRUNK_NAMES)


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1trunk_host as G
    declared = set(re.findall(r"\b(go1trunk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1trunk_clear", "go1trunk_accumulate", "go1trunk_reduce", "go1trunk_version"}
    out = g.build_trunk_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1trunk_" in line} == declared
    assert not re.search(r"\bgo1(eval|feet)_\w+", dynamic)


def test_sources_flags_and_stamp():
    import __graft_entry__ as g
    assert g.trunk_sources() == [SOURCE, TABLES, HEADER] and g.TRUNK_FLAGS == g.EVAL_FLAGS and "-ffp-contract=off" in g.TRUNK_FLAGS
    assert g.TRUNK_FLAGS is not g.EVAL_FLAGS
    for others in (g.sim_sources(), g.ppo_sources(), g.render_sources()):
        assert not set(others) & set(g.trunk_sources())
    for others in (g.eval_sources(), g.feet_sources()):                      # the metric libraries share one header, and nothing else
        assert set(others) & set(g.trunk_sources()) == {TABLES}
    code = re.sub(r"//.*", "", open(SOURCE).read())
    assert "go1eval" not in code and "go1feet" not in code                   # the library names nothing of the other two ...
    shared = re.sub(r"//.*", "", open(TABLES).read())                        # ... and the shared header names no library
    assert "go1eval" not in shared and "go1feet" not in shared and "go1trunk" not in shared
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["../../include/go1trunk.h", "go1_tables.h"]
    out = g.build_trunk_hip()
    assert os.path.basename(out) == "libgo1trunk.so" and g.library_stamp(out) == g.source_hash(g.trunk_sources(), g.TRUNK_FLAGS)
    lib = ctypes.CDLL(out)                                                   # dlopen needs no GPU
    lib.go1trunk_version.restype = ctypes.c_char_p
    assert lib.go1trunk_version() == b"go1trunk 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    import inspect
    assert "build_trunk_hip()" in inspect.getsource(g.build) and "libgo1trunk.so" in inspect.getsource(g.smoke)
    # the other two evaluation-side libraries' stamps are what their own sources give: this family changed neither
    csrc = os.path.join(REPO, "walk-these-ways_amd", "csrc")
    assert g.library_stamp(os.path.join(csrc, "libgo1eval.so")) in (None, g.source_hash(g.eval_sources(), g.EVAL_FLAGS))
    assert g.library_stamp(os.path.join(csrc, "libgo1feet.so")) in (None, g.source_hash(g.feet_sources(), g.FEET_FLAGS))


def test_a_missing_library_fails_loudly(tmp_path):
    import go1trunk_host as G
    with pytest.raises(G.Go1TrunkLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1trunk.so"))


# ---- 2. the refusals without a GPU (the helpers of tests/test_eval_return_codes.py) ----------------------------------------------------------
def trunk_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.segment_steps, c.dt, c.tilt_limit = 70, 2, 3, 50, 0.02, 0.25


TRUNK_ACC = ACCUMULATORS + T.STATE
BAD_CONFIG = [("dt = 0", -12, [cfg(dt=0.0)]), ("dt < 0", -12, [cfg(dt=-0.02)]), ("dt = inf", -12, [cfg(dt=INF)]), ("dt = NaN", -12, [cfg(dt=NAN)]),
              ("tilt_limit < 0", -12, [cfg(tilt_limit=-0.1)]), ("tilt_limit = inf", -12, [cfg(tilt_limit=INF)]),
              ("tilt_limit = NaN", -12, [cfg(tilt_limit=NAN)]), ("segment_steps = 0", -12, [cfg(segment_steps=0)]),
              ("segment_steps < 0", -12, [cfg(segment_steps=-5)])]
CASES = {
    "go1trunk_clear": nobody() + each(TRUNK_ACC, -2) + [
        ("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")])],
    "go1trunk_accumulate": nobody() + each(TRUNK_ACC, -2) + each(T.INPUTS, -3) + BAD_CONFIG + [
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no tilt_hist and no commands", -2, [null("tilt_hist", "commands")]),
        ("no seg_valid and dt = 0", -2, [null("seg_valid"), cfg(dt=0.0)]),
        ("no foot_positions and dt = NaN", -3, [null("foot_positions"), cfg(dt=NAN)]),
        ("no root_states and segment_steps = 0", -3, [null("root_states"), cfg(segment_steps=0)])],
    "go1trunk_reduce": nobody() + each(TRUNK_ACC, -2) + [
        ("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group", "results", "hist_results"], -5) + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no resets and no hist_results", -2, [null("resets", "hist_results")]),
        ("no seg_command and num_groups = 0", -2, [null("seg_command"), cfg(num_groups=0)])],
}


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    """every case fails validation, so nothing is launched: there is no GPU.  The valid settings of good values (tilt_limit 0,
    segment_steps 1) are not refused: with an input missing they get as far as -3."""
    import __graft_entry__ as g
    import go1trunk_host as G
    g.build_trunk_hip()
    fn = getattr(G.load_library(), symbol)
    assert len({label for label, _, _ in CASES[symbol]}) == len(CASES[symbol])
    assert sum(len(spoilers) > 1 for _, _, spoilers in CASES[symbol]) >= 1          # two conditions at once: precedence
    for label, code, spoilers in CASES[symbol]:
        a = Call(G.Go1TrunkConfig, G.Go1TrunkBuffers, trunk_base)
        for spoil in spoilers:
            spoil(a)
        assert fn(None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b), None) == code, (symbol, label)
    if symbol == "go1trunk_accumulate":
        for good in (cfg(tilt_limit=0.0), cfg(segment_steps=1), cfg(tilt_limit=5.0)):
            a = Call(G.Go1TrunkConfig, G.Go1TrunkBuffers, trunk_base)
            good(a)
            null("reset_buf")(a)
            assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -3
    else:                                                                    # the clear and the reduction read no input, no dt and no limit
        a = Call(G.Go1TrunkConfig, G.Go1TrunkBuffers, trunk_base)
        null(*T.INPUTS)(a)
        cfg(dt=0.0, tilt_limit=NAN, segment_steps=0)(a)
        null("count")(a)
        assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -2


# ---- 3. the host-side definition against the reference's reward terms -------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_trunk_terms_are_the_reference_rewards(seed):
    from go1_gym_learn.eval_metrics import trunk
    z = np.load(os.path.join(REPO, "tests", "golden", "trunk_metrics.npz"))
    env = types.SimpleNamespace(num_envs=64, **{k: torch.from_numpy(z[f"s{seed}_in_{k}"]) for k in ("projected_gravity", "base_lin_vel", "base_ang_vel")})
    assert env.projected_gravity.shape == (64, 3)
    terms = trunk.trunk_terms(env)
    assert list(terms) == trunk.TRUNK_TERMS and all(t.shape == (64,) and t.dtype == torch.float32 for t in terms.values())
    for name in ("orientation", "lin_vel_z", "ang_vel_xy"):
        got, want = terms[name].numpy(), z[f"s{seed}_out_{name}"]
        assert got.tobytes() == want.tobytes(), (name, np.abs(got - want).max())
    assert z[f"s{seed}_out_orientation"].min() == 0.0 and z[f"s{seed}_out_orientation"].max() == 1.0       # upright, and on its nose
    # the model's rows are the same numbers: one environment per fixture row, every one folded once
    snap = blank(64)
    snap["projected_gravity"][:] = z[f"s{seed}_in_projected_gravity"].T
    snap["base_lin_vel"][:] = z[f"s{seed}_in_base_lin_vel"].T
    snap["base_ang_vel"][:] = z[f"s{seed}_in_base_ang_vel"].T
    st = T.State(64)
    T.accumulate(st, T.config(), snap)
    assert (st.count[:7] == 1).all()
    row = lambda m: st.max[m]
    for name, m in (("roll_sin", T.ROLL_SIN), ("pitch_sin", T.PITCH_SIN), ("roll_rate", T.ROLL_RATE), ("pitch_rate", T.PITCH_RATE), ("vertical_vel", T.VERTICAL_VEL)):
        assert bits(row(m)) == bits(terms[name].numpy()), name
    # tilt is the correctly rounded root of the reference's term, and its square the square of that.  (trunk_terms takes the root with
    # torch.sqrt, whose vectorised CPU form is not correctly rounded everywhere: it may lie one ulp off, no more.)
    root = np.sqrt(terms["orientation"].numpy())
    assert root.dtype == f32 and bits(row(T.TILT)) == bits(root) == bits(np.sqrt(z[f"s{seed}_out_orientation"])) and bits(row(T.TILT) * row(T.TILT)) == bits(root * root)
    assert (np.abs(terms["tilt"].numpy().astype(np.float64) - root) <= np.spacing(root)).all()
    assert bits(row(T.VERTICAL_VEL) * row(T.VERTICAL_VEL)) == bits(terms["lin_vel_z"].numpy()) == bits(z[f"s{seed}_out_lin_vel_z"])
    assert bits(row(T.ROLL_RATE) * row(T.ROLL_RATE) + row(T.PITCH_RATE) * row(T.PITCH_RATE)) == bits(terms["ang_vel_xy"].numpy()) == bits(z[f"s{seed}_out_ang_vel_xy"])


# ---- 4. the model by hand ---------------------------------------------------------------------------------------------------------------------
def blank(N):
    """N upright robots at the origin, heading along x, at rest, their feet on a square of side 0.4 about the base and loaded with 30 N,
    commanded 0.5 m/s straight ahead, well past any warm-up"""
    s = dict(root_states=np.zeros((13, N), f32), base_lin_vel=np.zeros((3, N), f32), base_ang_vel=np.zeros((3, N), f32),
             projected_gravity=np.zeros((3, N), f32), commands=np.zeros((15, N), f32), contact_forces=np.zeros((51, N), f32),
             foot_positions=np.zeros((12, N), f32), reset_buf=np.zeros(N, np.uint8), episode_length_buf=np.full(N, 100, np.int32))
    s["root_states"][6] = 1.0
    s["projected_gravity"][2] = -1.0
    s["commands"][0] = 0.5
    for f, (x, y) in enumerate(((0.2, 0.2), (0.2, -0.2), (-0.2, 0.2), (-0.2, -0.2))):
        s["foot_positions"][3 * f], s["foot_positions"][3 * f + 1] = x, y
        s["contact_forces"][12 * (f + 1) + 2] = 30.0
    return s


def snap_of(p=(0.0, 0.0), yaw_q=(0.0, 0.0, 0.0, 1.0), v=(0.0, 0.0, 0.0), w=(0.0, 0.0, 0.0), g=(0.0, 0.0), fz=(30.0,) * 4, feet=None, cmd=(0.5, 0.0, 0.0),
            bv=0.0, bw=(0.0, 0.0), reset=0, age=100):
    """one environment"""
    s = blank(1)
    s["root_states"][0:2, 0], s["root_states"][3:7, 0], s["root_states"][7:10, 0], s["root_states"][10:13, 0] = p, yaw_q, v, w
    s["projected_gravity"][0:2, 0], s["commands"][0:3, 0] = g, cmd
    s["base_lin_vel"][2, 0], s["base_ang_vel"][0:2, 0] = bv, bw
    for f in range(4):
        s["contact_forces"][12 * (f + 1) + 2, 0] = fz[f]
        if feet is not None:
            s["foot_positions"][3 * f:3 * f + 2, 0] = feet[f]
    s["reset_buf"][0], s["episode_length_buf"][0] = reset, age
    return s


def play(cfg_, steps):
    st = T.State(1)
    for kw in steps:
        T.accumulate(st, cfg_, snap_of(**kw))
    return st


def folded(st):
    """{metric: (count, nonfinite, min, max)} of environment 0"""
    return {name: (int(st.count[m, 0]), int(st.nonfinite[m, 0]), float(st.min[m, 0]), float(st.max[m, 0])) for m, name in enumerate(T.METRICS)}


NOTHING = (0, 0, INF, -INF)
one = lambda v: (1, 0, float(v), float(v))


def test_model_support_polygon():
    got = folded(play(T.config(), [dict()]))                                 # a square stance of side 0.4, the base at its centre
    assert got["support_feet"] == one(4.0) and got["support_margin"] == one(f32(0.2) * f32(0.4) / f32(0.4)) and got["margin_negative"] == one(0.0)
    assert abs(got["support_margin"][2] - 0.2) < 1e-7 and got["support_line_dist"] == NOTHING
    got = folded(play(T.config(), [dict(fz=(30.0, 0.5, 30.0, 30.0))]))       # FR lifted: the triangle FL, RL, RR; its edge RR -> FL passes through the base
    assert got["support_feet"] == one(3.0) and got["support_margin"][:2] == (1, 0) and abs(got["support_margin"][2]) < 1e-7
    got = folded(play(T.config(), [dict(fz=(30.0, 0.5, 30.0, 30.0), p=(-0.1, 0.1))]))          # the base well inside that triangle
    want = min(0.1, 0.1, 0.2 / np.sqrt(2.0))                                 # from the edges FL -> RL, RL -> RR, and the diagonal RR -> FL
    assert got["support_feet"] == one(3.0) and abs(got["support_margin"][2] - want) < 1e-6 and got["margin_negative"] == one(0.0)
    got = folded(play(T.config(), [dict(fz=(30.0, 0.0, 0.0, 30.0), p=(0.1, -0.1))]))           # the diagonal pair FL + RR: the base off the line
    assert got["support_feet"] == one(2.0) and got["support_margin"] == NOTHING and got["margin_negative"] == NOTHING
    assert abs(got["support_line_dist"][2] - 0.2 / np.sqrt(2.0)) < 1e-6 and got["support_line_dist"][0] == 1
    got = folded(play(T.config(), [dict(p=(0.5, 0.0))]))                     # the base 0.3 in front of the square
    assert got["support_feet"] == one(4.0) and abs(got["support_margin"][2] + 0.3) < 1e-6 and got["margin_negative"] == one(1.0)
    got = folded(play(T.config(), [dict(fz=(30.0, 0.0, 1.0, NAN))]))         # 1.0 is no contact, nor is a NaN: one foot
    assert got["support_feet"] == one(1.0) and got["support_margin"] == NOTHING and got["support_line_dist"] == NOTHING
    for feet in ([(0.2, 0.2), (0.2, -0.2), (0.2, 0.2), (-0.2, -0.2)],         # FL and RL in one place: a zero-length edge, wherever it comes
                 [(0.2, 0.2), (0.2, 0.2), (-0.2, 0.2), (-0.2, -0.2)], [(0.2, 0.2), (0.2, -0.2), (-0.2, -0.2), (-0.2, -0.2)]):
        got = folded(play(T.config(), [dict(feet=feet)]))
        assert got["support_margin"] == (0, 1, INF, -INF) and got["margin_negative"] == one(0.0) and got["support_feet"] == one(4.0)


def yaw(angle):
    return (0.0, 0.0, float(np.sin(angle / 2)), float(np.cos(angle / 2)))


def test_model_a_segment_closes():
    """heading along y (a yaw of 90 degrees), segments of 3 steps, commanded 0.5 m/s ahead and 0.25 m/s to the left"""
    dt = f32(0.02)
    c = T.config(segment_steps=3)
    q = (0.0, 0.0, float(f32(np.sqrt(0.5))), float(f32(np.sqrt(0.5))))
    cmd = (0.5, 0.25, 0.0)
    steps = [dict(p=(1.0, 2.0), yaw_q=q, cmd=cmd), dict(p=(1.0, 2.01), yaw_q=q, cmd=cmd), dict(p=(1.0, 2.02), yaw_q=q, cmd=cmd)]
    st = play(c, steps)
    assert folded(st)["lateral_drift"] == NOTHING and st.seg_valid[0] == 1 and st.seg_steps[0] == 2
    assert st.seg_anchor[:2, 0].tolist() == [1.0, 2.0] and abs(st.seg_anchor[2, 0]) < 1e-7 and st.seg_anchor[3, 0] == 1.0
    assert st.seg_command[0, 0] == f32(0.5) * dt + f32(0.5) * dt and st.seg_command[1, 0] == f32(0.25) * dt + f32(0.25) * dt
    # the close: 0.04 m ahead (along y), 0.005 m to the right (towards + x), turned 0.1 rad to the left
    st = play(c, steps + [dict(p=(1.005, 2.04), yaw_q=yaw(np.pi / 2 + 0.1), cmd=cmd)])
    got = folded(st)
    sx, sy = (f32(0.5) * dt + f32(0.5) * dt) + f32(0.5) * dt, (f32(0.25) * dt + f32(0.25) * dt) + f32(0.25) * dt
    assert got["progress_err"][0] == 1 and abs(got["progress_err"][2] - (0.04 - float(sx))) < 1e-6 and abs(float(sx) - 0.03) < 1e-7
    assert abs(got["lateral_drift"][2] - (-0.005 - float(sy))) < 1e-6 and abs(got["heading_drift"][2] - np.sin(0.1)) < 1e-6
    assert st.seg_valid[0] == 1 and st.seg_steps[0] == 0 and st.seg_command[:, 0].tolist() == [0.0, 0.0] and st.segments_dropped[0] == 0
    assert st.seg_anchor[0, 0] == f32(1.005) and st.seg_anchor[1, 0] == f32(2.04)                           # anchored again at the close
    st = play(c, steps + [dict(p=(1.005, 2.04), yaw_q=yaw(np.pi / 2 + 0.1), cmd=cmd)] + [dict(p=(1.005, 2.04), yaw_q=yaw(np.pi / 2 + 0.1), cmd=cmd)] * 3)
    got = folded(st)                                                         # the next one: stood still, so behind by what was commanded
    assert got["progress_err"][0] == 2 and abs(got["progress_err"][2] + float(sx)) < 1e-6 and abs(got["heading_drift"][2]) < 1e-6


def test_model_segments_drop_reset_and_warm_up():
    c = T.config(segment_steps=3)
    go = dict(p=(0.0, 0.0))
    for spoiled in (dict(cmd=(0.5, 0.0, 0.1)), dict(cmd=(0.5, 0.0, NAN)), dict(yaw_q=(0.5, 0.5, 0.5, -0.5)), dict(p=(NAN, 0.0)), dict(p=(0.0, INF))):
        st = play(c, [go, go, spoiled])
        assert st.segments_dropped[0] == 1 and st.seg_valid[0] == 0 and folded(st)["lateral_drift"] == NOTHING, spoiled
        st = play(c, [go, go, spoiled, go, go, go, go])                      # no segment on the dropping step; the next step opens one
        assert st.segments_dropped[0] == 1 and folded(st)["lateral_drift"][0] == 1 and st.seg_steps[0] == 0
    assert play(c, [go, go, dict(cmd=(0.5, 0.0, -0.0)), go]).segments_dropped[0] == 0            # -0 is 0
    st = play(c, [dict(cmd=(0.5, 0.0, 0.3))])                                # the opening step does not look at the yaw command
    assert st.seg_valid[0] == 1 and st.segments_dropped[0] == 0
    st = play(c, [go, go, dict(reset=1, age=0), go, go, go])                 # a reset inside: forgotten, not dropped
    assert st.segments_dropped[0] == 0 and (st.steps[0], st.resets[0]) == (6, 1) and folded(st)["lateral_drift"] == NOTHING and st.seg_steps[0] == 2
    assert folded(st)["tilt"][0] == 5 and folded(st)["accel_vertical"][0] == 3                   # and it breaks the velocity difference
    after = play(c, [go, go, dict(reset=1, age=0)])
    assert after.seg_valid[0] == 0 and after.prev_valid[0] == 0 and after.seg_steps[0] == 1
    ages = [1, 2, 3, 4, 5, 6, 7]                                             # warm-up 3: nothing before age 4; the segment opens there
    st = play(T.config(segment_steps=3, warmup_steps=3), [dict(p=(0.01 * a, 0.0), age=a) for a in ages])
    got = folded(st)
    assert got["tilt"][0] == 4 and got["accel_vertical"][0] == 3 and got["lateral_drift"][0] == 1 and st.steps[0] == 7
    assert abs(got["progress_err"][2] - (0.03 - 0.03)) < 1e-6 and st.seg_anchor[0, 0] == f32(0.07)
    st = play(c, [dict(yaw_q=(0.5, 0.5, 0.5, -0.5))] * 4)                   # a vertical robot: n = 0, no heading, no segment, nothing dropped
    assert st.seg_valid[0] == 0 and st.segments_dropped[0] == 0 and folded(st)["heading_drift"] == NOTHING and folded(st)["tilt"][0] == 4


def test_model_rates_and_accelerations():
    dt = f32(0.02)
    st = play(T.config(tilt_limit=0.25), [dict(v=(0.5, 0.0, 0.1), w=(0.0, 0.0, 1.0), g=(0.3, 0.4), bv=0.2, bw=(1.0, -2.0)),
                                          dict(v=(0.53, 0.04, 0.0), w=(0.2, 0.0, 1.0), g=(0.15, 0.2), bv=-0.1, bw=(0.0, 0.0))])
    got = folded(st)
    assert got["roll_sin"] == (2, 0, float(f32(0.2)), float(f32(0.4))) and got["pitch_sin"] == (2, 0, float(f32(0.15)), float(f32(0.3)))
    assert got["tilt"][0] == 2 and abs(got["tilt"][3] - 0.5) < 1e-7 and abs(got["tilt"][2] - 0.25) < 1e-7
    assert st.sum[T.TILT_EXCEEDED, 0] == 1.0 and got["tilt_exceeded"][0] == 2
    assert got["roll_rate"] == (2, 0, 0.0, 1.0) and got["pitch_rate"] == (2, 0, -2.0, 0.0) and got["vertical_vel"] == (2, 0, float(f32(-0.1)), float(f32(0.2)))
    ax, ay = (f32(0.53) - f32(0.5)) / dt, (f32(0.04) - f32(0.0)) / dt
    assert got["accel_horizontal"] == one(np.sqrt(ax * ax + ay * ay)) and abs(got["accel_horizontal"][2] - 2.5) < 1e-5
    assert got["accel_vertical"] == one((f32(0.0) - f32(0.1)) / dt) and got["ang_accel"] == one((f32(0.2) - f32(0.0)) / dt)
    assert st.prev_valid[0] == 1 and st.prev_lin_vel[:, 0].tolist() == [f32(0.53), f32(0.04), 0.0] and st.prev_ang_vel[:, 0].tolist() == [f32(0.2), 0.0, 1.0]
    assert st.tilt_hist[:, 0].tolist() == [0] * 8 + [1] + [0] * 6 + [1]       # 0.25 * 32 = 8; 0.5 is in the last bin


def test_model_tilt_histogram_and_tables():
    tilt = np.array([0.0, 0.03125, 0.031249998, 0.46875, 0.46874997, 0.9, 3.0, 1e30, -0.0], f32)
    assert T.tilt_bin(tilt).tolist() == [0, 1, 0, 15, 14, 15, 15, 15, 0]
    for value, want in ((0.0, 0), (0.03125, 1), (0.46875, 15), (0.46874997, 14), (2.0, 15), (NAN, None), (INF, None)):
        st = play(T.config(), [dict(g=(value, 0.0))])
        assert st.tilt_hist[:, 0].tolist() == [1 if k == want else 0 for k in range(16)], value
    c = T.config(segment_steps=2)
    st = play(c, [dict(), dict(), dict(cmd=(0.5, 0.0, 1.0)), dict(g=(0.5, 0.0))])
    table, hist = T.reduce(st, [0], 2)
    assert table.shape == (2, 18, 6) and hist.shape == (2, 16)
    assert table[0, 17].tolist() == [1.0, 4.0, 0.0, 1.0, 0.0, 0.0] and table[1, 17].tolist() == [0.0] * 6
    assert hist[0].tolist() == [3.0] + [0.0] * 14 + [1.0] and not hist[1].any()
    assert table[0, T.SUPPORT_FEET].tolist() == [4.0, 4.0, 0.0, 4.0, 4.0, 0.0] and np.isnan(table[1, :17, 1:5]).all()
    assert table[0, T.TILT_EXCEEDED, :2].tolist() == [4.0, 0.25]


def test_model_nonfinite_inputs():
    """NaN and +-inf in each input: counted in nonfinite of the rows the input enters, no sum is spoiled, the histogram skips the step"""
    base = [dict(), dict()]
    for bad in (NAN, INF, -INF):
        for kw, rows in ((dict(g=(bad, 0.0)), ["pitch_sin", "tilt"]), (dict(g=(0.0, bad)), ["roll_sin", "tilt"]), (dict(bv=bad), ["vertical_vel"]),
                         (dict(bw=(bad, 0.0)), ["roll_rate"]), (dict(bw=(0.0, bad)), ["pitch_rate"]), (dict(v=(bad, 0.0, 0.0)), ["accel_horizontal"]),
                         (dict(v=(0.0, 0.0, bad)), ["accel_vertical"]), (dict(w=(0.0, bad, 0.0)), ["ang_accel"]),
                         (dict(p=(bad, 0.0)), ["support_margin"]), (dict(feet=[(0.2, 0.2), (0.2, -0.2), (bad, 0.2), (-0.2, -0.2)]), ["support_margin"])):
            st = play(T.config(), base + [kw])
            got = folded(st)
            for name in T.METRICS[:14]:
                want = (2, 1) if name in rows else ((3, 0) if name not in ("accel_horizontal", "accel_vertical", "ang_accel") else (2, 0))
                if name in rows and name.startswith(("accel", "ang_accel")):
                    want = (1, 1)
                if name in ("support_line_dist",):
                    want = (0, 0)
                assert got[name][:2] == want, (bad, kw, name, got[name])
            assert np.isfinite(st.sum).all() and np.isfinite(st.sumsq).all()
            assert st.tilt_hist[:, 0].sum() == (2 if "g" in kw else 3)
    got = folded(play(T.config(), base + [dict(fz=(30.0, INF, NAN, -INF))]))     # +inf is a contact, NaN and -inf are none
    assert got["support_feet"] == (3, 0, 2.0, 4.0) and got["support_line_dist"][0] == 1
    st = play(T.config(segment_steps=2), [dict(), dict(cmd=(NAN, 0.0, 0.0)), dict()])                 # a NaN command spoils what it is summed into only
    got = folded(st)
    assert got["progress_err"][:2] == (0, 1) and got["lateral_drift"][:2] == (1, 0) and got["heading_drift"][:2] == (1, 0)
    got = folded(play(T.config(segment_steps=2), [dict(), dict(), dict(cmd=(0.5, -INF, 0.0))]))
    assert got["lateral_drift"][:2] == (0, 1) and got["progress_err"][:2] == (1, 0)
    for q in ((NAN, 0.0, 0.0, 1.0), (0.0, INF, 0.0, 1.0), (0.0, 0.0, -INF, 1.0), (0.0, 0.0, 0.5, NAN)):      # no heading: the open segment is dropped
        st = play(T.config(segment_steps=2), [dict(), dict(yaw_q=q)])
        assert st.segments_dropped[0] == 1 and st.seg_valid[0] == 0, q


# ---- 5. go1trunk.hip under the SIMT emulator against the model --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1trunk_host as G
    return G.load_library(build_emu(g.trunk_sources(), "libgo1trunk_emu.so"))


SHAPES_OF_INPUTS = dict(root_states=13, base_lin_vel=3, base_ang_vel=3, projected_gravity=3, commands=15, contact_forces=51, foot_positions=12)


def trunk_on(device, cfg_, N, lib=None):
    """a go1trunk_host.Go1Trunk on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1trunk_host as G
    tensors = {k: torch.zeros(rows, N, device=device) for k, rows in SHAPES_OF_INPUTS.items()}
    tensors.update(reset_buf=torch.zeros(N, dtype=torch.uint8, device=device), episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    tm = G.Go1Trunk(types.SimpleNamespace(num_envs=N), B, cfg_.dt, segment_steps=cfg_.segment_steps, tilt_limit=cfg_.tilt_limit, lib=lib)
    if torch.device(device).type == "cpu":
        tm._stream = lambda: None
    return tm, B


def trunk_groups(rng, N, groups=3):
    """three groups of which group 1 is empty, some environments at -1 and (from three environments on) one id outside the tables"""
    assert groups == 3
    group = rng.integers(-1, groups, N).astype(np.int32)
    group[group == 1] = 2
    group[0] = groups - 1
    if N >= 3:
        group[1], group[2] = -1, groups
    return group


def drive(tm, B, cfg_, snaps, group, groups):
    """the scripted steps through the library: arm for `groups` groups, upload a snapshot, accumulate, ...; returns read() and the
    accumulators.  arm() sizes the tables by the largest id it is given, so the ids outside the tables are handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    tm.arm(inside, cfg_.warmup_steps)
    tm.group.copy_(torch.from_numpy(group))
    for s in snaps:
        for k, a in s.items():
            getattr(B, k).copy_(torch.from_numpy(a))
        tm.accumulate()
    tm.disarm()
    res = tm.read()
    acc = {k: t.cpu().numpy() for k, t in tm.acc.items()}
    return res, acc


def check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N):
    """accumulators, state, histogram and both result tables against tests/trunk_ref.py, bit for bit; then what the script was written
    to drive"""
    st = T.run(cfg_, snaps, N)
    for k in ACCUMULATORS:
        assert acc[k].shape == (17, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in T.STATE:
        name = "env_" + k if k == "tilt_hist" else k
        assert res[name].shape == getattr(st, k).shape and bits(res[name].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    assert bits(res["env_max_tilt"]) == bits(st.max[T.TILT])
    want, want_hist = T.reduce(st, group, groups)
    table = np.concatenate([np.stack([res["metrics"][m] for m in T.METRICS], axis=1), np.zeros((groups, 1, 6))], axis=1)
    table[:, 17, :4] = res["groups"]
    assert table.shape == want.shape == (groups, T.ROWS, 6)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and bits(table) == bits(want)
    assert res["tilt_hist"].shape == (groups, 16) and bits(res["tilt_hist"]) == bits(want_hist) and res["tilt_edges"][1] == 0.03125
    steps = len(snaps)
    assert (res["steps"] == steps).all()
    if N >= len(T.KINDS):
        count, nonfinite = st.count, st.nonfinite
        walks = kind == 0
        # segments close one after the other; a reset or the warm-up breaks them
        quiet = walks & (st.resets == 0)
        assert quiet.any() and (count[T.LATERAL_DRIFT, quiet] == (steps - cfg_.warmup_steps - 1) // cfg_.segment_steps).all() and (st.segments_dropped[quiet] == 0).all()
        assert (res["resets"][kind == 1] >= 4).all() and snaps[0]["reset_buf"][kind == 1].all() and (count[T.LATERAL_DRIFT, kind == 1] == 0).all()
        assert (count[T.TILT, kind == 1] <= 4).all() and count[T.TILT].max() == steps - cfg_.warmup_steps
        # a yaw command and a NaN command dropped a segment each, and segments closed in between
        turns = kind == 2
        assert (st.segments_dropped[turns & (st.resets == 0)] == 2).all() and count[T.LATERAL_DRIFT, turns].sum() > 0
        # every number of supporting feet from the pattern; both kinds of support row folded
        assert count[T.SUPPORT_MARGIN, walks].sum() > 0 and count[T.SUPPORT_LINE_DIST, walks].sum() > 0
        assert st.min[T.SUPPORT_FEET, walks].min() == 1.0 and st.max[T.SUPPORT_FEET, walks].max() == 4.0
        # +-inf and NaN were met and entered no sum; coincident feet gave a non-finite margin
        odd = kind == 4
        assert nonfinite[:, odd].sum() > 0 and nonfinite[T.SUPPORT_MARGIN, odd].sum() > 0 and np.isfinite(st.sum).all() and np.isfinite(st.sumsq).all()
        # a robot that stands on its square: four feet, the margin 0.14 (half the stance's width), on every folded step
        stands = (kind == 5) & (count[T.TILT] > 0)
        assert (st.min[T.SUPPORT_FEET, stands] == 4.0).all() and (np.abs(st.min[T.SUPPORT_MARGIN, stands] - 0.14) < 1e-5).all()
        assert (count[T.SUPPORT_MARGIN, kind == 5] == count[T.TILT, kind == 5]).all()
        # the vertical ones: the last bin was filled, and the steps without a heading dropped their segment
        up = kind == 6
        assert st.tilt_hist[15, up].sum() > 0 and (st.segments_dropped[up & (st.resets == 0)] >= 1).all()
        sane = ~odd
        assert (st.tilt_hist.sum(axis=0)[sane] == count[T.TILT, sane]).all()
    g = res["groups"]
    assert g[:, 0].sum() == np.isin(group, range(groups)).sum() and (g[:, 1] == steps * g[:, 0]).all() and g[1].tolist() == [0.0] * 4
    assert np.isnan(want[1, :17, 1:5]).all() and not want_hist[1].any()
    return st


# 1: one thread; 64: one wavefront; 257: two blocks with a ragged tail; 600: three terms per reduction thread and 38 environments per
# histogram slice
SHAPES = [1, 64, 257, 600]


@pytest.mark.parametrize("N", SHAPES)
def test_emulated_trunk_kernels_follow_the_model(emu, N):
    groups = 3
    rng = np.random.default_rng(500 + N)
    cfg_, snaps, kind = T.scripted_steps(rng, N)
    assert len(snaps) >= 12 and cfg_.segment_steps == 3 and (N < len(T.KINDS) or set(kind.tolist()) == set(range(len(T.KINDS))))
    group = trunk_groups(rng, N, groups)
    tm, B = trunk_on("cpu", cfg_, N, lib=emu)
    res, acc = drive(tm, B, cfg_, snaps, group, groups)
    assert tm.cfg.num_groups == groups and (N < 3 or {-1, groups} <= set(group.tolist()))
    check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N)
    with pytest.raises(RuntimeError, match="go1trunk_accumulate failed: -12"):
        tm.cfg.segment_steps = 0
        tm.accumulate()


# ---- 6. the environment hooks without a GPU ---------------------------------------------------------------------------------------------------
def test_trunk_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    for module in ("go1eval_host", "go1feet_host", "go1trunk_host"):
        monkeypatch.delitem(sys.modules, module, raising=False)
    c = apply_train_config(make_cfg(), num_envs=16)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_trunk_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_trunk_metrics, env.read_trunk_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert all(m not in sys.modules for m in ("go1eval_host", "go1feet_host", "go1trunk_host")) and env._trunk is None      # never measured: no host module
    env.step(torch.zeros(16, 12))                                             # and stepping goes on
    import inspect
    signature = inspect.signature(env.start_trunk_metrics)
    assert {k: p.default for k, p in signature.parameters.items() if k != "groups"} == dict(warmup_steps=0, segment_steps=50, tilt_limit=0.25)
    assert "placeholder" in env.start_trunk_metrics.__doc__


# ---- 6b. the two scenarios of the GPU tests, through the fp64 oracle here ----------------------------------------------------------------------
TROT_STEPS, TROT_WARMUP, TROT_SEGMENT, TROT_PAUSE = 80, 2, 10, 3
STANDING_WARMUP, STANDING_STEPS = 50, 100
# the oracle on the standing scenario (test_standing_robot_through_the_oracle prints and pins both): the mean support margin of its fp64
# build, and how far its fp32 build's lies from that
STANDING_MARGIN_FP64 = 0.156953          # m
STANDING_MARGIN_FP32_DEVIATION = 6.2e-9   # m


def oracle_rollout(env, actions, cfg_, straight=True):
    """the model of tests/trunk_ref.py replayed on the buffers after every step of `actions` (an iterable of (N, 12) tensors); with
    `straight` the yaw command is held at 0, as a sweep's cell would.  Returns (state, what every step formed)"""
    st, formed = T.State(env.num_envs), []
    for action in actions:
        if straight:
            env.commands[:, 2] = 0.0
        env.step(action)
        formed.append(T.accumulate(st, cfg_, {n: getattr(env.buffers, n).cpu().numpy().copy() for n in T.INPUTS}))
    return st, formed


def set_down(env):
    """put every robot of a freshly reset environment down at rest in its default pose, where reset() put its base.  reset() spawns with random joint angles
    (+- 0.5 rad about the default pose) and random velocities (up to 0.5 m/s and more than 1 rad/s): with zero actions about three
    robots in 64 tumble from that and end sitting on their rump, the front feet loaded and the hind feet in the air"""
    B = env.buffers
    B.root_states[7:13] = 0.0
    B.dof_pos[:] = env.default_dof_pos.reshape(-1)[:12].to(B.dof_pos.device)[:, None]
    B.dof_vel.zero_()
    # and make it the nominal robot: the randomised parameters are drawn with the device's generator, so a CPU and a GPU environment of one
    # seed would otherwise be different robots, and their stances a few millimetres apart (motor offsets of +- 0.02 rad)
    B.motor_offsets.zero_(), B.motor_strengths.fill_(1.0), B.payloads.zero_(), B.friction_coeffs.fill_(1.0), B.restitutions.zero_()


def standing_rollout(device):
    """the standing scenario (test_foot_metrics.standing_env, the robots set down at rest) through the model: (state, what every step
    formed)"""
    from test_foot_metrics import standing_env
    env = standing_env(64, device)
    env.reset()
    set_down(env)
    cfg_ = T.config(dt=float(env.dt), warmup_steps=STANDING_WARMUP)
    return oracle_rollout(env, (torch.zeros(64, 12, device=env.device) for _ in range(STANDING_WARMUP + STANDING_STEPS)), cfg_)


def mean_margin(st):
    return float(st.sum[T.SUPPORT_MARGIN].sum() / st.count[T.SUPPORT_MARGIN].sum())


def test_standing_robot_through_the_oracle(monkeypatch):
    """the scenario of test_gpu_trunk_metrics.test_a_standing_robot_is_over_its_feet on the CPU oracle: four supporting feet and a
    positive margin on every folded step.  The same scenario through the oracle's fp32 build gives the deviation that the GPU test's
    allowance is twice of: both figures are printed and pinned here."""
    import fake_sim
    import go1sim_host as H
    import pyoracle
    fake_sim.install(monkeypatch)
    st, _ = standing_rollout("cuda:0")
    assert st.resets.sum() == 0 and (st.count[T.TILT] == STANDING_STEPS + 1).all()          # reset() took the first step of the episode
    assert (st.min[T.SUPPORT_FEET] == 4.0).all() and (st.max[T.SUPPORT_FEET] == 4.0).all() and (st.count[T.SUPPORT_MARGIN] == STANDING_STEPS + 1).all()
    assert (st.min[T.SUPPORT_MARGIN] > 0.0).all() and st.sum[T.MARGIN_NEGATIVE].sum() == 0.0

    class Fp32Sim(fake_sim.OracleBackedSim):
        def __init__(self, S, buffers, device_index=0):
            super().__init__(S, buffers, device_index)
            self.orc = pyoracle.Oracle(S, buffers, fp32=True)
    monkeypatch.setattr(H, "Go1Sim", Fp32Sim)
    single, _ = standing_rollout("cuda:0")
    mean, deviation = mean_margin(st), mean_margin(single) - mean_margin(st)
    print(f"\noracle: mean support margin of the standing robot {mean:.6f} m (smallest {st.min[T.SUPPORT_MARGIN].min():.6f} m); its fp32 build "
          f"{mean_margin(single):.6f} m: a deviation of {deviation:+.3e} m; mean tilt {st.sum[T.TILT].sum() / st.count[T.TILT].sum():.5f}, "
          f"segments closed {int(st.count[T.LATERAL_DRIFT].sum())}")
    assert (single.min[T.SUPPORT_FEET] == 4.0).all() and single.resets.sum() == 0
    assert abs(mean - STANDING_MARGIN_FP64) < 2e-6 and abs(deviation - STANDING_MARGIN_FP32_DEVIATION) < 1e-6


def trot_with_pauses(step, N):
    """test_foot_metrics.trot_action with every pair's lift cut short by TROT_PAUSE steps, so that between the two diagonal pairs'
    swings all four feet are down for a while: steps on two feet, and steps on three and four"""
    from test_foot_metrics import TROT_PERIOD, trot_action
    env = torch.arange(N)
    phase = (step + (env % 4 == 3) * (TROT_PERIOD // 2)) % (TROT_PERIOD // 2)
    return trot_action(step, N) * (phase < TROT_PERIOD // 2 - TROT_PAUSE).float()[:, None]


def test_the_trot_script_produces_events_on_the_oracle(monkeypatch):
    """the scenario of test_gpu_trunk_metrics.test_trunk_through_the_environment on the CPU oracle: under the foot family's trot script
    (with pauses) every environment has at least one step on three or more feet, one on exactly two, and one closed segment"""
    import fake_sim
    from test_gpu_response_trace import make_env
    fake_sim.install(monkeypatch)
    N = 64
    env = make_env(N, "plane", 20.0, seed=4)
    env.reset()
    cfg_ = T.config(dt=float(env.dt), segment_steps=TROT_SEGMENT, warmup_steps=TROT_WARMUP)
    st, formed = oracle_rollout(env, (trot_with_pauses(step, N) for step in range(TROT_STEPS)), cfg_)
    events = trot_events(st)
    print(f"\noracle: per environment, the fewest steps on >= 3 feet {events[0].min()}, on 2 feet {events[1].min()}, closed segments {events[2].min()}; "
          f"resets {int(st.resets.sum())}, dropped {int(st.segments_dropped.sum())}")
    assert all((e >= 1).all() for e in events)


def trot_events(st):
    """per environment: steps folded with n_c >= 3, with n_c == 2, and closed segments"""
    return (st.count[T.SUPPORT_MARGIN] + st.nonfinite[T.SUPPORT_MARGIN], st.count[T.SUPPORT_LINE_DIST] + st.nonfinite[T.SUPPORT_LINE_DIST],
            st.count[T.LATERAL_DRIFT] + st.nonfinite[T.LATERAL_DRIFT])


# ---- 7. the sweep's host pieces and the tool --------------------------------------------------------------------------------------------------
def fixed_result():
    import go1trunk_host as G
    row = lambda mean, top: np.array([[30.0, mean, 0.5, -top, top, 0.0], [10.0, 2 * mean, 0.5, -2 * top, 2 * top, 1.0]])
    trunk = {m: row(0.25, 2.0) for m in T.METRICS}
    trunk["tilt"], trunk["support_feet"], trunk["accel_vertical"] = row(0.1, 0.3), row(2.5, 4.0), row(0.0, 9.81)
    trunk["support_line_dist"][1] = [0.0, NAN, NAN, NAN, NAN, 0.0]            # a cell that never stood on two feet
    hist = np.zeros((2, 16))
    hist[:, :4] = [[100.0, 50.0, 10.0, 1.0]] * 2
    return dict(preset="static_medium", cells=[(0.5, 0.0, (0.5, 0.0, 0.0)), (1.0, 0.0, (0.5, 0.0, 0.0))], trunk=trunk,
                trunk_groups=np.array([[8.0, 320.0, 1.0, 2.0], [8.0, 320.0, 0.0, 0.0]]), tilt_hist=hist, tilt_edges=G.tilt_edges(), metrics={},
                groups=np.zeros((2, 5)), segment_steps=50, tilt_limit=0.25, num_envs=16, steps=40, warmup_steps=5, seed=1, dt=0.02)


def test_trunk_table_json_and_figure(tmp_path):
    from go1_gym_learn.eval_metrics import trunk
    res = fixed_result()
    md = trunk.trunk_markdown_table(res).splitlines()
    assert md[0].startswith("| vx | yaw | mean tilt [deg] | max tilt [deg] | beyond limit | rms roll rate | rms pitch rate | rms vz | rms a_h [g] |") and len(md) == 2 + 2
    assert md[0].count("|") == md[1].count("|") == md[2].count("|") == md[3].count("|") == 22
    tilt_deg, top_deg = np.degrees(np.arcsin(0.1)), np.degrees(np.arcsin(0.3))
    rms = np.sqrt(0.25 + 0.0625)
    assert md[2].startswith(f"| 0.5 | 0 | {tilt_deg:.2f} | {top_deg:.2f} | 0.2500 | {rms:.3f} | {rms:.3f} | {rms:.3f} | {rms / 9.81:.3f} | {2.0 / 9.81:.3f} | {0.5 / 9.81:.3f} | 1.000 | 2.50 |")
    assert md[2].endswith("| 30 | 2 |") and md[3].endswith("| 11 | 0 |") and "| – |" in md[3] and "| – |" not in md[2]
    js = json.loads(json.dumps(trunk.trunk_to_json(res), allow_nan=False))
    assert js["cells"][1] == dict(vx=1.0, yaw=0.0, gait=[0.5, 0.0, 0.0]) and js["group_fields"] == T.GROUP_FIELDS and js["tilt_limit"] == 0.25
    assert js["trunk"]["tilt"][0][1] == 0.1 and js["trunk"]["support_line_dist"][1][1] is None and js["tilt_hist"][1][:4] == [100.0, 50.0, 10.0, 1.0]
    assert len(js["tilt_edges"]) == 17 and js["tilt_edges"][16] is None and js["segment_steps"] == 50 and js["trunk_groups"][0][3] == 2.0
    path = tmp_path / "tilt.png"
    trunk.plot_tilt(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000


def test_tool_accepts_a_trunk_sweep(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import trunk
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--trunk", "--vx", "0.5", "1.0", "--envs", "16", "--steps", "40", "--warmup-steps", "5", "--presets", "static_medium",
                                      "--segment-steps", "20", "--tilt-limit", "0.3"])
    assert a.trunk and not a.feet and not a.joints and not a.tiles and (a.vx, a.envs, a.steps, a.terrain, a.segment_steps, a.tilt_limit) == ([0.5, 1.0], 16, 40, None, 20, 0.3)
    plain = eval_sweep.parse_args(base + ["--trunk"])
    assert (plain.segment_steps, plain.tilt_limit) == (50, 0.25) and not eval_sweep.parse_args(base).trunk
    assert eval_sweep.parse_args(base + ["--trunk", "--terrain", "plane"]).terrain == "plane"
    for bad in (["--trunk", "--terrain"], ["--trunk", "--behaviour"], ["--trunk", "--joints"], ["--trunk", "--feet"], ["--trunk", "--response", "--switch", "vx", "0", "1"],
                ["--trunk", "--push", "--magnitude", "1", "--direction", "0"], ["--segment-steps", "20"], ["--feet", "--tilt-limit", "0.3"],
                ["--trunk", "--segment-steps", "0"], ["--trunk", "--tilt-limit", "-0.1"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(base + bad)
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(trunk, "run_trunk_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    eval_sweep.run_trunk(a, None, dict(vx=a.vx, yaw=a.yaw, gait=[(0.5, 0.0, 0.0)]))
    assert seen == dict(preset="static_medium", grid=dict(vx=[0.5, 1.0], yaw=[0.0], gait=[(0.5, 0.0, 0.0)]), num_envs=16, steps=40, warmup_steps=5, seed=1,
                        terrain=None, segment_steps=20, tilt_limit=0.3)
    js = json.load(open(tmp_path / "eval" / "static_medium_trunk.json"))
    assert js["preset"] == "static_medium" and js["tilt_hist"][0][0] == 100.0
    md = (tmp_path / "eval" / "static_medium_trunk.md").read_text()
    assert "| 0.5 | 0 | 5.74 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_tilt.png").read_bytes()[:4] == b"\x89PNG"
