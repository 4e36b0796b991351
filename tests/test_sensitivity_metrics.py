"""CPU checks of the sensitivity family (include/go1sens.h, libgo1sens.so): the ctypes mirrors and the exported symbols against the
header, the build's source list (as the compiler reads it), flags and stamp, the refusals without a GPU, the model of tests/sens_ref.py on
hand-computed three-step cases, hazard, Wilson interval, effect and ranking by hand, go1sens.hip itself under the SIMT emulator against
that model bit for bit (accumulators, state and the four result tables), the environment hooks where there is no GPU, the default ranges,
the tool's parsing, the sweep's files, and the GPU environment test's rollout on the oracle-backed simulator with the emulated kernels
stepped by the environment itself."""
import ctypes
import functools
import inspect
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

import sens_ref as T
from test_eval_return_codes import Call, cfg, each, element, nobody, null
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from util import build_emu

HEADER = os.path.join(REPO, "include", "go1sens.h")
SOURCE = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1sens.hip")
TABLES = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1_tables.h")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]
TABLE_NAMES = ["results", "curves", "counts", "pair_results"]


# ---- 1. mirrors, symbols, sources, stamp ---------------------------------------------------------------------------------------------------
def test_sensitivity_mirrors_match_the_header():
    import go1sens_host as G
    src = open(HEADER).read()
    for macro, value in (("GO1SENS_NUM", G.NUM_PARAMETERS), ("GO1SENS_BINS", G.BINS), ("GO1SENS_NUM_QUANT", G.NUM_QUANT), ("GO1SENS_NUM_COUNTS", G.NUM_COUNTS),
                         ("GO1SENS_PAIR_SIDE", G.PAIR_SIDE), ("GO1SENS_PAIR_CELLS", G.PAIR_CELLS), ("GO1SENS_PAIR_QUANT", G.PAIR_QUANT),
                         ("GO1SENS_NUM_FIELDS", 6), ("GO1SENS_REDUCE_THREADS", 256)):
        assert re.search(rf"#define {macro} {value}\n", src), macro
    assert (G.NUM_PARAMETERS, G.BINS, G.NUM_QUANT, G.NUM_COUNTS, G.PAIR_CELLS, G.PAIR_QUANT) == (9, 16, 8, 3, 64, 4) == (T.P, T.BINS, len(T.QUANTITIES), len(T.COUNTS), T.CELLS, len(T.PAIR_QUANTITIES))
    want = struct_fields(src, "Go1SensConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1SensConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "pair_a", "pair_b", "active", "lo", "scale"]
    arrays = {"int32_t[GO1SENS_NUM]": ctypes.c_int32 * 9, "float[GO1SENS_NUM]": ctypes.c_float * 9}
    for (field, ctext), (_, ctype) in zip(want, G.Go1SensConfig._fields_):
        assert ctype is C_TYPES[ctext] if ctext in C_TYPES else (ctype._type_, ctype._length_) == (arrays[ctext]._type_, 9), field
    assert ctypes.sizeof(G.Go1SensConfig) == 5 * 4 + 3 * 9 * 4
    want = struct_fields(src, "Go1SensBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1SensBuffers._fields_] == T.INPUTS + ACCUMULATORS + T.STATE + ["group"] + TABLE_NAMES
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1SensBuffers._fields_)
    types_ = dict(want)
    assert types_["cur"] == types_["pair_cur"] == "float*" and types_["reset_buf"] == types_["time_out_buf"] == "const uint8_t*"
    assert all(types_[k] == "const float*" for k in T.PARAMETER_INPUTS) and types_["episode_length_buf"] == "const int32_t*"
    assert all(types_[k] == "uint32_t*" for k in ("steps", "measured", "falls", "timeouts", "unbinned", "redraws", "bad", "launches", "pair_steps", "pair_falls", "pair_measured"))
    assert all(types_[k] == "double*" for k in ("reward_sum", "lin_err_sum", "yaw_err_sum", "power_sum", "pair_lin_err_sum") + tuple(TABLE_NAMES))
    assert G._SENS_INPUTS == T.INPUTS and G._SENS_STATE == T.STATE == list(G.Go1Sensitivity.STATE) and G._SENS_TABLES == TABLE_NAMES
    st = T.clear(2, T.script_config(), {k: np.zeros((3, 2) if k == "com_displacements" else (12, 2) if k[0] in "mK" else 2, f32) for k in T.PARAMETER_INPUTS})
    for name, (dtype, lead) in G.Go1Sensitivity.STATE.items():                # the model's formats are the host's (uint32 read as int32)
        assert getattr(st, name).shape == (*lead, 2) and getattr(st, name).dtype.itemsize == torch.zeros(1, dtype=dtype).element_size(), name
    names = [n.replace("kp_factor", "Kp_factor").replace("kd_factor", "Kd_factor") for n in enum_order(src, "Go1SensParam", "GO1SENS_")]
    assert names == G.PARAMETERS == T.PARAMETERS and len(names) == 9
    assert enum_order(src, "Go1SensQuantity", "GO1SENS_Q_") == G.QUANTITIES == T.QUANTITIES
    assert enum_order(src, "Go1SensCount", "GO1SENS_C_") == G.COUNTS == T.COUNTS
    assert enum_order(src, "Go1SensPairQuantity", "GO1SENS_P_") == G.PAIR_QUANTITIES == T.PAIR_QUANTITIES
    assert enum_order(src, "Go1SensGroupField", "GO1SENS_G_") == G.SENS_GROUP_FIELDS == T.GROUP_FIELDS
    import go1eval_host as E
    assert enum_order(src, "Go1SensField", "GO1SENS_F_") == E.FIELD_NAMES
    assert issubclass(G.Go1Sensitivity, E._Table) and G.Go1Sensitivity.ROWS == 9 and G.Go1Sensitivity.TABLE_ROWS == 10
    assert list(G.DOMAIN_RAND) == G.PARAMETERS
    from go1_gym_learn.eval_metrics import sensitivity
    assert sensitivity.PARAMETERS == G.PARAMETERS and sensitivity.QUANTITIES == G.QUANTITIES and sensitivity.COUNTS == G.COUNTS and sensitivity.BINS == G.BINS
    # the memory the header's layout takes per environment: the estimate the documents quote
    per_env = {n: int(np.prod(lead, dtype=np.int64)) * torch.zeros(1, dtype=dt).element_size() for n, (dt, lead) in G.Go1Sensitivity.STATE.items()}
    assert sum(per_env[q] for q in T.QUANTITIES) == 9 * 16 * (4 * 4 + 4 * 8) == 6912 and sum(v for k, v in per_env.items() if k.startswith("pair_") and k != "pair_cur") == 1280


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1sens_host as G
    declared = set(re.findall(r"\b(go1sens_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1sens_clear", "go1sens_snapshot", "go1sens_accumulate", "go1sens_reduce", "go1sens_version"}
    out = g.build_sens_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1sens_" in line} == declared
    assert not re.search(r"\bgo1(eval|feet|trunk|gait|episode)_\w+", dynamic)


def test_sources_flags_and_stamp():
    import __graft_entry__ as g
    assert g.sens_sources() == [SOURCE, TABLES, HEADER] and g.SENS_FLAGS == g.EPISODE_FLAGS == g.EVAL_FLAGS and "-ffp-contract=off" in g.SENS_FLAGS
    assert g.SENS_FLAGS is not g.EVAL_FLAGS and g.SENS_FLAGS is not g.EPISODE_FLAGS
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc] + g.SENS_FLAGS + ["--cuda-host-only", "-MM", SOURCE], cwd=g.CSRC, check=True, capture_output=True, text=True).stdout
    read = {os.path.normpath(os.path.join(g.CSRC, f)) for f in out.split(":", 1)[1].replace("\\\n", " ").split()}
    assert {f for f in read if not f.startswith("/opt/")} == {os.path.normpath(f) for f in g.sens_sources()}
    for others in (g.sim_sources(), g.ppo_sources(), g.render_sources(), g.state_sources()):
        assert not set(others) & set(g.sens_sources())
    for others in (g.eval_sources(), g.feet_sources(), g.trunk_sources(), g.gait_sources(), g.spectrum_sources(), g.place_sources(), g.reward_sources(), g.episode_sources()):
        assert set(others) & set(g.sens_sources()) == {TABLES}                   # one shared header, and nothing else
    code = re.sub(r"//.*", "", open(SOURCE).read())
    assert not re.search(r"go1(eval|feet|trunk|gait|episode)", code) and "GO1_TABLES_MATCH(GO1SENS)" in code
    assert "go1sens" not in re.sub(r"//.*", "", open(TABLES).read())             # the shared header names no library
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["../../include/go1sens.h", "go1_tables.h"]
    for banned in ("atomic", "sinf", "cosf", "atan2f", "expf", "powf"):
        assert banned not in code, banned
    accumulate = code[code.index("sens_accumulate_kernel(const SensArgs A)"):code.index("sens_reduce_kernel(const SensArgs A)")]
    assert "__shared__" not in accumulate and "__syncthreads" not in accumulate and "row_thread(N, NP + 1" in accumulate
    out = g.build_sens_hip()
    assert os.path.basename(out) == "libgo1sens.so" and g.library_stamp(out) == g.source_hash(g.sens_sources(), g.SENS_FLAGS)
    lib = ctypes.CDLL(out)                                                       # dlopen needs no GPU
    lib.go1sens_version.restype = ctypes.c_char_p
    assert lib.go1sens_version() == b"go1sens 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    assert "build_sens_hip()" in inspect.getsource(g.build) and "libgo1sens.so" in inspect.getsource(g.smoke)
    # the other table libraries' stamps are what their own sources give: this family changed none of them
    for name, sources, flags in (("eval", g.eval_sources(), g.EVAL_FLAGS), ("feet", g.feet_sources(), g.FEET_FLAGS), ("episode", g.episode_sources(), g.EPISODE_FLAGS)):
        assert g.library_stamp(os.path.join(g.CSRC, f"libgo1{name}.so")) in (None, g.source_hash(sources, flags)), name


def test_a_missing_library_fails_loudly(tmp_path):
    import go1sens_host as G
    with pytest.raises(G.Go1SensLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1sens.so"))


# ---- 2. the refusals without a GPU (the helpers of tests/test_eval_return_codes.py) ----------------------------------------------------------
def sens_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.pair_a, c.pair_b = 70, 2, 3, 0, 6
    for p in range(9):
        c.active[p], c.lo[p], c.scale[p] = 1, -0.5, 4.0


SENS_ACC = ACCUMULATORS + T.STATE
BAD_CONFIG = [("scale = 0", -12, [element("scale", 2, 0.0)]), ("scale < 0", -12, [element("scale", 0, -4.0)]), ("scale NaN", -12, [element("scale", 8, NAN)]),
              ("scale inf", -12, [element("scale", 5, INF)]), ("lo NaN", -12, [element("lo", 3, NAN)]), ("lo inf", -12, [element("lo", 3, -INF)]),
              ("pair_a = 9", -12, [cfg(pair_a=9)]), ("pair_a = -2", -12, [cfg(pair_a=-2)]), ("pair_b = 9", -12, [cfg(pair_b=9)]), ("pair_b = -2", -12, [cfg(pair_b=-2)]),
              ("a pair of equal indices", -12, [cfg(pair_a=3, pair_b=3)]), ("half a pair", -12, [cfg(pair_a=-1, pair_b=3)]), ("the other half", -12, [cfg(pair_a=3, pair_b=-1)]),
              ("pair_a inactive", -12, [element("active", 0, 0)]), ("pair_b inactive", -12, [element("active", 6, 0)])]
TAKES = nobody() + each(SENS_ACC, -2) + each(T.PARAMETER_INPUTS, -3) + [
    ("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")]),
    ("no cur and no payloads", -2, [null("cur", "payloads")])]
CASES = {
    "go1sens_clear": TAKES,
    "go1sens_snapshot": TAKES,
    "go1sens_accumulate": nobody() + each(SENS_ACC, -2) + each(T.INPUTS, -3) + BAD_CONFIG + [
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no steps and no rew_buf", -2, [null("steps", "rew_buf")]),
        ("no pair_cur and scale = 0", -2, [null("pair_cur"), element("scale", 1, 0.0)]),
        ("no Kd_factors and scale = 0", -3, [null("Kd_factors"), element("scale", 1, 0.0)]),
        ("no reset_buf and pair_a = 9", -3, [null("reset_buf"), cfg(pair_a=9)])],
    "go1sens_reduce": nobody() + each(SENS_ACC, -2) + [
        ("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group"] + TABLE_NAMES, -5) + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no bad and no curves", -2, [null("bad", "curves")]),
        ("no launches and num_groups = 0", -2, [null("launches"), cfg(num_groups=0)])],
}


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    """every case fails validation, so nothing is launched: there is no GPU.  What is not refused (an inactive parameter without bins, no
    pair, a pair the other way round) gets as far as -3 with an input missing."""
    import __graft_entry__ as g
    import go1sens_host as G
    g.build_sens_hip()
    fn = getattr(G.load_library(), symbol)
    assert len({label for label, _, _ in CASES[symbol]}) == len(CASES[symbol])
    assert sum(len(spoilers) > 1 for _, _, spoilers in CASES[symbol]) >= 1          # two conditions at once: precedence
    for label, code, spoilers in CASES[symbol]:
        a = Call(G.Go1SensConfig, G.Go1SensBuffers, sens_base)
        for spoil in spoilers:
            spoil(a)
        assert fn(None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b), None) == code, (symbol, label)
    if symbol == "go1sens_accumulate":
        inactive = lambda a: (element("active", 4, 0)(a), element("scale", 4, NAN)(a), element("lo", 4, INF)(a))
        for good in (inactive, cfg(pair_a=-1, pair_b=-1), cfg(pair_a=8, pair_b=0), element("scale", 2, 1e-30), element("lo", 2, -3e38)):
            a = Call(G.Go1SensConfig, G.Go1SensBuffers, sens_base)
            good(a)
            null("reset_buf")(a)
            assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -3
    else:                                                                    # the others read no step input and test no bins and no pair
        a = Call(G.Go1SensConfig, G.Go1SensBuffers, sens_base)
        null(*T.STEP_INPUTS)(a)
        cfg(pair_a=9)(a)
        element("scale", 0, NAN)(a)
        null("count")(a)
        assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -2


# ---- 3. the model by hand ---------------------------------------------------------------------------------------------------------------------
def params_of(friction=1.0, motor=1.0, payload=0.0):
    """the seven parameter buffers of one environment"""
    return dict(friction_coeffs=np.full(1, friction, f32), restitutions=np.full(1, 0.5, f32), payloads=np.full(1, payload, f32),
                com_displacements=np.zeros((3, 1), f32), motor_strengths=np.full((12, 1), motor, f32), Kp_factors=np.ones((12, 1), f32), Kd_factors=np.ones((12, 1), f32))


def snap_of(r=0.0, reset=0, timed=0, age=5, vel=(0.0, 0.0), wz=0.0, cmd=(0.0, 0.0, 0.0), tau=0.0, qd=0.0, **params):
    """one environment after a step"""
    s = dict(rew_buf=np.full(1, r, f32), reset_buf=np.full(1, reset, np.uint8), time_out_buf=np.full(1, timed, np.uint8), episode_length_buf=np.full(1, age, np.int32),
             base_lin_vel=np.zeros((3, 1), f32), base_ang_vel=np.zeros((3, 1), f32), commands=np.zeros((15, 1), f32), torques=np.full((12, 1), tau, f32),
             dof_vel=np.full((12, 1), qd, f32), **params_of(**params))
    s["base_lin_vel"][:2, 0], s["base_ang_vel"][2, 0], s["commands"][:3, 0] = vel, wz, cmd
    return s


# friction in [0, 4): bins a quarter wide; motor strength in [0, 2): bins an eighth wide; payload in [-1, 3).  Every figure below is exact
HAND = dict(friction=(0.0, 4.0), motor_strength=(0.0, 2.0), payload=(-1.0, 3.0))
FRICTION, PAYLOAD, COM_Y, MOTOR = 0, 2, 4, 6


def play(cfg_, first, steps):
    """the model on one environment: a clear on params_of(**first), then a launch per entry of `steps` = [snap_of's keywords]"""
    st, did = T.clear(1, cfg_, params_of(**first)), []
    for kw in steps:
        did.append(T.accumulate(st, cfg_, snap_of(**kw)))
    return st, did


def per_bin(words, p):
    return words[p, :, 0].tolist()


def only(bin_, value=1):
    return [value if k == bin_ else 0 for k in range(16)]


@pytest.mark.parametrize("timed", [0, 1])
def test_model_a_redraw_between_two_launches_is_charged_to_the_old_bin(timed):
    """friction 1.0 (bin 4) is in force for two steps; the second is a reset step whose buffers already hold the respawned robot's friction
    3.0 (bin 12) and motor strength 0.5 (bin 4, from 1.0: bin 8): the exposure of both launches and the fall (or the time-out, which is
    no fall) belong to the old bins, the third launch to the new ones"""
    steps = [dict(r=0.5, vel=(3.0, 4.0), wz=-0.5, tau=0.5, qd=2.0), dict(r=-1.0, reset=1, timed=timed, age=0, vel=(9.0, 9.0), friction=3.0, motor=0.5),
             dict(r=0.25, age=1, cmd=(1.0, 0.0, 0.25), friction=3.0, motor=0.5)]
    st, did = play(T.config(HAND, pair=("friction", "motor_strength")), dict(), steps)
    assert [d["bin"][FRICTION, 0] for d in did] == [4, 4, 12] and [d["bin"][MOTOR, 0] for d in did] == [8, 8, 4] and [d["bin"][PAYLOAD, 0] for d in did] == [4, 4, 4]
    assert per_bin(st.steps, FRICTION) == [2 if k == 4 else 1 if k == 12 else 0 for k in range(16)]
    gone, other = (st.timeouts, st.falls) if timed else (st.falls, st.timeouts)
    assert per_bin(gone, FRICTION) == only(4) and per_bin(gone, MOTOR) == only(8) and per_bin(gone, PAYLOAD) == only(4) and not other.any()
    assert per_bin(st.reward_sum, FRICTION) == [-0.5 if k == 4 else 0.25 if k == 12 else 0.0 for k in range(16)]
    # the reset step enters no outcome: its velocities are the respawned robot's
    assert per_bin(st.measured, FRICTION) == [1 if k in (4, 12) else 0 for k in range(16)]
    assert per_bin(st.lin_err_sum, FRICTION) == [5.0 if k == 4 else 1.0 if k == 12 else 0.0 for k in range(16)]
    assert per_bin(st.yaw_err_sum, MOTOR) == [0.5 if k == 8 else 0.25 if k == 4 else 0.0 for k in range(16)]
    assert per_bin(st.power_sum, PAYLOAD) == only(4, 12.0)
    assert st.redraws[:, 0].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 0] and st.cur[FRICTION, 0] == 3.0 and st.cur[MOTOR, 0] == 0.5 and st.launches[0] == 3
    assert (st.count[FRICTION, 0], st.min[FRICTION, 0], st.max[FRICTION, 0], st.sum[FRICTION, 0]) == (3, 1.0, 3.0, 5.0) and st.count[COM_Y, 0] == 0
    # the pair map: cell 8 * (4 >> 1) + (8 >> 1) twice, then 8 * (12 >> 1) + (4 >> 1)
    assert st.pair_steps[:, 0].tolist() == [2 if k == 20 else 1 if k == 50 else 0 for k in range(64)]
    assert st.pair_falls[:, 0].tolist() == [1 - timed if k == 20 else 0 for k in range(64)]
    assert st.pair_measured[:, 0].tolist() == [1 if k in (20, 50) else 0 for k in range(64)] and st.pair_lin_err_sum[20, 0] == 5.0 and st.pair_cur[:, 0].tolist() == [3.0, 0.5]
    table, curves, counts, pair = T.reduce(st, [0], 1)
    assert table[0, 9].tolist() == [1.0, 3.0, 0.0, 0.0, 0.0, 0.0] and table[0, FRICTION, :5].tolist() == [3.0, 5.0 / 3.0, np.sqrt(max(11.0 / 3.0 - (5.0 / 3.0) ** 2, 0.0)), 1.0, 3.0]
    assert curves[0, FRICTION, T.QUANTITIES.index("falls")].tolist() == only(4, 1.0 - timed) and curves[0, FRICTION, 0].sum() == 3.0
    assert counts[0].tolist() == [[0.0, float(p in (FRICTION, MOTOR)), 0.0] for p in range(9)] and pair[0, 0].reshape(8, 8)[2, 4] == 2.0 and pair[0, 0].reshape(8, 8)[6, 2] == 1.0


def test_model_values_without_a_bin_outside_the_range_and_inactive():
    # a NaN friction: three launches unbinned, nothing else of those steps; the re-draw back to a number is seen
    st, did = play(T.config(HAND), dict(friction=NAN), [dict(friction=NAN, r=1.0), dict(friction=NAN, reset=1, r=1.0), dict(friction=2.0, r=1.0), dict(friction=2.0, r=1.0)])
    assert st.unbinned[:, 0].tolist() == [3, 0, 0, 0, 0, 0, 0, 0, 0] and per_bin(st.steps, FRICTION) == only(8) and per_bin(st.falls, FRICTION) == only(99, 0)
    assert per_bin(st.falls, MOTOR) == only(8) and st.nonfinite[FRICTION, 0] == 3 and st.count[FRICTION, 0] == 1 and st.redraws[FRICTION, 0] == 1
    assert [d["bin"][FRICTION, 0] for d in did] == [-1, -1, -1, 8] and per_bin(st.reward_sum, FRICTION) == only(8, 1.0)
    # an infinite payload has no bin either, and a NaN that stays a NaN with the same bits is no re-draw
    st, _ = play(T.config(HAND), dict(payload=INF), [dict(payload=INF)])
    assert st.unbinned[PAYLOAD, 0] == 1 and st.redraws[PAYLOAD, 0] == 0 and not st.steps[PAYLOAD].any()
    # values outside the range land in the end bins, and the value row shows them
    st, did = play(T.config(HAND), dict(friction=-2.0, payload=7.5, motor=2.0), [dict(friction=-2.0, payload=7.5, motor=2.0)] * 2)
    assert per_bin(st.steps, FRICTION) == only(0, 2) and per_bin(st.steps, PAYLOAD) == only(15, 2) and per_bin(st.steps, MOTOR) == only(15, 2)
    assert st.min[FRICTION, 0] == -2.0 and st.max[PAYLOAD, 0] == 7.5 and not st.unbinned.any()
    # the upper edge of a bin belongs to the next one
    st, _ = play(T.config(HAND), dict(friction=0.25), [dict(friction=0.25)])
    assert per_bin(st.steps, FRICTION) == only(1)
    # an inactive parameter touches nothing: not its accumulators, not its counters, not even its value in force
    st, _ = play(T.config(dict(friction=(0.0, 4.0))), dict(motor=1.0), [dict(motor=0.5, reset=1), dict(motor=0.25)])
    assert st.cur[MOTOR, 0] == 1.0 and st.cur[FRICTION, 0] == 1.0 and not st.count[1:].any() and not st.steps[1:].any() and not st.falls[1:].any() and not st.redraws.any()
    assert per_bin(st.falls, FRICTION) == only(4) and st.launches[0] == 2 and not st.pair_steps.any() and st.pair_cur.tolist() == [[0.0], [0.0]]


def test_model_a_nan_velocity_counts_in_bad_and_the_warm_up_is_honoured():
    steps = [dict(vel=(NAN, 0.0), r=0.5), dict(tau=INF, qd=1.0, r=0.5), dict(r=NAN, vel=(3.0, 4.0)), dict(r=INF, reset=1), dict(vel=(6.0, 8.0), r=0.5)]
    st, did = play(T.config(HAND, pair=("friction", "payload")), dict(), steps)
    assert st.bad[:, 0].tolist() == [4, 0, 4, 0, 0, 0, 4, 0, 0] and per_bin(st.steps, FRICTION) == only(4, 5) and per_bin(st.measured, FRICTION) == only(4, 2)
    assert per_bin(st.lin_err_sum, FRICTION) == only(4, 15.0) and per_bin(st.reward_sum, FRICTION) == only(4, 1.5) and per_bin(st.falls, FRICTION) == only(4)
    assert np.isfinite(st.lin_err_sum).all() and np.isfinite(st.power_sum).all() and np.isfinite(st.reward_sum).all()
    assert [bool(d["measured"][0]) for d in did] == [False, False, True, False, True] and st.pair_measured[:, 0].sum() == 2 and st.pair_steps[:, 0].sum() == 5
    # the warm-up: steps with episode_length_buf <= warmup_steps are exposure and reward, and enter no outcome; a fall counts all the same
    steps = [dict(age=1, vel=(3.0, 4.0), r=1.0), dict(age=2, vel=(3.0, 4.0), r=1.0), dict(age=3, vel=(3.0, 4.0), r=1.0), dict(age=0, reset=1, r=1.0)]
    st, _ = play(T.config(HAND, warmup_steps=2), dict(), steps)
    assert per_bin(st.steps, MOTOR) == only(8, 4) and per_bin(st.measured, MOTOR) == only(8) and per_bin(st.lin_err_sum, MOTOR) == only(8, 5.0)
    assert per_bin(st.reward_sum, MOTOR) == only(8, 4.0) and per_bin(st.falls, MOTOR) == only(8) and not st.bad.any()
    # a snapshot takes the values in force again and counts no re-draw
    st = T.clear(1, T.config(HAND, pair=("friction", "motor_strength")), params_of())
    T.snapshot(st, T.config(HAND, pair=("friction", "motor_strength")), params_of(motor=0.5))
    T.accumulate(st, T.config(HAND, pair=("friction", "motor_strength")), snap_of(motor=0.5))
    assert per_bin(st.steps, MOTOR) == only(4) and not st.redraws.any() and st.pair_steps[:, 0].tolist() == [1 if k == 8 * 2 + 2 else 0 for k in range(64)]


# ---- 4. hazard, Wilson interval, effect and ranking by hand ---------------------------------------------------------------------------------
def fixed_result(pair=True):
    """two cells, friction and payload active; cell 0 falls at low friction, cell 1 never falls"""
    from go1_gym_learn.eval_metrics import sweep
    curves = {q: np.zeros((2, 9, 16)) for q in T.QUANTITIES}
    for g in range(2):
        for p in (FRICTION, PAYLOAD):
            curves["steps"][g, p], curves["measured"][g, p] = 1000.0, 800.0
            curves["lin_err_sum"][g, p], curves["yaw_err_sum"][g, p], curves["power_sum"][g, p], curves["reward_sum"][g, p] = 80.0, 40.0, 8000.0, 10.0
    curves["falls"][0, FRICTION, :4] = [8.0, 4.0, 2.0, 2.0]
    curves["steps"][0, FRICTION, 15], curves["measured"][0, FRICTION, 15], curves["falls"][0, FRICTION, 15] = 100.0, 0.0, 5.0      # too little exposure for an effect
    curves["lin_err_sum"][0, PAYLOAD] = 100.0 + 100.0 * np.arange(16)                    # means of 0.125 + 0.125 k: exact
    active = np.array([p in (FRICTION, PAYLOAD) for p in range(9)])
    edges = np.full((9, 17), NAN)
    edges[FRICTION], edges[PAYLOAD] = np.linspace(0.04, 6.0, 17), np.linspace(-1.5, 4.0, 17)
    row = lambda lo, hi: np.array([[16000.0, 0.5 * (lo + hi), 1.0, lo, hi, 0.0]] * 2)
    value = {name: np.full((2, 6), NAN) for name in T.PARAMETERS}
    value["friction"], value["payload"] = row(0.05, 5.9), row(-1.4, 4.25)
    counts = np.zeros((2, 9, 3))
    counts[:, FRICTION], counts[:, PAYLOAD] = [0.0, 7.0, 1.0], [3.0, 7.0, 1.0]
    pair_map = np.zeros((2, 4, 8, 8))
    pair_map[:, 0], pair_map[0, 1, 0, 7] = 250.0, 5.0
    return dict(preset="rand_large", cells=sweep.grid_cells(dict(vx=[0.5, 1.0], yaw=[0.0], gait=[sweep.GAITS["trotting"]])), parameters=["friction", "payload"], active=active,
                edges=edges, ranges=dict(friction=(0.04, 6.0), payload=(-1.5, 4.0)), value=value, curves=curves, counts=counts, sens_groups=np.array([[32.0, 500.0]] * 2),
                pair=("friction", "payload") if pair else None, pair_map=pair_map if pair else None, min_exposure=200, metrics={}, groups=np.zeros((2, 5)), num_envs=64,
                steps=500, warmup_steps=25, seed=1, dt=0.02)


def test_hazard_wilson_effect_and_ranking_by_hand():
    from go1_gym_learn.eval_metrics import sensitivity as S
    h = S.hazard([2.0, 0.0, 3.0], [1000.0, 0.0, 1500.0])
    assert h[0] == 2.0 and np.isnan(h[1]) and h[2] == 2.0 and S.hazard(1.0, 200.0, per=100) == 0.5
    low, high = S.wilson([0.0, 5.0, 10.0, 0.0], [0.0, 10.0, 10.0, 100.0])
    z = 1.96
    assert np.isnan(low[0]) and np.isnan(high[0])
    assert abs(low[1] - (0.5 + z * z / 20 - z * np.sqrt(0.025 + z * z / 400)) / (1 + z * z / 10)) < 1e-15 and abs(low[1] + high[1] - 2 * (0.5 + z * z / 20) / (1 + z * z / 10)) < 1e-15
    assert abs(high[2] - 1.0) < 1e-12 and abs(low[2] - 10.0 / (10.0 + z * z)) < 1e-12 and abs(low[3]) < 1e-12 and abs(high[3] - z * z / (100.0 + z * z)) < 1e-12
    assert 0.2365 < low[1] < 0.2367 and 0.7633 < high[1] < 0.7635                                   # the textbook figures for 5 of 10: 0.2366, 0.7634
    curve, steps = np.array([1.0, 9.0, 4.0, NAN] + [2.0] * 12), np.array([500.0, 100.0, 200.0, 900.0] + [0.0] * 12)
    assert S.effect(curve, steps, 200) == 3.0 and S.effect(curve, steps, 100) == 8.0 and np.isnan(S.effect(curve, steps, 300)) and np.isnan(S.effect(curve, steps, 1000))
    res = fixed_result()
    assert S.reported(res) == [FRICTION, PAYLOAD]
    s = S.parameter_summary(res, 0, FRICTION)
    assert (s["hazard_low"], s["hazard_high"], s["exposure"]) == (16.0 / 4000.0 * 1000.0, 5.0 / 3100.0 * 1000.0, 15100.0)
    assert s["effect_hazard"] == 8.0 and s["effect_lin_vel_err"] == 0.0 and (s["lo"], s["hi"], s["realised_min"], s["realised_max"]) == (0.04, 6.0, 0.05, 5.9)
    assert (s["lin_vel_err_low"], s["power_low"], s["redraws"], s["unbinned"], s["bad"]) == (0.1, 10.0, 7.0, 0.0, 1.0)
    assert S.rank_parameters(res, 0) == [("friction", 8.0), ("payload", 0.0)]
    assert S.rank_parameters(res, 0, "effect_lin_vel_err") == [("payload", 1.875), ("friction", 0.0)]
    assert S.rank_parameters(res, 1) == [("friction", 0.0), ("payload", 0.0)]                            # a tie keeps the parameters' order
    res["min_exposure"] = 5000
    assert [name for name, _ in S.rank_parameters(res, 0)] == ["friction", "payload"] and all(np.isnan(x) for _, x in S.rank_parameters(res, 0))
    res = fixed_result()
    res["parameters"] = ["payload"]
    assert S.reported(res) == [PAYLOAD]
    assert S.MIN_EXPOSURE == 200 and "placeholder" in S.__doc__


# ---- 5. go1sens.hip under the SIMT emulator against the model ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1sens_host as G
    return G.load_library(build_emu(g.sens_sources(), "libgo1sens_emu.so"))


SHAPES_OF_INPUTS = dict(base_lin_vel=3, base_ang_vel=3, commands=T.SCRIPT_COMMANDS, torques=12, dof_vel=12, com_displacements=3, motor_strengths=12, Kp_factors=12,
                        Kd_factors=12)


def sens_on(device, N, lib=None):
    """a go1sens_host.Go1Sensitivity on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1sens_host as G
    tensors = {k: torch.zeros(rows, N, device=device) for k, rows in SHAPES_OF_INPUTS.items()}
    tensors.update({k: torch.zeros(N, device=device) for k in ("rew_buf", "friction_coeffs", "restitutions", "payloads")})
    tensors.update(reset_buf=torch.zeros(N, dtype=torch.uint8, device=device), time_out_buf=torch.zeros(N, dtype=torch.uint8, device=device),
                   episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    family = G.Go1Sensitivity(types.SimpleNamespace(num_envs=N), B, lib=lib)
    if torch.device(device).type == "cpu":
        family._stream = lambda: None
    return family, B


def sens_groups(rng, N, groups=3):
    """three groups of which group 1 is empty, some environments at -1 and (from three environments on) one id outside the tables"""
    assert groups == 3
    group = rng.integers(-1, groups, N).astype(np.int32)
    group[group == 1] = 2
    group[0] = groups - 1
    if N >= 3:
        group[1], group[2] = -1, groups
    return group


def upload(B, arrays):
    for k, a in arrays.items():
        getattr(B, k).copy_(torch.from_numpy(a))


def drive(family, B, cfg_, first, snaps, outside, group, groups):
    """the scripted steps through the library: the buffers at the clear, arm for `groups` groups, then per launch a snapshot of the
    input buffers uploaded and an accumulate, with a go1sens_snapshot on the `outside` buffers in front of the launches it names;
    returns read() and the accumulators.  arm() sizes the tables by the largest id it is given, so the ids outside the tables are
    handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    upload(B, first)
    family.arm(inside, cfg_.warmup_steps, ranges=cfg_.ranges, pair=cfg_.pair)
    family.group.copy_(torch.from_numpy(group))
    for k, s in enumerate(snaps):
        if k in outside:
            upload(B, outside[k])
            family.snapshot()
        upload(B, s)
        family.accumulate()
    family.disarm()
    res = family.read()
    acc = {k: t.cpu().numpy() for k, t in family.acc.items()}
    return res, acc


def canon(a):
    """`a` with every NaN of a floating-point array replaced by one NaN (a table's NaN for an empty row has no fixed sign)"""
    a = np.array(a)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


def same(a, b):
    return np.shape(a) == np.shape(b) and bits(canon(a)) == bits(canon(b))


def same_as_the_model(res, acc, st, cfg_, group, groups):
    """accumulators, state and the four result tables against the model's state `st`, bit for bit"""
    N = st.N
    for k in ACCUMULATORS:
        assert acc[k].shape == (T.P, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in T.STATE:
        want = getattr(st, k)
        assert res["env_" + k].shape == want.shape and bits(res["env_" + k].view(want.dtype)) == bits(want), k
    table, curves, counts, pair = T.reduce(st, group, groups)
    got = np.stack([res["value"][name] for name in T.PARAMETERS], axis=1)
    assert got.shape == (groups, T.P, 6) and np.array_equal(np.isnan(got), np.isnan(table[:, :T.P])) and same(got, table[:, :T.P])
    assert res["groups"].shape == (groups, 2) and bits(res["groups"]) == bits(table[:, T.P, :2]) and not table[:, T.P, 2:].any()
    for k, q in enumerate(T.QUANTITIES):
        assert res["curves"][q].shape == (groups, T.P, 16) and bits(res["curves"][q]) == bits(curves[:, :, k]), q
    assert res["counts"].shape == (groups, T.P, 3) and bits(res["counts"]) == bits(counts)
    if cfg_.pair:
        assert res["pair"] == tuple(cfg_.pair) and res["pair_map"].shape == (groups, 4, 8, 8) and bits(res["pair_map"]) == bits(pair.reshape(groups, 4, 8, 8))
    else:
        assert res["pair"] is None and res["pair_map"] is None and not pair.any()
    assert res["parameters"] == T.PARAMETERS and res["active"].tolist() == cfg_.active.tolist() and res["edges"].shape == (9, 17)
    for p, name in enumerate(T.PARAMETERS):
        if name in cfg_.ranges:
            lo, hi = cfg_.ranges[name]
            assert res["edges"][p, 0] == lo and res["edges"][p, 16] == hi and np.allclose(np.diff(res["edges"][p]), (hi - lo) / 16, rtol=1e-12, atol=0)
        else:
            assert np.isnan(res["edges"][p]).all()
    return table, curves, counts, pair


def check_against_the_model(res, acc, cfg_, first, snaps, outside, kind, group, groups, N):
    """the library's results against tests/sens_ref.py, bit for bit; then that the script drove every event it was written to drive"""
    st, did = T.run(cfg_, first, snaps, N, outside)
    table, curves, counts, pair = same_as_the_model(res, acc, st, cfg_, group, groups)
    steps = len(snaps)
    active = np.nonzero(cfg_.active)[0]
    assert (st.launches == steps).all() and active.tolist() == [0, 1, 2, 3, 5, 6, 8]
    total = lambda words: words.astype(np.int64).sum(axis=1)                               # over the bins: (9, N)
    assert (total(st.steps)[active] + st.unbinned[active] == steps).all() and (total(st.measured) <= total(st.steps)).all()
    for sums in (st.reward_sum, st.lin_err_sum, st.yaw_err_sum, st.power_sum, st.pair_lin_err_sum, st.sum, st.sumsq):
        assert np.isfinite(sums).all()
    for idle in (COM_Y, 7):                                                               # inactive: nothing touched, not even the value in force
        assert not st.count[idle].any() and not st.steps[idle].any() and not st.redraws[idle].any() and not st.unbinned[idle].any() and not st.bad[idle].any()
        assert bits(st.cur[idle]) == bits(T.now(outside[T.SCRIPT_SNAPSHOT], idle))   # (the clear and the snapshot take all nine)
    if N >= len(T.KINDS):
        steady, redrawn, falls, times_out, odd_value, outside_, odd_velocity, random_ = (kind == k for k in range(len(T.KINDS)))
        # the fall of launch 4 belongs to the bins of the values carried into it; the buffers of that launch hold other values
        assert did[4]["fall"][redrawn].all() and did[4]["redrawn"][np.ix_(active, redrawn)].all()
        old = did[4]["bin"][:, redrawn]
        new = np.stack([T.bin_of(T.now(snaps[4], p), cfg_.lo[p], cfg_.scale[p]) for p in range(T.P)])[:, redrawn]
        assert (old[active] != new[active]).any() and (total(st.falls)[np.ix_(active, redrawn)] == 1).all()
        for p in active:
            e = np.nonzero(redrawn)[0]
            assert (st.falls[p, old[p], e] == 1).all()
        assert (total(st.falls)[np.ix_(active, falls)] == 2).all() and (st.redraws[MOTOR, falls] == 2).all() and (st.redraws[FRICTION, falls] == 0).all()
        # a time-out is not a fall
        assert did[6]["timeout"][times_out].all() and not total(st.falls)[:, times_out].any() and (total(st.timeouts)[np.ix_(active, times_out)] == 1).all()
        # a value that is not finite has no bin: launches 2, 3 and 4 carry it
        assert (st.unbinned[FRICTION, odd_value] == 3).all() and (st.unbinned[PAYLOAD, odd_value] == 3).all() and (st.nonfinite[FRICTION, odd_value] == 3).all()
        assert st.unbinned.sum() == 6 * odd_value.sum() and (st.redraws[FRICTION, odd_value] == 2).all()
        # values outside the range: the end bins, for every launch
        assert (st.steps[FRICTION, 0, outside_] == steps).all() and (st.steps[PAYLOAD, 15, outside_] == steps).all() and (st.steps[3, 15, outside_] == steps).all()
        assert (st.min[FRICTION, outside_] == f32(-0.5)).all() and (st.max[PAYLOAD, outside_] == f32(7.0)).all()
        # a NaN velocity, a NaN torque, an infinite and a NaN reward: four in bad, and in no sum
        assert (st.bad[np.ix_(active, odd_velocity)] == 4).all() and st.bad.sum() == 4 * len(active) * odd_velocity.sum()
        assert (total(st.measured)[np.ix_(active, odd_velocity)] == total(st.measured)[np.ix_(active, steady)].max() - 2).all() or N > 8
        # a change from outside followed by a snapshot is no re-draw
        assert not st.redraws[:, steady].any() and (st.cur[MOTOR, steady] != first["motor_strengths"][0, steady]).all() and (st.cur[FRICTION, steady] == first["friction_coeffs"][steady]).all()
        assert st.falls.sum() > 0 and st.timeouts.sum() > 0 and st.redraws[:, random_].sum() > 0
        if cfg_.pair:
            assert (st.pair_steps.astype(np.int64).sum(axis=0) + np.maximum(st.unbinned[FRICTION], st.unbinned[MOTOR]) == steps).all()
            assert (st.pair_falls.astype(np.int64).sum(axis=0)[~odd_value] == total(st.falls)[FRICTION, ~odd_value]).all()
    assert res["groups"][:, 0].sum() == np.isin(group, range(groups)).sum() and (res["groups"][:, 1] == steps * res["groups"][:, 0]).all() and res["groups"][1].tolist() == [0.0, 0.0]
    assert np.isnan(table[1, :T.P, 1:5]).all() and not curves[1].any() and not counts[1].any()
    return st


# (N, with a pair).  1: one thread per row; 64: one wavefront; 257: a workgroup plus one lane per row; 600: three ragged workgroups per
# row, three terms per reduction thread and 38 environments per bin slice
SCRIPTS = [(1, True), (64, False), (257, True), (600, True)]


@pytest.mark.parametrize("N,pair", SCRIPTS)
def test_emulated_sensitivity_kernels_follow_the_model(emu, N, pair):
    groups = 3
    rng = np.random.default_rng(1300 + N)
    cfg_, first, snaps, outside, kind = T.scripted_steps(rng, N, pair=pair)
    assert len(snaps) == T.SCRIPT_STEPS == 12 and list(outside) == [T.SCRIPT_SNAPSHOT] and cfg_.warmup_steps == 2
    assert N < len(T.KINDS) or set(kind.tolist()) == set(range(len(T.KINDS)))
    group = sens_groups(rng, N, groups)
    family, B = sens_on("cpu", N, lib=emu)
    res, acc = drive(family, B, cfg_, first, snaps, outside, group, groups)
    c = family.cfg
    assert c.num_groups == groups and (N < 3 or {-1, groups} <= set(group.tolist())) and (c.pair_a, c.pair_b) == ((0, 6) if pair else (-1, -1))
    assert list(c.active) == cfg_.active.astype(int).tolist() and bits(np.array(list(c.lo), f32)) == bits(cfg_.lo) and bits(np.array(list(c.scale), f32)) == bits(cfg_.scale)
    check_against_the_model(res, acc, cfg_, first, snaps, outside, kind, group, groups, N)
    again = family.read()                                                    # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ["groups", "counts"] + ["env_" + k for k in T.STATE])
    assert all(bits(again["curves"][q]) == bits(res["curves"][q]) for q in T.QUANTITIES) and all(same(again["value"][m], res["value"][m]) for m in T.PARAMETERS)
    for bad in (dict(ranges=dict(grip=(0.0, 1.0))), dict(ranges=dict(friction=(0.0, NAN))), dict(ranges=dict(friction=(INF, 0.0))), dict(ranges=dict(friction=(1.0, 1.0))),
                dict(ranges=dict(friction=(2.0, 1.0))), dict(ranges=dict(friction=(0.0, 1.0)), pair=("friction", "payload")),
                dict(ranges=dict(friction=(0.0, 1.0), payload=(0.0, 1.0)), pair=("friction", "friction")), dict(ranges=dict(friction=(0.0, 1.0)), pair=("friction",))):
        with pytest.raises(ValueError, match="sensitivity:"):
            family.arm(np.zeros(N, np.int32), **bad)
    with pytest.raises(RuntimeError, match="go1sens_accumulate failed: -12"):
        family.cfg.scale[0] = 0.0
        family.accumulate()


# ---- 6. the environment hooks without a GPU -----------------------------------------------------------------------------------------------------
def plane_env(monkeypatch, num_envs=16):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    for module in ("go1eval_host", "go1sens_host"):
        monkeypatch.delitem(sys.modules, module, raising=False)
    c = apply_train_config(make_cfg(), num_envs=num_envs)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    return VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)


def test_sensitivity_hooks_on_cpu_buffers(monkeypatch):
    from go1_gym.envs.base.legged_robot import LeggedRobot
    from test_family_wiring import FAMILIES, REWARD, STATE_FAMILIES, Stub
    import test_family_wiring as wiring
    # stubs for the families up to the reward family only: the later ones stay None unless this test puts its own stub there, so the
    # launch-order and refusal checks below name exactly the families they set
    STEPPED = wiring.STEPPED[:REWARD + 1]
    put_stubs = functools.partial(wiring.put_stubs, stepped=STEPPED)
    env = plane_env(monkeypatch)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_sensitivity_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_sensitivity_metrics, env.read_sensitivity_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert all(m not in sys.modules for m in ("go1eval_host", "go1sens_host")) and env._sens is None              # never measured: no host module
    env.step(torch.zeros(16, 12))                                             # and stepping goes on
    signature = inspect.signature(env.start_sensitivity_metrics)
    assert {k: p.default for k, p in signature.parameters.items() if k != "groups"} == dict(warmup_steps=0, ranges=None, pair=None)
    assert list(signature.parameters) == ["groups", "warmup_steps", "ranges", "pair"]
    for name in ("start_sensitivity_metrics", "stop_sensitivity_metrics", "read_sensitivity_metrics"):
        assert (getattr(LeggedRobot, name).__doc__ or "").strip(), name
    # its row of the one table, directly after the episode family's
    k = [row[0] for row in env._FAMILIES].index("sensitivity")
    assert env._FAMILIES == FAMILIES and env._FAMILIES[k] == ("sensitivity", "_sens", "go1sens_host", "Go1Sensitivity", "accumulate") and env._FAMILIES[k - 1][0] == "episodes"
    assert env._STATE_FAMILIES == STATE_FAMILIES and env._STATE_FAMILIES[k] == ("sensitivity", "_sens") and env._STEPPED[k - 2:k] == (("_episodes", "accumulate"), ("_sens", "accumulate"))
    assert env._HOST["_sens"] == ("go1sens_host", "Go1Sensitivity") and all(len(row) == 5 for row in env._FAMILIES)
    # launched last, after the episode family's
    log = []

    class SensStub(Stub):
        def snapshot(self, *args):
            self.log.append((self.attr, "snapshot", args))
    put_stubs(env, log)
    env._episodes, env._sens = Stub("_episodes", log), SensStub("_sens", log)
    env.step(torch.zeros(16, 12))
    assert [(attr, method) for attr, method, _ in log] == STEPPED + [("_episodes", "accumulate"), ("_sens", "accumulate")] and log[-1][2] == ()
    env._sens.armed = False
    del log[:]
    env.step(torch.zeros(16, 12))
    assert [(attr, method) for attr, method, _ in log] == STEPPED + [("_episodes", "accumulate")]
    # a reset from outside re-draws the motor parameters: an armed family takes the values in force again, a stopped one does not
    env._reward = None
    del log[:]
    env.reset_idx(torch.tensor([1, 3]))
    assert log == []
    env._sens.armed = True
    env.reset_idx(torch.tensor([1, 3]))
    env.reset_idx(torch.tensor([], dtype=torch.int64))
    assert log == [("_sens", "snapshot", ())]
    # load_state() names it after the episode family and before the camera
    put_stubs(env, log)
    env._state = types.SimpleNamespace(restore=lambda *a, **k: pytest.fail("restored"))
    env._render = types.SimpleNamespace(any_armed=True)
    with pytest.raises(RuntimeError) as e:
        env.load_state(None)
    assert "refused while metrics, behaviour, trace, terrain, joints, feet, trunk, gait, spectrum, placement, rewards, episodes, sensitivity, camera are armed" in str(e.value)
    env._render = None
    put_stubs(env, [], armed=False)
    env._episodes.armed = False
    with pytest.raises(RuntimeError, match=r"refused while sensitivity is armed: stop it first"):
        env.load_state(None)


def test_default_ranges_come_from_the_configuration():
    import go1sens_host as G
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym_learn.eval_metrics.domain_randomization import DR_SETTINGS
    c = make_cfg()
    DR_SETTINGS["rand_large"](c)
    want = dict(friction=(0.04, 6.0), restitution=(0.0, 1.0), payload=(-1.5, 4.0), com_x=(-0.13, 0.13), com_y=(-0.13, 0.13), com_z=(-0.13, 0.13), motor_strength=(0.88, 1.12))
    assert G.default_ranges(c.domain_rand) == want and list(G.default_ranges(c.domain_rand)) == G.PARAMETERS[:7]
    family = types.SimpleNamespace()
    ranges_of = lambda *a: G.Go1Sensitivity.ranges_of(family, *a)
    assert ranges_of(c.domain_rand) == want
    assert ranges_of(c.domain_rand, {"Kp_factor": (0.8, 1.3)}) == dict(want, Kp_factor=(0.8, 1.3))          # a parameter whose switch is off, named
    assert ranges_of(c.domain_rand, {"Kd_factor": None, "friction": (0.0, 1.0)}) == dict(want, friction=(0.0, 1.0), Kd_factor=(0.5, 1.5))
    assert list(ranges_of(c.domain_rand, {"Kd_factor": None, "Kp_factor": None})) == G.PARAMETERS
    DR_SETTINGS["static_low"](c)
    assert G.default_ranges(c.domain_rand)["motor_strength"] == (-0.99, 0.9) and G.default_ranges(c.domain_rand)["payload"] == (-1.0, -0.99)
    c.domain_rand.randomize_friction, c.domain_rand.restitution_range = False, [0.5, 0.5]
    assert "friction" not in G.default_ranges(c.domain_rand) and "restitution" not in G.default_ranges(c.domain_rand)          # off, and a range of no width
    for bad in ({"grip": (0.0, 1.0)}, {"friction": (0.0, INF)}, {"friction": (NAN, 1.0)}, {"friction": (1.0, 1.0)}, {"friction": (2.0, 1.0)}, {"grip": None}):
        with pytest.raises(ValueError, match="sensitivity:"):
            ranges_of(c.domain_rand, bad)
    edges = G.bin_edges(dict(friction=(0.0, 4.0)))
    assert edges.shape == (9, 17) and edges[0].tolist() == [0.25 * k for k in range(17)] and np.isnan(edges[1:]).all()


# ---- 7. the tool and the sweep's host pieces --------------------------------------------------------------------------------------------------
def test_sensitivity_table_json_and_figure(tmp_path):
    from go1_gym_learn.eval_metrics import sensitivity as S
    res = fixed_result()
    md = S.sensitivity_markdown_table(res).splitlines()
    assert md[0].startswith("| vx | yaw | gait | parameter | range | realised min / max | exposure | hazard low / high [1/1000 steps] | lin vel err low / high | power low / high [W] |")
    assert md[0].endswith("| effect on hazard | effect on lin vel err | re-draws | unbinned |") and md[0].count("|") == 15
    assert len(md) == 2 + 4 + 2 + 2 and len({line.count("|") for line in md[:6]}) == 1
    assert md[2] == "| 0.5 | 0 | 0.5/0/0 | friction | 0.04 .. 6 | 0.05 / 5.9 | 15100 | 4 / 1.61 | 0.1 / 0.133 | 10 / 13.3 | 8 | 0 | 7 | 0 |"          # (the last bin measured nothing: 320 / 2400)
    assert md[3].startswith("| 0.5 | 0 | 0.5/0/0 | payload | -1.5 .. 4 | -1.4 / 4.25 | 16000 | 0 / 0 |") and md[3].endswith("| 0 / 0 | 0.312 / 1.81 | 10 / 10 | 0 | 1.88 | 7 | 3 |")
    assert md[6] == "" and "at least 200 steps (a placeholder)" in md[7] and "marginal" in md[7]
    assert md[8] == "- vx 0.5, yaw 0, gait 0.5/0/0: by effect on the hazard: friction (8), payload (0); on lin vel err: payload (1.88), friction (0)"
    js = json.loads(json.dumps(S.sensitivity_to_json(res), allow_nan=False))
    assert js["parameters"] == T.PARAMETERS and js["reported"] == ["friction", "payload"] and js["active"] == [True, False, True] + [False] * 6 and js["quantities"] == T.QUANTITIES
    assert js["edges"][1][0] is None and js["edges"][0][16] == 6.0 and js["value"]["com_x"][0][1] is None and js["value"]["friction"][1][3] == 0.05
    assert np.array(js["curves"]["falls"]).shape == (2, 9, 16) and js["curves"]["falls"][0][0][:4] == [8.0, 4.0, 2.0, 2.0] and np.array(js["counts"]).shape == (2, 9, 3)
    assert js["summary"][0][0]["effect_hazard"] == 8.0 and js["summary"][1][1]["parameter"] == "payload" and js["ranking"][0] == [["friction", 8.0], ["payload", 0.0]]
    assert js["pair"] == ["friction", "payload"] and np.array(js["pair_map"]).shape == (2, 4, 8, 8) and js["min_exposure"] == 200 and js["cells"][1]["vx"] == 1.0
    path = tmp_path / "sensitivity.png"
    S.plot_sensitivity(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000
    single = fixed_result(pair=False)
    js = json.loads(json.dumps(S.sensitivity_to_json(single), allow_nan=False))
    assert js["pair"] is None and js["pair_map"] is None
    S.plot_sensitivity(single, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


def test_tool_accepts_a_sensitivity_sweep(tmp_path, monkeypatch, capsys):
    from test_family_wiring import MODES
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sensitivity, sweep
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--sensitivity", "--vx", "0.5", "1.0", "--envs", "64", "--steps", "40", "--warmup-steps", "5", "--presets", "rand_large",
                                      "--parameters", "friction", "payload", "--pair", "friction", "payload", "--min-exposure", "50"])
    assert a.sensitivity and not a.episodes and (a.vx, a.envs, a.steps, a.parameters, a.pair, a.min_exposure) == ([0.5, 1.0], 64, 40, ["friction", "payload"], ["friction", "payload"], 50)
    plain = eval_sweep.parse_args(base + ["--sensitivity"])
    assert (plain.parameters, plain.pair, plain.min_exposure) == (None, None, 200) and plain.sensitivity
    nothing = eval_sweep.parse_args(base)
    assert not nothing.sensitivity and nothing.parameters is None and nothing.pair is None and nothing.min_exposure is None
    assert eval_sweep.parse_args(base + ["--sensitivity", "--terrain", "plane"]).terrain == "plane"
    assert eval_sweep.parse_args(base + ["--sensitivity", "--parameters", "Kp_factor"]).parameters == ["Kp_factor"]
    for other in list(MODES.values()) + [["--episodes"]]:                    # every other mode excludes it, whichever comes first
        for argv in (["--sensitivity"] + other, other + ["--sensitivity"]):
            with pytest.raises(SystemExit) as e:
                eval_sweep.parse_args(base + argv)
            assert e.value.code == 2, argv
    for bad in (["--parameters", "friction"], ["--pair", "friction", "payload"], ["--min-exposure", "50"], ["--trunk", "--min-exposure", "50"], ["--episodes", "--parameters", "friction"],
                ["--joints", "--pair", "friction", "payload"], ["--sensitivity", "--parameters", "grip"], ["--sensitivity", "--pair", "friction", "grip"],
                ["--sensitivity", "--pair", "friction"], ["--sensitivity", "--pair", "friction", "friction"], ["--sensitivity", "--min-exposure", "0"],
                ["--sensitivity", "--min-exposure", "-3"], ["--sensitivity", "--gamma", "0.9"], ["--sensitivity", "--map-cell", "0.05"]):
        with pytest.raises(SystemExit) as e:
            eval_sweep.parse_args(base + bad)
        assert e.value.code == 2, bad
    assert callable(eval_sweep.run_sensitivity) and len(inspect.signature(eval_sweep.run_sensitivity).parameters) == 3
    assert "--sensitivity --presets rand_large" in eval_sweep.__doc__ and "a placeholder" in eval_sweep.__doc__
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(sensitivity, "run_sensitivity_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    grid = dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits])
    eval_sweep.run_sensitivity(a, None, grid)
    assert seen == dict(preset="rand_large", grid=grid, num_envs=64, steps=40, warmup_steps=5, seed=1, terrain=None, parameters=["friction", "payload"],
                        pair=["friction", "payload"], min_exposure=50)
    js = json.load(open(tmp_path / "eval" / "rand_large_sensitivity.json"))
    assert js["preset"] == "rand_large" and js["summary"][0][0]["exposure"] == 15100.0
    md = (tmp_path / "eval" / "rand_large_sensitivity.md").read_text()
    assert "| friction | 0.04 .. 6 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "rand_large_sensitivity.png").read_bytes()[:4] == b"\x89PNG"


def test_the_sweep_runs_beside_the_scalar_table(monkeypatch):
    """a recording environment as tests/test_family_wiring.py's: the shared call sequence, the start's keywords and the result's keys"""
    from go1_gym_learn.eval_metrics import sensitivity, sweep
    from test_family_wiring import COMMON_KEYS, N, NUM_COMMANDS, STEPS, WARMUP, RecordingEnv, ZeroPolicy
    cells_in = dict(vx=[0.5, 1.0], yaw=[0.0, 0.5], gait=[sweep.GAITS["trotting"]])
    cells = sweep.grid_cells(cells_in)
    family = dict(parameters=T.PARAMETERS, active=np.array([True, False, True] + [False] * 6), edges=np.zeros((9, 17)), ranges=dict(friction=(0.0, 1.0), payload=(0.0, 1.0)),
                  value={"friction": np.zeros((4, 6))}, curves={"steps": np.zeros((4, 9, 16))}, counts=np.zeros((4, 9, 3)), groups=np.ones((4, 2)), pair=("friction", "payload"),
                  pair_map=np.zeros((4, 4, 8, 8)))

    class Env(RecordingEnv):
        def __init__(self, spoil=False):
            super().__init__("gait", 4, spoil)               # (any stem the recording base knows: the family below replaces what it cans)
            self.env.family = family
    built_env = Env()
    monkeypatch.setattr(sweep, "build_eval_env", lambda preset, num_envs, seed, terrain=None, configure=None: (built_env, None))
    res = sensitivity.run_sensitivity_sweep(ZeroPolicy(), "rand_large", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5, terrain="plane",
                                            parameters=["payload"], pair=["friction", "payload"], min_exposure=7)
    log = built_env.env.log
    assert [entry[0] for entry in log] == ["start_metrics", "start_sensitivity_metrics", "step", "step", "step", "stop_metrics", "stop_sensitivity_metrics", "read_metrics",
                                           "read_sensitivity_metrics"]
    assert log[1][1][0] is log[0][1][0] and log[1][2] == dict(warmup_steps=WARMUP, ranges=dict(payload=None, friction=None), pair=("friction", "payload"))
    assert torch.equal(built_env.first, sweep.command_table(cells, NUM_COMMANDS, "cpu")[(torch.arange(N) % 4).long()])
    own = ["parameters", "active", "edges", "ranges", "value", "curves", "counts", "sens_groups", "pair", "pair_map", "min_exposure"]
    assert sorted(res) == sorted(COMMON_KEYS + own) and res["parameters"] == ["payload"] and res["min_exposure"] == 7 and res["sens_groups"] is family["groups"]
    assert all(res[k] is family[k] for k in ("active", "edges", "value", "curves", "counts", "pair_map")) and (res["preset"], res["cells"], res["dt"]) == ("rand_large", cells, 0.02)
    built_env = Env()
    res = sensitivity.run_sensitivity_sweep(ZeroPolicy(), "rand_large", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5)
    assert built_env.env.log[1][2] == dict(warmup_steps=WARMUP, ranges=None, pair=None) and res["parameters"] == ["friction", "payload"] and res["min_exposure"] == 200
    for bad in (dict(parameters=["grip"]), dict(pair=["friction", "grip"]), dict(min_exposure=0)):
        with pytest.raises(ValueError, match="run_sensitivity_sweep:"):
            sensitivity.run_sensitivity_sweep(ZeroPolicy(), "rand_large", cells_in, num_envs=N, steps=STEPS, **bad)
    built_env = Env(spoil=True)
    with pytest.raises(RuntimeError) as e:
        sensitivity.run_sensitivity_sweep(ZeroPolicy(), "rand_large", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5)
    assert str(e.value) == "run_sensitivity_sweep: an environment left its grid cell's commands during the rollout"


# ---- 8. the scenario of the GPU test, through the fp64 oracle here -------------------------------------------------------------------------------
# N = 64 on the plane, episodes of 1 s, every one of the seven randomisations on, the rigid-body parameters re-drawn after the start, all of
# them every 0.2 s (ten steps); the scalar table and the family armed after reset(), then 120 steps of 2.0 * randn actions from a seeded
# generator on the environment's device, three groups, a warm-up of 5, a pair of friction and motor strength, and before step 60 a
# reset_idx of four environments (a reset from outside: the family takes the values in force again).
ROLL_N, ROLL_STEPS, ROLL_WARMUP, ROLL_GROUPS, ROLL_SEED, ROLL_CUT_STEP, ROLL_CUTS = 64, 120, 5, 3, 11, 60, 4
ROLL_PAIR = ("friction", "motor_strength")
ROLL_SWITCHES = ("randomize_friction", "randomize_restitution", "randomize_base_mass", "randomize_com_displacement", "randomize_motor_strength", "randomize_Kp_factor",
                 "randomize_Kd_factor")


def make_env(N, seed=4, device="cuda:0"):
    """the recipe of tests/test_gpu_response_trace.py::make_env on the plane, with the randomisations of the scenario"""
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    c = apply_train_config(make_cfg(), num_envs=N)
    c.terrain.mesh_type = "plane"
    c.env.episode_length_s = 1.0
    dr = c.domain_rand
    for switch in ROLL_SWITCHES:
        setattr(dr, switch, True)
    dr.randomize_rigids_after_start, dr.rand_interval_s = True, 0.2
    torch.manual_seed(seed)
    np.random.seed(seed)
    return VelocityTrackingEasyEnv(sim_device=device, headless=True, cfg=c)


def snapshot(env):
    """host copies of the buffers go1sens_accumulate reads, as they stand now"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in T.INPUTS}


def rollout_steps(envs):
    """the scenario on `envs` (the same actions and the same outside resets for each): yields ("reset", -1) after their reset(),
    ("outside", k) after the reset_idx in front of step k, and ("step", k) after step k"""
    device = envs[0].device
    g = torch.Generator(device=device).manual_seed(ROLL_SEED)
    for e in envs:
        e.reset()
    yield "reset", -1
    for k in range(ROLL_STEPS):
        if k == ROLL_CUT_STEP:
            running = torch.nonzero(envs[0].reset_buf == 0).reshape(-1)[:ROLL_CUTS]      # (a host read, once: not part of a measurement loop)
            assert running.numel() == ROLL_CUTS
            for e in envs:
                e.reset_idx(running.clone())
            yield "outside", k
        action = 2.0 * torch.randn(ROLL_N, 12, device=device, generator=g)
        for e in envs:
            e.step(action)
        yield "step", k


def rollout_config(env):
    import go1sens_host as G
    ranges = G.default_ranges(env.cfg.domain_rand)
    assert list(ranges) == T.PARAMETERS                                       # all nine are active
    return T.config(ranges, warmup_steps=ROLL_WARMUP, pair=ROLL_PAIR)


def replay(cfg_, events):
    """the model on the recorded events [(what, buffers)]: a clear on the first, a snapshot per outside reset, a launch per step.
    Returns (state, what every launch did, the buffers of every launch)"""
    (what, first), rest = events[0], events[1:]
    assert what == "reset"
    st, did, snaps = T.clear(ROLL_N, cfg_, first), [], []
    for what, s in rest:
        if what == "outside":
            T.snapshot(st, cfg_, s)
        else:
            did.append(T.accumulate(st, cfg_, s))
            snaps.append(s)
    return st, did, snaps


def assert_rollout_events(cfg_, st, did, snaps, label):
    """the conditions of the comparison, not measurements: at least one fall; at least one fall charged to a bin other than the bin of
    the value the buffer holds after that step; at least 64 re-draws"""
    falls = int(st.falls[0].sum())
    elsewhere = 0
    for d, s in zip(did, snaps):
        for p in range(T.P):
            after = T.bin_of(T.now(s, p), cfg_.lo[p], cfg_.scale[p])
            elsewhere += int((d["fall"] & (d["bin"][p] >= 0) & (d["bin"][p] != after)).sum())
    print(f"\n{label}: falls {falls}, time-outs {int(st.timeouts[0].sum())}, falls charged to another bin than the buffer's (over the nine parameters) {elsewhere}, "
          f"re-draws {int(st.redraws.sum())} (friction {int(st.redraws[0].sum())}, motor strength {int(st.redraws[6].sum())}), unbinned {int(st.unbinned.sum())}")
    assert falls >= 1 and elsewhere >= 1 and st.redraws.sum() >= 64 and st.redraws[0].sum() >= 64 and st.timeouts[0].sum() >= 1
    return falls


def test_the_rollout_script_produces_events_on_the_oracle(monkeypatch, emu):
    """the scenario of test_gpu_sensitivity_metrics.test_sensitivity_through_the_environment on the CPU oracle, the model replayed on the
    buffers after every step: falls, falls charged to a bin the buffers no longer show, time-outs and re-draws all occur.  The emulated
    kernels are stepped by the environment itself (the family object put where start_sensitivity_metrics would put it), its reset_idx
    snapshot included, and end bit-equal to the model."""
    import fake_sim
    import go1sens_host as G
    fake_sim.install(monkeypatch)
    env = make_env(ROLL_N)
    cfg_ = rollout_config(env)
    assert env.sim_config.randomize_rigids_after_start == 1 and env.sim_config.rand_interval == int(np.ceil(0.2 / env.dt))
    group = (torch.arange(ROLL_N) % ROLL_GROUPS).to(torch.int32)
    events = []
    for what, k in rollout_steps([env]):
        events.append((what, snapshot(env)))
        if what == "reset":                                                   # what start_sensitivity_metrics does where there is a GPU
            env._sens = G.Go1Sensitivity(env.sim_config, env.buffers, lib=emu)
            env._sens._stream = lambda: None
            env._sens.arm(group, ROLL_WARMUP, ranges=env._sens.ranges_of(env.cfg.domain_rand), pair=ROLL_PAIR)
    env._sens.disarm()
    st, did, snaps = replay(cfg_, events)
    assert len(did) == ROLL_STEPS and [what for what, _ in events].count("outside") == 1
    assert_rollout_events(cfg_, st, did, snaps, "oracle")
    res = env._sens.read()
    same_as_the_model(res, {k: t.numpy() for k, t in env._sens.acc.items()}, st, cfg_, group.numpy(), ROLL_GROUPS)
    total = lambda q: res["curves"][q].sum(axis=(0, 2))
    assert (total("steps") + res["counts"][:, :, 0].sum(axis=0) == ROLL_N * ROLL_STEPS).all() and (total("falls") == total("falls")[0]).all()
