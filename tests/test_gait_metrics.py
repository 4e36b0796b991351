"""CPU checks of the gait family (include/go1gait.h, libgo1gait.so): the ctypes mirrors and the exported symbols against the header, the
build's source list (as the compiler reads it), flags and stamp, the refusals without a GPU, the model of tests/gait_ref.py on
hand-scripted gaits with known answers, go1gait.hip itself under the SIMT emulator against that model bit for bit (accumulators, state,
histograms and both result tables), the environment hooks where there is no GPU, the scenario of the GPU test through the fp64 oracle,
and the sweep's host pieces."""
import ctypes
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

import gait_ref as T
from test_eval_return_codes import Call, cfg, each, nobody, null
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from util import build_emu

HEADER = os.path.join(REPO, "include", "go1gait.h")
SOURCE = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1gait.hip")
TABLES = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1_tables.h")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]


# ---- 1. mirrors, symbols, sources, stamp ---------------------------------------------------------------------------------------------------
def test_gait_mirrors_match_the_header():
    import go1gait_host as G
    src = open(HEADER).read()
    for macro, value in (("GO1GAIT_NUM", G.NUM_GAIT_METRICS), ("GO1GAIT_BINS", G.BINS), ("GO1GAIT_NUM_HISTS", G.NUM_HISTS), ("GO1GAIT_NUM_FIELDS", 6),
                         ("GO1GAIT_REDUCE_THREADS", 256), ("GO1GAIT_CONTACT_FORCE", G.CONTACT_FORCE)):
        assert re.search(rf"#define {macro} {value}\n", src), macro
    assert (G.NUM_GAIT_METRICS, G.BINS, G.NUM_HISTS) == (15, 16, 4) == (T.M, T.BINS, T.HISTS)
    want = struct_fields(src, "Go1GaitConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1GaitConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "min_stride_steps", "max_stride_steps"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1GaitConfig._fields_):
        assert ctype is C_TYPES[ctext], field
    assert ctypes.sizeof(G.Go1GaitConfig) == 20
    want = struct_fields(src, "Go1GaitBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1GaitBuffers._fields_] == T.INPUTS + ACCUMULATORS + T.STATE + ["group", "results", "hist_results"]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1GaitBuffers._fields_)
    types_ = dict(want)
    assert types_["prev_contact"] == "uint8_t*" and types_["ref_steps"] == types_["last_td"] == types_["td_count"] == "int32_t*"
    assert types_["hist_results"] == types_["results"] == "double*" and types_["support_hist"] == types_["phase_hist"] == types_["strides"] == "uint32_t*"
    assert G._GAIT_INPUTS == T.INPUTS and G._GAIT_STATE == T.STATE == list(G.Go1Gait.STATE)
    assert enum_order(src, "Go1GaitMetric", "GO1GAIT_") == [m.lower() for m in G.GAIT_NAMES] and G.GAIT_NAMES == T.METRICS and len(T.METRICS) == 15
    assert G.GAIT_NAMES[:6] == ["sync_FL_FR", "sync_FL_RL", "sync_FL_RR", "sync_FR_RL", "sync_FR_RR", "sync_RL_RR"] and G.PAIRS == T.PAIRS
    assert G.GAIT_NAMES[6:] == [f"{k}_{f}" for k in ("phase_err", "phase_abs_err", "touchdowns") for f in ("FR", "RL", "RR")]
    assert enum_order(src, "Go1GaitGroupField", "GO1GAIT_G_") == G.GAIT_GROUP_FIELDS == T.GROUP_FIELDS
    import go1eval_host as E
    assert enum_order(src, "Go1GaitField", "GO1GAIT_F_") == E.FIELD_NAMES
    assert issubclass(G.Go1Gait, E._Table) and G.Go1Gait.ROWS == 15 and G.Go1Gait.TABLE_ROWS == 16
    assert G.phase_centres().tolist() == [k / 16 for k in range(16)]
    assert len(G.SUPPORT_PATTERNS) == 16 and G.SUPPORT_PATTERNS[0] == "-" and G.SUPPORT_PATTERNS[9] == "FL+RR" and G.SUPPORT_PATTERNS[6] == "FR+RL"
    assert G.SUPPORT_PATTERNS[15] == "FL+FR+RL+RR" and G.SUPPORT_PATTERNS[1] == "FL" and G.SUPPORT_PATTERNS[8] == "RR" and len(set(G.SUPPORT_PATTERNS)) == 16
    from go1_gym_learn.eval_metrics import gait
    assert gait.GAIT_METRICS == G.GAIT_NAMES and gait.BINS == G.BINS
    assert sorted(m for masks in gait.SUPPORT_SHARES.values() for m in masks) == list(range(16))          # every pattern in exactly one share


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1gait_host as G
    declared = set(re.findall(r"\b(go1gait_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1gait_clear", "go1gait_accumulate", "go1gait_reduce", "go1gait_version"}
    out = g.build_gait_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1gait_" in line} == declared
    assert not re.search(r"\bgo1(eval|feet|trunk)_\w+", dynamic)


def test_sources_flags_and_stamp():
    import __graft_entry__ as g
    assert g.gait_sources() == [SOURCE, TABLES, HEADER] and g.GAIT_FLAGS == g.EVAL_FLAGS and "-ffp-contract=off" in g.GAIT_FLAGS
    assert g.GAIT_FLAGS is not g.EVAL_FLAGS
    # the list is what the compiler reads (tests/test_abi.py::test_source_lists_are_what_the_compiler_reads, for this library)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc] + g.GAIT_FLAGS + ["--cuda-host-only", "-MM", SOURCE], cwd=g.CSRC, check=True, capture_output=True, text=True).stdout
    read = {os.path.normpath(os.path.join(g.CSRC, f)) for f in out.split(":", 1)[1].replace("\\\n", " ").split()}
    assert {f for f in read if not f.startswith("/opt/")} == {os.path.normpath(f) for f in g.gait_sources()}
    for others in (g.sim_sources(), g.ppo_sources(), g.render_sources(), g.state_sources()):
        assert not set(others) & set(g.gait_sources())
    for others in (g.eval_sources(), g.feet_sources(), g.trunk_sources(), g.reward_sources()):      # one shared header, and nothing else
        assert set(others) & set(g.gait_sources()) == {TABLES}
    code = re.sub(r"//.*", "", open(SOURCE).read())
    assert not re.search(r"go1(eval|feet|trunk)", code) and "GO1_TABLES_MATCH(GO1GAIT)" in code
    assert "go1gait" not in re.sub(r"//.*", "", open(TABLES).read())        # the shared header names no library
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["../../include/go1gait.h", "go1_tables.h"]
    for banned in ("atomic", "sinf", "cosf", "atan2f", "sincosf"):            # no atomics, no trigonometric function on the device
        assert banned not in code, banned
    accumulate = code[code.index("gait_accumulate_kernel"):code.index("gait_reduce_kernel")]
    assert "__shared__" not in accumulate and "__syncthreads" not in accumulate
    out = g.build_gait_hip()
    assert os.path.basename(out) == "libgo1gait.so" and g.library_stamp(out) == g.source_hash(g.gait_sources(), g.GAIT_FLAGS)
    lib = ctypes.CDLL(out)                                                   # dlopen needs no GPU
    lib.go1gait_version.restype = ctypes.c_char_p
    assert lib.go1gait_version() == b"go1gait 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    assert "build_gait_hip()" in inspect.getsource(g.build) and "libgo1gait.so" in inspect.getsource(g.smoke)
    # the other table libraries' stamps are what their own sources give: this family changed none of them
    for name, sources, flags in (("eval", g.eval_sources(), g.EVAL_FLAGS), ("feet", g.feet_sources(), g.FEET_FLAGS), ("trunk", g.trunk_sources(), g.TRUNK_FLAGS)):
        assert g.library_stamp(os.path.join(g.CSRC, f"libgo1{name}.so")) in (None, g.source_hash(sources, flags)), name


def test_a_missing_library_fails_loudly(tmp_path):
    import go1gait_host as G
    with pytest.raises(G.Go1GaitLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1gait.so"))


# ---- 2. the refusals without a GPU (the helpers of tests/test_eval_return_codes.py) ----------------------------------------------------------
def gait_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.min_stride_steps, c.max_stride_steps = 70, 2, 3, 1, 100


GAIT_ACC = ACCUMULATORS + T.STATE
BAD_CONFIG = [("min_stride_steps = 0", -12, [cfg(min_stride_steps=0)]), ("min_stride_steps < 0", -12, [cfg(min_stride_steps=-4)]),
              ("max_stride_steps < min_stride_steps", -12, [cfg(min_stride_steps=5, max_stride_steps=4)]), ("max_stride_steps = 0", -12, [cfg(max_stride_steps=0)])]
CASES = {
    "go1gait_clear": nobody() + each(GAIT_ACC, -2) + [
        ("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")])],
    "go1gait_accumulate": nobody() + each(GAIT_ACC, -2) + each(T.INPUTS, -3) + BAD_CONFIG + [
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no phase_hist and no foot_indices", -2, [null("phase_hist", "foot_indices")]),
        ("no ref_steps and min_stride_steps = 0", -2, [null("ref_steps"), cfg(min_stride_steps=0)]),
        ("no contact_forces and min_stride_steps = 0", -3, [null("contact_forces"), cfg(min_stride_steps=0)]),
        ("no reset_buf and max_stride_steps = 0", -3, [null("reset_buf"), cfg(max_stride_steps=0)])],
    "go1gait_reduce": nobody() + each(GAIT_ACC, -2) + [
        ("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group", "results", "hist_results"], -5) + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no resets and no hist_results", -2, [null("resets", "hist_results")]),
        ("no td_count and num_groups = 0", -2, [null("td_count"), cfg(num_groups=0)])],
}


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    """every case fails validation, so nothing is launched: there is no GPU.  The smallest good limits (min = max = 1) are not refused:
    with an input missing they get as far as -3."""
    import __graft_entry__ as g
    import go1gait_host as G
    g.build_gait_hip()
    fn = getattr(G.load_library(), symbol)
    assert len({label for label, _, _ in CASES[symbol]}) == len(CASES[symbol])
    assert sum(len(spoilers) > 1 for _, _, spoilers in CASES[symbol]) >= 1          # two conditions at once: precedence
    for label, code, spoilers in CASES[symbol]:
        a = Call(G.Go1GaitConfig, G.Go1GaitBuffers, gait_base)
        for spoil in spoilers:
            spoil(a)
        assert fn(None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b), None) == code, (symbol, label)
    if symbol == "go1gait_accumulate":
        for good in (cfg(min_stride_steps=1, max_stride_steps=1), cfg(min_stride_steps=7, max_stride_steps=7), cfg(max_stride_steps=2 ** 31 - 1)):
            a = Call(G.Go1GaitConfig, G.Go1GaitBuffers, gait_base)
            good(a)
            null("reset_buf")(a)
            assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -3
    else:                                                                    # the clear and the reduction read no input and no stride limit
        a = Call(G.Go1GaitConfig, G.Go1GaitBuffers, gait_base)
        null(*T.INPUTS)(a)
        cfg(min_stride_steps=0, max_stride_steps=-1)(a)
        null("count")(a)
        assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -2


# ---- 3. the model by hand -----------------------------------------------------------------------------------------------------------------------
def snap_of(contact, clocks=(0.0, 0.0, 0.0, 0.0), reset=0, age=100, force=30.0):
    """one environment: `contact` = who is on the ground (FL, FR, RL, RR; a float is taken as the vertical force itself)"""
    s = dict(contact_forces=np.zeros((51, 1), f32), foot_indices=np.zeros((4, 1), f32), reset_buf=np.full(1, reset, np.uint8),
             episode_length_buf=np.full(1, age, np.int32))
    for f in range(4):
        s["contact_forces"][12 * (f + 1) + 2, 0] = contact[f] if isinstance(contact[f], float) else (force if contact[f] else 0.0)
        s["foot_indices"][f, 0] = clocks[f]
    return s


def play(cfg_, steps):
    """the model on one environment over `steps` = [snap_of's keywords]: (state, what every step did)"""
    st, did = T.State(1), []
    for kw in steps:
        did.append(T.accumulate(st, cfg_, snap_of(**kw)))
    return st, did


PERIOD = 20


def gait_steps(shifts, steps, period=PERIOD, **spoil):
    """a perfect gait of `period`-step strides with a duty factor of one half: foot f touches down `shifts[f]` steps after FL (shifts[0]
    = 0) and its clock is the simulator's: it wraps to 0 at the touchdown.  spoil: {step: keywords that replace that step's}"""
    out = []
    for t in range(steps):
        tick = [(t - s) % period for s in shifts]
        kw = dict(contact=[k < period // 2 for k in tick], clocks=[k / period for k in tick])
        kw.update(spoil.get("at", {}).get(t, {}))
        out.append(kw)
    return out


def folded(st):
    """{metric: (count, nonfinite, min, max)} of environment 0"""
    return {name: (int(st.count[m, 0]), int(st.nonfinite[m, 0]), float(st.min[m, 0]), float(st.max[m, 0])) for m, name in enumerate(T.METRICS)}


NOTHING = (0, 0, INF, -INF)
LEGS = ("FR", "RL", "RR")


@pytest.mark.parametrize("name,bins", [("trotting", (8, 8, 0)), ("pacing", (8, 0, 8)), ("bounding", (0, 8, 8)), ("pronking", (0, 0, 0))])
def test_model_perfect_gaits(name, bins):
    """strides of 20 steps under the matching command: the touchdown bins are exactly the gait's, phase_err is exactly 0, the pairs that
    move together have synchrony 1 and the others 0 (all 1 for the pronk), and the support pattern is the gait's two pairs"""
    from go1_gym_learn.eval_metrics import gait, sweep
    commanded = gait.commanded_phases(sweep.GAITS[name])
    assert tuple(int(round(16 * c)) % 16 for c in commanded) == bins
    shifts = [0] + [int(round(PERIOD * c)) for c in commanded]
    st, did = play(T.config(), gait_steps(shifts, 100))
    got = folded(st)
    assert st.strides[0] == 3 and st.strides_dropped[0] == 0 and st.steps[0] == 100                      # FL lands at 20 (opens), 40, 60, 80
    assert [d["length"][0] for d in did if d["closed"][0]] == [PERIOD] * 3
    for k, leg in enumerate(LEGS):
        assert st.phase_hist[k, :, 0].tolist() == [3 if b == bins[k] else 0 for b in range(16)], leg
        assert got[f"phase_err_{leg}"] == (3, 0, 0.0, 0.0) and got[f"phase_abs_err_{leg}"] == (3, 0, 0.0, 0.0) and got[f"touchdowns_{leg}"] == (3, 0, 1.0, 1.0)
    for k, (i, j) in enumerate(T.PAIRS):
        together = shifts[i] == shifts[j]
        assert got[T.METRICS[k]] == (100, 0, float(together), float(together)), T.METRICS[k]
    first = sum(1 << f for f in range(4) if shifts[f] == 0)
    want = {15: 50, 0: 50} if name == "pronking" else {first: 50, 15 - first: 50}
    assert {int(b): int(n) for b, n in enumerate(st.support_hist[:, 0]) if n} == want
    table, hist = T.reduce(st, [0], 1)
    realised = [gait.circular_stats(hist[0, 1 + k])[0] for k in range(3)]
    assert gait.classify(realised) == (name, 0.0) and all(gait.circular_stats(hist[0, 1 + k])[1] == pytest.approx(1.0) for k in range(3))


def test_model_the_sign_of_the_commanded_phase():
    """FR touches down a quarter of a stride after FL, so its clock is a quarter BEHIND FL's: frac(clock_FL - clock_FR) = 0.25 is the
    commanded phase and the error is 0.  Taken the other way round (FR minus FL: 0.75) the error would be -0.5 on every stride."""
    st, _ = play(T.config(), gait_steps([0, 5, 10, 15], 100))
    got = folded(st)
    assert st.strides[0] == 3
    assert [int(st.phase_hist[k, :, 0].argmax()) for k in range(3)] == [4, 8, 12] and (st.phase_hist.sum(axis=1)[:, 0] == 3).all()
    for leg in LEGS:
        assert got[f"phase_err_{leg}"] == (3, 0, 0.0, 0.0) and got[f"phase_abs_err_{leg}"] == (3, 0, 0.0, 0.0), leg
    # a foot that is late against its clock: FR lands at step 7 of 20 under the same clocks: + 0.1 (rounded as the header rounds)
    late = gait_steps([0, 5, 10, 15], 100)
    for t, kw in enumerate(late):
        kw["contact"][1] = (t - 7) % PERIOD < PERIOD // 2
    got = folded(play(T.config(), late)[0])
    p, cmd = f32(7.0) / f32(20.0), f32(0.0) - f32(0.75)
    cmd = cmd - np.floor(cmd)
    err = p - cmd
    err = err - np.floor(err + f32(0.5))
    assert got["phase_err_FR"] == (3, 0, float(err), float(err)) and abs(float(err) - 0.1) < 1e-7 and got["phase_err_RL"] == (3, 0, 0.0, 0.0)
    # the simulator's own assignment: a triple (phase, offset, bound) puts FR at phase + bound, RL at phase + offset, RR at offset + bound
    from go1_gym_learn.eval_metrics import gait
    p_, o_, b_ = 0.25, 0.125, 0.0625
    gi = 0.3
    clock = [(gi + p_ + o_ + b_) % 1, (gi + o_) % 1, (gi + b_) % 1, (gi + p_) % 1]                      # csrc/go1_maps.h: f0, f1, f2, f3
    assert gait.commanded_phases((p_, o_, b_)) == pytest.approx([(clock[0] - clock[f]) % 1 for f in (1, 2, 3)])


def test_model_a_reset_or_a_warm_up_inside_a_stride_folds_nothing():
    quiet, _ = play(T.config(), gait_steps([0, 10, 10, 0], 100))
    assert quiet.strides[0] == 3
    for spoil in (dict(reset=1, age=0), dict(age=2)):                        # a reset; a step inside the warm-up (warm-up 2 below)
        st, did = play(T.config(warmup_steps=2), gait_steps([0, 10, 10, 0], 100, at={45: spoil}))
        got = folded(st)
        # the stride opened at 40 is forgotten, not dropped; FL is seen in the air from 50 on, lands at 60 (opens) and at 80 (closes)
        assert st.strides[0] == 2 and st.strides_dropped[0] == 0 and (st.steps[0], st.resets[0]) == (100, spoil.get("reset", 0))
        assert [t for t, d in enumerate(did) if d["closed"][0]] == [40, 80] and [t for t, d in enumerate(did) if d["opened"][0]] == [20, 60]
        assert got["sync_FL_RR"][0] == 99 and st.support_hist[:, 0].sum() == 99 and got["touchdowns_FR"] == (2, 0, 1.0, 1.0)
        assert not did[45]["live"][0] and st.phase_hist[0, 8, 0] == 2
    st, _ = play(T.config(), gait_steps([0, 10, 10, 0], 46, at={45: dict(reset=1, age=0)}))
    assert st.ref_steps[0] == -1 and st.prev_contact[:, 0].tolist() == [2, 2, 2, 2] and st.strides[0] == 1
    # a warm-up that never ends: steps and nothing else
    st, _ = play(T.config(warmup_steps=1000), gait_steps([0, 10, 10, 0], 60))
    assert st.steps[0] == 60 and st.count.sum() == 0 and st.support_hist.sum() == 0 and st.strides[0] == 0 and st.ref_steps[0] == -1


def chatter_steps():
    """FL lands at step 2, bounces (in the air at 3, down again at 4), stands until 9, swings and lands at 14; FR lands at 8"""
    fl = [0, 0, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1]
    fr = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    return [dict(contact=[bool(a), bool(b), True, True]) for a, b in zip(fl, fr)]


def test_model_chatter_is_ignored_or_folded():
    st, did = play(T.config(min_stride_steps=3), chatter_steps())
    assert [t for t, d in enumerate(did) if d["chatter"][0]] == [4] and [t for t, d in enumerate(did) if d["closed"][0]] == [14]
    assert st.strides[0] == 1 and did[14]["length"][0] == 12 and st.phase_hist[0, :, 0].tolist() == [0] * 8 + [1] + [0] * 7      # 6 / 12: bin 8
    assert folded(st)["touchdowns_FR"] == (1, 0, 1.0, 1.0) and folded(st)["touchdowns_RL"] == (1, 0, 0.0, 0.0) and folded(st)["phase_err_RL"] == NOTHING
    st, did = play(T.config(min_stride_steps=1), chatter_steps())           # no debounce: the bounce closes a stride of two steps
    assert [t for t, d in enumerate(did) if d["closed"][0]] == [4, 14] and not any(d["chatter"][0] for d in did)
    assert [int(did[t]["length"][0]) for t in (4, 14)] == [2, 10] and st.strides[0] == 2
    assert st.phase_hist[0, :, 0].tolist() == [0] * 6 + [1] + [0] * 9       # FR at step 4 of 10: floor(6.4 + 0.5) = 6
    assert folded(st)["touchdowns_FR"] == (2, 0, 0.0, 1.0)


def test_model_an_overlong_stride_is_dropped():
    steps = [dict(contact=[t in (2, 3, 110, 111), t == 50, True, False]) for t in range(115)]
    st, did = play(T.config(), steps)                                        # 108 steps between FL's touchdowns, the limit 100
    assert [t for t, d in enumerate(did) if d["dropped"][0]] == [103] and st.strides_dropped[0] == 1 and st.strides[0] == 0
    assert [t for t, d in enumerate(did) if d["opened"][0]] == [2, 110] and st.ref_steps[0] == 4 and st.count[T.TOUCHDOWNS:].sum() == 0
    st, did = play(T.config(max_stride_steps=108), steps)                    # the limit itself is allowed
    assert st.strides[0] == 1 and st.strides_dropped[0] == 0 and did[110]["length"][0] == 108 and folded(st)["touchdowns_FR"] == (1, 0, 1.0, 1.0)
    assert st.phase_hist[0, :, 0].tolist() == [0] * 7 + [1] + [0] * 8       # 48 / 108: floor(7.11 + 0.5) = 7


def test_model_bins_touchdowns_and_tables():
    p = np.array([0.0, 0.03124, 0.03125, 0.5, 0.96874, 0.96875, 0.99], f32)
    assert T.phase_bin(p).tolist() == [0, 0, 1, 8, 15, 0, 0] and T.raw_phase_bin(p).tolist() == [0, 0, 1, 8, 15, 16, 16]
    # a stride of 32 steps: FR lands on its last step (31 / 32: bin 16 -> 0), RL three times, RR on the opening step and never again
    steps = [dict(contact=[t in (2, 34), t == 33, t in (5, 9, 20), t in (2, 34)]) for t in range(36)]
    st, did = play(T.config(), steps)
    got = folded(st)
    assert did[2]["opening_touchdown"][0] and did[34]["closed"][0] and did[34]["wrapped"][0] and did[34]["several"][0] and did[34]["length"][0] == 32
    assert st.phase_hist[0, 0, 0] == 1 and st.phase_hist[1, 9, 0] == 1 and st.phase_hist[2, 0, 0] == 1 and st.phase_hist.sum() == 3      # 18 / 32 * 16 = 9
    assert got["touchdowns_FR"] == (1, 0, 1.0, 1.0) and got["touchdowns_RL"] == (1, 0, 3.0, 3.0) and got["touchdowns_RR"] == (1, 0, 1.0, 1.0)
    assert st.last_td[:, 0].tolist() == [-1, -1, 0] and st.td_count[:, 0].tolist() == [0, 0, 1] and st.ref_steps[0] == 1
    # NaN, -inf and 1.0 are in the air, +inf and the next float above 1 are on the ground
    st, _ = play(T.config(), [dict(contact=[NAN, -INF, 1.0, INF])] * 2 + [dict(contact=[float(np.nextafter(f32(1), f32(2))), 0.5, 30.0, 0.0])])
    assert st.support_hist[:, 0].tolist() == [0] * 5 + [1, 0, 0, 2] + [0] * 7 and st.nonfinite.sum() == 0
    # a non-finite clock: the error is counted in nonfinite, the histogram still gets the stride
    bad = gait_steps([0, 10, 10, 0], 45, at={40: dict(clocks=[0.0, NAN, INF, 0.0])})
    for kw in bad[40:41]:
        kw.setdefault("contact", [True, False, False, True])
    st, did = play(T.config(), bad)
    got = folded(st)
    assert did[40]["bad_clock"][0] and got["phase_err_FR"] == (0, 1, INF, -INF) and got["phase_abs_err_RL"] == (0, 1, INF, -INF) and got["phase_err_RR"] == (1, 0, 0.0, 0.0)
    assert st.phase_hist[:, :, 0].sum() == 3 and np.isfinite(st.sum).all()
    table, hist = T.reduce(st, [0], 2)
    assert table.shape == (2, 16, 6) and hist.shape == (2, 4, 16) and table[0, 15].tolist() == [1.0, 45.0, 0.0, 1.0, 0.0, 0.0] and not table[1, 15].any()
    assert hist[0, 0].sum() == 45 and hist[0, 1:].sum() == 3 and not hist[1].any() and np.isnan(table[1, :15, 1:5]).all()
    assert table[0, T.PHASE_ERR, [0, 5]].tolist() == [0.0, 1.0] and np.isnan(table[0, T.PHASE_ERR, 1])


# ---- 4. go1gait.hip under the SIMT emulator against the model ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1gait_host as G
    return G.load_library(build_emu(g.gait_sources(), "libgo1gait_emu.so"))


SHAPES_OF_INPUTS = dict(contact_forces=51, foot_indices=4)


def gait_on(device, cfg_, N, lib=None):
    """a go1gait_host.Go1Gait on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1gait_host as G
    tensors = {k: torch.zeros(rows, N, device=device) for k, rows in SHAPES_OF_INPUTS.items()}
    tensors.update(reset_buf=torch.zeros(N, dtype=torch.uint8, device=device), episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    gm = G.Go1Gait(types.SimpleNamespace(num_envs=N), B, min_stride_steps=cfg_.min_stride_steps, max_stride_steps=cfg_.max_stride_steps, lib=lib)
    if torch.device(device).type == "cpu":
        gm._stream = lambda: None
    return gm, B


def gait_groups(rng, N, groups=3):
    """three groups of which group 1 is empty, some environments at -1 and (from three environments on) one id outside the tables"""
    assert groups == 3
    group = rng.integers(-1, groups, N).astype(np.int32)
    group[group == 1] = 2
    group[0] = groups - 1
    if N >= 3:
        group[1], group[2] = -1, groups
    return group


def drive(gm, B, cfg_, snaps, group, groups):
    """the scripted steps through the library: arm for `groups` groups, upload a snapshot, accumulate, ...; returns read() and the
    accumulators.  arm() sizes the tables by the largest id it is given, so the ids outside the tables are handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    gm.arm(inside, cfg_.warmup_steps)
    gm.group.copy_(torch.from_numpy(group))
    for s in snaps:
        for k, a in s.items():
            getattr(B, k).copy_(torch.from_numpy(a))
        gm.accumulate()
    gm.disarm()
    res = gm.read()
    acc = {k: t.cpu().numpy() for k, t in gm.acc.items()}
    return res, acc


def state_name(k):
    return "env_" + k if k.endswith("_hist") else k


def same_as_the_model(res, acc, st, group, groups):
    """accumulators, state, histograms and both result tables against the model's state `st`, bit for bit"""
    N = st.N
    for k in ACCUMULATORS:
        assert acc[k].shape == (15, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in T.STATE:
        assert res[state_name(k)].shape == getattr(st, k).shape and bits(res[state_name(k)].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    want, want_hist = T.reduce(st, group, groups)
    table = np.concatenate([np.stack([res["metrics"][m] for m in T.METRICS], axis=1), np.zeros((groups, 1, 6))], axis=1)
    table[:, 15, :5] = res["groups"]
    assert table.shape == want.shape == (groups, T.ROWS, 6)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and bits(table) == bits(want)
    assert res["support_hist"].shape == (groups, 16) and bits(res["support_hist"]) == bits(want_hist[:, 0])
    assert res["phase_hist"].shape == (groups, 3, 16) and bits(res["phase_hist"]) == bits(want_hist[:, 1:])
    return want, want_hist


def check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N):
    """the library's results against tests/gait_ref.py, bit for bit; then that the script drove every branch it was written to drive"""
    st, did = T.run(cfg_, snaps, N)
    want, want_hist = same_as_the_model(res, acc, st, group, groups)
    steps = len(snaps)
    assert (res["steps"] == steps).all() and res["phase_centres"][1] == 0.0625
    ever = lambda key: np.any([d[key] for d in did], axis=0)
    count = lambda key: np.sum([d[key] for d in did], axis=0)
    if N >= len(T.KINDS):
        trots, resets, chatters, slow, odd, stands, threshold = (kind == k for k in range(len(T.KINDS)))
        quiet = trots & (st.resets == 0)
        # the trot: strides of ten steps close one after the other, every one with RR's touchdown on its opening step and an error below
        # the clocks' jitter; a reset or the warm-up breaks them
        assert quiet.any() and (st.strides[quiet] == (steps - 10) // T.TROT_PERIOD - 1 + 1).all() and ever("opening_touchdown")[quiet].all()
        assert (st.max[T.PHASE_ABS_ERR:T.PHASE_ABS_ERR + 3][:, quiet] < 0.011).all() and (st.strides_dropped[quiet] == 0).all()
        assert (st.phase_hist[0, 8, quiet] == st.strides[quiet]).all() and (st.phase_hist[2, 0, quiet] == st.strides[quiet]).all()
        assert (res["resets"][resets] >= 4).all() and snaps[0]["reset_buf"][resets].all() and (st.strides[resets] < st.strides[quiet].max()).all()
        assert any((~d["live"] & (s["reset_buf"] == 0)).any() for d, s in zip(did, snaps))                  # warm-up steps that are no resets
        # chatter inside min_stride_steps; several touchdowns and none in one stride
        assert (count("chatter")[chatters] >= 6).all() and (st.strides[chatters] == (steps - 1) // T.CHATTER_PERIOD - 1).all()
        assert (st.max[T.TOUCHDOWNS, chatters] == 4.0).all() and (st.max[T.TOUCHDOWNS + 1, chatters] == 0.0).all() and ever("several")[chatters].all()
        assert ever("none")[chatters].all() and (st.count[T.PHASE_ERR + 1, chatters] == 0).all() and (st.count[T.TOUCHDOWNS + 1, chatters] > 0).all()
        # the slow ones: a stride of 32 steps whose last touchdown wraps from bin 16 to 0, one dropped as too long, one of ten steps
        assert (st.strides[slow] == 2).all() and (st.strides_dropped[slow] == 1).all() and ever("wrapped")[slow].all() and count("opened")[slow].tolist() == [2] * slow.sum()
        assert (st.phase_hist[2, 0, slow] == 1).all() and (st.phase_hist[2].sum(axis=0)[slow] == 1).all() and not ever("wrapped")[quiet].any()
        assert sorted({int(x) for d in did for x in d["length"][slow] if x}) == [10, 32]
        # +-inf and NaN in forces and clocks were met; the clocks' entered no sum
        assert ever("bad_clock")[odd].all() and st.nonfinite[T.PHASE_ERR:T.TOUCHDOWNS][:, odd].sum() > 0 and st.nonfinite[:T.PHASE_ERR].sum() == 0
        assert np.isfinite(st.sum).all() and np.isfinite(st.sumsq).all() and any(np.isnan(s["contact_forces"][14::12][:, odd]).any() for s in snaps)
        # a robot that stands: bin 15 only, every pair in step, no stride
        assert (st.support_hist[15, stands] == steps - cfg_.warmup_steps).all() and (st.support_hist[:15, stands] == 0).all() and (st.strides[stands] == 0).all()
        assert (st.min[:6][:, stands] == 1.0).all() and (st.ref_steps[stands] == -1).all()
        # one ulp either side of the threshold gives both contact states
        assert (st.support_hist[:, threshold] > 0).sum(axis=0).min() >= 3
        sane = ~(resets | trots | threshold)
        assert (st.support_hist.sum(axis=0)[sane] == steps - cfg_.warmup_steps).all() and (st.support_hist.sum(axis=0) == st.count[0]).all()
    g = res["groups"]
    assert g[:, 0].sum() == np.isin(group, range(groups)).sum() and (g[:, 1] == steps * g[:, 0]).all() and g[1].tolist() == [0.0] * 5
    assert np.isnan(want[1, :15, 1:5]).all() and not want_hist[1].any()
    return st


# 1: one thread; 64: one wavefront; 257: two blocks with a ragged tail; 600: three terms per reduction thread and 38 environments per
# histogram slice
SHAPES = [1, 64, 257, 600]


@pytest.mark.parametrize("N", SHAPES)
def test_emulated_gait_kernels_follow_the_model(emu, N):
    groups = 3
    rng = np.random.default_rng(900 + N)
    cfg_, snaps, kind = T.scripted_steps(rng, N)
    assert len(snaps) == T.SCRIPT_STEPS and (cfg_.min_stride_steps, cfg_.max_stride_steps) == (3, 40)
    assert N < len(T.KINDS) or set(kind.tolist()) == set(range(len(T.KINDS)))
    group = gait_groups(rng, N, groups)
    gm, B = gait_on("cpu", cfg_, N, lib=emu)
    res, acc = drive(gm, B, cfg_, snaps, group, groups)
    assert gm.cfg.num_groups == groups and (N < 3 or {-1, groups} <= set(group.tolist()))
    check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N)
    again = gm.read()                                                        # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ("groups", "support_hist", "phase_hist", "env_phase_hist", "last_td", "strides"))
    assert all(bits(again["metrics"][m]) == bits(res["metrics"][m]) for m in T.METRICS)
    with pytest.raises(RuntimeError, match="go1gait_accumulate failed: -12"):
        gm.cfg.min_stride_steps = 0
        gm.accumulate()


# ---- 5. the environment hooks without a GPU -----------------------------------------------------------------------------------------------------
def test_gait_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    for module in ("go1eval_host", "go1gait_host"):
        monkeypatch.delitem(sys.modules, module, raising=False)
    c = apply_train_config(make_cfg(), num_envs=16)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_gait_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_gait_metrics, env.read_gait_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert all(m not in sys.modules for m in ("go1eval_host", "go1gait_host")) and env._gait is None          # never measured: no host module
    env.step(torch.zeros(16, 12))                                             # and stepping goes on
    signature = inspect.signature(env.start_gait_metrics)
    assert {k: p.default for k, p in signature.parameters.items() if k != "groups"} == dict(warmup_steps=0, min_stride_steps=1, max_stride_steps=100)
    assert ("gait", "_gait") in env._STATE_FAMILIES


# ---- 6. the scenario of the GPU test, through the fp64 oracle here -----------------------------------------------------------------------------
TROT_STEPS, TROT_WARMUP = 80, 2
DIAGONAL, OTHERS = (T.SYNC + 2, T.SYNC + 3), (T.SYNC + 0, T.SYNC + 1, T.SYNC + 4, T.SYNC + 5)            # FL-RR and FR-RL; the four other pairs


def trot_events(st, did):
    """what the GPU test relies on, per environment: closed reference strides; closed strides in which all three other feet touched
    down; and per pair the mean synchrony over all environments"""
    complete = np.sum([d["closed"] & ~d["none"] for d in did], axis=0)
    sync = st.sum[:6].sum(axis=1) / st.count[:6].sum(axis=1)
    return st.strides.astype(np.int64), complete, sync


def assert_trot_events(st, did, label):
    strides, complete, sync = trot_events(st, did)
    lengths = [int(x) for d in did for x in d["length"] if x]
    print(f"\n{label}: resets {int(st.resets.sum())}; closed strides per environment {strides.min()} to {strides.max()}, complete ones {complete.min()} to "
          f"{complete.max()}, stride lengths {min(lengths)} to {max(lengths)} steps, dropped {int(st.strides_dropped.sum())}; mean synchrony FL-RR / FR-RL "
          f"{sync[2]:.2f} / {sync[3]:.2f}, the four other pairs {min(sync[[0, 1, 4, 5]]):.2f} to {max(sync[[0, 1, 4, 5]]):.2f}")
    assert (strides >= 1).all() and (complete >= 1).all()
    assert min(sync[2], sync[3]) > max(sync[[0, 1, 4, 5]])


def test_the_trot_script_produces_strides_on_the_oracle(monkeypatch):
    """the scenario of test_gpu_gait_metrics.test_gait_through_the_environment on the CPU oracle: under the foot family's trot script every
    environment closes a reference stride, closes one in which all three other feet touched down, and both diagonal pairs move together
    more than any other pair"""
    import fake_sim
    from test_foot_metrics import trot_action
    from test_gpu_response_trace import make_env
    fake_sim.install(monkeypatch)
    N = 64
    env = make_env(N, "plane", 20.0, seed=4)
    env.reset()
    cfg_ = T.config(warmup_steps=TROT_WARMUP, min_stride_steps=1, max_stride_steps=100)
    st, did = T.State(N), []
    for step in range(TROT_STEPS):
        env.step(trot_action(step, N))
        did.append(T.accumulate(st, cfg_, {n: getattr(env.buffers, n).cpu().numpy().copy() for n in T.INPUTS}))
    assert_trot_events(st, did, "oracle")
    assert st.resets.sum() == 0


# ---- 7. the sweep's host pieces and the tool ------------------------------------------------------------------------------------------------------
def test_classify_and_circular_statistics():
    from go1_gym_learn.eval_metrics import gait, sweep
    assert gait.classify((0.5, 0.5, 0.0)) == ("trotting", 0.0) and gait.classify((0.5, 0.0, 0.5)) == ("pacing", 0.0)
    assert gait.classify((0.0, 0.5, 0.5)) == ("bounding", 0.0) and gait.classify((0.0, 0.0, 0.0)) == ("pronking", 0.0)
    for name, triple in sweep.GAITS.items():
        assert gait.classify(gait.commanded_phases(triple)) == (name, 0.0) and gait.gait_name(triple) == name
    name, distance = gait.classify((0.5625, 0.4375, 0.96875))                # a trot that is a little off, across the wrap
    assert name == "trotting" and distance == pytest.approx(0.0625 + 0.0625 + 0.03125)
    assert gait.classify((0.45, 0.1, 0.55))[0] == "pacing" and gait.classify((0.9, 0.4, 0.6))[0] == "bounding"
    for missing in ((NAN, 0.5, 0.0), (0.5, NAN, 0.0), (0.5, 0.5, NAN), (NAN, NAN, NAN)):
        name, distance = gait.classify(missing)
        assert name == "none" and np.isnan(distance)
    assert gait.gait_name((0.25, 0.0, 0.0)) == "(0.25, 0, 0)"
    assert gait.circular_distance(0.95, 0.05) == pytest.approx(0.1) and gait.circular_distance(0.25, 0.75) == 0.5
    hist = np.zeros(16)
    assert all(np.isnan(x) for x in gait.circular_stats(hist))
    hist[8] = 7.0
    assert gait.circular_stats(hist) == (pytest.approx(0.5), pytest.approx(1.0))
    hist[:] = 0.0
    hist[15], hist[1] = 3.0, 3.0                                             # either side of the wrap: the mean is 0, not 0.5
    mean, length = gait.circular_stats(hist)
    assert min(mean, 1.0 - mean) < 1e-9 and length == pytest.approx(np.cos(2 * np.pi / 16))
    hist[:] = 1.0
    mean, length = gait.circular_stats(hist)
    assert np.isnan(mean) and length == 0.0


def fixed_result():
    import go1gait_host as G
    from go1_gym_learn.eval_metrics import sweep
    row = lambda n, mean, std=0.0: np.array([[n, mean, std, mean - std, mean + std, 0.0]] * 3)
    empty = [0.0, NAN, NAN, NAN, NAN, 0.0]
    t = {m: row(300.0, 0.25) for m in T.METRICS[:6]}
    t["sync_FL_RR"], t["sync_FR_RL"] = row(300.0, 0.9), row(300.0, 0.8)
    for leg in LEGS:
        t[f"phase_err_{leg}"], t[f"phase_abs_err_{leg}"], t[f"touchdowns_{leg}"] = row(20.0, 0.01, 0.02), row(20.0, 0.02, 0.01), row(20.0, 1.0, 0.25)
    # cell 1 is commanded to pace and trots all the same: RL and RR half a cycle from their command
    for leg in ("RL", "RR"):
        t[f"phase_err_{leg}"][1], t[f"phase_abs_err_{leg}"][1] = [20.0, -0.05, 0.48, -0.5, 0.49, 0.0], [20.0, 0.48, 0.01, 0.45, 0.5, 0.0]
    # cell 2 never lifted RL: no phase for it
    t["phase_err_RL"][2], t["phase_abs_err_RL"][2], t["touchdowns_RL"][2] = empty, empty, [20.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    phase = np.zeros((3, 3, 16))
    phase[:, 0, 8], phase[:, 1, 8], phase[:, 2, 0] = 20.0, 20.0, 20.0
    phase[2, 1] = 0.0
    support = np.zeros((3, 16))
    support[:, [9, 6, 15, 0, 1, 7]] = [150.0, 120.0, 15.0, 9.0, 3.0, 3.0]
    trot, pace = sweep.GAITS["trotting"], sweep.GAITS["pacing"]
    return dict(preset="static_medium", cells=[(1.0, 0.0, trot), (1.0, 0.0, pace), (1.0, 0.0, trot)], gait=t,
                gait_groups=np.array([[8.0, 320.0, 0.0, 20.0, 1.0]] * 3), support_hist=support, phase_hist=phase, phase_centres=G.phase_centres(),
                support_patterns=list(G.SUPPORT_PATTERNS), metrics={}, groups=np.zeros((3, 5)), min_stride_steps=1, max_stride_steps=100, num_envs=24,
                steps=40, warmup_steps=5, seed=1, dt=0.02)


def test_gait_table_json_and_figure(tmp_path):
    from go1_gym_learn.eval_metrics import gait
    res = fixed_result()
    md = gait.gait_markdown_table(res).splitlines()
    assert md[0].startswith("| vx | yaw | commanded | realised | distance | FR cmd / real / err | RL cmd / real / err | RR cmd / real / err | resultant FR / RL / RR |")
    assert len(md) == 2 + 3 and len({line.count("|") for line in md}) == 1 and md[0].count("|") == 23
    assert md[2].startswith("| 1 | 0 | trotting | trotting | 0.000 | 0.500 / 0.500 / +0.010 ± 0.020 | 0.500 / 0.500 / +0.010 ± 0.020 | 0.000 / 0.000 / +0.010 ± 0.020 | 1.00 / 1.00 / 1.00 |")
    assert "| 0.850 | 0.250 | 0.250 | 0.030 | 0.010 | 0.900 | 0.000 | 0.000 | 0.010 | 0.050 | 1.00 / 1.00 / 1.00 | 20 | 1 |" in md[2]
    # commanded to pace, trotting: FR at 0.5 is the pace's FR too; RL at 0.5 against 0 and RR at 0 against 0.5: the wrapped errors' mean
    # is not shown, the histogram's figure is; and the class says trotting (the distance is the one to the class, not to the command)
    assert md[3].startswith("| 1 | 0 | pacing | trotting | 0.000 | 0.500 / 0.500 / +0.010 ± 0.020 | 0.000 / 0.500 / ~-0.500 | 0.500 / 0.000 / ~-0.500 |")
    assert md[4].startswith("| 1 | 0 | trotting | none | – | 0.500 / 0.500 / +0.010 ± 0.020 | 0.500 / – / – ± – |") and "| 1.00 / – / 1.00 |" in md[4] and "1.00 / 0.00 / 1.00 | 20 | 1 |" in md[4]
    s = gait.cell_summary(res, 1)
    assert s["err_from_histogram"] == [False, True, True] and s["class"] == "trotting" and s["support"]["diagonal"] == 0.9 and s["sync"]["diagonal"] == pytest.approx(0.85)
    js = json.loads(json.dumps(gait.gait_to_json(res), allow_nan=False))
    assert js["cells"][1] == dict(vx=1.0, yaw=0.0, gait=[0.0, 0.0, 0.5], gait_name="pacing") and js["group_fields"] == T.GROUP_FIELDS
    assert js["gait"]["phase_err_RL"][2][1] is None and js["gait"]["sync_FL_RR"][0][1] == 0.9 and js["phase_hist"][0][2][0] == 20.0 and js["legs"] == list(LEGS)
    assert js["summary"][2]["class"] == "none" and js["summary"][2]["class_distance"] is None and js["summary"][0]["realised"] == pytest.approx([0.5, 0.5, 0.0])
    assert len(js["support_patterns"]) == 16 and js["max_stride_steps"] == 100 and js["gait_groups"][0][3] == 20.0 and len(js["phase_centres"]) == 16
    path = tmp_path / "gait.png"
    gait.plot_gait(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000


def test_tool_accepts_a_coordination_sweep(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import gait, sweep
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--coordination", "--vx", "1.0", "--gaits", "trotting", "pacing", "--envs", "24", "--steps", "40", "--warmup-steps", "5",
                                      "--presets", "static_medium", "--min-stride-steps", "3", "--max-stride-steps", "60"])
    assert a.coordination and not a.trunk and not a.feet and (a.vx, a.gaits, a.envs, a.steps, a.min_stride_steps, a.max_stride_steps) == ([1.0], ["trotting", "pacing"], 24, 40, 3, 60)
    plain = eval_sweep.parse_args(base + ["--coordination"])
    assert (plain.min_stride_steps, plain.max_stride_steps) == (1, 100) and not eval_sweep.parse_args(base).coordination
    assert eval_sweep.parse_args(base + ["--coordination", "--terrain", "plane"]).terrain == "plane"
    for bad in (["--coordination", "--terrain"], ["--coordination", "--behaviour"], ["--coordination", "--joints"], ["--coordination", "--feet"], ["--coordination", "--trunk"],
                ["--coordination", "--rewards"], ["--coordination", "--response", "--switch", "vx", "0", "1"], ["--coordination", "--push", "--magnitude", "1", "--direction", "0"],
                ["--min-stride-steps", "3"], ["--trunk", "--max-stride-steps", "50"], ["--coordination", "--min-stride-steps", "0"],
                ["--coordination", "--min-stride-steps", "5", "--max-stride-steps", "4"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(base + bad)
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(gait, "run_gait_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    grid = dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits])
    eval_sweep.run_gait(a, None, grid)
    assert seen == dict(preset="static_medium", grid=grid, num_envs=24, steps=40, warmup_steps=5, seed=1, terrain=None, min_stride_steps=3, max_stride_steps=60)
    js = json.load(open(tmp_path / "eval" / "static_medium_gait.json"))
    assert js["preset"] == "static_medium" and js["summary"][1]["class"] == "trotting"
    md = (tmp_path / "eval" / "static_medium_gait.md").read_text()
    assert "| pacing | trotting | 0.000 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_gait.png").read_bytes()[:4] == b"\x89PNG"
