"""CPU checks of foot loading (include/go1feet.h, libgo1feet.so): the ctypes mirrors and the exported symbols against the header, the
build's source lists and stamp, the refusals without a GPU, the host-side definition against the reference's two per-foot reward
terms, the model of tests/feet_ref.py on hand-computable cases, go1feet.hip itself under the SIMT emulator against that model bit for
bit (accumulators, state, profile and the three result tables), the environment hooks where there is no GPU, and the sweep's host
pieces."""
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

import feet_ref as F
from test_eval_return_codes import Call, cfg, each, nobody, null
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from util import build_emu

HEADER = os.path.join(REPO, "include", "go1feet.h")
SOURCE = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1feet.hip")
TABLES = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1_tables.h")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]


# ---- 1. mirrors, symbols, sources, stamp ---------------------------------------------------------------------------------------------------
def test_feet_mirrors_match_the_header():
    import go1feet_host as G
    src = open(HEADER).read()
    for macro, value in (("GO1FEET_NUM", G.NUM_FEET_METRICS), ("GO1FEET_NUM_FEET", G.NUM_FEET), ("GO1FEET_PHASE_BINS", G.PHASE_BINS),
                         ("GO1FEET_NUM_FIELDS", 6), ("GO1FEET_REDUCE_THREADS", 256), ("GO1FEET_CONTACT_FORCE", G.CONTACT_FORCE)):
        assert re.search(rf"#define {macro} {value}\n", src), macro
    assert (G.NUM_FEET_METRICS, G.NUM_FEET, G.PHASE_BINS) == (12, 4, 16) == (F.M, F.FEET, F.BINS)
    want = struct_fields(src, "Go1FeetConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1FeetConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "dt", "terrain_friction", "max_contact_force"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1FeetConfig._fields_):
        assert ctype is C_TYPES[ctext], field
    assert ctypes.sizeof(G.Go1FeetConfig) == 24
    want = struct_fields(src, "Go1FeetBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1FeetBuffers._fields_] == F.INPUTS + ACCUMULATORS + F.STATE + ["group", "results", "profile_results"]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1FeetBuffers._fields_)
    types_ = dict(want)
    assert types_["prev_contact"] == types_["stance_valid"] == "uint8_t*" and types_["stance_steps"] == "int32_t*" and types_["stance_impulse"] == "float*"
    assert types_["profile_sum"] == types_["profile_results"] == types_["results"] == "double*" and types_["profile_count"] == "uint32_t*"
    assert G._FEET_INPUTS == F.INPUTS and G._FEET_STATE == F.STATE
    assert enum_order(src, "Go1FeetMetric", "GO1FEET_") == G.FEET_NAMES == F.METRICS and len(F.METRICS) == G.NUM_FEET_METRICS
    assert enum_order(src, "Go1FeetGroupField", "GO1FEET_G_") == G.FEET_GROUP_FIELDS == F.GROUP_FIELDS
    import go1eval_host as E
    assert enum_order(src, "Go1FeetField", "GO1FEET_F_") == E.FIELD_NAMES and G.CONTACT_FORCE == 1.0
    assert issubclass(G.Go1Feet, E._Table) and G.Go1Feet.ROWS == 48 and G.Go1Feet.TABLE_ROWS == 49
    from go1_gym_learn.eval_metrics import feet
    assert feet.FEET_METRICS == G.FEET_NAMES and feet.FOOT_NAMES == G.FOOT_NAMES == ["FL", "FR", "RL", "RR"]
    assert feet.FOOT_TERMS == G.STEP_NAMES + G.TOUCHDOWN_NAMES and G.STANCE_NAMES == F.METRICS[8:]


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1feet_host as G
    declared = set(re.findall(r"\b(go1feet_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1feet_clear", "go1feet_accumulate", "go1feet_reduce", "go1feet_version"}
    out = g.build_feet_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1feet_" in line} == declared
    assert not re.search(r"\bgo1eval_\w+", dynamic)


def test_sources_flags_and_stamp():
    import __graft_entry__ as g
    assert g.feet_sources() == [SOURCE, TABLES, HEADER] and g.FEET_FLAGS == g.EVAL_FLAGS and "-ffp-contract=off" in g.FEET_FLAGS
    assert g.eval_sources() == [os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1eval.hip"), TABLES, os.path.join(REPO, "include", "go1eval.h")]
    for others in (g.sim_sources(), g.ppo_sources(), g.render_sources()):
        assert not set(others) & set(g.feet_sources())
    for others in (g.eval_sources(), g.trunk_sources()):                      # the metric libraries share one header, and nothing else
        assert set(others) & set(g.feet_sources()) == {TABLES}
    assert "go1eval" not in re.sub(r"//.*", "", open(SOURCE).read())          # the library names nothing of libgo1eval ...
    shared = re.sub(r"//.*", "", open(TABLES).read())                         # ... and the shared header names no library
    assert "go1eval" not in shared and "go1feet" not in shared and "go1trunk" not in shared
    out = g.build_feet_hip()
    assert os.path.basename(out) == "libgo1feet.so" and g.library_stamp(out) == g.source_hash(g.feet_sources(), g.FEET_FLAGS)
    lib = ctypes.CDLL(out)                                                   # dlopen needs no GPU
    lib.go1feet_version.restype = ctypes.c_char_p
    assert lib.go1feet_version() == b"go1feet 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    assert g.library_stamp(os.path.join(REPO, "walk-these-ways_amd", "csrc", "libgo1eval.so")) in (None, g.source_hash(g.eval_sources(), g.EVAL_FLAGS))


def test_a_missing_library_fails_loudly(tmp_path):
    import go1feet_host as G
    with pytest.raises(G.Go1FeetLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1feet.so"))


# ---- 2. the refusals without a GPU (the helpers of tests/test_eval_return_codes.py) ----------------------------------------------------------
def feet_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.dt, c.terrain_friction, c.max_contact_force = 70, 2, 3, 0.02, 1.0, 100.0


FEET_ACC = ACCUMULATORS + F.STATE
BAD_CONFIG = [("dt = 0", -12, [cfg(dt=0.0)]), ("dt < 0", -12, [cfg(dt=-0.02)]), ("dt = inf", -12, [cfg(dt=INF)]), ("dt = NaN", -12, [cfg(dt=NAN)]),
              ("terrain_friction < 0", -12, [cfg(terrain_friction=-0.1)]), ("terrain_friction = inf", -12, [cfg(terrain_friction=INF)]),
              ("terrain_friction = NaN", -12, [cfg(terrain_friction=NAN)]), ("max_contact_force = NaN", -12, [cfg(max_contact_force=NAN)]),
              ("max_contact_force = -inf", -12, [cfg(max_contact_force=-INF)])]
CASES = {
    "go1feet_clear": nobody() + each(FEET_ACC, -2) + [
        ("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")])],
    "go1feet_accumulate": nobody() + each(FEET_ACC, -2) + each(F.INPUTS, -3) + BAD_CONFIG + [
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no profile_sum and no foot_indices", -2, [null("profile_sum", "foot_indices")]),
        ("no stance_valid and dt = 0", -2, [null("stance_valid"), cfg(dt=0.0)]),
        ("no friction_coeffs and dt = NaN", -3, [null("friction_coeffs"), cfg(dt=NAN)]),
        ("no prev_foot_velocities and terrain_friction < 0", -3, [null("prev_foot_velocities"), cfg(terrain_friction=-1.0)])],
    "go1feet_reduce": nobody() + each(FEET_ACC, -2) + [
        ("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group", "results", "profile_results"], -5) + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no resets and no profile_results", -2, [null("resets", "profile_results")]),
        ("no stance_slip and num_groups = 0", -2, [null("stance_slip"), cfg(num_groups=0)])],
}


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    """every case fails validation, so nothing is launched: there is no GPU.  The valid settings of good values (terrain_friction 0,
    a negative max_contact_force) are not refused: with an input missing they get as far as -3."""
    import __graft_entry__ as g
    import go1feet_host as G
    g.build_feet_hip()
    fn = getattr(G.load_library(), symbol)
    assert len({label for label, _, _ in CASES[symbol]}) == len(CASES[symbol])
    assert sum(len(spoilers) > 1 for _, _, spoilers in CASES[symbol]) >= 1          # two conditions at once: precedence
    for label, code, spoilers in CASES[symbol]:
        a = Call(G.Go1FeetConfig, G.Go1FeetBuffers, feet_base)
        for spoil in spoilers:
            spoil(a)
        assert fn(None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b), None) == code, (symbol, label)
    if symbol == "go1feet_accumulate":
        for good in (cfg(terrain_friction=0.0), cfg(max_contact_force=-5.0), cfg(max_contact_force=0.0)):
            a = Call(G.Go1FeetConfig, G.Go1FeetBuffers, feet_base)
            good(a)
            null("reset_buf")(a)
            assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -3
    else:                                                                    # the clear and the reduction read no input and no dt
        a = Call(G.Go1FeetConfig, G.Go1FeetBuffers, feet_base)
        null(*F.INPUTS)(a)
        cfg(dt=0.0, terrain_friction=NAN)(a)
        null("count")(a)
        assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -2


# ---- 3. the host-side definition against the reference's reward terms -------------------------------------------------------------------------
def ulps_apart(a, b):
    """how many fp32 values lie between the finite np.float32 arrays a and b, elementwise"""
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return np.abs(key(np.ascontiguousarray(a, f32)) - key(np.ascontiguousarray(b, f32)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_foot_terms_sum_to_the_reference_rewards(seed):
    from go1_gym_learn.eval_metrics import feet
    z = np.load(os.path.join(REPO, "tests", "golden", "foot_metrics.npz"))
    forces, prev = torch.from_numpy(z[f"s{seed}_in_contact_forces"]), torch.from_numpy(z[f"s{seed}_in_prev_foot_velocities"])
    limit = float(z["max_contact_force"])
    assert limit == 100.0 and z["feet_indices"].tolist() == [4, 8, 12, 16] and forces.shape == (64, 17, 3)
    rng = np.random.default_rng(seed)
    env = types.SimpleNamespace(num_envs=64, contact_forces=forces, prev_foot_velocities=prev, feet_indices=torch.tensor([4, 8, 12, 16]),
                                foot_velocities=torch.zeros(64, 4, 3), friction_coeffs=torch.from_numpy(rng.uniform(0.2, 2.0, (64, 1)).astype(f32)),
                                cfg=types.SimpleNamespace(rewards=types.SimpleNamespace(max_contact_force=limit)))
    terms = feet.foot_terms(env, terrain_friction=0.7)
    assert list(terms) == feet.FOOT_TERMS and all(t.shape == (64, 4) and t.dtype == torch.float32 for t in terms.values())
    for term, reward in (("force_excess", "feet_contact_forces"), ("impact_vel_sq", "feet_impact_vel")):
        got, want = terms[term].sum(dim=1).numpy(), z[f"s{seed}_out_{reward}"]
        assert got.tobytes() == want.tobytes(), (term, np.abs(got - want).max())
    # what the inputs were written to hold: feet in the air, forces beyond the limit, upward and downward speeds, speeds beyond the clip
    fn = torch.norm(forces[:, [4, 8, 12, 16], :], dim=-1).numpy()
    assert (fn < 1.0).any() and (fn > limit).any() and (prev[:, :, 2] > 0).any() and (prev[:, :, 2] < -100.0).any()
    assert (np.abs(fn - 1.0) > 1e-3).all() and (np.abs(fn - limit) > 1e-3).all()                 # the condition impact_vel_sq's equality rests on
    assert z[f"s{seed}_out_feet_contact_forces"].min() == 0.0 < z[f"s{seed}_out_feet_contact_forces"].max()
    # and the model's per-foot values are the same numbers: bit for bit where the expression has no norm; within the stated ulps where it has
    mcfg = F.config(terrain_friction=0.7, max_contact_force=limit)
    mu = f32(0.5) * (env.friction_coeffs[:, 0].numpy() + f32(0.7))
    worst = {}
    for f in range(4):
        fx, fy, fz = (np.ascontiguousarray(forces[:, 4 * (f + 1), k].numpy()) for k in range(3))
        c, _, values = F.step_values(mcfg, fx, fy, fz, np.zeros(64, f32), np.zeros(64, f32), np.ascontiguousarray(prev[:, f, 2].numpy()), mu)
        for name in ("contact", "force_normal", "impact_vel_sq", "touchdown_speed", "touchdown_force"):
            assert bits(values[name]) == bits(terms[name][:, f].numpy()), (name, f)
        # force_excess: one rounding of the sum of squares, one of the square root and torch.norm's own half ulp: at most 2 ulps OF fn
        with np.errstate(all="ignore"):
            model_fn = np.sqrt((fx * fx + fy * fy) + fz * fz)
        gap = np.abs(values["force_excess"].astype(np.float64) - terms["force_excess"][:, f].numpy().astype(np.float64))
        assert (gap <= 2.0 * np.spacing(model_fn).astype(np.float64)).all(), (f, gap.max())
        assert ((values["force_excess"] > 0) == (terms["force_excess"][:, f].numpy() > 0)).all()
        worst["force_excess [ulps of fn]"] = max(worst.get("force_excess [ulps of fn]", 0.0), float((gap / np.spacing(model_fn)).max()))
        # force_tangent: the same budget in its own ulps; friction_use: that error through one division, one ulp more
        worst["force_tangent [ulps]"] = max(worst.get("force_tangent [ulps]", 0), int(ulps_apart(values["force_tangent"], terms["force_tangent"][:, f].numpy()).max()))
        worst["friction_use [ulps]"] = max(worst.get("friction_use [ulps]", 0), int(ulps_apart(values["friction_use"][c], terms["friction_use"][:, f].numpy()[c]).max()))
    print(f"\nseed {seed}: largest difference between the model and foot_terms: {worst}")
    assert worst["force_tangent [ulps]"] <= 2 and worst["friction_use [ulps]"] <= 3


def test_total_mass_is_the_model_datas():
    from go1_gym_learn.eval_metrics import feet
    assert abs(feet.total_mass() - (4.801 + 4 * (0.510299 + 0.898919 + 0.218015))) < 1e-9


# ---- 4. the model by hand ---------------------------------------------------------------------------------------------------------------------
def snap_of(fz, fx=0.0, fy=0.0, vx=0.0, vy=0.0, pvz=0.0, ph=0.5, mu=1.0, reset=0, age=5):
    """one environment whose four feet all carry the same values"""
    s = dict(contact_forces=np.zeros((51, 1), f32), foot_velocities=np.zeros((12, 1), f32), prev_foot_velocities=np.zeros((12, 1), f32),
             foot_indices=np.full((4, 1), ph, f32), friction_coeffs=np.array([mu], f32), reset_buf=np.array([reset], np.uint8),
             episode_length_buf=np.array([age], np.int32))
    for f in range(4):
        s["contact_forces"][12 * (f + 1):12 * (f + 1) + 3, 0] = (fx, fy, fz)
        s["foot_velocities"][3 * f:3 * f + 2, 0] = (vx, vy)
        s["prev_foot_velocities"][3 * f + 2, 0] = pvz
    return s


def play(cfg_, steps):
    st = F.State(1)
    for kw in steps:
        F.accumulate(st, cfg_, snap_of(**kw))
    return st


def folded(st, f=0):
    """{metric: (count, nonfinite, min, max)} of foot f of environment 0"""
    return {name: (int(st.count[f * F.M + m, 0]), int(st.nonfinite[f * F.M + m, 0]), float(st.min[f * F.M + m, 0]), float(st.max[f * F.M + m, 0]))
            for m, name in enumerate(F.METRICS)}


NOTHING = (0, 0, INF, -INF)
STANCE = [dict(fz=0.0), dict(fz=0.5, pvz=-0.25),                                   # unknown -> air, air
          dict(fz=40.0, fx=3.0, fy=4.0, vx=0.3, vy=0.4, pvz=-1.5, ph=0.0625),      # touchdown
          dict(fz=80.0, fx=6.0, fy=8.0, vx=0.0, vy=0.5, pvz=0.2), dict(fz=60.0, vx=0.25), dict(fz=20.0),      # three stance steps
          dict(fz=0.25)]                                                           # lift-off


def test_model_a_scripted_stance():
    dt = f32(0.02)
    st = play(F.config(), STANCE)
    got = folded(st, 2)
    one = lambda v: (1, 0, float(v), float(v))
    assert got["contact"] == (7, 0, 0.0, 1.0) and st.sum[2 * F.M + F.CONTACT, 0] == 4.0                      # duty factor 4 / 7
    assert got["force_normal"] == (4, 0, 20.0, 80.0) and got["force_tangent"] == (4, 0, 0.0, 10.0)
    assert got["friction_use"] == (4, 0, 0.0, 0.125) and st.sum[2 * F.M + F.FRICTION_USE, 0] == 0.25         # mu = 0.5 (1 + 1) = 1
    assert got["force_excess"] == (7, 0, 0.0, 0.0)
    assert got["impact_vel_sq"] == (7, 0, 0.0, 2.25)                                                         # only on the touchdown step: fn > 1, pvz < 0
    assert got["touchdown_speed"] == one(1.5) and got["touchdown_force"] == one(40.0)
    impulse = ((f32(40.0) * dt + f32(80.0) * dt) + f32(60.0) * dt) + f32(20.0) * dt
    first = np.sqrt(f32(0.3) * f32(0.3) + f32(0.4) * f32(0.4))
    slip = ((first * dt + f32(0.5) * dt) + f32(0.25) * dt) + f32(0.0) * dt
    assert got["stance_peak_force"] == one(80.0) and got["stance_impulse"] == one(impulse) and got["stance_slip"] == one(slip)
    assert got["stance_time"] == one(f32(4.0) * dt)
    assert (st.prev_contact == F.AIR).all() and (st.stance_valid == 0).all() and (st.stance_steps == 4).all()
    assert folded(st, 0) == got and st.steps[0] == 7 and st.resets[0] == 0
    assert st.profile_count[0, :, 0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 6] + [0] * 7 and st.profile_sum[0, 1, 0] == 40.0 and st.profile_sum[0, 8, 0] == 160.75
    heavy = play(F.config(max_contact_force=50.0), [dict(fz=80.0, fx=6.0, fy=8.0)])
    fn = np.sqrt(f32(100.0) + f32(6400.0))
    assert folded(heavy)["force_excess"] == one(fn - f32(50.0)) and folded(heavy)["touchdown_force"] == NOTHING      # first contact seen from unknown


def test_model_a_reset_inside_the_stance_folds_nothing():
    steps = STANCE[:4] + [dict(fz=60.0, reset=1, age=0)] + STANCE[5:]
    st = play(F.config(), steps)
    got = folded(st)
    assert all(got[m] == NOTHING for m in F.METRICS[8:]) and got["touchdown_force"][0] == 1 and got["contact"][0] == 6
    assert (st.steps[0], st.resets[0]) == (7, 1) and (st.prev_contact == F.AIR).all()
    after = play(F.config(), steps[:5])
    assert (after.prev_contact == F.UNKNOWN).all() and (after.stance_valid == 0).all() and (after.stance_steps == 2).all()     # the other words keep what they hold
    more = play(F.config(), steps + STANCE[2:])                                                               # the next stance is seen whole
    assert folded(more)["stance_time"] == (1, 0, float(f32(4.0) * f32(0.02)), float(f32(4.0) * f32(0.02))) and folded(more)["touchdown_force"][0] == 2


def test_model_a_stance_begun_in_the_warm_up_is_never_folded():
    ages = [1, 2, 3, 4, 5, 6, 7]                                                     # warm-up 3: the touchdown step (age 3) is still warm-up
    st = play(F.config(warmup_steps=3), [dict(kw, age=a) for kw, a in zip(STANCE, ages)])
    got = folded(st)
    assert got["contact"] == (4, 0, 0.0, 1.0) and got["touchdown_force"] == NOTHING and all(got[m] == NOTHING for m in F.METRICS[8:])
    assert st.steps[0] == 7 and st.profile_count[0, :, 0].sum() == 4
    st = play(F.config(warmup_steps=3), [dict(kw, age=a) for kw, a in zip(STANCE, ages)] + [dict(kw, age=8 + k) for k, kw in enumerate(STANCE[2:])])
    assert folded(st)["stance_peak_force"] == (1, 0, 80.0, 80.0)


def test_model_nan_force_and_no_friction():
    st = play(F.config(), STANCE[:4] + [dict(fz=NAN)])                                 # a NaN compares false: in the air, so a lift-off
    got = folded(st)
    assert got["contact"] == (5, 0, 0.0, 1.0) and got["stance_time"][0] == 1 and got["stance_peak_force"] == (1, 0, 80.0, 80.0)
    assert got["force_excess"][:2] == (4, 1) and got["impact_vel_sq"] == (5, 0, 0.0, 2.25) and st.profile_count[0, :, 0].sum() == 4
    assert np.isfinite(st.sum).all() and np.isfinite(st.profile_sum).all()
    st = play(F.config(terrain_friction=0.0), [dict(fz=0.0, mu=0.0), dict(fz=40.0, fx=3.0, mu=0.0), dict(fz=40.0, mu=0.0)])
    got = folded(st)                                                                   # mu = 0: 3 / 0 = inf, then 0 / 0 = NaN: both counted, none summed
    assert got["friction_use"] == (0, 2, INF, -INF) and got["force_tangent"] == (2, 0, 0.0, 3.0) and got["touchdown_force"][0] == 1
    st = play(F.config(), [dict(fz=0.0), dict(fz=INF), dict(fz=0.0)])                  # an infinite load: counted in nonfinite of what it enters
    got = folded(st)
    assert got["force_normal"][:2] == (0, 1) and got["stance_peak_force"][:2] == (0, 1) and got["stance_time"] == (1, 0, float(f32(0.02)), float(f32(0.02)))
    assert st.profile_count[0, :, 0].sum() == 2


def test_model_phase_bins():
    ph = np.array([0.0, 0.0625, 0.9999999, 1.0, -0.1, 0.5, 0.99, 16.0, 1e30, -1e30, -0.0], f32)
    assert F.phase_bin(ph).tolist() == [0, 1, 15, 15, 0, 8, 15, 15, 15, 0, 0]
    for value, want in ((0.0, 0), (0.0625, 1), (0.9999999, 15), (1.0, 15), (-0.1, 0), (NAN, None), (INF, None)):
        st = play(F.config(), [dict(fz=30.0, ph=value)])
        assert st.profile_count[1, :, 0].tolist() == [1 if k == want else 0 for k in range(16)], value
    table, profile = F.reduce(play(F.config(), STANCE), [0], 2)
    assert table.shape == (2, 49, 6) and profile.shape == (2, 4, 16, 2)
    assert table[0, 48].tolist() == [1.0, 7.0, 0.0, 0.0, 0.0, 0.0] and table[1, 48].tolist() == [0.0] * 6
    assert profile[0, 3, 8].tolist() == [160.75, 6.0] and profile[0, 3, 1].tolist() == [40.0, 1.0] and not profile[1].any()
    assert table[0, 3 * F.M + F.CONTACT].tolist()[:2] == [7.0, 4.0 / 7.0] and np.isnan(table[1, :48, 1:5]).all()


# ---- 5. go1feet.hip under the SIMT emulator against the model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1feet_host as G
    return G.load_library(build_emu(g.feet_sources(), "libgo1feet_emu.so"))


def feet_on(device, cfg_, N, lib=None):
    """a go1feet_host.Go1Feet on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1feet_host as G
    shapes = dict(contact_forces=(51, N), foot_velocities=(12, N), prev_foot_velocities=(12, N), foot_indices=(4, N), friction_coeffs=(N,))
    tensors = {k: torch.zeros(*shape, device=device) for k, shape in shapes.items()}
    tensors.update(reset_buf=torch.zeros(N, dtype=torch.uint8, device=device), episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    S = types.SimpleNamespace(num_envs=N, terrain_friction=cfg_.terrain_friction, max_contact_force=cfg_.max_contact_force)
    fm = G.Go1Feet(S, B, cfg_.dt, lib=lib)
    if torch.device(device).type == "cpu":
        fm._stream = lambda: None
    return fm, B


def feet_groups(rng, N, groups=3):
    """three groups of which group 1 is empty, some environments at -1 and (from three environments on) one id outside the tables"""
    assert groups == 3
    group = rng.integers(-1, groups, N).astype(np.int32)
    group[group == 1] = 2
    group[0] = groups - 1
    if N >= 3:
        group[1], group[2] = -1, groups
    return group


def drive(fm, B, cfg_, snaps, group, groups):
    """the scripted steps through the library: arm for `groups` groups, upload a snapshot, accumulate, ...; returns read() and the
    accumulators.  arm() sizes the tables by the largest id it is given, so the ids outside the tables are handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    fm.arm(inside, cfg_.warmup_steps)
    fm.group.copy_(torch.from_numpy(group))
    for s in snaps:
        for k, a in s.items():
            getattr(B, k).copy_(torch.from_numpy(a))
        fm.accumulate()
    fm.disarm()
    res = fm.read()
    acc = {k: t.cpu().numpy() for k, t in fm.acc.items()}
    return res, acc


def check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N):
    """accumulators, state, profile and the three result tables against tests/feet_ref.py, bit for bit; then what the script was
    written to drive"""
    st = F.run(cfg_, snaps, N)
    for k in ACCUMULATORS:
        assert acc[k].shape == (48, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in F.STATE:
        name = "env_" + k if k.startswith("profile") else k
        assert res[name].shape == getattr(st, k).shape and bits(res[name].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    want, want_profile = F.reduce(st, group, groups)
    table = np.concatenate([np.stack([res["metrics"][m] for m in F.METRICS], axis=2).reshape(groups, 48, 6), np.zeros((groups, 1, 6))], axis=1)
    table[:, 48, :3] = res["groups"]
    assert table.shape == want.shape == (groups, F.ROWS, 6)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and bits(table) == bits(want)
    assert res["profile_sum"].shape == (groups, 4, 16) and bits(np.stack([res["profile_sum"], res["profile_count"]], axis=-1)) == bits(want_profile)
    with np.errstate(all="ignore"):
        mean = np.where(want_profile[..., 1] > 0, want_profile[..., 0] / want_profile[..., 1], np.nan)
    assert np.array_equal(np.isnan(res["profile"]), np.isnan(mean)) and bits(res["profile"]) == bits(mean) and res["phase_edges"].tolist() == [k / 16 for k in range(17)]
    steps = len(snaps)
    count, nonfinite = st.count.reshape(4, 12, N), st.nonfinite.reshape(4, 12, N)
    assert (res["steps"] == steps).all()
    if N >= len(F.KINDS):
        # events on every foot: touchdowns and completed stances, of more than one length; a reset or the warm-up breaks them
        assert (count[:, F.TOUCHDOWN_FORCE, kind == 0].sum(axis=1) > 0).all() and (count[:, F.STANCE_TIME, kind == 0].sum(axis=1) > 0).all()
        assert len(set(st.max.reshape(4, 12, N)[:, F.STANCE_TIME][count[:, F.STANCE_TIME] > 0].tolist())) >= 2
        assert (res["resets"][kind == 1] >= 4).all() and snaps[0]["reset_buf"][kind == 1].all()
        assert (count[:, F.CONTACT, kind == 1] <= 2).all() and count[:, F.CONTACT].max() == steps - cfg_.warmup_steps
        assert (count[:, F.STANCE_TIME, kind == 1] == 0).all()
        # the heavy ones went beyond max_contact_force and beyond the clip of the impact speed (100^2)
        assert st.max.reshape(4, 12, N)[:, F.FORCE_EXCESS, kind == 2].max() > 100.0 and st.max.reshape(4, 12, N)[:, F.IMPACT_VEL_SQ, kind == 2].max() == 10000.0
        # the threshold: 1.0 and one ulp below it are in the air, one ulp above it is on the ground
        normal = st.min.reshape(4, 12, N)[:, F.FORCE_NORMAL, kind == 3]
        assert normal.min() == np.nextafter(f32(1.0), f32(2))
        # +-inf and NaN were met and entered no sum
        odd = kind == 4
        assert nonfinite[:, [F.FORCE_EXCESS, F.IMPACT_VEL_SQ], :][:, :, odd].sum() > 0 and np.isfinite(st.sum).all() and np.isfinite(st.profile_sum).all()
        assert (st.profile_count.sum(axis=1)[:, odd] < count[:, F.CONTACT, odd]).any()
        # a robot that stands: one unobserved stance, never folded; contact on every folded step
        stands = kind == 5
        assert (count[:, F.TOUCHDOWN_FORCE:, stands] == 0).all() and (st.min.reshape(4, 12, N)[:, F.CONTACT, stands][count[:, F.CONTACT, stands] > 0] == 1.0).all()
        # no friction of its own on a ground with some is finite; the phases outside [0, 1) landed in the end bins
        assert nonfinite[:, F.FRICTION_USE, kind == 6].sum() == 0 and st.profile_count[:, 15, kind == 6].sum() > 0
        quiet = ~odd & (kind != 6)
        assert (st.profile_count.sum(axis=1)[:, quiet] == count[:, F.CONTACT, quiet]).all()
    g = res["groups"]
    assert g[:, 0].sum() == np.isin(group, range(groups)).sum() and (g[:, 1] == steps * g[:, 0]).all() and g[1].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(want[1, :48, 1:5]).all() and not want_profile[1].any()
    return st


# 1: one thread; 64: one wavefront; 257: two blocks per foot with a ragged tail (the block-to-foot mapping); 600: three terms per
# reduction thread and 38 environments per profile slice
SHAPES = [1, 64, 257, 600]


@pytest.mark.parametrize("N", SHAPES)
def test_emulated_feet_kernels_follow_the_model(emu, N):
    groups = 3
    rng = np.random.default_rng(300 + N)
    cfg_, snaps, kind = F.scripted_steps(rng, N)
    assert len(snaps) == 12 and (N < len(F.KINDS) or set(kind.tolist()) == set(range(len(F.KINDS))))
    group = feet_groups(rng, N, groups)
    fm, B = feet_on("cpu", cfg_, N, lib=emu)
    res, acc = drive(fm, B, cfg_, snaps, group, groups)
    assert fm.cfg.num_groups == groups and (N < 3 or {-1, groups} <= set(group.tolist()))
    check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N)
    with pytest.raises(RuntimeError, match="go1feet_accumulate failed: -12"):
        fm.cfg.dt = 0.0
        fm.accumulate()


# ---- 6. the environment hooks without a GPU ---------------------------------------------------------------------------------------------------
def test_foot_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    monkeypatch.delitem(sys.modules, "go1eval_host", raising=False)
    monkeypatch.delitem(sys.modules, "go1feet_host", raising=False)
    c = apply_train_config(make_cfg(), num_envs=16)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_foot_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_foot_metrics, env.read_foot_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert "go1eval_host" not in sys.modules and "go1feet_host" not in sys.modules and env._feet is None     # never measured: neither host module
    env.step(torch.zeros(16, 12))                                             # and stepping goes on


# ---- 6b. the two scenarios of the GPU tests, through the fp64 oracle here ----------------------------------------------------------------------
STANDING_D = -0.0365     # the oracle's relative deviation of the standing robot's vertical load from its weight (the test below pins it)
TROT_PERIOD = 20         # policy steps of one cycle of the scripted trot: 0.4 s


def standing_env(N, device, seed=7):
    """the training configuration on the plane without gravity randomisation (the weight is to be compared with mass x 9.81), 20 s episodes"""
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    c = apply_train_config(make_cfg(), num_envs=N)
    c.terrain.mesh_type = "plane"
    c.env.episode_length_s = 20.0
    c.domain_rand.randomize_gravity = False
    torch.manual_seed(seed)
    np.random.seed(seed)
    return VelocityTrackingEasyEnv(sim_device=device, headless=True, cfg=c)


def trot_action(step, N):
    """(N, 12) actions of a trot-like script: the diagonal pair FL + RR folds its legs (thigh forward, knee bent: the foot leaves the
    ground) during the first half of every cycle, FR + RL during the second; a quarter of the robots runs the cycle half a period
    late, and the lift grows a little with the environment's index, so the feet's events fall on different steps"""
    env = torch.arange(N)
    phase = (step + (env % 4 == 3) * (TROT_PERIOD // 2)) % TROT_PERIOD
    first = phase < TROT_PERIOD // 2
    lift = 1.0 + 0.5 * (env % 8) / 8.0
    action = torch.zeros(N, 12)
    for leg, with_first in ((0, True), (1, False), (2, False), (3, True)):
        up = (first if with_first else ~first).float() * lift
        action[:, 3 * leg + 1] = 2.0 * up
        action[:, 3 * leg + 2] = -4.0 * up
    return action


def oracle_rollout(env, actions, warmup_steps):
    """the model of tests/feet_ref.py replayed on the buffers after every step of `actions` (an iterable of (N, 12) tensors)"""
    S, N = env.sim_config, env.num_envs
    cfg_ = F.config(dt=float(env.dt), terrain_friction=float(S.terrain_friction), max_contact_force=float(S.max_contact_force), warmup_steps=warmup_steps)
    st = F.State(N)
    for action in actions:
        env.step(action)
        F.accumulate(st, cfg_, {n: getattr(env.buffers, n).cpu().numpy().copy() for n in F.INPUTS})
    return st


def test_standing_robot_through_the_oracle(monkeypatch):
    """the scenario of test_gpu_foot_metrics.test_a_standing_robot_loads_its_feet_with_its_weight on the CPU oracle, which reports the
    same one substep in four: where STANDING_D, the margin of that test, comes from"""
    import fake_sim
    from go1_gym_learn.eval_metrics import feet
    fake_sim.install(monkeypatch)
    N, WARMUP, STEPS = 64, 50, 100
    env = standing_env(N, "cuda:0")
    env.reset()
    st = oracle_rollout(env, (torch.zeros(N, 12) for _ in range(WARMUP + STEPS)), WARMUP)
    _, profile = F.reduce(st, np.zeros(N, np.int32), 1)
    assert st.resets.sum() == 0 and (profile[0, :, :, 1].sum(axis=1) == N * (STEPS + 1)).all()
    load = (profile[0, :, :, 0].sum(axis=1) / profile[0, :, :, 1].sum(axis=1)).sum()
    weight = (feet.total_mass() + float(env.payloads.mean())) * 9.81
    d = load / weight - 1.0
    print(f"\noracle: vertical load {load:.3f} N against a weight of {weight:.3f} N: d = {100.0 * d:+.3f} %")
    assert abs(d - STANDING_D) < 5e-4


def test_the_trot_script_produces_events_on_the_oracle(monkeypatch):
    """the scenario of test_gpu_foot_metrics.test_feet_through_the_environment on the CPU oracle: the script is there to produce
    touchdowns and completed stances on every foot"""
    import fake_sim
    from test_gpu_response_trace import make_env
    fake_sim.install(monkeypatch)
    N, STEPS, WARMUP = 64, 80, 2
    env = make_env(N, "plane", 20.0, seed=4)
    env.reset()
    st = oracle_rollout(env, (trot_action(step, N) for step in range(STEPS)), WARMUP)
    count = st.count.reshape(4, 12, N)
    touchdowns, stances = count[:, F.TOUCHDOWN_FORCE].sum(axis=1), count[:, F.STANCE_TIME].sum(axis=1)
    print(f"\noracle: touchdowns per foot {touchdowns.tolist()}, completed stances per foot {stances.tolist()}, resets {int(st.resets.sum())}")
    assert (touchdowns >= N // 2).all() and (stances >= N // 2).all()


# ---- 7. the sweep's host pieces and the tool --------------------------------------------------------------------------------------------------
def fixed_result():
    import go1feet_host as G
    row = lambda mean, top: np.array([[[30.0, mean, 0.5, 0.0, top, 0.0]] * 4, [[10.0, 2 * mean, 0.5, 0.0, 2 * top, 1.0]] * 4])
    feet = {m: row(0.25, 2.0) for m in F.METRICS}
    feet["contact"], feet["force_normal"], feet["stance_peak_force"] = row(0.5, 1.0), row(50.0, 90.0), row(70.0, 100.0)
    feet["stance_slip"][1] = [[0.0, NAN, NAN, NAN, NAN, 0.0]] * 4             # a cell that completed no stance
    profile = np.zeros((2, 4, 16))
    profile[:, :, :8] = [[[60.0], [40.0], [30.0], [20.0]]] * 2                # stance in the first half of the cycle
    count = np.full((2, 4, 16), 5.0)
    profile[1, :, 15], count[1, :, 15] = NAN, 0.0
    return dict(preset="static_medium", cells=[(0.5, 0.0, (0.5, 0.0, 0.0)), (1.0, 0.0, (0.5, 0.0, 0.0))], feet=feet,
                feet_groups=np.array([[8.0, 320.0, 1.0], [8.0, 320.0, 0.0]]), profile=profile, profile_count=count, phase_edges=G.phase_edges(),
                metrics={}, groups=np.zeros((2, 5)), body_weight=100.0, terrain_friction=1.0, max_contact_force=100.0, foot_names=list(G.FOOT_NAMES),
                num_envs=16, steps=40, warmup_steps=5, seed=1, dt=0.02)


def test_foot_table_json_and_figure(tmp_path):
    from go1_gym_learn.eval_metrics import feet
    res = fixed_result()
    shares = feet.load_shares(res["profile"], res["profile_count"])
    assert shares.shape == (2, 4) and np.allclose(shares[0], [0.4, 4 / 15, 0.2, 2 / 15]) and np.allclose(shares.sum(axis=1), 1.0)
    md = feet.foot_markdown_table(res).splitlines()
    assert md[0].startswith("| vx | yaw | foot | duty | mean Fz [N] | mean Fz [BW] | peak Fz [N] | peak Fz [BW] | mean friction use |") and len(md) == 2 + 8
    assert md[0].count("|") == md[1].count("|") == md[2].count("|") == 18
    assert md[2] == "| 0.5 | 0 | FL | 0.500 | 50.0 | 0.500 | 90.0 | 0.900 | 0.250 | 2.000 | 0.250 | 2.000 | 0.25 | 0.2500 | 0.400 | 0.667 | 0.600 |"
    assert md[3].startswith("| 0.5 | 0 | FR | 0.500 |") and md[3].endswith("| 0.267 |  |  |") and "| – |" in md[6]
    js = json.loads(json.dumps(feet.foot_to_json(res), allow_nan=False))
    assert js["cells"][1] == dict(vx=1.0, yaw=0.0, gait=[0.5, 0.0, 0.0]) and js["group_fields"] == F.GROUP_FIELDS and js["foot_names"] == ["FL", "FR", "RL", "RR"]
    assert js["feet"]["force_normal"][0][3][1] == 50.0 and js["feet"]["stance_slip"][1][0][1] is None and js["profile"][1][0][15] is None
    assert np.array(js["profile_count"]).shape == (2, 4, 16) and len(js["phase_edges"]) == 17 and js["body_weight"] == 100.0 and len(js["load_share"][0]) == 4
    path = tmp_path / "grf.png"
    feet.plot_grf(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000


def test_tool_accepts_a_foot_sweep(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import feet
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--feet", "--vx", "0.5", "1.0", "--envs", "16", "--steps", "40", "--warmup-steps", "5", "--presets", "static_medium"])
    assert a.feet and not a.joints and not a.tiles and (a.vx, a.envs, a.steps, a.terrain) == ([0.5, 1.0], 16, 40, None)
    assert not eval_sweep.parse_args(base).feet and eval_sweep.parse_args(base + ["--feet", "--terrain", "plane"]).terrain == "plane"
    for bad in (["--feet", "--terrain"], ["--feet", "--behaviour"], ["--feet", "--joints"], ["--feet", "--response", "--switch", "vx", "0", "1"],
                ["--feet", "--push", "--magnitude", "1", "--direction", "0"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(base + bad)
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(feet, "run_foot_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    eval_sweep.run_feet(a, None, dict(vx=a.vx, yaw=a.yaw, gait=[(0.5, 0.0, 0.0)]))
    assert seen == dict(preset="static_medium", grid=dict(vx=[0.5, 1.0], yaw=[0.0], gait=[(0.5, 0.0, 0.0)]), num_envs=16, steps=40, warmup_steps=5, seed=1,
                        terrain=None)
    js = json.load(open(tmp_path / "eval" / "static_medium_feet.json"))
    assert js["preset"] == "static_medium" and js["profile"][0][0][0] == 60.0
    md = (tmp_path / "eval" / "static_medium_feet.md").read_text()
    assert "| 0.5 | 0 | FL | 0.500 | 50.0 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_grf.png").read_bytes()[:4] == b"\x89PNG"
