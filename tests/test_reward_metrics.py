"""CPU checks of the reward family (include/go1reward.h, libgo1reward.so): the ctypes mirrors and the exported symbols against the
header, the build's source list, flags and stamp, the refusals, go1reward.hip itself under the SIMT emulator against the reference's
golden maps fixtures and against the fp64 model of tests/reward_ref.py, the model's bookkeeping on hand-made steps, the kernel's
independence of where an environment sits, the fixed-order group table bit for bit, the environment hooks where there is no GPU, the
sweep's host pieces and the tool, and the scripted trot of the GPU test through the oracle."""
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

import reward_ref as R
from golden.variants import FUZZ_VARIANTS
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from util import build_emu, load_maps_fixture, make_sim, maps_fixture_stream, maps_keep

HEADER = os.path.join(REPO, "include", "go1reward.h")
CSRC = os.path.join(REPO, "walk-these-ways_amd", "csrc")
SOURCE = os.path.join(CSRC, "go1reward.hip")
NAN, INF = float("nan"), float("inf")
f32, f64 = np.float32, np.float64
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]
STATE = ["snap_last_last_actions", "snap_last_last_joint_pos_target", "snap_last_dof_vel", "snap_last_contacts", "last_raw", "last_scaled",
         "last_valid", "measured", "resets", "teleported"]
MAPS = [("train", "maps_train.npz"), ("alt", "maps_alt_mild.npz"), ("alt2", "maps_alt2.npz"), ("alt2", "maps_alt2_mild.npz"),
        ("train_noise", "maps_train_noise_mild.npz")] + [(f"fuzz{k}", f"maps_fuzz{k}_mild.npz") for k in range(FUZZ_VARIANTS)]
# (the parametrisation of test_emu_parity.test_emulated_post_physics_maps_match_reference_golden)


# ---- 1. mirrors, symbols, sources, flags, stamp ---------------------------------------------------------------------------------------------
def test_reward_mirrors_match_the_header():
    import go1eval_host as E
    import go1reward_host as G
    src = open(HEADER).read()
    for macro, value in (("GO1REWARD_EXTRA_ROWS", 4), ("GO1REWARD_NUM_FIELDS", 6), ("GO1REWARD_REDUCE_THREADS", 256),
                         ("GO1REWARD_ENVS_PER_BLOCK", G.ENVS_PER_BLOCK), ("GO1REWARD_TELEPORT_DISTANCE", G.TELEPORT_DISTANCE)):
        assert re.search(rf"#define {macro} {value}\n", src), macro
    assert G.TELEPORT_DISTANCE == R.TELEPORT_DISTANCE and G.ENVS_PER_BLOCK == 64
    want = struct_fields(src, "Go1RewardConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1RewardConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "num_rewards"]
    assert all(C_TYPES[ctext] is ctype for (_, ctext), (_, ctype) in zip(want, G.Go1RewardConfig._fields_)) and ctypes.sizeof(G.Go1RewardConfig) == 16
    want = struct_fields(src, "Go1RewardBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1RewardBuffers._fields_] == ACCUMULATORS + STATE + ["group", "results", "group_results"]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1RewardBuffers._fields_)
    types_ = dict(want)
    assert types_["snap_last_contacts"] == types_["last_valid"] == "uint8_t*" and types_["last_raw"] == types_["snap_last_dof_vel"] == "float*"
    assert types_["results"] == types_["group_results"] == "double*" and types_["measured"] == types_["teleported"] == "uint32_t*"
    assert enum_order(src, "Go1RewardExtraRow", "GO1REWARD_X_") == list(G.REWARD_EXTRA_ROWS) == R.EXTRA
    assert enum_order(src, "Go1RewardGroupField", "GO1REWARD_G_") == G.REWARD_GROUP_FIELDS == R.GROUP_FIELDS
    assert enum_order(src, "Go1RewardField", "GO1REWARD_F_") == E.FIELD_NAMES
    assert issubclass(G.Go1Reward, E._Table) and G.REWARD_EXTRA_ROWS == ("sum", "positive", "negative", "total")
    # the model's term names are the simulator's reward ids, and what the kernel reads is what the model's test data fills
    import go1sim_abi as abi
    assert [n for n, _ in sorted(abi.REWARD_IDS.items(), key=lambda p: p[1])] == R.TERMS and len(R.TERMS) == 24
    assert set(G.SIM_INPUTS) | {"measured_heights"} == set(R.BUFFERS)


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1reward_host as G
    declared = set(re.findall(r"\b(go1reward_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1reward_create", "go1reward_destroy", "go1reward_arm", "go1reward_snapshot",
                                                   "go1reward_accumulate", "go1reward_reduce", "go1reward_version"}
    out = g.build_reward_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1reward_" in line} == declared
    assert not re.search(r"\bgo1(eval|feet|trunk|sim|state)_\w+", dynamic)


def test_sources_flags_and_stamp():
    import inspect
    import __graft_entry__ as g
    names = [os.path.basename(p) for p in g.reward_sources()]
    assert names == ["go1reward.hip", "go1_maps.h", "go1_math.h", "go1_tables.h", "go1reward.h", "go1sim.h"] and all(os.path.exists(p) for p in g.reward_sources())
    # the step kernel's flags, not the metric libraries': the point is its arithmetic, contraction included
    assert g.REWARD_FLAGS == g.SIM_FLAGS and g.REWARD_FLAGS is not g.SIM_FLAGS and "-ffp-contract=off" not in g.REWARD_FLAGS and g.REWARD_FLAGS != g.EVAL_FLAGS
    code = re.sub(r"//.*", "", open(SOURCE).read())
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["../../include/go1reward.h", "go1_maps.h", "go1_tables.h"]
    for fn in ("load_reward_inputs", "reward_partial", "reward_raw_sign", "hf_sample_min3", "quad_sum", "clear_rows", "fold", "reduce_metric_row", "GO1_TABLES_MATCH"):
        assert re.search(rf"\b{fn}\(", code), fn
    assert not re.search(r"\bcase GO1_REW_|\bexpf\(-|erff\(", code)            # the terms are not written a third time (expf: the ji22 clip alone)
    assert code.count("expf(") == 1
    out = g.build_reward_hip()
    assert os.path.basename(out) == "libgo1reward.so" and g.library_stamp(out) == g.source_hash(g.reward_sources(), g.REWARD_FLAGS)
    lib = ctypes.CDLL(out)                                                   # dlopen needs no GPU
    lib.go1reward_version.restype = ctypes.c_char_p
    assert lib.go1reward_version() == b"go1reward 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    assert "build_reward_hip()" in inspect.getsource(g.build) and "libgo1reward.so" in inspect.getsource(g.smoke)
    # the simulator's sources and stamp are what they were: this family changed no file of theirs
    assert [os.path.basename(p) for p in g.sim_sources()] == ["go1sim.hip", "go1_math.h", "go1_maps.h", "go1_physics.h", "go1_model_data.h", "go1_actuator_data.h", "go1sim.h"]
    assert g.library_stamp(os.path.join(CSRC, "libgo1sim.so")) in (None, g.source_hash(g.sim_sources(), g.SIM_FLAGS))


def test_a_missing_library_fails_loudly(tmp_path):
    import go1reward_host as G
    with pytest.raises(G.Go1RewardLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1reward.so"))


# ---- the library under the SIMT emulator ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1reward_host as G
    return G.load_library(build_emu(g.reward_sources(), "libgo1reward_emu.so"))


def family(S, B, lib, names=None):
    """a go1reward_host.Go1Reward on CPU buffers, as the environment would build it"""
    import go1reward_host as G
    fam = G.Go1Reward(S, B, names, lib=lib)
    fam._stream = lambda: None
    return fam


def test_validation_codes_and_their_precedence(emu):
    """every code of include/go1reward.h short of the device's own (-10, -12, -13, -20): the emulator's allocations and launches do not
    fail.  Without a GPU the shipped library refuses what needs none: a missing handle, config or simulator, and a num_rewards of 0."""
    import __graft_entry__ as g
    import go1reward_host as G
    cfg_, S, meta, B = make_sim("train", 8)
    K = int(S.num_rewards)
    real = G.load_library(g.build_reward_hip())
    for lib in (real, emu):
        h = ctypes.c_void_p()
        assert lib.go1reward_create(None, ctypes.byref(B.struct), 0, ctypes.byref(h)) == -1
        assert lib.go1reward_create(ctypes.byref(S), None, 0, ctypes.byref(h)) == -1
        assert lib.go1reward_create(ctypes.byref(S), ctypes.byref(B.struct), 0, None) == -1
        for bad in (0, -1, 33):
            S.num_rewards = bad
            assert lib.go1reward_create(ctypes.byref(S), ctypes.byref(B.struct), 0, ctypes.byref(h)) == -1, bad        # a num_rewards of 0 is refused
        S.num_rewards, S.num_envs = K, 0
        assert lib.go1reward_create(ctypes.byref(S), ctypes.byref(B.struct), 0, ctypes.byref(h)) == -1
        S.num_envs = 8
        g3 = (ctypes.c_float * 3)(0.0, 0.0, -9.8)
        assert lib.go1reward_destroy(None) == lib.go1reward_snapshot(None, None) == lib.go1reward_reduce(None, None) == -1
        assert lib.go1reward_accumulate(None, g3, None) == lib.go1reward_arm(None, None, None, None) == -1
    fam = family(S, B, emu)
    lib, h = emu, fam.handle
    g3 = (ctypes.c_float * 3)(0.0, 0.0, -9.8)
    # before the first arm the handle has no config: -1
    assert lib.go1reward_snapshot(h, None) == lib.go1reward_accumulate(h, g3, None) == lib.go1reward_reduce(h, None) == -1
    fam.arm(np.zeros(8, np.int32))
    assert lib.go1reward_accumulate(h, None, None) == -1

    def arm(spoil_cfg=None, spoil_buf=(), no_cfg=False, no_buf=False):
        c, b = G.Go1RewardConfig(), G.Go1RewardBuffers()
        ctypes.pointer(c)[0], ctypes.pointer(b)[0] = fam.cfg, fam.buf
        for k, v in (spoil_cfg or {}).items():
            setattr(c, k, v)
        for k in spoil_buf:
            setattr(b, k, None)
        return lib.go1reward_arm(h, None if no_cfg else ctypes.byref(c), None if no_buf else ctypes.byref(b), None)
    assert arm(no_cfg=True) == arm(no_buf=True) == arm(dict(num_envs=0)) == arm(dict(num_envs=-2)) == -1
    assert arm(dict(num_envs=9)) == arm(dict(num_rewards=K + 1)) == arm(dict(num_rewards=0)) == -1      # not the simulator's sizes
    for name in ACCUMULATORS + STATE:
        assert arm(spoil_buf=[name]) == -2, name
    assert arm(dict(num_envs=0), ["count"]) == -1 and arm(dict(num_rewards=0), ["last_raw"]) == -1       # precedence: -1 before -2
    assert arm(dict(num_groups=0), ["group", "results"]) == 0                                            # the table is the reduction's business
    assert lib.go1reward_reduce(h, None) == -5
    for spoiled in (dict(spoil_cfg=dict(num_groups=-1)), dict(spoil_buf=["group"]), dict(spoil_buf=["results"]), dict(spoil_buf=["group_results"])):
        assert arm(**spoiled) == 0 and lib.go1reward_reduce(h, None) == -5, spoiled
    assert arm() == 0 and lib.go1reward_reduce(h, None) == 0
    # a simulator buffer missing: -3 from every launch that reads the simulator, after -2; the reduction reads none
    import go1sim_abi as abi
    for name in G.SIM_INPUTS:
        sim_buf = abi.Go1SimBuffers()
        ctypes.pointer(sim_buf)[0] = B.struct
        setattr(sim_buf, name, None)
        h2 = ctypes.c_void_p()
        assert lib.go1reward_create(ctypes.byref(S), ctypes.byref(sim_buf), 0, ctypes.byref(h2)) == 0
        assert lib.go1reward_arm(h2, ctypes.byref(fam.cfg), ctypes.byref(fam.buf), None) == -3, name
        b = G.Go1RewardBuffers()
        ctypes.pointer(b)[0] = fam.buf
        b.sum = None
        assert lib.go1reward_arm(h2, ctypes.byref(fam.cfg), ctypes.byref(b), None) == -2, name           # precedence: -2 before -3
        assert lib.go1reward_destroy(h2) == 0
    for optional in ("measured_heights", "height_samples"):
        sim_buf = abi.Go1SimBuffers()
        ctypes.pointer(sim_buf)[0] = B.struct
        setattr(sim_buf, optional, None)
        h2 = ctypes.c_void_p()
        assert lib.go1reward_create(ctypes.byref(S), ctypes.byref(sim_buf), 0, ctypes.byref(h2)) == 0
        assert lib.go1reward_arm(h2, ctypes.byref(fam.cfg), ctypes.byref(fam.buf), None) == 0
        assert lib.go1reward_accumulate(h2, g3, None) == 0 and lib.go1reward_destroy(h2) == 0


# ---- 2, 3. the reference's terms: the golden maps fixtures ---------------------------------------------------------------------------------
_maps_cache = {}


def maps_run(emu, variant, fname):
    """arm the family on a fixture's pre-step buffers, run the emulated post-physics maps, accumulate.  Computed once per fixture and
    shared: (fixture, S, keep, the model's state, what the kernel holds as numpy arrays)"""
    if fname not in _maps_cache:
        sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
        import emu_sim
        N = 48
        seed, counter = maps_fixture_stream(fname)
        cfg_, S, meta, B = make_sim(variant, N, seed=seed)
        d = load_maps_fixture(fname, S, meta, B)
        fam = family(S, B, emu, meta["reward_names"])
        fam.arm(np.zeros(N, np.int32))
        model = R.State(S, R.read(B))
        sums_in = B.episode_sums.numpy().copy()
        sim = emu_sim.EmuSim(S, B)
        sim.set_counters(counter, 0)
        sim.post_physics(d["gravity"])
        fam.accumulate(d["gravity"])
        post = R.read(B)
        view = R.step_view(post, model.snap)
        got = {k: v.numpy().copy() for k, v in fam.state.items()}
        _maps_cache[fname] = (d, S, meta, maps_keep(d, S), sums_in, view, post, got)
    return _maps_cache[fname]


@pytest.mark.parametrize("variant,fname", MAPS)
def test_emulated_terms_meet_the_reference_golden(emu, variant, fname):
    """row k of last_scaled plus the fixture's episode_sums[k] meets the reference's out_episode_sums[k], `total` its out_rew_buf, with
    the tolerances tests/test_oracle_golden.py applies to those arrays; exactly the environments of out_reset_buf are skipped"""
    d, S, meta, keep, sums_in, view, post, got = maps_run(emu, variant, fname)
    K = int(S.num_rewards)
    reset = d["out_reset_buf"].astype(bool)
    skipped = int(reset.sum())
    assert skipped == (2 if fname.endswith("_mild.npz") else skipped) and (fname.endswith("_mild.npz") or skipped in (13, 14)), skipped
    np.testing.assert_array_equal(got["last_valid"] == 0, reset)             # those, and no other environment
    np.testing.assert_array_equal(got["resets"], reset.astype(np.int32))
    assert got["teleported"].sum() == 0 and np.array_equal(got["measured"], (~reset).astype(np.int32))
    assert np.isnan(got["last_scaled"][:, reset]).all() and np.isnan(got["last_raw"][:, reset]).all() and keep.sum() >= 30
    assert np.isfinite(got["last_scaled"][:, ~reset]).all()
    np.testing.assert_allclose((got["last_scaled"][:K] + sums_in[:K])[:, keep], d["out_episode_sums"][:K][:, keep], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(got["last_scaled"][K + 3][~reset], d["out_rew_buf"][~reset], rtol=1e-4, atol=1e-7)
    # the raw table is the scaled one before the scale, and the snapshot is the simulator's buffers after the step
    scales = np.array([S.reward_scales[k] for k in range(K)], f32)
    assert bits((got["last_raw"] * scales[:, None])[:, ~reset]) == bits(got["last_scaled"][:K][:, ~reset])
    for k in R.SNAPSHOT:
        assert bits(got["snap_" + k]) == bits(post[k]), k


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, f64)).astype(f32)).astype(f64)


def check_against_fp64(S, view, gravity, got_raw, got_scaled, live, label):
    """the parity gate's rule, per term (raw, and scaled): the largest |kernel - fp64 model| over the live environments is at most twice
    the largest |fp32 numpy evaluation of the model - fp64 model|, plus 4 fp32 ulps of the value.  All three are the same statistic
    over the same environments, the largest, as the gate's table takes one statistic of kernel, fp32 evaluation and ulp floor alike
    (tests/test_gpu_parity.py bulk_table: `floor = the same statistic of BULK_FLOOR_ULPS ulps of the reference value`): the ulp is that
    of the largest reference value among them.  This is the intended reading, and the looser of two: taken per environment instead
    (dev_e <= 2 max fp32 error + 4 ulp(ref_e)) the floor shrinks with the smallest values of a term while the fp32 evaluation's largest
    error, over at most 48 environments, stays one sample of a maximum; the emulated kernel then misses on one term of one fixture
    (raibert_heuristic, maps_fuzz2_mild: 3.56e-8 at a value of 0.027 against 2 x 1.11e-8 + 4 x 1.9e-9) and meets it everywhere else.  Returns
    {(term, "raw" | "scaled"): (kernel's largest deviation, the fp32 evaluation's)}.  The four rows after the terms are functions of
    the kernel's own K values: check_extra_rows."""
    want, single = R.terms(S, view, gravity, f64), R.terms(S, view, gravity, f32)
    rows64, rows32 = R.rows(S, want, f64), R.rows(S, single, f32)
    out = {}
    for k, (name, _) in enumerate(R.active(S)):
        for what, kernel, ref, fp32 in (("raw", got_raw[k], want[name], single[name]), ("scaled", got_scaled[k], rows64[k], rows32[k])):
            kernel, ref, fp32 = kernel[live].astype(f64), ref[live], fp32[live].astype(f64)
            assert np.isfinite(ref).all(), (label, name)
            dev, allowed = np.abs(kernel - ref), 2.0 * np.abs(fp32 - ref).max() + 4.0 * ulp32(ref).max()
            print(f"{label} {name} {what}: kernel {dev.max():.3e} fp32 numpy {np.abs(fp32 - ref).max():.3e} allowed {allowed:.3e}")
            assert dev.max() <= allowed, (label, name, what, float(dev.max()), float(np.abs(fp32 - ref).max()), float(allowed), int(np.argmax(dev)))
            out[(name, what)] = (float(dev.max()), float(np.abs(fp32 - ref).max()))
    check_extra_rows(S, got_scaled, live, label)
    return out


def check_extra_rows(S, got_scaled, live, label):
    """sum, positive, negative and total against the fp64 combination of the kernel's OWN K scaled terms (so this is about the order, the
    split and the clip, not about the terms).  Bounds from the arithmetic: a sum of at most K fp32 additions is off by at most K half
    ulps of the sum of the magnitudes; max(sum, 0) inherits that; the ji22 total pos * expf(neg / sigma) is off by pos's and neg's
    errors carried through (relative |x| eps for an exponent x known to relative eps) plus a few ulps of its own operations
    (division, expf, product: 4 ulps allowed, as the gate's floor)."""
    K = int(S.num_rewards)
    terms_ = got_scaled[:K][:, live]
    want = R.combine(S, terms_, f64)
    got = got_scaled[K:][:, live].astype(f64)
    eps = 2.0 ** -24
    magnitude = np.abs(terms_.astype(f64)).sum(axis=0)
    slack = K * eps * magnitude                                               # of sum, positive and negative
    for x in range(3):
        assert (np.abs(got[x] - want[x]) <= slack).all(), (label, R.EXTRA[x], float(np.abs(got[x] - want[x]).max()))
    if S.only_positive_rewards or not S.only_positive_rewards_ji22_style:
        assert (np.abs(got[3] - want[3]) <= slack).all(), (label, "total")
        assert bits(got_scaled[K + 3][live]) == bits(np.maximum(got_scaled[K][live], f32(0)) if S.only_positive_rewards else got_scaled[K][live])
    else:
        sigma = float(S.sigma_rew_neg)
        x = np.abs(want[2] / sigma)
        factor = np.exp(want[2] / sigma)
        allowed = slack * factor * (1.0 + want[1] / sigma) + np.abs(want[3]) * (x * 2 * eps + 8 * eps)
        assert (np.abs(got[3] - want[3]) <= allowed).all(), (label, "total", float((np.abs(got[3] - want[3]) / np.maximum(allowed, 1e-300)).max()))


@pytest.mark.parametrize("variant,fname", MAPS)
def test_emulated_terms_against_fp64(emu, variant, fname):
    d, S, meta, keep, sums_in, view, post, got = maps_run(emu, variant, fname)
    assert [n for n, _ in R.active(S)] == meta["reward_names"]
    check_against_fp64(S, view, d["gravity"], got["last_raw"], got["last_scaled"], keep, fname)


# ---- 4. the model's bookkeeping, by hand -----------------------------------------------------------------------------------------------------
GRAVITY = np.array([0.3, -0.2, -9.6], f32)


def quiet(S, M=4, steps=3, seed=11):
    """`steps` buffer sets of M environments without events"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        cols = [R.synthetic_env(rng, S, events=False) for _ in range(M)]
        out.append({k: np.stack([c[k] for c in cols], axis=-1) for k in R.BUFFERS})
    return out


def variant(S, **fields):
    S2 = type(S).from_buffer_copy(S)
    for k, v in fields.items():
        setattr(S2, k, v)
    return S2


def row_of(S, name):
    return [n for n, _ in R.active(S)].index(name)


def test_model_second_step_uses_the_first_steps_snapshot():
    _, S, meta, _ = make_sim("train", 4)
    p0, p1, p2 = quiet(S)
    st = R.State(S, p0)
    st.accumulate(p1, GRAVITY)
    first = st.last_raw.copy()
    assert all(bits(st.snap[k]) == bits(p1[k]) for k in R.SNAPSHOT)
    st.accumulate(p2, GRAVITY)
    dt = f64(S.dt)
    want = (((p1["last_dof_vel"].astype(f64) - p2["dof_vel"]) / dt) ** 2).sum(axis=0)
    np.testing.assert_allclose(st.last_raw[row_of(S, "dof_acc")], want, rtol=1e-12)
    np.testing.assert_allclose(first[row_of(S, "dof_acc")], (((p0["last_dof_vel"].astype(f64) - p1["dof_vel"]) / dt) ** 2).sum(axis=0), rtol=1e-12)
    jpt, ljpt, lljpt = (x.astype(f64) for x in (p2["joint_pos_target"], p2["last_last_joint_pos_target"], p1["last_last_joint_pos_target"]))
    mask = (p2["last_last_actions"] != 0) & (p1["last_last_actions"] != 0)
    np.testing.assert_allclose(st.last_raw[row_of(S, "action_smoothness_2")], ((jpt - 2 * ljpt + lljpt) ** 2 * mask).sum(axis=0), rtol=1e-12)
    fv = p2["foot_velocities"].astype(f64).reshape(4, 3, -1)
    filt = (p2["contact_forces"][[14, 26, 38, 50]] > 1.0) | (p1["last_contacts"] != 0)
    np.testing.assert_allclose(st.last_raw[row_of(S, "feet_slip")], (filt * (fv[:, 0] ** 2 + fv[:, 1] ** 2)).sum(axis=0), rtol=1e-12)
    assert (filt != (p2["contact_forces"][[14, 26, 38, 50]] > 1.0)).any()      # the snapshot's contacts matter in this data
    assert (st.count == 2).all() and st.measured.tolist() == [2] * 4 and st.last_valid.tolist() == [1] * 4


def test_model_resets_teleports_and_warm_up():
    _, S, meta, _ = make_sim("train", 4)
    p0, p1, p2 = quiet(S)
    acc = row_of(S, "dof_acc")
    # a reset inside step 1 (environment 1): counted, not folded; the post-reset histories are what step 2 reads: dof_acc against 0
    p1["reset_buf"][1] = 1
    p1["last_dof_vel"][:, 1] = 0
    p1["root_states"][0, 2] += f32(4.0)                                       # and environment 2's base is teleported in step 1
    st = R.State(S, p0)
    st.accumulate(p1, GRAVITY)
    assert st.resets.tolist() == [0, 1, 0, 0] and st.teleported.tolist() == [0, 0, 1, 0] and st.measured.tolist() == [1, 0, 0, 1]
    assert st.last_valid.tolist() == [1, 0, 0, 1] and np.isnan(st.last_scaled[:, 1:3]).all() and np.isfinite(st.last_scaled[:, [0, 3]]).all()
    assert (st.count[:, 1:3] == 0).all() and (st.count[:, [0, 3]] == 1).all() and (st.nonfinite == 0).all()
    st.accumulate(p2, GRAVITY)
    assert st.measured.tolist() == [2, 1, 1, 2] and (st.count[:, 1:3] == 1).all()
    np.testing.assert_allclose(st.last_raw[acc, 1], ((p2["dof_vel"][:, 1].astype(f64) / f64(S.dt)) ** 2).sum(), rtol=1e-12)
    # a reset and a teleport at once is a reset; a reset from the host between two steps: re-snapshot, dof_acc of the next step against 0
    both = {k: v.copy() for k, v in p1.items()}
    both["root_states"][0, 1] += f32(4.0)
    st = R.State(S, p0)
    st.accumulate(both, GRAVITY)
    assert st.resets.tolist() == [0, 1, 0, 0] and st.teleported.tolist() == [0, 0, 1, 0]
    st = R.State(S, p0)
    host = {k: v.copy() for k, v in p0.items()}
    host["last_dof_vel"][:, 3] = 0
    host["last_last_actions"][:, 3] = 0
    stale = R.State(S, p0)
    st.snapshot(host)
    clean = {k: v.copy() for k, v in quiet(S)[1].items()}
    st.accumulate(clean, GRAVITY), stale.accumulate(clean, GRAVITY)
    np.testing.assert_allclose(st.last_raw[acc, 3], ((clean["dof_vel"][:, 3].astype(f64) / f64(S.dt)) ** 2).sum(), rtol=1e-12)
    assert st.last_raw[row_of(S, "action_smoothness_2"), 3] == 0.0 and stale.last_raw[row_of(S, "action_smoothness_2"), 3] > 0.0
    assert stale.last_raw[acc, 3] != st.last_raw[acc, 3] and bits(stale.last_raw[:, :3]) == bits(st.last_raw[:, :3])
    # warm-up: steps of an episode not older than warmup_steps fold nothing and are not counted; the snapshot moves on
    young = {k: v.copy() for k, v in quiet(S)[1].items()}
    young["episode_length_buf"][:] = [1, 3, 4, 50]
    st = R.State(S, p0, warmup_steps=3)
    st.accumulate(young, GRAVITY)
    assert st.measured.tolist() == [0, 0, 1, 1] and st.resets.sum() == 0 and st.teleported.sum() == 0 and st.last_valid.tolist() == [0, 0, 1, 1]
    assert all(bits(st.snap[k]) == bits(young[k]) for k in R.SNAPSHOT)


def test_model_clip_split_and_nonfinite():
    _, S, meta, _ = make_sim("train", 4)
    p0, p1, _ = quiet(S)
    K = int(S.num_rewards)
    tables = {}
    for label, fields in (("only_positive", dict(only_positive_rewards=1, only_positive_rewards_ji22_style=0)),
                          ("ji22", dict(only_positive_rewards=0, only_positive_rewards_ji22_style=1, sigma_rew_neg=0.02)),
                          ("neither", dict(only_positive_rewards=0, only_positive_rewards_ji22_style=0))):
        st = R.State(variant(S, **fields), p0)
        tables[label] = st.accumulate(p1, GRAVITY)
    t = tables["neither"]
    np.testing.assert_allclose(t[K], t[:K].sum(axis=0), rtol=1e-12)
    np.testing.assert_allclose(t[K + 1] + t[K + 2], t[K], rtol=1e-9, atol=1e-15)
    assert (t[K + 1] >= 0).all() and (t[K + 2] <= 0).all() and bits(t[K + 3]) == bits(t[K])
    scales = dict(R.active(S))
    assert scales["tracking_lin_vel"] > 0 > scales["torques"] and scales["tracking_contacts_shaped_force"] > 0
    pos_rows = [k for k, (n, s) in enumerate(R.active(S)) if (-1 if n in R.NEGATIVE_RAW else 1) * s >= 0]
    assert row_of(S, "tracking_contacts_shaped_force") not in pos_rows and row_of(S, "tracking_lin_vel") in pos_rows       # a negative raw term times a positive scale costs
    np.testing.assert_allclose(t[K + 1], t[pos_rows].sum(axis=0), rtol=1e-12)
    assert bits(tables["only_positive"][K + 3]) == bits(np.maximum(t[K], 0)) and bits(tables["only_positive"][:K + 3]) == bits(t[:K + 3])
    np.testing.assert_allclose(tables["ji22"][K + 3], t[K + 1] * np.exp(t[K + 2] / f64(f32(0.02))), rtol=1e-12)
    assert (t[K] < 0).any() or (t[K] > 0).any()
    # a non-finite input: the rows it reaches go to `nonfinite`, the others fold
    bad = {k: v.copy() for k, v in p1.items()}
    bad["torques"][5, 2] = np.nan
    st = R.State(S, p0)
    st.accumulate(bad, GRAVITY)
    tq = row_of(S, "torques")
    reached = [tq, K, K + 2, K + 3]
    assert st.nonfinite[reached, 2].tolist() == [1] * 4 and st.count[reached, 2].tolist() == [0] * 4 and st.measured[2] == 1 and st.last_valid[2] == 1
    others = [k for k in range(K + 4) if k not in reached]
    assert (st.count[others, 2] == 1).all() and (st.nonfinite[others] == 0).all() and (st.count[:, [0, 1, 3]] == 1).all()


# ---- 5. shapes through the emulator: an environment's rows do not depend on where it sits; the group table bit for bit ------------------------
SHAPES = [1, 64, 65, 257]
STEPS, WARMUP = 3, 3


def groups_of(rng, N):
    """three groups of which group 1 is empty, some environments in no group (-1); most in group 0"""
    group = np.where(rng.random(N) < 0.7, 0, rng.integers(-1, 3, N)).astype(np.int32)
    group[group == 1] = 2
    group[0] = 0
    if N >= 3:
        group[1], group[2] = -1, 2
    return group


def drive(S, meta, B, fam, posts, group, warmup=WARMUP):
    """arm on posts[0], accumulate posts[1:]; the per-step (last_raw, last_scaled, last_valid), then everything read back"""
    R.load(B, posts[0])
    fam.arm(group, warmup)
    per_step = []
    for post in posts[1:]:
        R.load(B, post)
        fam.accumulate(GRAVITY)
        per_step.append({k: fam.state[k].cpu().numpy().copy() for k in ("last_raw", "last_scaled", "last_valid")})
    res = fam.read()
    acc = {k: v.cpu().numpy().copy() for k, v in fam.acc.items()}
    state = {k: v.cpu().numpy().copy() for k, v in fam.state.items()}
    return per_step, res, acc, state


def check_bookkeeping(S, posts, group, per_step, res, acc, state, warmup=WARMUP):
    """the model's bookkeeping replayed with the kernel's own rows as values: accumulators, counts, snapshot and both tables bit for bit"""
    G = int(group.max()) + 1
    st = R.State(S, posts[0], warmup)
    for post, step in zip(posts[1:], per_step):
        st.accumulate(post, GRAVITY, values=step["last_scaled"])
        assert step["last_valid"].tolist() == st.last_valid.tolist()
        assert np.isnan(step["last_scaled"][:, st.last_valid == 0]).all() and np.isnan(step["last_raw"][:, st.last_valid == 0]).all()
    for k in ACCUMULATORS:
        assert acc[k].view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    for k in ("measured", "resets", "teleported"):
        assert state[k].view(np.uint32).tolist() == getattr(st, k).tolist(), k
    for k in R.SNAPSHOT:
        assert bits(state["snap_" + k]) == bits(posts[-1][k]), k
    want, want_groups = R.reduce(acc, {k: state[k].view(np.uint32) for k in ("measured", "resets", "teleported")}, group, G)
    K = int(S.num_rewards)
    for k, name in enumerate(res["names"]):
        assert res["terms"][name].shape == (G, 6) and bits(res["terms"][name]) == bits(want[:, k]), name
    for x, name in enumerate(R.EXTRA):
        assert bits(res[name]) == bits(want[:, K + x]), name
    assert bits(res["groups"]) == bits(want_groups) and res["groups"].shape == (G, 4)
    assert res["groups"][:, 0].tolist() == [float((group == g).sum()) for g in range(G)]
    assert (res["groups"][:, 1:].sum(axis=1) <= res["groups"][:, 0] * (len(posts) - 1)).all()
    means = np.stack([res["terms"][n][:, 1] for n in res["names"]], axis=1)
    for g in range(G):
        if res["groups"][g, 1] > 0:
            assert abs(sum(abs(res["share"][n][g]) for n in res["names"]) - 1.0) < 1e-12
            assert all(np.sign(res["share"][n][g]) == np.sign(means[g, k]) for k, n in enumerate(res["names"]))
        else:
            assert all(np.isnan(res["share"][n][g]) for n in res["names"])
    return st


def two_runs(rng, S_of, N, on, steps=STEPS):
    """run A: N distinct environments; run B: 2 N + 1 environments, A's permuted and tiled.  on(S, meta, B) -> family"""
    _, S, meta, B = S_of(N)
    posts = R.synthetic_steps(rng, S, N, steps + 1)
    if N >= 3:
        posts[2]["torques"][4, N // 2] = np.nan                               # a non-finite input in one step of one environment
    index = np.concatenate([rng.permutation(N), rng.permutation(N), [0]])
    rng.shuffle(index)
    out = []
    for idx in (np.arange(N), index):
        _, S2, meta2, B2 = S_of(len(idx))
        placed = [R.place(p, idx) for p in posts]
        group = groups_of(rng, len(idx))
        fam = on(S2, meta2, B2)
        out.append((S2, placed, group) + drive(S2, meta2, B2, fam, placed, group))
    return index, out


def check_two_runs(index, runs):
    (S, posts, group, per_step, res, acc, state), (S2, posts2, group2, per_step2, res2, acc2, state2) = runs
    for a, b in zip(per_step, per_step2):                                     # an environment's rows do not depend on its workgroup
        for k in a:
            assert bits(a[k][..., index]) == bits(b[k]), k
    for k in ACCUMULATORS:
        assert bits(acc[k][:, index]) == bits(acc2[k]), k
    for k in state:
        assert bits(state[k][..., index]) == bits(state2[k]), k
    st = check_bookkeeping(S, posts, group, per_step, res, acc, state)
    check_bookkeeping(S2, posts2, group2, per_step2, res2, acc2, state2)
    return st


@pytest.mark.parametrize("N", SHAPES)
def test_emulated_kernel_shapes_and_group_table(emu, N):
    rng = np.random.default_rng(900 + N)
    index, runs = two_runs(rng, lambda n: make_sim("train", n), N, lambda S, meta, B: family(S, B, emu, meta["reward_names"]))
    st = check_two_runs(index, runs)
    if N == 257:
        group2 = runs[1][2]
        assert (group2 == 0).sum() > 256 and (group2 == 1).sum() == 0 and (group2 == -1).sum() > 0
        assert st.resets.sum() > 0 and st.teleported.sum() > 0 and st.nonfinite.sum() > 0 and (st.measured < STEPS).sum() > st.resets.sum() + st.teleported.sum()
    # and the terms themselves against the fp64 model, step by step (the rule of test_emulated_terms_against_fp64)
    S, posts, group, per_step = runs[0][:4]
    model = R.State(S, posts[0], WARMUP)
    for post, step in zip(posts[1:], per_step):
        view = R.step_view(post, model.snap)
        model.accumulate(post, GRAVITY)
        live = (model.last_valid != 0) & np.isfinite(post["torques"]).all(axis=0)
        if live.any():
            check_against_fp64(S, view, GRAVITY, step["last_raw"], step["last_scaled"], live, f"N={N}")


# ---- 5b. the hand-made cases of section 4 through the kernel itself ------------------------------------------------------------------------
@pytest.mark.parametrize("clip", ["only_positive", "ji22", "neither"])
def test_emulated_clip_variants_resnapshot_and_precedence(emu, clip):
    """the three clip settings on the emulated kernel (bookkeeping bit for bit, the four derived rows by check_extra_rows, the terms by the
    fp64 rule), a reset and a teleport at once counted as a reset, and a re-snapshot after a host-side reset: dof_acc against 0"""
    fields = dict(only_positive=dict(only_positive_rewards=1, only_positive_rewards_ji22_style=0),
                  ji22=dict(only_positive_rewards=0, only_positive_rewards_ji22_style=1, sigma_rew_neg=0.02),
                  neither=dict(only_positive_rewards=0, only_positive_rewards_ji22_style=0))[clip]
    N = 6
    _, S0, meta, B = make_sim("train", N)
    S = variant(S0, **fields)
    p0, p1, p2 = quiet(S, N, 3, seed=23)
    p1["reset_buf"][1] = 1
    p1["root_states"][0, 1] += f32(4.0)                                        # environment 1: reset and teleported at once
    p1["root_states"][0, 2] += f32(4.0)                                        # environment 2: teleported
    fam = family(S, B, emu, meta["reward_names"])
    group = np.array([0, 0, 1, 1, -1, 0], np.int32)
    per_step, res, acc, state = drive(S, meta, B, fam, [p0, p1, p2], group, warmup=0)
    st = check_bookkeeping(S, [p0, p1, p2], group, per_step, res, acc, state, warmup=0)
    assert st.resets.tolist() == [0, 1, 0, 0, 0, 0] and st.teleported.tolist() == [0, 0, 1, 0, 0, 0] and st.measured.tolist() == [2, 1, 1, 2, 2, 2]
    model = R.State(S, p0)
    K = int(S.num_rewards)
    for post, step in zip((p1, p2), per_step):
        view = R.step_view(post, model.snap)
        model.accumulate(post, GRAVITY)
        live = model.last_valid != 0
        check_against_fp64(S, view, GRAVITY, step["last_raw"], step["last_scaled"], live, clip)
        total, plain = step["last_scaled"][K + 3][live], step["last_scaled"][K][live]
        if clip == "only_positive":
            assert bits(total) == bits(np.maximum(plain, f32(0))) and (plain < 0).any()
        elif clip == "neither":
            assert bits(total) == bits(plain)
        else:
            assert (total >= 0).all() and (total <= step["last_scaled"][K + 1][live]).all() and not np.array_equal(total, plain)
    # a reset from the host between two steps: the simulator's histories are cleared, the family takes its snapshot again
    host = {k: v.copy() for k, v in p2.items()}
    host["last_dof_vel"][:, 3] = 0
    host["last_last_actions"][:, 3] = 0
    R.load(B, host)
    fam.snapshot()
    nxt = quiet(S, N, 1, seed=29)[0]
    R.load(B, nxt)
    fam.accumulate(GRAVITY)
    raw = fam.state["last_raw"].numpy()
    want = ((nxt["dof_vel"][:, 3].astype(f64) / f64(S.dt)) ** 2).sum()
    assert abs(raw[row_of(S, "dof_acc"), 3] - want) <= 1e-6 * want and raw[row_of(S, "action_smoothness_2"), 3] == 0.0
    other = (((p2["last_dof_vel"][:, 0].astype(f64) - nxt["dof_vel"][:, 0]) / f64(S.dt)) ** 2).sum()
    assert abs(raw[row_of(S, "dof_acc"), 0] - other) <= 1e-6 * other       # the others still against the step before


# ---- 6. the environment hooks without a GPU ---------------------------------------------------------------------------------------------------
def test_reward_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from go1_gym_learn.eval_metrics.metrics import METRICS_FNS
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    monkeypatch.delitem(sys.modules, "go1reward_host", raising=False)
    c = apply_train_config(make_cfg(), num_envs=16)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_reward_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_reward_metrics, env.read_reward_metrics, env.last_reward_terms):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert "go1reward_host" not in sys.modules and env._reward is None         # never measured: no host module
    assert not hasattr(env, "reward_functions")
    with pytest.raises(NotImplementedError, match=r"this environment has no `reward_functions` \(the rewards are computed by the step kernel\)"):
        METRICS_FNS["auxiliary_rewards"](env, None, None)
    with pytest.raises(AttributeError, match="no attribute 'no_such_thing'"):
        env.no_such_thing
    env.reset_idx(torch.tensor([1, 2]))
    env.step(torch.zeros(16, 12))                                             # and stepping goes on
    assert ("rewards", "_reward") in env._STATE_FAMILIES and len(METRICS_FNS) == 14


# ---- 7. the sweep's host pieces and the tool --------------------------------------------------------------------------------------------------
def fixed_result():
    import go1reward_host as G
    names = ["tracking_lin_vel", "torques", "feet_slip"]
    means = np.array([[0.016, -0.004, -0.002], [0.010, -0.012, NAN]])
    row = lambda mean: [30.0, mean, 0.001, mean - 0.01, mean + 0.01, 0.0] if np.isfinite(mean) else [0.0, NAN, NAN, NAN, NAN, 2.0]
    terms = {n: np.array([row(means[g, k]) for g in range(2)]) for k, n in enumerate(names)}
    total = np.nansum(means, axis=1)
    out = dict(preset="static_medium", cells=[(0.5, 0.0, (0.5, 0.0, 0.0)), (1.0, 0.0, (0.5, 0.0, 0.0))], names=names,
               scales=np.array([0.02, -2e-6, -8e-4], f32), terms=terms, share=G.shares(means, names),
               reward_groups=np.array([[8.0, 300.0, 12.0, 8.0], [8.0, 310.0, 10.0, 0.0]]), metrics={}, groups=np.zeros((2, 5)), num_envs=16, steps=40,
               warmup_steps=5, seed=1, dt=0.02)
    out["sum"] = np.array([row(t) for t in total])
    out["positive"] = np.array([row(m) for m in means[:, 0]])
    out["negative"] = np.array([row(t - m) for t, m in zip(total, means[:, 0])])
    out["total"] = np.array([row(max(t, 0.0)) for t in total])
    return out


def test_shares_table_json_and_figure(tmp_path):
    import go1reward_host as G
    from go1_gym_learn.eval_metrics import rewards
    assert rewards.EXTRA_ROWS == G.REWARD_EXTRA_ROWS and rewards.GROUP_FIELDS == G.REWARD_GROUP_FIELDS
    res = fixed_result()
    share = res["share"]
    assert abs(share["tracking_lin_vel"][0] - 0.016 / 0.022) < 1e-15 and abs(share["torques"][0] + 0.004 / 0.022) < 1e-15
    assert abs(sum(abs(share[n][0]) for n in res["names"]) - 1.0) < 1e-15
    assert np.isnan(share["feet_slip"][1]) and abs(abs(share["tracking_lin_vel"][1]) + abs(share["torques"][1]) - 1.0) < 1e-15      # a term never measured
    assert all(np.isnan(v[0]) for v in G.shares(np.zeros((1, 3)), res["names"]).values())
    md = rewards.reward_table(res).splitlines()
    assert md[0] == "| term | scale | vx 0.5, yaw 0 | vx 1, yaw 0 |" and len(md) == 2 + 3 + 4 + 1 + 3
    assert md[2] == "| tracking_lin_vel | 0.02 | 0.016 (+72.7 %) | 0.01 (+45.5 %) |" and md[4] == "| feet_slip | -0.0008 | -0.002 (-9.1 %) | – (– %) |"
    assert md[5].startswith("| **sum** |  | 0.01 | -0.002 |") and md[8] == "| **total** |  | 0.01 | 0 |"
    assert md[9] == "| **forgiven by the clip** |  | 0 | 0.002 |"
    assert md[10:] == ["| measured env-steps |  | 300 | 310 |", "| reset env-steps |  | 12 | 10 |", "| teleported env-steps |  | 8 | 0 |"]
    assert len({line.count("|") for line in md}) == 1
    js = json.loads(json.dumps(rewards.reward_to_json(res), allow_nan=False))
    assert js["cells"][1] == dict(vx=1.0, yaw=0.0, gait=[0.5, 0.0, 0.0]) and js["group_fields"] == R.GROUP_FIELDS and js["names"] == res["names"]
    assert js["terms"]["feet_slip"][1][1] is None and js["terms"]["torques"][0][1] == -0.004 and js["share"]["feet_slip"][1] is None
    assert js["reward_groups"][0] == [8.0, 300.0, 12.0, 8.0] and abs(js["forgiven"][1] - 0.002) < 1e-15 and js["total"][1][1] == 0.0
    path = tmp_path / "rewards.png"
    rewards.plot_reward_shares(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000


def test_tool_accepts_a_reward_sweep(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import rewards
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--rewards", "--vx", "0.5", "1.0", "--envs", "16", "--steps", "40", "--warmup-steps", "5", "--presets", "static_medium"])
    assert a.rewards and not a.trunk and not a.feet and not a.joints and not a.tiles and (a.vx, a.envs, a.steps, a.terrain) == ([0.5, 1.0], 16, 40, None)
    assert not eval_sweep.parse_args(base).rewards and eval_sweep.parse_args(base + ["--rewards", "--terrain", "plane"]).terrain == "plane"
    for bad in (["--rewards", "--terrain"], ["--rewards", "--behaviour"], ["--rewards", "--joints"], ["--rewards", "--feet"], ["--rewards", "--trunk"],
                ["--rewards", "--response", "--switch", "vx", "0", "1"], ["--rewards", "--push", "--magnitude", "1", "--direction", "0"],
                ["--rewards", "--segment-steps", "20"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(base + bad)
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(rewards, "run_reward_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    eval_sweep.run_rewards(a, None, dict(vx=a.vx, yaw=a.yaw, gait=[(0.5, 0.0, 0.0)]))
    assert seen == dict(preset="static_medium", grid=dict(vx=[0.5, 1.0], yaw=[0.0], gait=[(0.5, 0.0, 0.0)]), num_envs=16, steps=40, warmup_steps=5, seed=1,
                        terrain=None)
    js = json.load(open(tmp_path / "eval" / "static_medium_rewards.json"))
    assert js["preset"] == "static_medium" and js["terms"]["tracking_lin_vel"][0][1] == 0.016
    md = (tmp_path / "eval" / "static_medium_rewards.md").read_text()
    assert "| tracking_lin_vel | 0.02 | 0.016 (+72.7 %) |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_rewards.png").read_bytes()[:4] == b"\x89PNG"


# ---- 8. the scripted trot of the GPU test, through the oracle here ----------------------------------------------------------------------------
TROT_WINDOW = 60                 # steps the GPU test compares against the step kernel's episode_sums
TROT_RESET_CAP = 0.25            # at most one env-step in four of the window has reset_buf set: asserted here on the oracle, relied on there


def test_the_trot_script_resets_within_the_cap_on_the_oracle(monkeypatch):
    import fake_sim
    from test_gpu_response_trace import make_env
    from test_trunk_metrics import trot_with_pauses
    fake_sim.install(monkeypatch)
    N = 64
    env = make_env(N, "plane", 20.0, seed=4)
    env.reset()
    resets = 0
    for step in range(TROT_WINDOW):
        env.step(trot_with_pauses(step, N))
        resets += int(env.reset_buf.sum())
    print(f"\noracle: {resets} of {N * TROT_WINDOW} env-steps of the trot window have reset_buf set ({resets / (N * TROT_WINDOW):.4f}; cap {TROT_RESET_CAP})")
    assert resets <= TROT_RESET_CAP * N * TROT_WINDOW
