"""CPU checks of the observation family (include/go1obs.h, libgo1obs.so): the ctypes mirrors and the exported symbols against the header,
the build's source list (as the compiler reads it), flags and stamp, the refusals without a GPU, the model of tests/obs_ref.py on
hand-computed cases, go1obs.hip itself under the SIMT emulator against that model bit for bit (accumulators, state and the three result
tables), the environment hooks where there is no GPU, the channel names against the configuration's switches and, on the oracle-backed
simulator, against the buffers they are named after, shift and ranking by hand, profile_from_array against the model, the sweep's files
and the tool's parsing."""
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

import obs_ref as T
from test_eval_return_codes import Call, cfg, each, element, nobody, null
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from test_sensitivity_metrics import canon, same
from util import build_emu

HEADER = os.path.join(REPO, "include", "go1obs.h")
SOURCE = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1obs.hip")
TABLES = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1_tables.h")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]
TABLE_NAMES = ["results", "hist_results", "tails"]


# ---- 1. mirrors, symbols, sources, stamp ---------------------------------------------------------------------------------------------------
def test_observation_mirrors_match_the_header():
    import go1eval_host as E
    import go1obs_host as G
    import go1sim_abi as abi
    src = open(HEADER).read()
    for macro, value in (("GO1OBS_MAX_CHANNELS", G.MAX_CHANNELS), ("GO1OBS_BINS", G.BINS), ("GO1OBS_NUM_TAILS", G.NUM_TAILS), ("GO1OBS_NUM_FIELDS", 6),
                         ("GO1OBS_REDUCE_THREADS", 256)):
        assert re.search(rf"#define {macro} {value}\b", src), macro
    assert G.MAX_CHANNELS == abi.GO1_MAX_OBS + abi.GO1_MAX_PRIV_OBS == T.MAX_CHANNELS == 160 and (G.BINS, G.NUM_TAILS) == (T.BINS, len(T.TAILS)) == (16, 3)
    want = struct_fields(src, "Go1ObsConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1ObsConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "num_obs", "num_privileged_obs", "privileged",
                                                                              "num_break", "clip", "lo", "scale"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1ObsConfig._fields_):
        assert ctype is C_TYPES[ctext] if ctext in C_TYPES else (ctext, ctype._type_, ctype._length_) == ("float[GO1OBS_MAX_CHANNELS]", ctypes.c_float, 160), field
    want = struct_fields(src, "Go1ObsBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1ObsBuffers._fields_] == T.INPUTS + ACCUMULATORS + T.STATE + ["break_ids", "group"] + TABLE_NAMES
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1ObsBuffers._fields_)
    types_ = dict(want)
    assert types_["obs_buf"] == types_["privileged_obs_buf"] == "const float*" and types_["reset_buf"] == "const uint8_t*" and types_["break_ids"] == "const int64_t*"
    assert types_["prev"] == "float*" and all(types_[k] == "uint32_t*" for k in T.STATE[1:]) and all(types_[k] == "double*" for k in TABLE_NAMES)
    # the kernels take both structs by value: the argument stays under 4 KB
    assert ctypes.sizeof(G.Go1ObsConfig) == 8 * 4 + 2 * 160 * 4 and ctypes.sizeof(G.Go1ObsConfig) + ctypes.sizeof(G.Go1ObsBuffers) == 1312 + 22 * 8 < 4096
    assert G._OBS_INPUTS == T.INPUTS and G._OBS_STATE == T.STATE == list(G.Go1Observations.PER_CHANNEL) + list(G.Go1Observations.PER_ENV) and G._OBS_TABLES == TABLE_NAMES
    assert enum_order(src, "Go1ObsTail", "GO1OBS_T_") == G.TAILS == T.TAILS
    assert enum_order(src, "Go1ObsGroupField", "GO1OBS_G_") == G.OBS_GROUP_FIELDS == T.GROUP_FIELDS
    assert enum_order(src, "Go1ObsField", "GO1OBS_F_") == E.FIELD_NAMES
    assert issubclass(G.Go1Observations, E._Table)
    st = T.clear(2, T.config(T.script_spans(3), 3))
    for name, (dtype, lead) in list(G.Go1Observations.PER_CHANNEL.items()):            # the model's formats are the host's (uint32 read as int32)
        assert getattr(st, name).shape == (3, *lead, 2) and getattr(st, name).dtype.itemsize == torch.zeros(1, dtype=dtype).element_size(), name
    # the memory the header's layout takes per channel and environment: the estimate the documents quote
    per_channel = sum(int(np.prod(lead, dtype=np.int64)) * torch.zeros(1, dtype=dt).element_size() for dt, lead in G.Go1Observations.PER_CHANNEL.values())
    assert per_channel == 4 + 4 + 64 + 12 and per_channel + 2 * (4 + 8 + 8 + 4 + 4 + 4) == 148


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1obs_host as G
    declared = set(re.findall(r"\b(go1obs_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1obs_clear", "go1obs_break", "go1obs_accumulate", "go1obs_reduce", "go1obs_version"}
    out = g.build_obs_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1obs_" in line} == declared
    assert not re.search(r"\bgo1(eval|feet|trunk|gait|episode|sens)_\w+", dynamic)


def test_sources_flags_and_stamp():
    import __graft_entry__ as g
    assert g.obs_sources() == [SOURCE, TABLES, HEADER] and g.OBS_FLAGS == g.SENS_FLAGS == g.EVAL_FLAGS and "-ffp-contract=off" in g.OBS_FLAGS
    assert g.OBS_FLAGS is not g.EVAL_FLAGS and g.OBS_FLAGS is not g.SENS_FLAGS
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc] + g.OBS_FLAGS + ["--cuda-host-only", "-MM", SOURCE], cwd=g.CSRC, check=True, capture_output=True, text=True).stdout
    read = {os.path.normpath(os.path.join(g.CSRC, f)) for f in out.split(":", 1)[1].replace("\\\n", " ").split()}
    assert {f for f in read if not f.startswith("/opt/")} == {os.path.normpath(f) for f in g.obs_sources()}
    for others in (g.sim_sources(), g.ppo_sources(), g.render_sources(), g.state_sources()):
        assert not set(others) & set(g.obs_sources())
    for others in (g.eval_sources(), g.feet_sources(), g.trunk_sources(), g.gait_sources(), g.spectrum_sources(), g.place_sources(), g.reward_sources(), g.episode_sources(),
                   g.sens_sources()):
        assert set(others) & set(g.obs_sources()) == {TABLES}                    # one shared header, and nothing else
    code = re.sub(r"//.*", "", open(SOURCE).read())
    assert not re.search(r"go1(eval|feet|trunk|gait|episode|sens)", code) and "GO1_TABLES_MATCH(GO1OBS)" in code
    assert "go1obs" not in re.sub(r"//.*", "", open(TABLES).read())              # the shared header names no library
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["../../include/go1obs.h", "go1_tables.h"]
    for banned in ("atomic", "sinf", "cosf", "atan2f", "expf", "powf", "sqrtf"):
        assert banned not in code, banned
    accumulate = code[code.index("obs_accumulate_kernel(const ObsArgs A)"):code.index("obs_reduce_kernel(const ObsArgs A)")]
    assert "__shared__" not in accumulate and "__syncthreads" not in accumulate and "row_thread(N, C" in accumulate
    assert "sizeof(Go1ObsConfig) + sizeof(Go1ObsBuffers) < 4096" in code
    out = g.build_obs_hip()
    assert os.path.basename(out) == "libgo1obs.so" and g.library_stamp(out) == g.source_hash(g.obs_sources(), g.OBS_FLAGS)
    lib = ctypes.CDLL(out)                                                       # dlopen needs no GPU
    lib.go1obs_version.restype = ctypes.c_char_p
    assert lib.go1obs_version() == b"go1obs 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    assert "build_obs_hip()" in inspect.getsource(g.build) and "libgo1obs.so" in inspect.getsource(g.smoke)
    # the other table libraries' stamps are what their own sources give: this family changed none of them
    for name, sources, flags in (("eval", g.eval_sources(), g.EVAL_FLAGS), ("sens", g.sens_sources(), g.SENS_FLAGS), ("episode", g.episode_sources(), g.EPISODE_FLAGS)):
        assert g.library_stamp(os.path.join(g.CSRC, f"libgo1{name}.so")) in (None, g.source_hash(sources, flags)), name


def test_a_missing_library_fails_loudly(tmp_path):
    import go1obs_host as G
    with pytest.raises(G.Go1ObsLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1obs.so"))


# ---- 2. the refusals without a GPU (the helpers of tests/test_eval_return_codes.py) ----------------------------------------------------------
def obs_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.num_obs, c.num_privileged_obs, c.privileged, c.num_break, c.clip = 70, 2, 3, 70, 9, 1, 4, 100.0
    for k in range(160):
        c.lo[k], c.scale[k] = -1.0, 8.0


OBS_ACC = ACCUMULATORS + T.STATE
BAD_CHANNELS = [("num_obs = 0", -12, [cfg(num_obs=0)]), ("num_obs < 0", -12, [cfg(num_obs=-5)]), ("num_obs = 161", -12, [cfg(num_obs=161)]),
                ("num_privileged_obs < 0", -12, [cfg(num_privileged_obs=-1)]), ("C = 161", -12, [cfg(num_obs=96, num_privileged_obs=65)]),
                ("C overflows", -12, [cfg(num_obs=2 ** 31 - 1, num_privileged_obs=2 ** 31 - 1)])]
BAD_BINS = [("scale = 0", -12, [element("scale", 2, 0.0)]), ("scale < 0", -12, [element("scale", 0, -4.0)]), ("scale NaN", -12, [element("scale", 78, NAN)]),
            ("scale inf", -12, [element("scale", 5, INF)]), ("lo NaN", -12, [element("lo", 3, NAN)]), ("lo inf", -12, [element("lo", 70, -INF)]),
            ("clip NaN", -12, [cfg(clip=NAN)])]
CASES = {
    "go1obs_clear": nobody() + each(OBS_ACC, -2) + BAD_CHANNELS + [
        ("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")]), ("no prev and num_obs = 0", -2, [null("prev"), cfg(num_obs=0)])],
    "go1obs_break": nobody() + each(OBS_ACC, -2) + BAD_CHANNELS + [
        ("num_break < 0", -12, [cfg(num_break=-1)]), ("num_envs = 0 and no age", -1, [cfg(num_envs=0), null("age")]),
        ("no age and num_break < 0", -2, [null("age"), cfg(num_break=-1)])],
    "go1obs_accumulate": nobody() + each(OBS_ACC, -2) + each(T.INPUTS, -3) + BAD_CHANNELS + BAD_BINS + [
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no hist and no obs_buf", -2, [null("hist", "obs_buf")]),
        ("no resets and scale = 0", -2, [null("resets"), element("scale", 1, 0.0)]),
        ("no reset_buf and scale = 0", -3, [null("reset_buf"), element("scale", 1, 0.0)]),
        ("no obs_buf and num_obs = 0", -3, [null("obs_buf"), cfg(num_obs=0)])],
    "go1obs_reduce": nobody() + each(OBS_ACC, -2) + [
        ("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group"] + TABLE_NAMES, -5) + BAD_CHANNELS + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no above and no tails", -2, [null("above", "tails")]),
        ("no tails and num_obs = 0", -5, [null("tails"), cfg(num_obs=0)])],
}


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    """every case fails validation, so nothing is launched: there is no GPU.  What is not refused gets as far as the next code."""
    import __graft_entry__ as g
    import go1obs_host as G
    g.build_obs_hip()
    fn = getattr(G.load_library(), symbol)
    assert len({label for label, _, _ in CASES[symbol]}) == len(CASES[symbol])
    assert sum(len(spoilers) > 1 for _, _, spoilers in CASES[symbol]) >= 1          # two conditions at once: precedence
    for label, code, spoilers in CASES[symbol]:
        a = Call(G.Go1ObsConfig, G.Go1ObsBuffers, obs_base)
        for spoil in spoilers:
            spoil(a)
        assert fn(None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b), None) == code, (symbol, label)
    if symbol == "go1obs_accumulate":
        # without the privileged channels their buffer, their width and their bins are not looked at; an infinite clip is a clip
        unprivileged = lambda a: (cfg(privileged=0, num_privileged_obs=-7)(a), null("privileged_obs_buf")(a), element("scale", 70, NAN)(a))
        for good in (unprivileged, cfg(clip=INF), element("scale", 2, 1e-30), element("lo", 2, -3e38), element("scale", 79, NAN), cfg(num_obs=96, num_privileged_obs=64)):
            a = Call(G.Go1ObsConfig, G.Go1ObsBuffers, obs_base)
            good(a)
            null("reset_buf")(a)
            assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -3
    elif symbol == "go1obs_break":                                           # break_ids with no id: nothing to launch; without ids num_break is not looked at
        a = Call(G.Go1ObsConfig, G.Go1ObsBuffers, obs_base)
        cfg(num_break=0)(a)
        assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == 0
    if symbol != "go1obs_accumulate":                                        # the others read no step input and test no bins
        a = Call(G.Go1ObsConfig, G.Go1ObsBuffers, obs_base)
        null(*T.INPUTS)(a)
        element("scale", 0, NAN)(a)
        cfg(clip=NAN)(a)
        null("count")(a)
        assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -2


# ---- 3. the model by hand ---------------------------------------------------------------------------------------------------------------------
def play(values, resets=None, span=(0.0, 4.0), warmup_steps=0, clip=100.0, breaks=None):
    """the model on one environment with one channel: a launch per entry of `values`"""
    cfg_ = T.config([span], 1, warmup_steps=warmup_steps, clip=clip)
    resets = resets or [0] * len(values)
    snaps = [dict(obs_buf=np.full((1, 1), v, f32), reset_buf=np.full(1, r, np.uint8)) for v, r in zip(values, resets)]
    st, did = T.run(cfg_, snaps, 1, breaks)
    return st, [int(d["bin"][0, 0]) for d in did]


def only(bin_, value=1):
    return [value if k == bin_ else 0 for k in range(16)]


def test_model_edges_of_the_range_and_of_the_clip():
    # [0, 4): bins a quarter wide.  Exactly lo is bin 0, exactly hi is above, the upper edge of a bin belongs to the next one
    st, bins = play([0.0, 4.0, 0.25, 3.99, -0.0, -0.01, 1e9])
    assert bins == [0, 16, 1, 15, 0, -1, 16] and st.hist[0, :, 0].tolist() == [2, 1] + [0] * 13 + [1] and (st.below[0, 0], st.above[0, 0]) == (1, 2)
    assert st.count[0, 0] == 7 and st.min[0, 0] == f32(-0.01) and st.max[0, 0] == f32(1e9) and st.at_clip[0, 0] == 1
    # -0.0 is a zero: bin 0 of a range from 0, not below
    assert play([-0.0])[0].below[0, 0] == 0
    # exactly +-clip counts at the clip, the next fp32 below it does not
    st, _ = play([3.0, -3.0, np.nextafter(f32(3.0), f32(0.0)), 2.0, -INF, NAN], clip=3.0)
    assert st.at_clip[0, 0] == 3 and st.nonfinite[0, 0] == 2 and st.count[0, 0] == 4
    # NaN and the infinities have no bin and no tail; the fold counts them; the changes next to them are not finite either
    st, bins = play([1.0, NAN, 1.0, INF, -INF, 1.0])
    assert bins == [4, -2, 4, -2, -2, 4] and st.hist[0, :, 0].tolist() == only(4, 3) and (st.below[0, 0], st.above[0, 0], st.nonfinite[0, 0]) == (0, 0, 3)
    assert (st.count[1, 0], st.nonfinite[1, 0]) == (0, 5) and np.isfinite(st.sum).all() and np.isfinite(st.sumsq).all()
    # fp32 binning: the subtract and the multiply round as the kernel's do
    lo, hi = f32(-0.3), f32(0.7)
    st, bins = play([0.1], span=(-0.3, 0.7))
    assert bins == [int((f32(0.1) - lo) * (f32(16) / (hi - lo)))]


def test_model_constant_channel_warm_up_reset_and_first_step():
    # a constant channel: std 0, one bin, every change exactly 0
    st, _ = play([1.5] * 5)
    table, hist, tails = T.reduce(st, [0], 1)
    assert table[0, 0].tolist() == [5.0, 1.5, 0.0, 1.5, 1.5, 0.0] and table[0, 1].tolist() == [4.0, 0.0, 0.0, 0.0, 0.0, 0.0] and hist[0, 0].tolist() == only(6, 5.0)
    assert table[0, 2].tolist() == [1.0, 5.0, 5.0, 0.0, 0.0, 0.0] and not tails.any()
    # the first measured step folds no change; the changes are |v - prev| in fp32
    st, _ = play([1.0, 3.0, 2.5])
    assert (st.count[0, 0], st.count[1, 0], st.sum[1, 0], st.max[1, 0], st.min[1, 0]) == (3, 2, 2.5, 2.0, 0.5)
    # the warm-up boundary: launches 1 and 2 enter nothing (age <= 2), launch 3 is the first measured and folds no change, launch 4 does
    st, bins = play([1.0, 2.0, 3.0, 3.5], warmup_steps=2)
    assert bins == [-3, -3, 12, 14] and (st.count[0, 0], st.count[1, 0], st.sum[1, 0], st.launches[0], st.age[0, 0], st.prev[0, 0]) == (2, 1, 0.5, 4, 4, 3.5)
    assert T.reduce(st, [0], 1)[0][0, 2, :4].tolist() == [1.0, 4.0, 2.0, 0.0]
    # a reset between two steps: the reset step's value is measured, its change is not, the step after it folds the change from the respawned value
    st, _ = play([1.0, 2.0, 0.25, 0.5], resets=[0, 0, 1, 0])
    assert (st.count[0, 0], st.count[1, 0], st.sum[1, 0], st.resets[0]) == (4, 2, 1.25, 1) and st.hist[0, 1, 0] == 1
    # a reset during the warm-up is not a measured reset step
    st, _ = play([1.0, 2.0, 3.0], resets=[1, 0, 1], warmup_steps=1)
    assert (st.resets[0], st.count[0, 0], st.count[1, 0]) == (1, 2, 0)
    # a break from outside: the next launch is a first measured step; accumulators stay
    st, _ = play([1.0, 2.0, 7.0, 7.5], breaks={2: [0]})
    assert (st.count[0, 0], st.count[1, 0], st.sum[1, 0], st.launches[0], st.age[0, 0], st.resets[0]) == (4, 2, 1.5, 4, 2, 1)
    st, _ = play([1.0, 2.0, 3.0, 7.0, 7.5], breaks={3: None, 1: [5, -1]}, warmup_steps=1)      # (ids outside [0, N) are left alone)
    assert (st.count[0, 0], st.count[1, 0], st.sum[1, 0], st.age[0, 0], st.resets[0]) == (4, 2, 1.5, 3, 1)


# ---- 4. go1obs.hip under the SIMT emulator against the model --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1obs_host as G
    return G.load_library(build_emu(g.obs_sources(), "libgo1obs_emu.so"))


def obs_on(device, N, num_obs, num_privileged_obs, lib=None):
    """a go1obs_host.Go1Observations on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1obs_host as G
    B = types.SimpleNamespace(device=torch.device(device), obs_buf=torch.zeros(N, num_obs, device=device),
                              privileged_obs_buf=torch.zeros(N, max(num_privileged_obs, 1), device=device)[:, :num_privileged_obs].contiguous(),
                              reset_buf=torch.zeros(N, dtype=torch.uint8, device=device))
    S = types.SimpleNamespace(num_envs=N, num_obs=num_obs, num_privileged_obs=num_privileged_obs, clip_observations=T.SCRIPT_CLIP)
    family = G.Go1Observations(S, B, lib=lib)
    if torch.device(device).type == "cpu":
        family._stream = lambda: None
    return family, B


def obs_groups(rng, N, groups=3):
    """three groups of which group 1 is empty, some environments at -1 and (from three environments on) one id outside the tables"""
    group = rng.integers(-1, groups, N).astype(np.int32)
    group[group == 1] = 2
    group[0] = groups - 1
    if N >= 3:
        group[1], group[2] = -1, groups
    return group


def drive(family, B, cfg_, snaps, breaks, group, groups):
    """the scripted steps through the library: arm for `groups` groups, then per launch the buffers uploaded and an accumulate, with a
    note_reset in front of the launches `breaks` names; returns read() and the accumulators.  arm() sizes the tables by the largest id it
    is given, so the ids outside the tables are handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    family.arm(inside, cfg_.warmup_steps, spans=cfg_.spans, privileged=cfg_.privileged)
    family.group.copy_(torch.from_numpy(group))
    for k, s in enumerate(snaps):
        if k in breaks:
            family.note_reset(breaks[k])
        for name, a in s.items():
            if a.size:
                getattr(B, name).copy_(torch.from_numpy(a))
        family.accumulate()
    family.disarm()
    res = family.read()
    return res, {k: t.cpu().numpy() for k, t in family.acc.items()}


def same_as_the_model(res, acc, st, cfg_, group, groups):
    """accumulators, state and the three result tables against the model's state `st`, bit for bit"""
    C, N = st.C, st.N
    for k in ACCUMULATORS:
        assert acc[k].shape == (2 * C, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in T.STATE:
        want = getattr(st, k)
        assert res["env_" + k].shape == want.shape and bits(res["env_" + k].view(want.dtype)) == bits(want), k
    table, hist, tails = T.reduce(st, group, groups)
    for key, rows in (("value", table[:, :C]), ("delta", table[:, C:2 * C])):
        assert res[key].shape == (groups, C, 6) and np.array_equal(np.isnan(res[key]), np.isnan(rows)) and same(res[key], rows), key
    assert res["groups"].shape == (groups, 4) and bits(res["groups"]) == bits(table[:, 2 * C, :4]) and not table[:, 2 * C, 4:].any()
    assert res["hist"].shape == (groups, C, 16) and bits(res["hist"]) == bits(hist) and res["tails"].shape == (groups, C, 3) and bits(res["tails"]) == bits(tails)
    assert res["edges"].shape == (C, 17) and res["clip"] == float(cfg_.clip) and res["privileged"] == cfg_.privileged
    for c, (lo, hi) in enumerate(cfg_.spans):
        assert res["edges"][c, 0] == lo and res["edges"][c, 16] == hi
    return table, hist, tails


def check_against_the_model(res, acc, cfg_, snaps, breaks, kind, group, groups, N):
    """the library's results against tests/obs_ref.py, bit for bit; then that the script drove every event it was written to drive"""
    st, did = T.run(cfg_, snaps, N, breaks)
    table, hist, tails = same_as_the_model(res, acc, st, cfg_, group, groups)
    steps, C, measured = len(snaps), cfg_.C, len(snaps) - cfg_.warmup_steps
    broken = np.isin(np.arange(N), breaks[T.SCRIPT_BREAK])
    assert (st.launches == steps).all() and (st.age[:, ~broken] == steps).all() and (st.age[:, broken] == cfg_.warmup_steps + steps - T.SCRIPT_BREAK).all()
    total = st.hist.astype(np.int64).sum(axis=1) + st.below + st.above + st.nonfinite[:C]
    assert (total == measured).all() and (st.count[:C] + st.nonfinite[:C] == measured).all()
    resets = np.stack([(s["reset_buf"] != 0) for s in snaps[cfg_.warmup_steps:]]).sum(axis=0)
    assert (st.resets == resets + broken).all()                                             # (a break counts as a reset from outside)
    # a change per measured step but the first, the reset steps and the step after the break
    changes = st.count[C:].astype(np.int64) + st.nonfinite[C:]
    quiet = np.stack([s["reset_buf"] == 0 for s in snaps])                                # (steps, N): no reset step
    quiet[:cfg_.warmup_steps + 1] = False
    quiet[T.SCRIPT_BREAK, broken] = False
    assert (changes == quiet.sum(axis=0)[None, :]).all() and changes.max() <= measured - 1
    for sums in (st.sum, st.sumsq):
        assert np.isfinite(sums).all()
    if N >= len(T.KINDS):
        steady, resetting, constant, odd, outside, edges, random_ = (kind == k for k in range(len(T.KINDS)))
        even = np.arange(C) % 2 == 0
        assert (st.resets[resetting & ~broken] == 2).all() and not st.resets[steady & ~broken].any() and st.resets[random_].sum() > 0
        assert (st.max[C:][:, constant & ~broken] == 0).all() and (st.min[:C][:, constant] == st.max[:C][:, constant]).all()
        assert (st.nonfinite[:C][np.ix_(even, odd)] == 3).all() and not st.nonfinite[:C][np.ix_(~even, odd)].any() and (st.nonfinite[C:][np.ix_(even, odd & ~broken)] >= 4).all()
        assert (st.below[np.ix_(even, outside)] == measured).all() and (st.above[np.ix_(~even, outside)] == measured).all() and (st.at_clip[:, outside] == measured).all()
        # the walk through exactly lo (bin 0, launches 3 and 8), exactly hi (above, 4 and 10), +clip and -clip (5 and 6), -0.0 (7)
        assert (st.hist[:, 0, edges] >= 2).all() and (st.above[:, edges] >= 2).all() and (st.at_clip[:, edges] >= 2).all()
        assert all((did[t]["bin"][:, edges] == 0).all() for t in (3, 8)) and all((did[t]["bin"][:, edges] == 16).all() for t in (4, 10))
        assert st.at_clip[:, steady | random_].sum() > 0                          # the clipped normal reaches +-clip itself
    assert res["groups"][:, 0].sum() == np.isin(group, range(groups)).sum() and (res["groups"][:, 1] == steps * res["groups"][:, 0]).all()
    assert (res["groups"][:, 2] == measured * res["groups"][:, 0]).all() and res["groups"][1].tolist() == [0.0] * 4
    assert np.isnan(table[1, :2 * C, 1:5]).all() and not hist[1].any() and not tails[1].any()
    return st


# (N, num_obs, num_privileged_obs, privileged).  N = 1: one thread per channel; 64: one wavefront; 257: a workgroup plus one lane per
# channel; 600: three ragged workgroups per channel, three terms per reduction thread and 38 environments per bin slice.  C = 5 beside
# three privileged columns that are not measured; C = 70 + 9 with them
SCRIPTS = [(N, *shape) for shape in ((5, 3, False), (70, 9, True)) for N in (1, 64, 257, 600)]


@pytest.mark.parametrize("N,num_obs,num_priv,privileged", SCRIPTS)
def test_emulated_observation_kernels_follow_the_model(emu, N, num_obs, num_priv, privileged):
    groups = 3
    rng = np.random.default_rng(1700 + N + num_obs)
    cfg_, snaps, breaks, kind = T.scripted_steps(rng, N, num_obs, num_priv, privileged)
    assert len(snaps) == T.SCRIPT_STEPS == 12 and list(breaks) == [T.SCRIPT_BREAK] and cfg_.warmup_steps == 2 and cfg_.C == (79 if privileged else 5)
    assert N < len(T.KINDS) or set(kind.tolist()) == set(range(len(T.KINDS)))
    group = obs_groups(rng, N, groups)
    family, B = obs_on("cpu", N, num_obs, num_priv, lib=emu)
    res, acc = drive(family, B, cfg_, snaps, breaks, group, groups)
    c = family.cfg
    assert (c.num_envs, c.num_groups, c.num_obs, c.num_privileged_obs, c.privileged, c.num_break) == (N, groups, num_obs, num_priv, int(privileged), 0)
    assert bits(np.array(list(c.lo)[:cfg_.C], f32)) == bits(cfg_.lo) and bits(np.array(list(c.scale)[:cfg_.C], f32)) == bits(cfg_.scale) and c.clip == cfg_.clip
    check_against_the_model(res, acc, cfg_, snaps, breaks, kind, group, groups, N)
    again = family.read()                                                    # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ["groups", "hist", "tails"] + ["env_" + k for k in T.STATE]) and same(again["value"], res["value"])
    for bad in (dict(spans=cfg_.spans[:-1]), dict(spans=[(0.0, NAN)] + cfg_.spans[1:]), dict(spans=[(INF, 0.0)] + cfg_.spans[1:]),
                dict(spans=[(1.0, 1.0)] + cfg_.spans[1:]), dict(spans=[(2.0, 1.0)] + cfg_.spans[1:]), dict(spans=cfg_.spans, privileged=not privileged)):
        with pytest.raises(ValueError, match="observations:"):
            family.arm(np.zeros(N, np.int32), **dict(dict(privileged=privileged), **bad))
    with pytest.raises(RuntimeError, match="go1obs_accumulate failed: -12"):
        family.cfg.scale[0] = 0.0
        family.accumulate()


# ---- 5. the environment hooks without a GPU -----------------------------------------------------------------------------------------------------
def plane_env(monkeypatch, num_envs=16, noise=True):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    for module in ("go1eval_host", "go1obs_host"):
        monkeypatch.delitem(sys.modules, module, raising=False)
    c = apply_train_config(make_cfg(), num_envs=num_envs)
    c.terrain.mesh_type = "plane"
    c.noise.add_noise = noise
    torch.manual_seed(0)
    return VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)


def test_observation_hooks_on_cpu_buffers(monkeypatch):
    from go1_gym.envs.base.legged_robot import LeggedRobot
    from test_family_wiring import FAMILIES, REWARD, STATE_FAMILIES, Stub
    import test_family_wiring as wiring
    # stubs for the families up to the reward family only: the later ones stay None unless this test puts its own stub there, so the
    # launch-order and refusal checks below name exactly the families they set
    STEPPED = wiring.STEPPED[:REWARD + 1]
    put_stubs = functools.partial(wiring.put_stubs, stepped=STEPPED)
    env = plane_env(monkeypatch)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_observation_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_observation_metrics, env.read_observation_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert all(m not in sys.modules for m in ("go1eval_host", "go1obs_host")) and env._obs is None                # never measured: no host module
    env.step(torch.zeros(16, 12))                                             # and stepping goes on
    signature = inspect.signature(env.start_observation_metrics)
    assert {k: p.default for k, p in signature.parameters.items() if k != "groups"} == dict(warmup_steps=0, ranges=None, privileged=True)
    assert list(signature.parameters) == ["groups", "warmup_steps", "ranges", "privileged"]
    for name in ("start_observation_metrics", "stop_observation_metrics", "read_observation_metrics"):
        assert (getattr(LeggedRobot, name).__doc__ or "").strip(), name
    # its row of the one table, directly after the sensitivity family's
    k = [row[0] for row in env._FAMILIES].index("observations")
    assert env._FAMILIES == FAMILIES and env._FAMILIES[k] == ("observations", "_obs", "go1obs_host", "Go1Observations", "accumulate") and env._FAMILIES[k - 1][0] == "sensitivity"
    assert env._STATE_FAMILIES == STATE_FAMILIES and env._STATE_FAMILIES[k] == ("observations", "_obs") and env._STEPPED[k - 2:k] == (("_sens", "accumulate"), ("_obs", "accumulate"))
    assert env._HOST["_obs"] == ("go1obs_host", "Go1Observations") and all(len(row) == 5 for row in env._FAMILIES) and env._FAMILIES[-1][0] == "observations"
    assert list(env._HOST)[-2:] == ["_obs", "_push"] and len(env._HOST) == 15
    # launched last, after the sensitivity family's
    log = []

    class ObsStub(Stub):
        def note_reset(self, *args):
            self.log.append((self.attr, "note_reset", args))

        def snapshot(self, *args):
            self.log.append((self.attr, "snapshot", args))
    put_stubs(env, log)
    env._episodes, env._sens, env._obs = Stub("_episodes", log), ObsStub("_sens", log), ObsStub("_obs", log)
    env.step(torch.zeros(16, 12))
    assert [(attr, method) for attr, method, _ in log] == STEPPED + [("_episodes", "accumulate"), ("_sens", "accumulate"), ("_obs", "accumulate")] and log[-1][2] == ()
    env._obs.armed = False
    del log[:]
    env.step(torch.zeros(16, 12))
    assert [(attr, method) for attr, method, _ in log] == STEPPED + [("_episodes", "accumulate"), ("_sens", "accumulate")]
    # a reset from outside puts robots elsewhere between two steps: an armed family is told which, a stopped one is not
    env._reward = env._sens = None
    del log[:]
    env.reset_idx(torch.tensor([1, 3]))
    assert log == []
    env._obs.armed = True
    env.reset_idx(torch.tensor([1, 3]))
    env.reset_idx(torch.tensor([], dtype=torch.int64))
    env.reset_idx(torch.arange(16))
    assert [(a, m) for a, m, _ in log] == [("_obs", "note_reset")] * 2 and log[0][2][0].tolist() == [1, 3] and log[1][2] == (None,)
    # load_state() names it after the sensitivity family and before the camera
    put_stubs(env, log)
    env._sens = Stub("_sens", log)
    env._state = types.SimpleNamespace(restore=lambda *a, **k: pytest.fail("restored"))
    env._render = types.SimpleNamespace(any_armed=True)
    with pytest.raises(RuntimeError) as e:
        env.load_state(None)
    assert "refused while metrics, behaviour, trace, terrain, joints, feet, trunk, gait, spectrum, placement, rewards, episodes, sensitivity, observations, camera are armed" in str(e.value)
    env._render = None
    put_stubs(env, [], armed=False)
    env._episodes.armed = env._sens.armed = False
    with pytest.raises(RuntimeError, match=r"refused while observations is armed: stop it first"):
        env.load_state(None)


# ---- 6. the channels ----------------------------------------------------------------------------------------------------------------------------
def test_channel_names_follow_the_configurations_switches():
    from go1_gym_learn.eval_metrics import observations as O
    from go1_gym_learn.eval_metrics.behaviour import COMMAND_INDEX
    from golden.variants import VARIANTS
    from util import make_cfg_variant
    assert O.COMMANDS[:14] == sorted(COMMAND_INDEX, key=COMMAND_INDEX.get) and list(O.COMMAND_LIMITS) == O.COMMANDS
    for variant in ["train"] + sorted(VARIANTS):
        c = make_cfg_variant(variant)
        names, kinds = O.channel_names(c), O.channel_kinds(c)
        assert len(names) == len(kinds) == c.env.num_observations and len(set(names)) == len(names), variant
        assert [O.kind_of(n) for n in names] == kinds, variant
        both = O.channel_names(c, privileged=True)
        assert both[:len(names)] == names and both[len(names):] == [f"priv_{k}" for k in range(c.env.num_privileged_obs)], variant
        spans = O.channel_spans(c, both, O.channel_kinds(c, True))
        assert len(spans) == len(both) and all(np.isfinite(lo) and np.isfinite(hi) and f32(hi) > f32(lo) for lo, hi in spans), variant
    c = make_cfg_variant("train")
    names = O.channel_names(c)
    assert names[:3] == ["gravity_x", "gravity_y", "gravity_z"] and names[3:18] == ["cmd_" + n for n in O.COMMANDS] and names[18] == "dof_pos_FL_hip"
    assert names[29] == "dof_pos_RR_calf" and names[30] == "dof_vel_FL_hip" and names[42] == "action_FL_hip" and names[54] == "last_action_FL_hip"
    assert names[66:] == ["clock_FL", "clock_FR", "clock_RL", "clock_RR"] and len(names) == 70
    alt = O.channel_names(make_cfg_variant("alt"))
    assert alt[:9] == ["lin_vel_x", "lin_vel_y", "lin_vel_z", "ang_vel_x", "ang_vel_y", "ang_vel_z", "gravity_x", "gravity_y", "gravity_z"]
    assert alt[-10:] == ["timing"] + ["clock_" + leg for leg in O.LEGS] + ["yaw"] + ["contact_" + leg for leg in O.LEGS] and "last_action_FL_hip" not in alt
    # the default ranges: one rule per kind, overridden by name before kind
    d = O.default_ranges(c)
    assert d["gravity_z"] == (-1.0, 1.0) and d["clock_RL"] == (-1.0, 1.0) and d["action_FL_hip"] == (-c.normalization.clip_actions, c.normalization.clip_actions)
    assert d["cmd_vx"] == tuple(x * c.obs_scales.lin_vel for x in c.commands.limit_vel_x) and d["cmd_yaw"] == tuple(x * c.obs_scales.ang_vel for x in c.commands.limit_vel_yaw)
    assert d["dof_vel_RL_calf"] == (-30.0 * c.obs_scales.dof_vel, 30.0 * c.obs_scales.dof_vel) and d["priv_0"] == (-1.0, 1.0) and list(d) == O.channel_names(c, True)
    assert O.default_ranges(make_cfg_variant("alt"))["contact_FL"] == (0.0, 1.0)
    kinds = O.channel_kinds(c)
    spans = O.channel_spans(c, names, kinds, {"clock": (-2.0, 2.0), "clock_FR": (-3.0, 3.0), "gravity_x": (-0.5, 0.5)})
    assert spans[66] == (-2.0, 2.0) and spans[67] == (-3.0, 3.0) and spans[0] == (-0.5, 0.5) and spans[1] == (-1.0, 1.0)
    with pytest.raises(ValueError, match="observations: 'grip'"):
        O.channel_spans(c, names, kinds, {"grip": (0.0, 1.0)})
    assert "PLACEHOLDER" in O.default_ranges.__doc__ and "placeholder" in O.__doc__
    # ranges_from: the realised minimum and maximum, widened
    value = np.zeros((2, 3, 6))
    value[0, 0], value[1, 0], value[0, 1] = [5, 0, 0, -1.0, 2.0, 0], [5, 0, 0, -3.0, 1.0, 0], [4, 0, 0, 0.5, 0.5, 0]
    got = O.ranges_from(dict(channels=["a", "b", "c"], value=value), margin=0.1)
    assert got == dict(a=(-3.5, 2.5), b=(0.5 - O.MIN_WIDTH, 0.5 + O.MIN_WIDTH))


def test_named_columns_equal_their_definitions_on_the_oracle(monkeypatch, emu):
    """the oracle-backed environment with noise off, random actions: the columns channel_names() names hold what their names say; the
    emulated kernels are stepped by the environment itself and end bit-equal to the model fed the obs_buf copies"""
    import go1obs_host as G
    from go1_gym_learn.eval_metrics import observations as O
    N, STEPS = 16, 12
    env = plane_env(monkeypatch, N, noise=False)
    names = O.channel_names(env.cfg, privileged=True)
    kinds = O.channel_kinds(env.cfg, privileged=True)
    assert len(names) == env.num_obs + env.num_privileged_obs
    col = lambda prefix: [k for k, n in enumerate(names) if n.startswith(prefix)]
    env.reset()
    env._obs = G.Go1Observations(env.sim_config, env.buffers, lib=emu)        # what start_observation_metrics does where there is a GPU
    env._obs._stream = lambda: None
    env._obs.names, env._obs.kinds = names, kinds
    spans = O.channel_spans(env.cfg, names, kinds)
    group = (torch.arange(N) % 2).to(torch.int32)
    env._obs.arm(group, 1, spans=spans, privileged=True)
    g = torch.Generator().manual_seed(3)
    snaps = []
    for k in range(STEPS):
        if k == 6:
            env.reset_idx(torch.tensor([2, 5]))
        env.step(0.5 * torch.randn(N, 12, generator=g))
        obs = env.obs_buf
        assert torch.equal(obs[:, col("dof_pos_")], ((env.dof_pos - env.default_dof_pos) * env.obs_scales.dof_pos))
        assert torch.equal(obs[:, col("gravity_")], env.projected_gravity) and torch.equal(obs[:, col("cmd_")], env.commands * env.commands_scale)
        assert torch.equal(obs[:, col("action_")], env.actions) and torch.equal(obs[:, col("clock_")], env.clock_inputs)
        assert torch.equal(obs[:, col("dof_vel_")], env.dof_vel * env.obs_scales.dof_vel)
        snaps.append(dict(obs_buf=obs.numpy().copy(), privileged_obs_buf=env.privileged_obs_buf.numpy().copy(), reset_buf=env.reset_buf.numpy().astype(np.uint8)))
    env._obs.disarm()
    res = dict(env._obs.read(), channels=names, kinds=kinds)                  # (read_observation_metrics() without its refusal of CPU buffers)
    cfg_ = T.config(spans, env.num_obs, env.num_privileged_obs, True, warmup_steps=1, clip=env.cfg.normalization.clip_observations)
    st, _ = T.run(cfg_, snaps, N, {6: [2, 5]})
    same_as_the_model(res, {k: t.numpy() for k, t in env._obs.acc.items()}, st, cfg_, group.numpy(), 2)
    assert st.age[0].tolist() == [7 if e in (2, 5) else STEPS for e in range(N)] and res["groups"][:, 2].sum() == N * (STEPS - 1)
    assert res["channels"] == names and res["kinds"] == kinds


# ---- 7. profiles, shift and ranking by hand ---------------------------------------------------------------------------------------------------
def hand_profile(hist, below=0.0, above=0.0, mean=0.0, std=1.0, at_clip=0.0, delta_mean=0.1, lo=-1.0, hi=1.0, name="a"):
    n = float(np.sum(hist) + below + above)
    return dict(channels=[name], kinds=["other"], edges=[np.linspace(lo, hi, 17).tolist()], clip=100.0, count=[n], mean=[mean], std=[std], min=[lo], max=[hi], nonfinite=[0.0],
                hist=[list(map(float, hist))], below=[float(below)], above=[float(above)], at_clip=[at_clip], delta_count=[n - 1], delta_mean=[delta_mean], delta_std=[0.0],
                delta_max=[delta_mean], env_steps=n, resets=0.0)


def test_shift_and_ranking_by_hand():
    from go1_gym_learn.eval_metrics import observations as O
    a = hand_profile([4.0] * 16, below=2.0, above=2.0, at_clip=1.0)
    s = O.shift(a, a)
    assert s["channels"] == ["a"] and (s["mean_shift"], s["js"], s["novel"]) == ([0.0], [0.0], [0.0]) and s["std_ratio"] == [1.0] and s["jitter_ratio"] == [1.0]
    assert s["clip_share_a"] == s["clip_share_b"] == [1.0 / 68.0] and list(s) == ["channels"] + O.SHIFT_KEYS
    # disjoint histograms: one bit, and every sample of b lies where a has none
    left, right = hand_profile([8.0] * 8 + [0.0] * 8), hand_profile([0.0] * 8 + [8.0] * 8)
    s = O.shift(left, right)
    assert s["js"] == [1.0] and s["novel"] == [1.0]
    assert O.shift(hand_profile([8.0] * 16), hand_profile([0.0] * 16, above=5.0))["js"] == [1.0]          # the tails are cells
    # half of b in new cells: novel 0.5, and the divergence is 0.5 * (1 * log2(4/3)) + 0.5 * (0.5 * log2(2/3) + 0.5 * 1) by hand
    s = O.shift(left, hand_profile([4.0] * 16))
    assert s["novel"] == [0.5] and abs(s["js"][0] - (0.5 * np.log2(4.0 / 3.0) + 0.5 * (0.5 * np.log2(2.0 / 3.0) + 0.5))) < 1e-15
    # a doubled standard deviation, a mean one standard deviation up, twice the jitter
    s = O.shift(hand_profile([4.0] * 16, mean=0.25, std=0.5), hand_profile([4.0] * 16, mean=0.75, std=1.0, delta_mean=0.2))
    assert s["std_ratio"] == [2.0] and s["mean_shift"] == [1.0] and s["jitter_ratio"] == [2.0]
    # a constant baseline: the floor (hi - lo) / 1024 stands in for its standard deviation and for its jitter
    s = O.shift(hand_profile(only(8, 9), std=0.0, delta_mean=0.0), hand_profile(only(8, 9), mean=2.0 / 1024.0, std=4.0 / 1024.0, delta_mean=6.0 / 1024.0))
    assert s["mean_shift"] == [1.0] and s["std_ratio"] == [2.0] and s["jitter_ratio"] == [3.0]
    # nothing measured: NaN, not an error
    s = O.shift(hand_profile([0.0] * 16), left)
    assert np.isnan(s["js"][0]) and np.isnan(s["novel"][0])
    # refused: other edges, other channels
    with pytest.raises(ValueError, match="shift: the two profiles have other bin edges"):
        O.shift(left, hand_profile([8.0] * 16, hi=2.0))
    with pytest.raises(ValueError, match="shift: the two profiles have other channels"):
        O.shift(left, hand_profile([8.0] * 16, name="b"))
    fake = dict(channels=["p", "q", "r", "s"], js=[0.1, None, 0.4, 0.1], mean_shift=[-3.0, 2.0, NAN, 0.5], std_ratio=[0.25, 2.0, 1.0, None], novel=[0.0] * 4,
                clip_share_a=[0.0] * 4, clip_share_b=[0.0] * 4, jitter_ratio=[1.0] * 4)
    assert [n for n, _ in O.rank_channels(fake)] == ["r", "p", "s", "q"] and O.rank_channels(fake)[0] == ("r", 0.4)
    assert [n for n, _ in O.rank_channels(fake, "mean_shift")] == ["p", "q", "s", "r"] and [n for n, _ in O.rank_channels(fake, "std_ratio")] == ["p", "q", "r", "s"]
    assert [n for n, _ in O.rank_channels(fake, "novel")] == ["p", "q", "r", "s"]                        # a tie keeps the channels' order
    with pytest.raises(ValueError, match="rank_channels:"):
        O.rank_channels(fake, "kl")


def model_result(rng, N=40, T_=30, C=6, groups=2):
    """a read()-shaped result from the model on random rows, its inputs, and the (T, C) rows of every environment"""
    spans = T.script_spans(C)
    cfg_ = T.config(spans, C, clip=2.5)
    rows = np.clip((1.3 * rng.standard_normal((T_, N, C))).astype(f32), -2.5, 2.5)
    rows[:, :, 5] = f32(0.75)                                                 # a constant channel
    rows[3, 1, 2], rows[9, 2, 0] = np.nan, np.inf
    resets = rng.random((T_, N)) < 0.1
    snaps = [dict(obs_buf=rows[t], reset_buf=resets[t].astype(np.uint8)) for t in range(T_)]
    st, _ = T.run(cfg_, snaps, N)
    group = (np.arange(N) % groups).astype(np.int32)
    table, hist, tails = T.reduce(st, group, groups)
    import go1obs_host as G
    names = [f"ch{c}" for c in range(C)]
    res = dict(channels=names, kinds=["other"] * C, edges=G.bin_edges(cfg_.spans), clip=2.5, value=table[:, :C], delta=table[:, C:2 * C], hist=hist, tails=tails,
               groups=table[:, 2 * C, :4])
    return res, rows, resets, group


def test_profile_pooling_and_profile_from_array_against_the_model():
    from go1_gym_learn.eval_metrics import observations as O
    rng = np.random.default_rng(77)
    res, rows, resets, group = model_result(rng)
    T_, N, C = rows.shape
    exact = ("count", "nonfinite", "hist", "below", "above", "at_clip", "min", "max", "delta_count", "delta_max", "env_steps", "resets")
    close = ("mean", "std", "delta_mean", "delta_std")

    def stacked(members):
        """the rows of the environments `members` one after the other, the first row of each a reset (no change across the seam)"""
        obs = np.concatenate([rows[:, e] for e in members])
        first = np.concatenate([np.concatenate([[True], resets[1:, e]]) for e in members])
        return obs, first

    def compare(p, q):
        assert p["channels"] == q["channels"] and p["edges"] == q["edges"] and p["clip"] == q["clip"] and list(p) == list(q)
        for key in exact:
            assert p[key] == q[key], key
        for key in close:
            a, b = np.array(p[key], np.float64), np.array(q[key], np.float64)
            assert np.all(np.abs(a - b) <= 1e-9 * np.maximum(np.abs(b), 1e-300) + (b == 0) * 1e-12), key
    for g in (0, 1, None):
        members = [e for e in range(N) if g is None or group[e] == g]
        obs, first = stacked(members)
        p, q = O.profile(res, g), O.profile_from_array(obs, res["channels"], res["edges"], res["clip"], resets=first)
        # (the model counts the reset steps of row 0 as resets too; the array's first rows are seams: compare what both mean)
        q["resets"] = float(resets[:, members].sum())
        compare(p, q)
        json.dumps(p, allow_nan=False), json.dumps(q, allow_nan=False)
        assert p["count"][2] == len(members) * T_ - (1 in members) and p["nonfinite"][0] == float(2 in members) and p["std"][5] == 0.0 and p["delta_max"][5] == 0.0
    # pooling two groups equals the profile of their union: exact where sums of integers, 1e-9 where fp64 sums differ by order
    pooled = O.profile(res)
    for key in ("count", "hist", "below", "above", "at_clip", "delta_count"):
        assert np.array_equal(np.array(pooled[key]), np.array(O.profile(res, 0)[key]) + np.array(O.profile(res, 1)[key])), key
    assert pooled["min"] == np.minimum(O.profile(res, 0)["min"], O.profile(res, 1)["min"]).tolist()
    assert O.shift(pooled, pooled)["js"] == [0.0] * C
    with pytest.raises(ValueError, match="profile_from_array:"):
        O.profile_from_array(rows[:, 0], res["channels"][:-1], res["edges"], 2.5)
    assert "unpickl" not in inspect.getsource(O.profile_from_array).replace("no unpickling", "") and "pickle" not in inspect.getsource(O)


# ---- 8. the sweep's host pieces and the tool -----------------------------------------------------------------------------------------------------
def fixed_result(rng=None, baseline=None):
    """a run_observation_sweep result of two cells from the model"""
    from go1_gym_learn.eval_metrics import sweep
    res, _, _, _ = model_result(rng or np.random.default_rng(5))
    res["kinds"] = ["gravity", "gravity", "command", "dof_pos", "dof_pos", "clock"]
    res["obs_groups"] = res.pop("groups")
    return dict(res, preset="rand_large", cells=sweep.grid_cells(dict(vx=[0.5, 1.0], yaw=[0.0], gait=[sweep.GAITS["trotting"]])), privileged=True, baseline=baseline,
                metrics={}, groups=np.zeros((2, 5)), num_envs=40, steps=30, warmup_steps=0, seed=1, dt=0.02)


def test_observation_table_json_and_figure(tmp_path):
    from go1_gym_learn.eval_metrics import observations as O
    res = fixed_result()
    md = O.observation_markdown_table(res).splitlines()
    assert md[0] == "| vx | yaw | gait | kind | channels | samples | in range | below | above | at clip | mean delta |"
    assert len(md) == 2 + 2 * 4 + 2 + 2 and len({line.count("|") for line in md[:10]}) == 1 and md[2].startswith("| 0.5 | 0 | 0.5/0/0 | gravity | 2 | 1200 |")
    assert md[10] == "" and "placeholders" in md[11] and md[12].startswith("- vx 0.5, yaw 0, gait 0.5/0/0: by the share outside the range: ")
    js = json.loads(json.dumps(O.observation_to_json(res), allow_nan=False))
    assert js["channels"] == res["channels"] and js["preset"] == "rand_large" and len(js["profiles"]) == 2 and js["shift"] is None and js["ranking"] is None
    assert js["count"] == O.profile(res)["count"] and js["profiles"][1] == json.loads(json.dumps(O.profile(res, 1))) and js["cells"][1]["vx"] == 1.0
    assert np.array(js["hist"]).shape == (6, 16) and np.array(js["edges"]).shape == (6, 17) and js["obs_groups"][0][0] == 20.0
    path = tmp_path / "observations.png"
    O.plot_observations(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000
    # a second run against the first one's JSON: cell by cell when the cells are equal, against the pooled profile otherwise
    (tmp_path / "first.json").write_text(json.dumps(js))
    second = fixed_result(np.random.default_rng(6), baseline=O.load_baseline(str(tmp_path / "first.json")))
    assert O.baselines(second["baseline"], second["cells"]) == js["profiles"]
    shifts = O.cell_shifts(second)
    assert len(shifts) == 2 and shifts[0] == O.shift(js["profiles"][0], O.profile(second, 0)) and 0.0 < max(shifts[0]["js"][:5]) < 0.2 and shifts[0]["js"][5] == 0.0
    other = dict(second, cells=second["cells"][::-1])
    assert O.baselines(other["baseline"], other["cells"]) == [js, js] and O.cell_shifts(other)[1] == O.shift(js, O.profile(second, 1))
    md = O.observation_markdown_table(second).splitlines()
    assert md[0].endswith("| mean delta | js max [bit] | js mean [bit] | novel max |") and ": by js: " in md[12] and md[12].count("(") == 6
    js2 = json.loads(json.dumps(O.observation_to_json(second), allow_nan=False))
    assert js2["shift"][1]["channels"] == res["channels"] and [n for n, _ in js2["ranking"][0]] == [n for n, _ in O.rank_channels(shifts[0])]
    O.plot_observations(second, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    # a profile from an array is a baseline too
    log = O.profile_from_array(np.zeros((10, 6), f32), res["channels"], res["edges"], 2.5)
    assert O.baselines(log, second["cells"]) == [log, log]


def test_tool_accepts_an_observation_sweep(tmp_path, monkeypatch, capsys):
    from test_family_wiring import MODES
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import observations, sweep
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    earlier = tmp_path / "earlier.json"
    earlier.write_text("{}")
    a = eval_sweep.parse_args(base + ["--observations", "--vx", "0.5", "1.0", "--envs", "64", "--steps", "40", "--warmup-steps", "5", "--presets", "rand_large",
                                      "--against", str(earlier), "--no-privileged"])
    assert a.observations and not a.sensitivity and (a.vx, a.envs, a.steps, a.against, a.no_privileged) == ([0.5, 1.0], 64, 40, str(earlier), True)
    plain = eval_sweep.parse_args(base + ["--observations"])
    assert (plain.against, plain.no_privileged) == (None, False) and plain.observations
    nothing = eval_sweep.parse_args(base)
    assert not nothing.observations and nothing.against is None and nothing.no_privileged is None
    assert eval_sweep.parse_args(base + ["--observations", "--terrain", "plane"]).terrain == "plane"
    for other in list(MODES.values()) + [["--episodes"], ["--sensitivity"]]:  # every other mode excludes it, whichever comes first
        for argv in (["--observations"] + other, other + ["--observations"]):
            with pytest.raises(SystemExit) as e:
                eval_sweep.parse_args(base + argv)
            assert e.value.code == 2, argv
    for bad in (["--against", str(earlier)], ["--no-privileged"], ["--trunk", "--no-privileged"], ["--sensitivity", "--against", str(earlier)],
                ["--observations", "--against", str(tmp_path / "absent.json")], ["--observations", "--gamma", "0.9"], ["--observations", "--pair", "friction", "payload"]):
        with pytest.raises(SystemExit) as e:
            eval_sweep.parse_args(base + bad)
        assert e.value.code == 2, bad
    assert callable(eval_sweep.run_observations) and len(inspect.signature(eval_sweep.run_observations).parameters) == 3
    assert "--observations --presets rand_large --against" in eval_sweep.__doc__ and "placeholders" in eval_sweep.__doc__
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(observations, "run_observation_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    grid = dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits])
    eval_sweep.run_observations(a, None, grid)
    assert seen == dict(preset="rand_large", grid=grid, num_envs=64, steps=40, warmup_steps=5, seed=1, terrain=None, against=str(earlier), no_privileged=True)
    js = json.load(open(tmp_path / "eval" / "rand_large_observations.json"))
    assert js["preset"] == "rand_large" and js["channels"][0] == "ch0" and len(js["profiles"]) == 2
    md = (tmp_path / "eval" / "rand_large_observations.md").read_text()
    assert "| gravity | 2 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "rand_large_observations.png").read_bytes()[:4] == b"\x89PNG"


def test_the_sweep_runs_beside_the_scalar_table(monkeypatch, tmp_path):
    """a recording environment as tests/test_family_wiring.py's: the shared call sequence, the start's keywords and the result's keys"""
    from go1_gym_learn.eval_metrics import observations, sweep
    from test_family_wiring import COMMON_KEYS, N, NUM_COMMANDS, STEPS, WARMUP, RecordingEnv, ZeroPolicy
    cells_in = dict(vx=[0.5, 1.0], yaw=[0.0, 0.5], gait=[sweep.GAITS["trotting"]])
    cells = sweep.grid_cells(cells_in)
    family = dict(channels=["a", "b"], kinds=["gravity", "clock"], edges=np.zeros((2, 17)), clip=100.0, value=np.zeros((4, 2, 6)), delta=np.zeros((4, 2, 6)),
                  hist=np.zeros((4, 2, 16)), tails=np.zeros((4, 2, 3)), groups=np.ones((4, 4)))

    class Env(RecordingEnv):
        def __init__(self, spoil=False):
            super().__init__("gait", 4, spoil)               # (any stem the recording base knows: the family below replaces what it cans)
            self.env.family = family
    built_env = Env()
    monkeypatch.setattr(sweep, "build_eval_env", lambda preset, num_envs, seed, terrain=None, configure=None: (built_env, None))
    baseline = dict(channels=["a", "b"], edges=[np.linspace(-1, 1, 17).tolist(), np.linspace(0, 2, 17).tolist()])
    (tmp_path / "b.json").write_text(json.dumps(baseline))
    res = observations.run_observation_sweep(ZeroPolicy(), "rand_large", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5, terrain="plane",
                                             against=str(tmp_path / "b.json"), no_privileged=True, ranges=dict(b=(0.0, 4.0)))
    log = built_env.env.log
    assert [entry[0] for entry in log] == ["start_metrics", "start_observation_metrics", "step", "step", "step", "stop_metrics", "stop_observation_metrics", "read_metrics",
                                           "read_observation_metrics"]
    assert log[1][1][0] is log[0][1][0] and log[1][2] == dict(warmup_steps=WARMUP, ranges=dict(a=(-1.0, 1.0), b=(0.0, 4.0)), privileged=False)
    assert torch.equal(built_env.first, sweep.command_table(cells, NUM_COMMANDS, "cpu")[(torch.arange(N) % 4).long()])
    own = ["channels", "kinds", "edges", "clip", "value", "delta", "hist", "tails", "obs_groups", "privileged", "baseline"]
    assert sorted(res) == sorted(COMMON_KEYS + own) and res["obs_groups"] is family["groups"] and res["baseline"] == baseline and res["privileged"] is False
    assert all(res[k] is family[k] for k in ("edges", "value", "delta", "hist", "tails")) and (res["preset"], res["cells"], res["dt"]) == ("rand_large", cells, 0.02)
    built_env = Env()
    res = observations.run_observation_sweep(ZeroPolicy(), "rand_large", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5)
    assert built_env.env.log[1][2] == dict(warmup_steps=WARMUP, ranges=None, privileged=True) and res["baseline"] is None
    built_env = Env(spoil=True)
    with pytest.raises(RuntimeError) as e:
        observations.run_observation_sweep(ZeroPolicy(), "rand_large", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5)
    assert str(e.value) == "run_observation_sweep: an environment left its grid cell's commands during the rollout"
