"""CPU checks of the episode family (include/go1episode.h, libgo1episode.so): the ctypes mirrors and the exported symbols against the
header, the build's source list (as the compiler reads it), flags and stamp, the refusals without a GPU, the model of
tests/episode_ref.py on hand-computed episodes, the Kaplan-Meier estimate against a hand-computed example and against a per-episode
product-limit estimate, go1episode.hip itself under the SIMT emulator against that model bit for bit (accumulators, state, histograms
and both result tables), the environment hooks where there is no GPU, the tool's parsing and the order of the sweep's calls."""
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

import episode_ref as T
from test_eval_return_codes import Call, cfg, each, nobody, null
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from util import build_emu

HEADER = os.path.join(REPO, "include", "go1episode.h")
SOURCE = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1episode.hip")
TABLES = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1_tables.h")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]


# ---- 1. mirrors, symbols, sources, stamp ---------------------------------------------------------------------------------------------------
def test_episode_mirrors_match_the_header():
    import go1episode_host as G
    src = open(HEADER).read()
    for macro, value in (("GO1EPISODE_NUM", G.NUM_EPISODE_METRICS), ("GO1EPISODE_BINS", G.BINS), ("GO1EPISODE_NUM_HISTS", G.NUM_HISTS),
                         ("GO1EPISODE_NUM_FIELDS", 6), ("GO1EPISODE_REDUCE_THREADS", 256)):
        assert re.search(rf"#define {macro} {value}\n", src), macro
    assert (G.NUM_EPISODE_METRICS, G.BINS, G.NUM_HISTS) == (11, 16, 3) == (T.M, T.BINS, T.HISTS)
    want = struct_fields(src, "Go1EpisodeConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1EpisodeConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "return_row", "gamma", "bin_steps"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1EpisodeConfig._fields_):
        assert ctype is C_TYPES[ctext], field
    assert ctypes.sizeof(G.Go1EpisodeConfig) == 24
    want = struct_fields(src, "Go1EpisodeBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1EpisodeBuffers._fields_] == T.INPUTS + ACCUMULATORS + T.STATE + ["group", "results", "hist_results"]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1EpisodeBuffers._fields_)
    types_ = dict(want)
    assert types_["age"] == types_["track_steps"] == "int32_t*" and types_["whole"] == "uint8_t*" and types_["reset_buf"] == types_["time_out_buf"] == "const uint8_t*"
    assert types_["ret"] == types_["disc_ret"] == types_["disc_w"] == types_["first_pos"] == types_["prev_pos"] == types_["path"] == types_["lin_err"] == "float*"
    assert types_["hist_results"] == types_["results"] == "double*" and types_["fall_hist"] == types_["timeout_hist"] == types_["cut"] == types_["unseen"] == "uint32_t*"
    assert G._EPISODE_INPUTS == T.INPUTS and G._EPISODE_STATE == T.STATE == list(G.Go1Episodes.STATE)
    st = T.clear(2)
    for name, (dtype, lead) in G.Go1Episodes.STATE.items():                  # the model's formats are the host's (uint32 read as int32)
        assert getattr(st, name).shape == (*lead, 2) and getattr(st, name).dtype.itemsize == torch.zeros(1, dtype=dtype).element_size(), name
    assert enum_order(src, "Go1EpisodeMetric", "GO1EPISODE_") == G.EPISODE_NAMES == T.METRICS and len(T.METRICS) == 11
    assert enum_order(src, "Go1EpisodeGroupField", "GO1EPISODE_G_") + enum_order(src, "Go1EpisodeGroupField2", "GO1EPISODE_H_") == G.EPISODE_GROUP_FIELDS == T.GROUP_FIELDS
    import go1eval_host as E
    assert enum_order(src, "Go1EpisodeField", "GO1EPISODE_F_") == E.FIELD_NAMES
    assert issubclass(G.Go1Episodes, E._Table) and G.Go1Episodes.ROWS == 11 and G.Go1Episodes.TABLE_ROWS == 13
    assert G.bin_edges(3).tolist() == [3.0 * k for k in range(16)] + [INF]
    from go1_gym_learn.eval_metrics import episodes
    assert episodes.EPISODE_METRICS == G.EPISODE_NAMES and episodes.EPISODE_GROUP_FIELDS == G.EPISODE_GROUP_FIELDS and episodes.BINS == G.BINS


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1episode_host as G
    declared = set(re.findall(r"\b(go1episode_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1episode_clear", "go1episode_accumulate", "go1episode_reduce", "go1episode_version"}
    out = g.build_episode_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1episode_" in line} == declared
    assert not re.search(r"\bgo1(eval|feet|trunk|gait)_\w+", dynamic)


def test_sources_flags_and_stamp():
    import __graft_entry__ as g
    assert g.episode_sources() == [SOURCE, TABLES, HEADER] and g.EPISODE_FLAGS == g.EVAL_FLAGS and "-ffp-contract=off" in g.EPISODE_FLAGS
    assert g.EPISODE_FLAGS is not g.EVAL_FLAGS
    # the list is what the compiler reads (tests/test_abi.py::test_source_lists_are_what_the_compiler_reads, for this library)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc] + g.EPISODE_FLAGS + ["--cuda-host-only", "-MM", SOURCE], cwd=g.CSRC, check=True, capture_output=True, text=True).stdout
    read = {os.path.normpath(os.path.join(g.CSRC, f)) for f in out.split(":", 1)[1].replace("\\\n", " ").split()}
    assert {f for f in read if not f.startswith("/opt/")} == {os.path.normpath(f) for f in g.episode_sources()}
    for others in (g.sim_sources(), g.ppo_sources(), g.render_sources(), g.state_sources()):
        assert not set(others) & set(g.episode_sources())
    for others in (g.eval_sources(), g.feet_sources(), g.trunk_sources(), g.gait_sources(), g.spectrum_sources(), g.place_sources(), g.reward_sources()):
        assert set(others) & set(g.episode_sources()) == {TABLES}                # one shared header, and nothing else
    code = re.sub(r"//.*", "", open(SOURCE).read())
    assert not re.search(r"go1(eval|feet|trunk|gait)", code) and "GO1_TABLES_MATCH(GO1EPISODE)" in code
    assert "go1episode" not in re.sub(r"//.*", "", open(TABLES).read())          # the shared header names no library
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["../../include/go1episode.h", "go1_tables.h"]
    for banned in ("atomic", "sinf", "cosf", "atan2f", "expf", "powf"):
        assert banned not in code, banned
    accumulate = code[code.index("episode_accumulate_kernel"):code.index("episode_reduce_kernel")]
    assert "__shared__" not in accumulate and "__syncthreads" not in accumulate
    out = g.build_episode_hip()
    assert os.path.basename(out) == "libgo1episode.so" and g.library_stamp(out) == g.source_hash(g.episode_sources(), g.EPISODE_FLAGS)
    lib = ctypes.CDLL(out)                                                       # dlopen needs no GPU
    lib.go1episode_version.restype = ctypes.c_char_p
    assert lib.go1episode_version() == b"go1episode 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    assert "build_episode_hip()" in inspect.getsource(g.build) and "libgo1episode.so" in inspect.getsource(g.smoke)
    # the other table libraries' stamps are what their own sources give: this family changed none of them
    for name, sources, flags in (("eval", g.eval_sources(), g.EVAL_FLAGS), ("feet", g.feet_sources(), g.FEET_FLAGS), ("gait", g.gait_sources(), g.GAIT_FLAGS)):
        assert g.library_stamp(os.path.join(g.CSRC, f"libgo1{name}.so")) in (None, g.source_hash(sources, flags)), name


def test_a_missing_library_fails_loudly(tmp_path):
    import go1episode_host as G
    with pytest.raises(G.Go1EpisodeLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1episode.so"))


# ---- 2. the refusals without a GPU (the helpers of tests/test_eval_return_codes.py) ----------------------------------------------------------
def episode_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.return_row, c.gamma, c.bin_steps = 70, 2, 3, 3, 0.99, 63


EPISODE_ACC = ACCUMULATORS + T.STATE
BAD_GAMMA = [("gamma = 0", -12, [cfg(gamma=0.0)]), ("gamma < 0", -12, [cfg(gamma=-0.5)]), ("gamma > 1", -12, [cfg(gamma=float(np.nextafter(f32(1), f32(2))))]),
             ("gamma NaN", -12, [cfg(gamma=NAN)]), ("gamma inf", -12, [cfg(gamma=INF)])]
BAD_BINS = [("bin_steps = 0", -12, [cfg(bin_steps=0)]), ("bin_steps < 0", -12, [cfg(bin_steps=-2)])]
CASES = {
    "go1episode_clear": nobody() + each(EPISODE_ACC, -2) + [
        ("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")])],
    "go1episode_accumulate": nobody() + each(EPISODE_ACC, -2) + each(T.INPUTS, -3) + BAD_GAMMA + BAD_BINS + [
        ("return_row < 0", -12, [cfg(return_row=-1)]),
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no fall_hist and no rew_buf", -2, [null("fall_hist", "rew_buf")]),
        ("no age and gamma = 0", -2, [null("age"), cfg(gamma=0.0)]),
        ("no episode_sums and bin_steps = 0", -3, [null("episode_sums"), cfg(bin_steps=0)]),
        ("no reset_buf and gamma NaN", -3, [null("reset_buf"), cfg(gamma=NAN)])],
    "go1episode_reduce": nobody() + each(EPISODE_ACC, -2) + [
        ("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group", "results", "hist_results"], -5) + BAD_BINS + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no unseen and no hist_results", -2, [null("unseen", "hist_results")]),
        ("no track_steps and num_groups = 0", -2, [null("track_steps"), cfg(num_groups=0)]),
        ("no results and bin_steps = 0", -5, [null("results"), cfg(bin_steps=0)])],
}


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    """every case fails validation, so nothing is launched: there is no GPU.  The largest and a small good discount and the smallest bin
    are not refused: with an input missing they get as far as -3."""
    import __graft_entry__ as g
    import go1episode_host as G
    g.build_episode_hip()
    fn = getattr(G.load_library(), symbol)
    assert len({label for label, _, _ in CASES[symbol]}) == len(CASES[symbol])
    assert sum(len(spoilers) > 1 for _, _, spoilers in CASES[symbol]) >= 1          # two conditions at once: precedence
    for label, code, spoilers in CASES[symbol]:
        a = Call(G.Go1EpisodeConfig, G.Go1EpisodeBuffers, episode_base)
        for spoil in spoilers:
            spoil(a)
        assert fn(None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b), None) == code, (symbol, label)
    if symbol == "go1episode_accumulate":
        for good in (cfg(gamma=1.0), cfg(gamma=1e-30), cfg(bin_steps=1), cfg(bin_steps=2 ** 31 - 1), cfg(return_row=0)):
            a = Call(G.Go1EpisodeConfig, G.Go1EpisodeBuffers, episode_base)
            good(a)
            null("reset_buf")(a)
            assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -3
    else:                                                                    # the clear and the reduction read no input and no discount
        a = Call(G.Go1EpisodeConfig, G.Go1EpisodeBuffers, episode_base)
        null(*T.INPUTS)(a)
        cfg(gamma=NAN, return_row=-1)(a)
        null("count")(a)
        assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -2


# ---- 3. the model by hand -----------------------------------------------------------------------------------------------------------------------
def snap_of(r=0.0, reset=0, timed=0, age=0, pos=(0.0, 0.0), vel=(0.0, 0.0), wz=0.0, cmd=(0.0, 0.0, 0.0), total=0.0):
    """one environment after a step"""
    s = dict(rew_buf=np.full(1, r, f32), reset_buf=np.full(1, reset, np.uint8), time_out_buf=np.full(1, timed, np.uint8),
             episode_length_buf=np.full(1, age, np.int32), root_states=np.zeros((13, 1), f32), base_lin_vel=np.zeros((3, 1), f32),
             base_ang_vel=np.zeros((3, 1), f32), commands=np.zeros((15, 1), f32), episode_sums=np.full((4, 1), -99.0, f32))
    s["root_states"][:2, 0], s["base_lin_vel"][:2, 0], s["base_ang_vel"][2, 0], s["commands"][:3, 0], s["episode_sums"][3, 0] = pos, vel, wz, cmd, total
    return s


def play(cfg_, steps):
    """the model on one environment over `steps` = [snap_of's keywords]: (state, what every step did)"""
    st, did = T.clear(1), []
    for kw in steps:
        did.append(T.accumulate(st, cfg_, snap_of(**kw)))
    return st, did


def folded(st):
    """{metric: (count, nonfinite, min, max)} of environment 0"""
    return {name: (int(st.count[m, 0]), int(st.nonfinite[m, 0]), float(st.min[m, 0]), float(st.max[m, 0])) for m, name in enumerate(T.METRICS)}


NOTHING = (0, 0, INF, -INF)
ONCE = lambda v: (1, 0, float(v), float(v))
# a reset on the very first launch, two steps, and a terminal step: an episode of three steps.  gamma = 0.5 keeps every figure exact
THREE = [dict(reset=1, r=9.0, pos=(0.0, 0.0)), dict(age=1, r=0.5, pos=(3.0, 4.0), vel=(1.0, 0.0), wz=0.5), dict(age=2, r=0.25, pos=(3.0, 4.0), vel=(0.0, 1.0), wz=-0.5)]


@pytest.mark.parametrize("timed", [0, 1])
def test_model_a_three_step_fall_and_a_time_out(timed):
    st, did = play(T.config(gamma=0.5, bin_steps=2), THREE + [dict(reset=1, timed=timed, r=-1.0, pos=(7.0, 7.0), vel=(5.0, 5.0), wz=5.0)])
    got = folded(st)
    assert did[0]["unseen"][0] and not did[0]["closed"][0] and did[3]["closed"][0] and did[3]["length"][0] == 3 and did[3]["whole_close"][0]
    assert (st.unseen[0], st.closed[0], st.fell[0], st.timed_out[0], st.cut[0], st.steps[0]) == (1, 1, 1 - timed, timed, 0, 4)
    assert got["step_reward"] == (4, 0, -1.0, 9.0) and got["length"] == ONCE(3.0) and got["fell"] == ONCE(1.0 - timed)
    assert got["length_fell"] == (NOTHING if timed else ONCE(3.0))
    assert got["return"] == ONCE(-0.25) and got["reward_rate"] == ONCE(f32(-0.25) / f32(3.0))         # the terminal reward counts, the first launch's does not
    assert got["discounted_return"] == ONCE(0.5 + 0.5 * 0.25 + 0.25 * -1.0)
    assert got["displacement"] == ONCE(5.0) and got["path_length"] == ONCE(5.0)                        # the respawn pose of the terminal step is the next episode's
    assert got["lin_vel_err"] == ONCE(1.0) and got["yaw_vel_err"] == ONCE(0.5)                         # two steps; the terminal step's velocities enter nothing
    hist, other = (st.timeout_hist, st.fall_hist) if timed else (st.fall_hist, st.timeout_hist)
    assert hist[:, 0].tolist() == [0, 1] + [0] * 14 and not other.any()                                # (3 - 1) / 2 = 1
    # the next episode is open and whole, at the respawn pose
    assert (st.age[0], st.whole[0], st.ret[0], st.disc_ret[0], st.disc_w[0], st.path[0], st.track_steps[0]) == (0, 1, 0.0, 0.0, 1.0, 0.0, 0)
    assert st.first_pos[:, 0].tolist() == [7.0, 7.0] == st.prev_pos[:, 0].tolist()
    table, hists = T.reduce(st, T.config(bin_steps=2), [0], 1)
    assert T.groups_of(table)[0].tolist() == [1.0, 4.0, 1.0, 1.0 - timed, float(timed), 1.0, 0.0, 1.0, 0.0]
    assert hists[0, 2].tolist() == [1.0] + [0.0] * 15 and hists[0, timed].tolist() == [0.0, 1.0] + [0.0] * 14 and not hists[0, 1 - timed].any()


def test_model_a_cut_is_dropped_and_seen_anew():
    """episode_length_buf falls back to 1 without a reset flag: the carried episode is counted in cut and folds nothing; the new one is
    whole, its return comes from episode_sums, and it closes three steps long"""
    steps = THREE + [dict(age=1, r=0.125, total=0.125, pos=(1.0, 1.0)), dict(age=2, r=0.25, pos=(1.0, 2.0)), dict(reset=1, r=0.5)]
    st, did = play(T.config(gamma=0.5, bin_steps=1), steps)
    got = folded(st)
    assert did[3]["cut"][0] and did[3]["first"][0] and not any(d["closed"][0] for d in did[:5]) and (st.cut[0], st.closed[0]) == (1, 1)
    assert got["length"] == ONCE(3.0) and got["return"] == ONCE(0.875) and got["discounted_return"] == ONCE(0.125 + 0.5 * 0.25 + 0.25 * 0.5)
    assert got["displacement"] == ONCE(1.0) and got["path_length"] == ONCE(1.0) and st.fall_hist[:, 0].tolist() == [0, 0, 1] + [0] * 13
    # a jump forwards is a cut too, and what follows is not whole
    st, did = play(T.config(), THREE + [dict(age=9, r=1.0, total=4.0), dict(reset=1, r=1.0)])
    got = folded(st)
    assert did[3]["cut"][0] and st.cut[0] == 1 and got["length"] == ONCE(10.0) and got["return"] == ONCE(5.0)
    assert got["discounted_return"] == got["displacement"] == got["path_length"] == NOTHING


def test_model_a_first_sight_at_age_five_takes_its_return_from_episode_sums():
    steps = [dict(age=5, r=0.5, total=7.5, pos=(1.0, 0.0)), dict(age=6, r=0.25, total=-3.0, pos=(2.0, 0.0)), dict(reset=1, timed=1, r=0.25, total=-3.0)]
    st, did = play(T.config(warmup_steps=5, bin_steps=3), steps)
    got = folded(st)
    assert did[0]["first"][0] and not did[0]["cut"][0] and st.whole[0] == 1 and (st.closed[0], st.timed_out[0], st.unseen[0]) == (1, 1, 0)
    assert got["return"] == ONCE(8.0) and got["length"] == ONCE(7.0) and got["reward_rate"] == ONCE(f32(8.0) / f32(7.0))     # episode_sums is read once
    assert got["discounted_return"] == got["displacement"] == got["path_length"] == NOTHING and got["fell"] == ONCE(0.0)
    assert got["lin_vel_err"] == ONCE(0.0) and st.timeout_hist[:, 0].tolist() == [0, 0, 1] + [0] * 13                      # the step at age 6 alone is behind the warm-up
    # a warm-up longer than the episode: no tracking error is folded, everything else is
    st, _ = play(T.config(warmup_steps=50), THREE + [dict(reset=1, r=0.0)])
    got = folded(st)
    assert got["lin_vel_err"] == got["yaw_vel_err"] == NOTHING and got["length"] == ONCE(3.0) and got["path_length"] == ONCE(5.0)
    # a non-finite reward is counted, not summed; the clamp puts a long episode into the last bin
    st, _ = play(T.config(bin_steps=1), [dict(age=40, r=NAN, total=NAN), dict(reset=1, r=1.0)])
    got = folded(st)
    assert got["return"] == (0, 1, INF, -INF) and got["step_reward"] == (1, 1, 1.0, 1.0) and st.fall_hist[:, 0].tolist() == [0] * 15 + [1] and np.isfinite(st.sum).all()


# ---- 4. the Kaplan-Meier estimate ------------------------------------------------------------------------------------------------------------------
def test_kaplan_meier_by_hand_and_against_the_product_limit_estimate():
    from go1_gym_learn.eval_metrics.episodes import kaplan_meier
    pad = lambda head: head + [0] * (16 - len(head))
    s = kaplan_meier(pad([1, 0, 1]), pad([0, 1]), pad([0, 0, 0, 2]))           # at risk: 5, 4, 3, 2, then nobody
    assert s[:4].tolist() == [1.0 - 1.0 / 5.0, 1.0 - 1.0 / 5.0, (1.0 - 1.0 / 5.0) * (1.0 - 1.0 / 3.0), (1.0 - 1.0 / 5.0) * (1.0 - 1.0 / 3.0)] and np.isnan(s[4:]).all()
    assert np.isnan(kaplan_meier(pad([]), pad([]), pad([]))).all()
    assert kaplan_meier(pad([]), pad([]), pad([0] * 15 + [7])).tolist() == [1.0] * 16              # nobody fell
    assert kaplan_meier(pad([4]), pad([]), pad([])).tolist()[0] == 0.0                             # everybody fell at once
    # per episode: (length, event) with event 0 fall, 1 time-out, 2 still open; one bin per step, so bin = length - 1
    rng = np.random.default_rng(5)
    episodes = [(int(rng.integers(1, 17)), int(rng.integers(0, 3))) for _ in range(200)]
    hists = np.zeros((3, 16))
    for length, event in episodes:
        hists[event, length - 1] += 1
    want, survival = np.full(16, NAN), 1.0
    for length in range(1, 17):                                               # the product-limit estimate at every distinct time
        at_risk = sum(1 for L, _ in episodes if L >= length)
        if at_risk == 0:
            break
        survival = survival * (1.0 - sum(1 for L, ev in episodes if L == length and ev == 0) / at_risk)
        want[length - 1] = survival
    got = kaplan_meier(*hists)
    assert got.dtype == np.float64 and bits(got) == bits(want) and got[-1] < got[0] < 1.0
    both = kaplan_meier(*(np.stack([h, h[::-1]]) for h in hists))              # rows are estimated one by one
    assert bits(both[0]) == bits(want) and both.shape == (2, 16)


# ---- 5. go1episode.hip under the SIMT emulator against the model ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1episode_host as G
    return G.load_library(build_emu(g.episode_sources(), "libgo1episode_emu.so"))


SHAPES_OF_INPUTS = dict(root_states=13, base_lin_vel=3, base_ang_vel=3, commands=T.SCRIPT_COMMANDS, episode_sums=T.SCRIPT_RETURN_ROW + 1)


def episodes_on(device, cfg_, N, lib=None):
    """a go1episode_host.Go1Episodes on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1episode_host as G
    tensors = {k: torch.zeros(rows, N, device=device) for k, rows in SHAPES_OF_INPUTS.items()}
    tensors.update(rew_buf=torch.zeros(N, device=device), reset_buf=torch.zeros(N, dtype=torch.uint8, device=device),
                   time_out_buf=torch.zeros(N, dtype=torch.uint8, device=device), episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    ep = G.Go1Episodes(types.SimpleNamespace(num_envs=N, num_rewards=cfg_.return_row), B, lib=lib)
    if torch.device(device).type == "cpu":
        ep._stream = lambda: None
    return ep, B


def episode_groups(rng, N, groups=3):
    """three groups of which group 1 is empty, some environments at -1 and (from three environments on) one id outside the tables"""
    assert groups == 3
    group = rng.integers(-1, groups, N).astype(np.int32)
    group[group == 1] = 2
    group[0] = groups - 1
    if N >= 3:
        group[1], group[2] = -1, groups
    return group


def drive(ep, B, cfg_, snaps, group, groups):
    """the scripted steps through the library: arm for `groups` groups, upload a snapshot, accumulate, ...; returns read() and the
    accumulators.  arm() sizes the tables by the largest id it is given, so the ids outside the tables are handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    ep.arm(inside, cfg_.warmup_steps, gamma=cfg_.gamma, bin_steps=cfg_.bin_steps)
    ep.group.copy_(torch.from_numpy(group))
    for s in snaps:
        for k, a in s.items():
            getattr(B, k).copy_(torch.from_numpy(a))
        ep.accumulate()
    ep.disarm()
    res = ep.read()
    acc = {k: t.cpu().numpy() for k, t in ep.acc.items()}
    return res, acc


def state_name(k):
    return "env_" + k if k.endswith("_hist") else k


def canon(a):
    """`a` with every NaN of a floating-point array replaced by one NaN: the header orders the operations, not the sign and payload of a
    NaN an infinite reward leaves in the running sums (they differ between processors)"""
    a = np.array(a)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


def same_as_the_model(res, acc, st, cfg_, group, groups):
    """accumulators, state, histograms and both result tables against the model's state `st`, bit for bit"""
    N = st.N
    for k in ACCUMULATORS:
        assert acc[k].shape == (T.M, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in T.STATE:
        assert res[state_name(k)].shape == getattr(st, k).shape and bits(canon(res[state_name(k)].view(getattr(st, k).dtype))) == bits(canon(getattr(st, k))), k
    want, want_hist = T.reduce(st, cfg_, group, groups)
    table = np.stack([res["metrics"][m] for m in T.METRICS], axis=1)
    assert table.shape == want[:, :T.M].shape == (groups, T.M, 6)
    assert np.array_equal(np.isnan(table), np.isnan(want[:, :T.M])) and bits(table) == bits(want[:, :T.M])
    assert res["groups"].shape == (groups, 9) and bits(res["groups"]) == bits(T.groups_of(want)) and not want[:, T.M + 1, 3:].any()
    for h, name in enumerate(("fall_hist", "timeout_hist", "open_hist")):
        assert res[name].shape == (groups, 16) and bits(res[name]) == bits(want_hist[:, h]), name
    assert res["bin_edges"].tolist() == [float(k * cfg_.bin_steps) for k in range(16)] + [INF] and res["gamma"] == float(f32(cfg_.gamma))
    return want, want_hist


def check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N):
    """the library's results against tests/episode_ref.py, bit for bit; then that the script drove every branch it was written to drive"""
    st, did = T.run(cfg_, snaps, N)
    want, want_hist = same_as_the_model(res, acc, st, cfg_, group, groups)
    steps = len(snaps)
    assert (res["steps"] == steps).all()
    ever = lambda key: np.any([d[key] for d in did], axis=0)
    count = lambda key: np.sum([d[key] for d in did], axis=0)
    if N >= len(T.KINDS):
        long_, first_reset, short, cutk, odd, random_, fresh = (kind == k for k in range(len(T.KINDS)))
        # begun before the first launch: a first sight at an age of five or more, closed once (not whole) by the time-out of step 36
        assert did[0]["first"][long_].all() and (snaps[0]["episode_length_buf"][long_] >= 5).all() and did[36]["timed"][long_].all()
        assert (st.count[T.RETURN, long_] == 1).all() and (st.count[T.DISCOUNTED_RETURN, long_] == 0).all() and (did[36]["length"][long_] >= 41).all()
        assert cfg_.bin_steps > 2 or (did[36]["clamped"][long_].all() and (st.timeout_hist[15, long_] == 1).all())
        assert snaps[0]["reset_buf"][first_reset].all() and did[0]["unseen"][first_reset].all() and (st.unseen[first_reset] == 1).all() and st.unseen.sum() == first_reset.sum()
        # episodes shorter than the warm-up: closed, and no tracking error folded for them
        assert (count("closed")[short] >= 12).all() and ((count("closed") - count("tracked"))[short] >= 11).all() and (st.count[T.LIN_VEL_ERR, short] <= 1).all()
        assert (st.cut[cutk] == 2).all() and st.cut.sum() == 2 * cutk.sum() and did[10]["cut"][cutk].all() and did[25]["cut"][cutk].all()
        assert did[33]["closed"][cutk].all() and not did[33]["whole_close"][cutk].any()
        assert (st.nonfinite[T.STEP_REWARD, odd] > 0).all() and st.nonfinite[T.RETURN, odd].sum() > 0 and st.nonfinite[T.STEP_REWARD, ~odd].sum() == 0
        assert np.isfinite(st.sum).all() and np.isfinite(st.sumsq).all()
        assert st.fell.sum() > 0 and st.timed_out.sum() > 0 and st.fall_hist.sum() == st.fell.sum() and st.timeout_hist.sum() == st.timed_out.sum()
        assert did[0]["first"][fresh].all() and did[20]["whole_close"][fresh].all() and (did[20]["length"][fresh] == 21).all() and (st.count[T.PATH_LENGTH, fresh] == 1).all()
        assert (st.age >= 0).all() and (st.closed == st.fell + st.timed_out).all() and (st.count[T.LENGTH] == st.closed).all()
    g = res["groups"]
    assert g[:, 0].sum() == np.isin(group, range(groups)).sum() and (g[:, 1] == steps * g[:, 0]).all() and g[1].tolist() == [0.0] * 9
    assert (g[:, 2] == g[:, 3] + g[:, 4]).all() and (res["open_hist"].sum(axis=1) == g[:, 5]).all() and (g[:, 5] == g[:, 0]).all()
    assert np.isnan(want[1, :T.M, 1:5]).all() and not want_hist[1].any()
    return st


# (N, bin_steps).  1: one thread; 64: one wavefront; 257: a workgroup plus one lane; 600: three ragged workgroups, three terms per
# reduction thread and 38 environments per histogram slice.  One step per bin at 64, the clamp at 1 and 257, wide bins at 600
SCRIPTS = [(1, 2), (64, 1), (257, 2), (600, 3)]


@pytest.mark.parametrize("N,bin_steps", SCRIPTS)
def test_emulated_episode_kernels_follow_the_model(emu, N, bin_steps):
    groups = 3
    rng = np.random.default_rng(1200 + N)
    cfg_, snaps, kind = T.scripted_steps(rng, N, bin_steps=bin_steps)
    assert len(snaps) == T.SCRIPT_STEPS == 40 and (cfg_.warmup_steps, cfg_.bin_steps, cfg_.return_row) == (4, bin_steps, 3)
    assert N < len(T.KINDS) or set(kind.tolist()) == set(range(len(T.KINDS)))
    group = episode_groups(rng, N, groups)
    ep, B = episodes_on("cpu", cfg_, N, lib=emu)
    res, acc = drive(ep, B, cfg_, snaps, group, groups)
    assert ep.cfg.num_groups == groups and (N < 3 or {-1, groups} <= set(group.tolist()))
    check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N)
    again = ep.read()                                                        # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ("groups", "fall_hist", "timeout_hist", "open_hist", "env_fall_hist", "age", "ret", "closed"))
    assert all(bits(again["metrics"][m]) == bits(res["metrics"][m]) for m in T.METRICS)
    for bad in (dict(gamma=0.0), dict(gamma=1.5), dict(gamma=NAN), dict(bin_steps=0)):
        with pytest.raises(ValueError, match="episodes:"):
            ep.arm(np.zeros(N, np.int32), **bad)
    with pytest.raises(RuntimeError, match="go1episode_accumulate failed: -12"):
        ep.cfg.bin_steps = 0
        ep.accumulate()


# ---- 6. the environment hooks without a GPU -----------------------------------------------------------------------------------------------------
def plane_env(monkeypatch, num_envs=16):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    for module in ("go1eval_host", "go1episode_host"):
        monkeypatch.delitem(sys.modules, module, raising=False)
    c = apply_train_config(make_cfg(), num_envs=num_envs)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    return VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)


def test_episode_hooks_on_cpu_buffers(monkeypatch):
    from go1_gym.envs.base.legged_robot import LeggedRobot
    from test_family_wiring import FAMILIES, REWARD, STATE_FAMILIES, Stub
    import test_family_wiring as wiring
    # stubs for the families up to the reward family only: the later ones stay None unless this test puts its own stub there, so the
    # launch-order and refusal checks below name exactly the families they set
    STEPPED = wiring.STEPPED[:REWARD + 1]
    put_stubs = functools.partial(wiring.put_stubs, stepped=STEPPED)
    env = plane_env(monkeypatch)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_episode_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_episode_metrics, env.read_episode_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert all(m not in sys.modules for m in ("go1eval_host", "go1episode_host")) and env._episodes is None          # never measured: no host module
    env.step(torch.zeros(16, 12))                                             # and stepping goes on
    signature = inspect.signature(env.start_episode_metrics)
    assert {k: p.default for k, p in signature.parameters.items() if k != "groups"} == dict(warmup_steps=0, gamma=0.99, bin_steps=63)
    assert list(signature.parameters) == ["groups", "warmup_steps", "gamma", "bin_steps"]
    for name in ("start_episode_metrics", "stop_episode_metrics", "read_episode_metrics"):
        assert (getattr(LeggedRobot, name).__doc__ or "").strip(), name
    # its row of the one table, directly after the reward family's
    k = [row[0] for row in env._FAMILIES].index("episodes")
    assert env._FAMILIES == FAMILIES and env._FAMILIES[k] == ("episodes", "_episodes", "go1episode_host", "Go1Episodes", "accumulate") and env._FAMILIES[k - 1][0] == "rewards"
    assert env._STATE_FAMILIES == STATE_FAMILIES and env._STATE_FAMILIES[k] == ("episodes", "_episodes") and env._STEPPED[k - 2:k] == (("_reward", "accumulate"), ("_episodes", "accumulate"))
    assert env._HOST["_episodes"] == ("go1episode_host", "Go1Episodes") and all(len(row) == 5 for row in env._FAMILIES)
    # launched last, after the reward family's
    log = []
    put_stubs(env, log)
    env._episodes = Stub("_episodes", log)
    env.step(torch.zeros(16, 12))
    assert [(attr, method) for attr, method, _ in log] == STEPPED + [("_episodes", "accumulate")] and log[-1][2] == ()
    env._episodes.armed = False
    del log[:]
    env.step(torch.zeros(16, 12))
    assert [(attr, method) for attr, method, _ in log] == STEPPED
    # load_state() names it after the eleven and before the camera
    env._state = types.SimpleNamespace(restore=lambda *a, **k: pytest.fail("restored"))
    env._episodes.armed = True
    env._render = types.SimpleNamespace(any_armed=True)
    with pytest.raises(RuntimeError) as e:
        env.load_state(None)
    assert "refused while metrics, behaviour, trace, terrain, joints, feet, trunk, gait, spectrum, placement, rewards, episodes, camera are armed" in str(e.value)
    env._render = None
    put_stubs(env, [], armed=False)
    with pytest.raises(RuntimeError, match=r"refused while episodes is armed: stop it first"):
        env.load_state(None)


# ---- 7. the tool and the sweep's host pieces --------------------------------------------------------------------------------------------------
def fixed_result():
    from go1_gym_learn.eval_metrics import episodes, sweep
    row = lambda n, mean, std=0.0: np.array([[n, mean, std, mean - std, mean + std, 0.0]] * 2)
    t = dict(step_reward=row(960.0, 0.01), length=row(10.0, 30.0, 5.0), fell=row(10.0, 0.4), length_fell=row(4.0, 25.0, 2.0), **{"return": row(10.0, 1.5, 0.25)},
             reward_rate=row(10.0, 0.05), lin_vel_err=row(10.0, 0.2, 0.1), yaw_vel_err=row(10.0, 0.1), discounted_return=row(8.0, 1.2), displacement=row(8.0, 0.6),
             path_length=row(8.0, 0.7))
    t["length_fell"][1], t["fell"][1] = [0.0, NAN, NAN, NAN, NAN, 0.0], [10.0, 0.0, 0.0, 0.0, 0.0, 0.0]      # cell 1 never fell
    groups = np.array([[12.0, 480.0, 10.0, 4.0, 6.0, 12.0, 1.0, 0.0, 90.0], [12.0, 480.0, 10.0, 0.0, 10.0, 12.0, 0.0, 0.0, 80.0]])
    fall, timeout, opened = np.zeros((2, 16)), np.zeros((2, 16)), np.zeros((2, 16))
    fall[0, [2, 9]], timeout[:, 15], opened[:, 3] = [2.0, 2.0], [6.0, 10.0], 12.0
    return dict(preset="static_medium", cells=sweep.grid_cells(dict(vx=[0.5, 1.0], yaw=[0.0], gait=[sweep.GAITS["trotting"]])), episodes=t, episode_groups=groups,
                fall_hist=fall, timeout_hist=timeout, open_hist=opened, bin_edges=np.concatenate([np.arange(16.0) * 3, [INF]]),
                survival=episodes.kaplan_meier(fall, timeout, opened), gamma=0.99, bin_steps=3, metrics={}, groups=np.zeros((2, 5)), num_envs=24, steps=40,
                warmup_steps=5, seed=1, dt=0.02)


def test_episode_table_json_and_figure(tmp_path):
    from go1_gym_learn.eval_metrics import episodes
    res = fixed_result()
    md = episodes.episode_markdown_table(res).splitlines()
    assert md[0].startswith("| vx | yaw | gait | closed / open / cut | fall share | return | length | time to fall [s] | reward / step | discounted return |")
    assert len(md) == 2 + 2 and len({line.count("|") for line in md}) == 1 and md[0].count("|") == 19
    s0 = 1.0 - 2.0 / 22.0
    assert md[2].startswith("| 0.5 | 0 | 0.5/0/0 | 10 / 12 / 1 | 0.400 | 1.5 ± 0.25 | 30 ± 5 | 0.50 |") and md[2].endswith(f"| {s0:.3f} | {s0:.3f} | {s0 * (1 - 2.0 / 8.0):.3f} | 120 |")
    assert md[3].startswith("| 1 | 0 | 0.5/0/0 | 10 / 12 / 0 | 0.000 | 1.5 ± 0.25 | 30 ± 5 | – |") and md[3].endswith("| 1.000 | 1.000 | 1.000 | – |")
    js = json.loads(json.dumps(episodes.episode_to_json(res), allow_nan=False))
    assert js["group_fields"] == T.GROUP_FIELDS and js["episodes"]["length_fell"][1][1] is None and js["bin_edges"][-1] is None and js["bin_edges"][1] == 3.0
    assert js["summary"][1]["steps_per_fall"] is None and js["summary"][0]["steps_per_fall"] == 120.0 and js["summary"][0]["time_to_fall_s"] == 0.5
    assert np.array(js["survival"]).shape == (2, 16) and js["gamma"] == 0.99 and js["cells"][1]["vx"] == 1.0 and js["open_hist"][0][3] == 12.0
    path = tmp_path / "survival.png"
    episodes.plot_survival(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000


def test_tool_accepts_an_episode_sweep(tmp_path, monkeypatch, capsys):
    from test_family_wiring import MODES
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import episodes, sweep
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--episodes", "--vx", "0.5", "1.0", "--envs", "24", "--steps", "40", "--warmup-steps", "5", "--presets", "static_medium",
                                      "--gamma", "0.9", "--bin-steps", "3"])
    assert a.episodes and not a.coordination and (a.vx, a.envs, a.steps, a.gamma, a.bin_steps) == ([0.5, 1.0], 24, 40, 0.9, 3)
    plain = eval_sweep.parse_args(base + ["--episodes"])
    assert (plain.gamma, plain.bin_steps) == (0.99, 0) and plain.episodes
    nothing = eval_sweep.parse_args(base)
    assert not nothing.episodes and nothing.gamma is None and nothing.bin_steps is None
    assert eval_sweep.parse_args(base + ["--episodes", "--terrain", "plane"]).terrain == "plane"
    assert eval_sweep.parse_args(base + ["--episodes", "--gamma", "1"]).gamma == 1.0
    for other in MODES.values():                                             # every other mode excludes it, whichever comes first
        for argv in (["--episodes"] + other, other + ["--episodes"]):
            with pytest.raises(SystemExit) as e:
                eval_sweep.parse_args(base + argv)
            assert e.value.code == 2, argv
    for bad in (["--gamma", "0.9"], ["--bin-steps", "4"], ["--trunk", "--gamma", "0.9"], ["--joints", "--bin-steps", "4"], ["--episodes", "--gamma", "0"],
                ["--episodes", "--gamma", "1.01"], ["--episodes", "--gamma", "nan"], ["--episodes", "--gamma", "-0.5"], ["--episodes", "--bin-steps", "-1"],
                ["--episodes", "--map-cell", "0.05"]):
        with pytest.raises(SystemExit) as e:
            eval_sweep.parse_args(base + bad)
        assert e.value.code == 2, bad
    assert callable(eval_sweep.run_episodes) and len(inspect.signature(eval_sweep.run_episodes).parameters) == 3
    assert "--episodes --steps 1500" in eval_sweep.__doc__
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(episodes, "run_episode_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    grid = dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits])
    eval_sweep.run_episodes(a, None, grid)
    assert seen == dict(preset="static_medium", grid=grid, num_envs=24, steps=40, warmup_steps=5, seed=1, terrain=None, gamma=0.9, bin_steps=3)
    js = json.load(open(tmp_path / "eval" / "static_medium_episodes.json"))
    assert js["preset"] == "static_medium" and js["summary"][0]["closed"] == 10.0
    md = (tmp_path / "eval" / "static_medium_episodes.md").read_text()
    assert "| 10 / 12 / 1 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_survival.png").read_bytes()[:4] == b"\x89PNG"


def test_the_sweep_arms_both_tables_before_the_reset(monkeypatch):
    """a recording environment as tests/test_family_wiring.py's, with a reset() that is noted too: both starts come before it, so every
    environment's first episode is seen from its first step; bin_steps = 0 becomes ceil(steps / 16)"""
    from go1_gym_learn.eval_metrics import episodes, sweep
    from test_family_wiring import N, NUM_COMMANDS, STEPS, WARMUP, RecordingEnv, ZeroPolicy
    cells_in = dict(vx=[0.5, 1.0], yaw=[0.0, 0.5], gait=[sweep.GAITS["trotting"]])
    cells = sweep.grid_cells(cells_in)
    family = dict(metrics={"m": np.full((4, 6), 0.5)}, groups=np.ones((4, 9)), fall_hist=np.zeros((4, 16)), timeout_hist=np.zeros((4, 16)), open_hist=np.full((4, 16), 2.0),
                  bin_edges=np.arange(17.0), gamma=0.5, bin_steps=1)

    class Env(RecordingEnv):
        def __init__(self, spoil=False):
            super().__init__("gait", 4, spoil)               # (any stem the recording base knows: the family below replaces what it cans)
            self.env.family = family

        def reset(self):
            self.env.log.append(("reset", (), {}))
            return super().reset()
    built, built_env = [], Env()
    monkeypatch.setattr(sweep, "build_eval_env", lambda preset, num_envs, seed, terrain=None, configure=None: (built.append((preset, num_envs, seed, terrain)), (built_env, None))[1])
    policy = ZeroPolicy()
    res = episodes.run_episode_sweep(policy, "static_medium", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5, terrain="plane", gamma=0.5)
    log = built_env.env.log
    assert built == [("static_medium", N, 5, "plane")] and policy.evaluated == 1
    assert [entry[0] for entry in log] == ["start_metrics", "start_episode_metrics", "reset", "step", "step", "step", "stop_metrics", "stop_episode_metrics", "read_metrics",
                                           "read_episode_metrics"]
    group = (torch.arange(N) % 4).to(torch.int32)
    (_, scalar_args, scalar_kw), (_, family_args, family_kw) = log[0], log[1]
    assert len(scalar_args) == 1 and scalar_args[0] is family_args[0] and scalar_args[0].dtype == torch.int32 and torch.equal(scalar_args[0], group)
    assert scalar_kw == dict(warmup_steps=WARMUP) and family_kw == dict(warmup_steps=WARMUP, gamma=0.5, bin_steps=1)          # ceil(3 / 16)
    assert torch.equal(built_env.first, sweep.command_table(cells, NUM_COMMANDS, "cpu")[group.long()]) and [entry[1] for entry in log[3:6]] == [True] * 3
    assert res["episodes"] is family["metrics"] and res["episode_groups"] is family["groups"] and res["open_hist"] is family["open_hist"]
    assert (res["bin_steps"], res["gamma"], res["steps"], res["dt"], res["cells"]) == (1, 0.5, STEPS, 0.02, cells) and (res["survival"] == 1.0).all() and res["survival"].shape == (4, 16)
    assert res["groups"].shape == (4, 5) and list(res["metrics"]) == ["lin_vel_rmsd"]
    built_env = Env()
    assert episodes.run_episode_sweep(ZeroPolicy(), "static_medium", cells_in, num_envs=N, steps=40, warmup_steps=WARMUP, seed=5)["bin_steps"] == 3      # ceil(40 / 16)
    assert built_env.env.log[1][2]["bin_steps"] == 3 and episodes.run_episode_sweep.__defaults__[-2:] == (0.99, 0)
    built_env = Env(spoil=True)
    with pytest.raises(RuntimeError) as e:
        episodes.run_episode_sweep(ZeroPolicy(), "static_medium", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5, bin_steps=7)
    assert str(e.value) == "run_episode_sweep: an environment left its grid cell's commands during the rollout"
    assert [entry[0] for entry in built_env.env.log][-2:] == ["stop_metrics", "stop_episode_metrics"] and built_env.env.log[1][2]["bin_steps"] == 7


# ---- 8. the scenario of the GPU test, through the fp64 oracle here -------------------------------------------------------------------------------
# N = 64 on the plane, episodes of 1 s, the family armed before reset(), then 120 steps of 2.0 * randn actions from a seeded generator on the
# environment's device (the recipe of tests/test_gpu_eval_metrics.py for falls and time-outs alike), three groups, a warm-up of 5, and before
# step 60 a reset_idx of four environments that did not reset on the step before (so each of them is an episode cut from outside).
# Counted here with the oracle-backed environment of tests/fake_sim.py (the CPU generator's actions): 2 falls, 126 time-outs, 128 closed
# episodes of which 128 whole, 4 cuts, 0 unseen, 64 open at the end (on an MI355X, with the device generator's actions: 3 and 125).
ROLL_N, ROLL_STEPS, ROLL_WARMUP, ROLL_GROUPS, ROLL_SEED, ROLL_CUT_STEP, ROLL_CUTS, ROLL_GAMMA, ROLL_BIN_STEPS = 64, 120, 5, 3, 11, 60, 4, 0.99, 4


def snapshot(env):
    """host copies of the buffers go1episode_accumulate reads, as they stand after a step"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in T.INPUTS}


def rollout_steps(envs):
    """the scenario on `envs` (the same actions and the same cuts for each): yields -1 after their reset() and k after step k"""
    device = envs[0].device
    g = torch.Generator(device=device).manual_seed(ROLL_SEED)
    for e in envs:
        e.reset()
    yield -1
    for k in range(ROLL_STEPS):
        if k == ROLL_CUT_STEP:
            running = torch.nonzero(envs[0].reset_buf == 0).reshape(-1)[:ROLL_CUTS]      # (a host read, once: not part of a measurement loop)
            assert running.numel() == ROLL_CUTS
            for e in envs:
                e.reset_idx(running.clone())
        action = 2.0 * torch.randn(ROLL_N, 12, device=device, generator=g)
        for e in envs:
            e.step(action)
        yield k


def rollout_config(env):
    return T.config(warmup_steps=ROLL_WARMUP, gamma=ROLL_GAMMA, bin_steps=ROLL_BIN_STEPS, return_row=int(env.sim_config.num_rewards))


def assert_rollout_events(st, did, label):
    """at least one fall, one time-out and one whole closed episode, and exactly the four cuts: else a comparison would be empty"""
    whole = int(np.sum([d["whole_close"] for d in did]))
    print(f"\n{label}: falls {int(st.fell.sum())}, time-outs {int(st.timed_out.sum())}, closed {int(st.closed.sum())} of which whole {whole}, cuts {int(st.cut.sum())}, "
          f"unseen {int(st.unseen.sum())}, open at the end {int((st.age >= 0).sum())}")
    assert st.fell.sum() >= 1 and st.timed_out.sum() >= 1 and whole >= 1 and st.cut.sum() == ROLL_CUTS


def test_the_rollout_script_produces_events_on_the_oracle(monkeypatch):
    """the scenario of test_gpu_episode_metrics.test_episodes_through_the_environment on the CPU oracle, the model replayed on the buffers
    after every step: falls, time-outs, whole episodes and the four cuts all occur, and on every step without a reset the model's running
    return is the simulator's episode_sums total, bit for bit"""
    import fake_sim
    from test_gpu_response_trace import make_env
    fake_sim.install(monkeypatch)
    env = make_env(ROLL_N, "plane", 1.0, seed=4)
    cfg_ = rollout_config(env)
    st, did = T.clear(ROLL_N), []
    for k in rollout_steps([env]):
        s = snapshot(env)
        did.append(T.accumulate(st, cfg_, s))
        running = s["reset_buf"] == 0
        assert bits(st.ret[running]) == bits(s["episode_sums"][cfg_.return_row][running]), k
    assert_rollout_events(st, did, "oracle")
    assert len(did) == ROLL_STEPS + 1 and st.unseen.sum() == 0 and did[ROLL_CUT_STEP + 1]["cut"].sum() == ROLL_CUTS
    assert st.max[T.LENGTH].max() == env.max_episode_length + 1 == 52         # a time-out closes an episode of max_episode_length + 1 steps
