"""CPU checks of the foot-placement family (include/go1place.h, libgo1place.so): the ctypes mirrors and the exported symbols against the
header, the build's source list (as the compiler reads it), flags and stamp, the refusals without a GPU, the host definition pinned to
the reference's recorded raibert_heuristic, the model of tests/place_ref.py on hand-computed cases, go1place.hip itself under the SIMT
emulator against that model bit for bit (accumulators, state, map and both result tables), the environment hooks where there is no GPU,
the scenario of the GPU test through the fp64 oracle, and the sweep's host pieces."""
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

import place_ref as T
from test_eval_return_codes import Call, cfg, each, nobody, null
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from util import build_emu

HEADER = os.path.join(REPO, "include", "go1place.h")
SOURCE = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1place.hip")
TABLES = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1_tables.h")
GOLDEN = os.path.join(REPO, "tests", "golden")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]


# ---- 1. mirrors, symbols, sources, stamp ---------------------------------------------------------------------------------------------------
def test_place_mirrors_match_the_header():
    import go1place_host as G
    src = open(HEADER).read()
    for macro, value in (("GO1PLACE_NUM", G.NUM_PLACE_METRICS), ("GO1PLACE_NUM_FEET", G.NUM_FEET), ("GO1PLACE_MAP_SIDE", G.MAP_SIDE),
                         ("GO1PLACE_MAP_CELLS", G.MAP_CELLS), ("GO1PLACE_NUM_FIELDS", 6), ("GO1PLACE_REDUCE_THREADS", 256), ("GO1PLACE_CONTACT_FORCE", G.CONTACT_FORCE)):
        assert re.search(rf"#define {macro} {value}\n", src), macro
    assert (G.NUM_PLACE_METRICS, G.NUM_FEET, G.MAP_SIDE, G.MAP_CELLS) == (14, 4, 8, 64) == (T.M, T.FEET, T.SIDE, T.CELLS)
    want = struct_fields(src, "Go1PlaceConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1PlaceConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "num_commands", "map_cell"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1PlaceConfig._fields_):
        assert ctype is C_TYPES[ctext], field
    assert ctypes.sizeof(G.Go1PlaceConfig) == 20 and dict(want)["map_cell"] == "float"
    want = struct_fields(src, "Go1PlaceBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1PlaceBuffers._fields_] == T.INPUTS + ACCUMULATORS + T.STATE + ["group", "results", "map_results"]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1PlaceBuffers._fields_)
    types_ = dict(want)
    assert types_["prev_contact"] == types_["stance_open"] == types_["stride_open"] == "uint8_t*"
    assert all(types_[k] == "float*" for k in ("td_x", "last_x", "last_y", "td_world_x", "td_world_y"))
    assert all(types_[k] == "uint32_t*" for k in ("touchdowns", "liftoffs", "strides", "map_outside", "map", "steps", "resets"))
    assert types_["map_results"] == types_["results"] == "double*"
    assert G._PLACE_INPUTS == T.INPUTS and G._PLACE_STATE == T.STATE == list(G.Go1Place.STATE)
    assert enum_order(src, "Go1PlaceMetric", "GO1PLACE_") == G.PLACE_NAMES == T.METRICS and len(T.METRICS) == 14
    assert enum_order(src, "Go1PlaceGroupField", "GO1PLACE_G_") == G.PLACE_GROUP_FIELDS == T.GROUP_FIELDS
    assert G.PLACE_GROUP_FIELDS == ["envs", "steps", "resets", "touchdowns", "strides", "map_outside"]
    import go1eval_host as E
    assert enum_order(src, "Go1PlaceField", "GO1PLACE_F_") == E.FIELD_NAMES
    assert issubclass(G.Go1Place, E._Table) and G.Go1Place.ROWS == 56 and G.Go1Place.TABLE_ROWS == 57
    assert G.map_edges(0.03).shape == (9,) and G.map_edges(0.03)[[0, 4, 8]].tolist() == pytest.approx([-0.12, 0.0, 0.12], abs=1e-8)
    assert G.DEFAULT_MAP_CELL == 0.03
    from go1_gym_learn.eval_metrics import placement
    assert placement.PLACEMENT_METRICS == G.PLACE_NAMES and placement.PLACEMENT_GROUP_FIELDS == G.PLACE_GROUP_FIELDS and placement.FEET == G.FOOT_NAMES


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1place_host as G
    declared = set(re.findall(r"\b(go1place_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1place_clear", "go1place_accumulate", "go1place_reduce", "go1place_version"}
    out = g.build_place_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1place_" in line} == declared
    assert not re.search(r"\bgo1(eval|feet|trunk|gait|spectrum|reward|state)_\w+", dynamic)


def test_sources_flags_and_stamp():
    import __graft_entry__ as g
    assert g.place_sources() == [SOURCE, TABLES, HEADER] and g.PLACE_FLAGS == g.EVAL_FLAGS and "-ffp-contract=off" in g.PLACE_FLAGS
    assert g.PLACE_FLAGS is not g.EVAL_FLAGS
    # the list is what the compiler reads (tests/test_abi.py::test_source_lists_are_what_the_compiler_reads, for this library)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc] + g.PLACE_FLAGS + ["--cuda-host-only", "-MM", SOURCE], cwd=g.CSRC, check=True, capture_output=True, text=True).stdout
    read = {os.path.normpath(os.path.join(g.CSRC, f)) for f in out.split(":", 1)[1].replace("\\\n", " ").split()}
    assert {f for f in read if not f.startswith("/opt/")} == {os.path.normpath(f) for f in g.place_sources()}
    for others in (g.sim_sources(), g.ppo_sources(), g.render_sources(), g.state_sources()):
        assert not set(others) & set(g.place_sources())
    for others in (g.eval_sources(), g.feet_sources(), g.trunk_sources(), g.gait_sources(), g.spectrum_sources(), g.reward_sources()):
        assert set(others) & set(g.place_sources()) == {TABLES}                # one shared header, and nothing else
    code = re.sub(r"//.*", "", open(SOURCE).read())
    assert not re.search(r"go1(eval|feet|trunk|gait|spectrum|reward|state|sim)", code) and "GO1_TABLES_MATCH(GO1PLACE)" in code
    assert "go1place" not in re.sub(r"//.*", "", open(TABLES).read())        # the shared header names no library
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["../../include/go1place.h", "go1_tables.h"]
    for banned in ("atomic", "sinf", "cosf", "atan2f", "sincosf"):            # no atomics, no trigonometric function on the device
        assert banned not in code, banned
    accumulate = code[code.index("place_accumulate_kernel"):code.index("place_reduce_kernel")]
    assert "__shared__" not in accumulate and "__syncthreads" not in accumulate and "row_thread(N, FEET" in accumulate
    out = g.build_place_hip()
    assert os.path.basename(out) == "libgo1place.so" and g.library_stamp(out) == g.source_hash(g.place_sources(), g.PLACE_FLAGS)
    lib = ctypes.CDLL(out)                                                   # dlopen needs no GPU
    lib.go1place_version.restype = ctypes.c_char_p
    assert lib.go1place_version() == b"go1place 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    assert "build_place_hip()" in inspect.getsource(g.build) and "libgo1place.so" in inspect.getsource(g.smoke)
    # the other table libraries' stamps are what their own sources give: this family changed none of them
    for name, sources, flags in (("eval", g.eval_sources(), g.EVAL_FLAGS), ("feet", g.feet_sources(), g.FEET_FLAGS), ("trunk", g.trunk_sources(), g.TRUNK_FLAGS),
                                 ("gait", g.gait_sources(), g.GAIT_FLAGS), ("spectrum", g.spectrum_sources(), g.SPECTRUM_FLAGS)):
        assert g.library_stamp(os.path.join(g.CSRC, f"libgo1{name}.so")) in (None, g.source_hash(sources, flags)), name


def test_a_missing_library_fails_loudly(tmp_path):
    import go1place_host as G
    with pytest.raises(G.Go1PlaceLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1place.so"))


# ---- 2. the refusals without a GPU (the helpers of tests/test_eval_return_codes.py) ----------------------------------------------------------
def place_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.num_commands, c.map_cell = 70, 2, 3, 15, 0.03


PLACE_ACC = ACCUMULATORS + T.STATE
BAD_CONFIG = [("map_cell = 0", -12, [cfg(map_cell=0.0)]), ("map_cell < 0", -12, [cfg(map_cell=-0.03)]), ("map_cell = NaN", -12, [cfg(map_cell=NAN)]),
              ("map_cell = inf", -12, [cfg(map_cell=INF)]), ("num_commands = 4", -12, [cfg(num_commands=4)]), ("num_commands = 0", -12, [cfg(num_commands=0)])]
CASES = {
    "go1place_clear": nobody() + each(PLACE_ACC, -2) + [
        ("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")])],
    "go1place_accumulate": nobody() + each(PLACE_ACC, -2) + each(T.INPUTS, -3) + BAD_CONFIG + [
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no map and no foot_positions", -2, [null("map", "foot_positions")]),
        ("no td_x and map_cell = 0", -2, [null("td_x"), cfg(map_cell=0.0)]),
        ("no commands and map_cell = 0", -3, [null("commands"), cfg(map_cell=0.0)]),
        ("no reset_buf and num_commands = 4", -3, [null("reset_buf"), cfg(num_commands=4)])],
    "go1place_reduce": nobody() + each(PLACE_ACC, -2) + [
        ("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group", "results", "map_results"], -5) + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no resets and no map_results", -2, [null("resets", "map_results")]),
        ("no strides and num_groups = 0", -2, [null("strides"), cfg(num_groups=0)])],
}


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    """every case fails validation, so nothing is launched: there is no GPU.  The smallest good settings (num_commands = 5, a tiny
    map_cell) are not refused: with an input missing they get as far as -3."""
    import __graft_entry__ as g
    import go1place_host as G
    g.build_place_hip()
    fn = getattr(G.load_library(), symbol)
    assert len({label for label, _, _ in CASES[symbol]}) == len(CASES[symbol])
    assert sum(len(spoilers) > 1 for _, _, spoilers in CASES[symbol]) >= 1          # two conditions at once: precedence
    for label, code, spoilers in CASES[symbol]:
        a = Call(G.Go1PlaceConfig, G.Go1PlaceBuffers, place_base)
        for spoil in spoilers:
            spoil(a)
        assert fn(None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b), None) == code, (symbol, label)
    if symbol == "go1place_accumulate":
        for good in (cfg(num_commands=5), cfg(map_cell=1e-30), cfg(map_cell=3e38), cfg(num_commands=12)):
            a = Call(G.Go1PlaceConfig, G.Go1PlaceBuffers, place_base)
            good(a)
            null("reset_buf")(a)
            assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -3
    else:                                                                    # the clear and the reduction read no input and no map_cell
        a = Call(G.Go1PlaceConfig, G.Go1PlaceBuffers, place_base)
        null(*T.INPUTS)(a)
        cfg(map_cell=0.0, num_commands=0)(a)
        null("count")(a)
        assert fn(ctypes.byref(a.c), ctypes.byref(a.b), None) == -2


# ---- 3. pinned to the reference ----------------------------------------------------------------------------------------------------------------
FIXTURE_CASES = [(0, 15), (1, 13), (0, 12)]


def fixture_env(z, key, num_commands):
    """the environment views ([N, k]) of a case of tests/golden/behaviour_metrics.npz"""
    t = lambda k: torch.from_numpy(z[f"{key}_in_{k}"])
    N = t("commands").shape[0]
    env = types.SimpleNamespace(cfg=types.SimpleNamespace(commands=types.SimpleNamespace(num_commands=num_commands)))
    env.commands = t("commands")
    env.root_states = torch.zeros(N, 13)
    env.root_states[:, 0:7] = t("base_pose")
    env.contact_forces = torch.zeros(N, 17, 3)
    env.contact_forces[:, [4, 8, 12, 16], :] = t("foot_forces")
    env.foot_positions, env.foot_indices = t("foot_positions"), t("foot_indices")
    return env


def snapshot_of(env):
    """the SoA buffers ([k][N]) of an environment object with [N, k] views; the command vector padded to fifteen rows"""
    N = env.commands.shape[0]
    commands = np.zeros((15, N), f32)
    commands[:env.commands.shape[1]] = env.commands.t().numpy()
    return dict(commands=commands, root_states=np.ascontiguousarray(env.root_states.t().numpy()),
                contact_forces=np.ascontiguousarray(env.contact_forces.reshape(N, 51).t().numpy()),
                foot_positions=np.ascontiguousarray(env.foot_positions.reshape(N, 12).t().numpy()),
                foot_indices=np.ascontiguousarray(env.foot_indices.t().numpy()), reset_buf=np.zeros(N, np.uint8), episode_length_buf=np.full(N, 100, np.int32))


@pytest.mark.parametrize("seed,num_commands", FIXTURE_CASES)
def test_placement_errors_are_the_references_raibert_term(seed, num_commands):
    """the squares of placement_errors summed over feet and axes are the reference's recorded _reward_raibert_heuristic bit for bit, NaN
    pattern included; the model's ex, ey on the same inputs agree with them within the behaviour tests' tolerance for that comparison
    (not bit for bit: the host definition takes the yaw through atan2, sin and cos, the header through the normalised quaternion)"""
    from go1_gym_learn.eval_metrics import behaviour, placement
    z = np.load(os.path.join(GOLDEN, "behaviour_metrics.npz"))
    key = f"s{seed}_c{num_commands}"
    env = fixture_env(z, key, num_commands)
    err = placement.placement_errors(env)
    assert err.shape == (64, 4, 2) and err.dtype == torch.float32
    got, want = torch.square(err).sum(dim=(1, 2)).numpy(), z[f"{key}_out_raibert_heuristic"]
    assert got.dtype == want.dtype == f32 and bits(got[~np.isnan(want)]) == bits(want[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isfinite(got), np.isfinite(want))
    assert not np.isfinite(want[0]) and np.isfinite(want[1:]).all()                    # the robot commanded to 0 Hz
    assert bits(got) == bits(behaviour.raibert_heuristic(env).numpy())
    v = T.step_values(T.config(num_commands=num_commands), snapshot_of(env))
    for axis, name in enumerate(("ex", "ey")):
        host, model = err[:, :, axis].numpy().T.astype(np.float64), v[name].astype(np.float64)
        fin = np.isfinite(host)
        assert np.array_equal(fin, np.isfinite(model)), name
        assert np.allclose(host[fin], model[fin], rtol=2e-5, atol=2e-6), (name, np.abs(host[fin] - model[fin]).max())
        assert np.abs(host[fin]).max() > 0.01
    contact = z[f"{key}_in_foot_forces"][:, :, 2] > 1.0
    assert np.array_equal(v["c"], contact.T) and 0 < contact.mean() < 1


# ---- 4. the model by hand -----------------------------------------------------------------------------------------------------------------------
def snap_of(feet, contact=(True,) * 4, clocks=(0.25,) * 4, vx=0.0, vy=0.0, yaw_rate=0.0, freq=2.0, width=0.3, length=0.4, base=(0.0, 0.0), reset=0, age=100,
            world=None):
    """one environment that heads along +x (the yaw quaternion is the identity, so the yaw-aligned body frame is the world frame moved
    to `base`): `feet` = the four feet's (x, y) in the body frame, or `world` = in the world frame; `contact` = who is on the ground (a
    float is taken as the vertical force itself); clocks of 0.25 make the heuristic's offset exactly 0"""
    s = dict(commands=np.zeros((15, 1), f32), root_states=np.zeros((13, 1), f32), foot_positions=np.zeros((12, 1), f32), contact_forces=np.zeros((51, 1), f32),
             foot_indices=np.zeros((4, 1), f32), reset_buf=np.full(1, reset, np.uint8), episode_length_buf=np.full(1, age, np.int32))
    for k, value in ((0, vx), (1, vy), (2, yaw_rate), (4, freq), (12, width), (13, length)):
        s["commands"][k, 0] = value
    s["root_states"][0, 0], s["root_states"][1, 0], s["root_states"][2, 0], s["root_states"][6, 0] = base[0], base[1], 0.3, 1.0
    for f in range(4):
        x, y = world[f] if world is not None else (f32(base[0]) + f32(feet[f][0]), f32(base[1]) + f32(feet[f][1]))
        s["foot_positions"][3 * f, 0], s["foot_positions"][3 * f + 1, 0], s["foot_positions"][3 * f + 2, 0] = x, y, 0.02
        s["contact_forces"][12 * (f + 1) + 2, 0] = contact[f] if isinstance(contact[f], float) else (30.0 if contact[f] else 0.0)
        s["foot_indices"][f, 0] = clocks[f]
    return s


def nominal(width=0.3, length=0.4):
    """the four nominal stance points as the header forms them"""
    return [(f32(sx) * f32(length) / f32(2), f32(sy) * f32(width) / f32(2)) for sx, sy in zip((1, 1, -1, -1), (1, -1, 1, -1))]


def play(cfg_, steps):
    st, did = T.State(1), []
    for kw in steps:
        did.append(T.accumulate(st, cfg_, snap_of(**kw)))
    return st, did


def folded(st, f):
    """{metric: (count, nonfinite, min, max)} of foot f of environment 0"""
    return {name: (int(st.count[f * T.M + m, 0]), int(st.nonfinite[f * T.M + m, 0]), float(st.min[f * T.M + m, 0]), float(st.max[f * T.M + m, 0]))
            for m, name in enumerate(T.METRICS)}


NOTHING = (0, 0, INF, -INF)


def test_model_a_foot_on_the_target_has_no_error():
    st, did = play(T.config(), [dict(feet=nominal())])
    for f in range(4):
        got = folded(st, f)
        assert got["stance_err_x"] == got["stance_err_y"] == (1, 0, 0.0, 0.0) and got["swing_err_x"] == NOTHING, f
    assert not did[0]["values"]["px"].any() and not did[0]["values"]["py"].any() and st.touchdowns.sum() == 0          # the contact was unknown before
    # with the heuristic's offset: clock 0 is ph = 0.5, xo = 0.5 * 0.9 * (0.5 / 3), formed as the header forms it
    xo = f32(0.5) * f32(0.9) * (f32(0.5) / f32(3.0))
    assert abs(float(xo) - 0.075) < 1e-8
    feet = [(x + xo, y) for x, y in nominal()]
    st, did = play(T.config(), [dict(feet=feet, clocks=(0.0,) * 4, vx=0.9, freq=3.0, contact=(False,) * 4)])
    for f in range(4):
        got = folded(st, f)
        assert got["swing_err_x"] == got["swing_err_y"] == (1, 0, 0.0, 0.0) and got["stance_err_x"] == NOTHING, f
        assert did[0]["values"]["px"][f, 0] == xo and did[0]["values"]["xo"][f, 0] == xo
    # a foot 2 cm ahead of and 1 cm inside its target: realised minus commanded
    feet = [(x + f32(0.02), y - f32(0.01) * np.sign(y)) for x, y in nominal()]
    st, _ = play(T.config(), [dict(feet=feet)])
    for f in range(4):
        got = folded(st, f)
        assert got["stance_err_x"][2] == pytest.approx(0.02, abs=1e-7) and got["stance_err_y"][2] == pytest.approx(-0.01 if f % 2 == 0 else 0.01, abs=1e-7)


def test_model_the_hind_feet_offset_sign_and_the_short_command_vectors():
    # a yaw command of 1 rad/s at 2 Hz with length 0.4: cmd_vy = 0.2, half_period = 0.25, ph = 0.5: yo = +0.025 in front, -0.025 behind
    st, did = play(T.config(), [dict(feet=nominal(), clocks=(0.0,) * 4, yaw_rate=1.0)])
    yo = f32(0.5) * (f32(1.0) * f32(0.4) / f32(2)) * (f32(0.5) / f32(2.0))
    assert abs(float(yo) - 0.025) < 1e-8 and did[0]["values"]["yo"][:, 0].tolist() == [yo, yo, -yo, -yo]
    for f in range(4):
        got = folded(st, f)
        want = -0.025 if f < 2 else 0.025                                    # the foot stands at its nominal point: realised minus commanded = -yo
        assert got["stance_err_y"][2] == pytest.approx(want, abs=1e-7) and got["stance_err_x"] == (1, 0, 0.0, 0.0), f
    # twelve commands: width 0.3 and length 0.45 whatever rows 12 and 13 hold; thirteen: the width is read, the length is not
    for num_commands, width, length in ((12, 0.3, 0.45), (13, 0.2, 0.45), (14, 0.2, 0.36), (15, 0.2, 0.36)):
        s = snap_of(nominal(width, length), width=0.2, length=0.36)
        v = T.step_values(T.config(num_commands=num_commands), s)
        assert v["width"][0] == f32(width) and v["length"][0] == f32(length), num_commands
        assert not v["px"].any() and not v["py"].any() and not v["ex"].any(), num_commands
        assert v["xs"][:, 0].tolist() == [x for x, _ in nominal(width, length)] and v["ys"][:, 0].tolist() == [y for _, y in nominal(width, length)]


def foot0(xs, contacts, **kw):
    """steps in which foot 0 stands `xs[t]` ahead of its nominal point and the other feet on theirs, in the air"""
    home = nominal()
    return [dict(feet=[(home[0][0] + f32(x), home[0][1])] + home[1:], contact=(c, False, False, False), **kw) for x, c in zip(xs, contacts)]


def test_model_a_stance_from_touchdown_to_liftoff():
    st, did = play(T.config(), foot0([0.2, 0.10, 0.05, -0.02, -0.2], [False, True, True, True, False]))
    got = folded(st, 0)
    px = [float(d["values"]["px"][0, 0]) for d in did]
    assert px == pytest.approx([0.2, 0.10, 0.05, -0.02, -0.2], abs=1e-7)
    assert got["touchdown_x"] == (1, 0, px[1], px[1]) and got["touchdown_y"] == (1, 0, 0.0, 0.0) and got["touchdown_err_x"] == (1, 0, px[1], px[1])
    assert got["liftoff_x"] == (1, 0, px[3], px[3]) and got["liftoff_y"] == (1, 0, 0.0, 0.0)
    sweep = float(f32(px[1]) - f32(px[3]))
    assert got["stance_sweep"] == (1, 0, sweep, sweep) and sweep == pytest.approx(0.12, abs=1e-7) and sweep > 0          # backward under the body: positive
    assert got["stance_err_x"][0] == 3 and got["swing_err_x"][0] == 2 and got["stride_length"] == NOTHING
    assert (st.touchdowns[0, 0], st.liftoffs[0, 0], st.strides[0, 0], st.stance_open[0, 0], st.stride_open[0, 0], st.prev_contact[0, 0]) == (1, 1, 0, 0, 1, 0)
    assert [bool(d["touchdown"][0, 0]) for d in did] == [False, True, False, False, False] and [bool(d["liftoff"][0, 0]) for d in did] == [False] * 4 + [True]
    assert st.count[T.M:].sum() == 3 * 2 * 5                                 # the other feet: five swing steps each, two rows
    # a stance whose touchdown was not seen folds nothing at its liftoff
    st, did = play(T.config(), foot0([0.10, 0.05, -0.02, -0.2], [True, True, True, False]))
    got = folded(st, 0)
    assert got["touchdown_x"] == got["liftoff_x"] == got["stance_sweep"] == NOTHING and got["stance_err_x"][0] == 3
    assert did[3]["unseen_liftoff"][0, 0] and (st.touchdowns[0, 0], st.liftoffs[0, 0]) == (0, 0) and st.map.sum() == 0 and st.map_outside.sum() == 0


def walk(touchdowns_at, steps, speed=0.9, freq=3.0, **spoil):
    """a robot that moves along +x at `speed`; foot 0 is planted in the world from each step of `touchdowns_at` for three steps, half a
    commanded stride ahead of its nominal point, and swings otherwise"""
    home, out, planted = nominal(), [], None
    for t in range(steps):
        base = (speed * 0.02 * t, 0.0)
        if t in touchdowns_at:
            planted = (f32(base[0]) + home[0][0] + f32(0.05), home[0][1])
        down = planted is not None and any(0 <= t - t0 < 3 for t0 in touchdowns_at)
        world = [planted if down else (f32(base[0]) + home[0][0], home[0][1])] + [(f32(base[0]) + x, y) for x, y in home[1:]]
        kw = dict(feet=None, world=world, base=base, contact=(down, False, False, False), vx=speed, freq=freq)
        kw.update(spoil.get("at", {}).get(t, {}))
        out.append(kw)
    return out


def test_model_the_stride_length():
    """0.9 m/s at 3 Hz: a stride of 0.3 m.  Touchdowns 50 / 3 steps apart are not to be had; the foot is planted 0.3 m further instead"""
    steps = walk((2, 12), 16)
    first = steps[2]["world"][0][0]
    for kw in steps[12:15]:
        kw["world"][0] = (first + f32(0.3), kw["world"][0][1])
    st, did = play(T.config(), steps)
    got = folded(st, 0)
    assert (st.touchdowns[0, 0], st.strides[0, 0], st.liftoffs[0, 0]) == (2, 1, 2) and did[12]["stride"][0, 0] and not did[2]["stride"][0, 0]
    assert got["stride_length"][0] == 1 and got["stride_length"][2] == pytest.approx(0.3, abs=1e-7)
    assert got["stride_length_err"][0] == 1 and abs(got["stride_length_err"][2]) < 1e-6
    assert float(did[12]["values"]["commanded_stride"][0]) == pytest.approx(0.3, abs=1e-7)
    assert st.td_world_x[0, 0] == first + f32(0.3) and got["touchdown_x"][0] == 2
    # the lateral command counts, the yaw command does not
    st, _ = play(T.config(), [dict(kw, vy=1.2, yaw_rate=2.0) for kw in steps])
    assert folded(st, 0)["stride_length_err"][2] == pytest.approx(0.3 - 1.5 / 3.0, abs=1e-6)
    # cmd[4] = 0: the errors are not finite, and are counted
    st, _ = play(T.config(), [dict(kw, freq=0.0) for kw in steps])
    got = folded(st, 0)
    assert got["stride_length"][:2] == (1, 0) and got["stride_length_err"] == (0, 1, INF, -INF) and np.isfinite(st.sum).all()
    assert got["touchdown_x"][:2] == (2, 0) and got["touchdown_err_x"][:2] == (0, 2) and got["swing_err_x"][0] == 0 and got["swing_err_x"][1] > 0


@pytest.mark.parametrize("spoil", [dict(reset=1, age=0), dict(age=2)])
def test_model_a_reset_or_a_warm_up_inside_a_stance_or_stride_folds_nothing(spoil):
    quiet, _ = play(T.config(warmup_steps=2), walk((2, 8, 14), 20))
    assert (quiet.touchdowns[0, 0], quiet.strides[0, 0], quiet.liftoffs[0, 0]) == (3, 2, 3)
    # inside the second stance (step 9): that stance's liftoff is not folded, and the stride to the third touchdown is not either
    st, did = play(T.config(warmup_steps=2), walk((2, 8, 14), 20, at={9: spoil}))
    assert not did[9]["live"][0] and (st.touchdowns[0, 0], st.strides[0, 0], st.liftoffs[0, 0]) == (3, 1, 2) and did[11]["unseen_liftoff"][0, 0]
    assert (st.steps[0], st.resets[0]) == (20, spoil.get("reset", 0)) and folded(st, 0)["stance_err_x"][0] == 8
    # in the swing between the second and third stance (step 12): the stance is complete, the stride is broken
    st, did = play(T.config(warmup_steps=2), walk((2, 8, 14), 20, at={12: spoil}))
    assert (st.touchdowns[0, 0], st.strides[0, 0], st.liftoffs[0, 0]) == (3, 1, 3) and not did[14]["stride"][0, 0] and did[14]["touchdown"][0, 0]
    # right after the spoilt step the state is unknown and nothing is open
    st, _ = play(T.config(warmup_steps=2), walk((2, 8, 14), 10, at={9: spoil}))
    assert st.prev_contact[:, 0].tolist() == [2] * 4 and not st.stance_open.any() and not st.stride_open.any()
    # a warm-up that never ends: steps and nothing else
    st, _ = play(T.config(warmup_steps=1000), walk((2, 8, 14), 20))
    assert st.steps[0] == 20 and st.count.sum() == 0 and st.nonfinite.sum() == 0 and st.touchdowns.sum() == 0 and st.map.sum() == 0


def test_model_the_map_edges():
    cell = f32(0.03)
    low = f32(-4.0) * cell
    cases = [(low, 0, "the lower edge is inside"), (np.nextafter(low, f32(-1)), None, "one ulp below it"), (f32(4.0) * cell, None, "the upper edge is outside"),
             (np.nextafter(f32(4.0) * cell, f32(0)), 7, "one ulp below it"), (f32(0.0), 4, "the nominal point"), (f32(NAN), None, "a NaN"), (f32(INF), None, "inf"),
             (f32(-1e30), None, "far below")]
    for value, want, label in cases:
        # width = length = 0: the nominal points are the base, px is the foot's x itself and py is 0 (v = 4)
        steps = [dict(feet=[(0.0, 0.0)] * 4, contact=(False,) * 4, width=0.0, length=0.0), dict(feet=[(value, 0.0)] + [(0.0, 0.0)] * 3, width=0.0, length=0.0)]
        st, did = play(T.config(map_cell=0.03), steps)
        assert st.touchdowns[:, 0].tolist() == [1] * 4, label
        if np.isfinite(value):
            assert did[1]["values"]["px"][0, 0] == value, label
        assert st.map[0, :, 0].sum() + st.map_outside[0, 0] == 1 and st.map_outside[0, 0] == (want is None), label
        if want is not None:
            assert st.map[0, 8 * 4 + want, 0] == 1, label
        assert st.map[1:, 36, 0].tolist() == [1] * 3                         # the other feet on their nominal points: u = v = 4
        along_y = [dict(kw, feet=[(y, x) for x, y in kw["feet"]]) for kw in steps]
        st, _ = play(T.config(map_cell=0.03), along_y)                       # the same along y: the row index
        assert st.map_outside[0, 0] == (want is None) and (want is None or st.map[0, 8 * want + 4, 0] == 1), label
    assert T.map_coord(np.array([low], f32), 0.03)[0] == 0.0 and T.map_coord(np.array([np.nextafter(low, f32(-1))], f32), 0.03)[0] == -1.0


def test_model_the_track_width_error_sign():
    feet = [(0.2, 0.2), (0.2, -0.2), (-0.2, 0.1), (-0.2, -0.1)]             # the front feet 0.4 m apart, the hind feet 0.2 m, commanded 0.3 m
    st, _ = play(T.config(), [dict(feet=feet, contact=(False,) * 4), dict(feet=feet)])
    for f in range(4):
        got = folded(st, f)["track_width_err"]
        assert got[:2] == (1, 0) and got[2] == pytest.approx(0.1 if f < 2 else -0.1, abs=1e-7), f
    table, cells = T.reduce(st, [0], 2)
    assert table.shape == (2, 57, 6) and cells.shape == (2, 4, 64) and table[0, 56].tolist() == [1.0, 2.0, 0.0, 4.0, 0.0, 4.0 - cells[0].sum()]
    assert not table[1, 56].any() and np.isnan(table[1, :56, 1:5]).all() and not cells[1].any()


# ---- 5. go1place.hip under the SIMT emulator against the model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1place_host as G
    return G.load_library(build_emu(g.place_sources(), "libgo1place_emu.so"))


SHAPES_OF_INPUTS = dict(commands=15, root_states=13, foot_positions=12, contact_forces=51, foot_indices=4)


def place_on(device, cfg_, N, lib=None):
    """a go1place_host.Go1Place on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1place_host as G
    tensors = {k: torch.zeros(rows, N, device=device) for k, rows in SHAPES_OF_INPUTS.items()}
    tensors.update(reset_buf=torch.zeros(N, dtype=torch.uint8, device=device), episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    pm = G.Go1Place(types.SimpleNamespace(num_envs=N, num_commands=cfg_.num_commands), B, map_cell=cfg_.map_cell, lib=lib)
    if torch.device(device).type == "cpu":
        pm._stream = lambda: None
    return pm, B


def place_groups(rng, N, groups=3):
    """three groups of which group 1 is empty, some environments at -1 and (from three environments on) one id outside the tables"""
    assert groups == 3
    group = rng.integers(-1, groups, N).astype(np.int32)
    group[group == 1] = 2
    group[0] = groups - 1
    if N >= 3:
        group[1], group[2] = -1, groups
    return group


def drive(pm, B, cfg_, snaps, group, groups):
    """the scripted steps through the library: arm for `groups` groups, upload a snapshot, accumulate, ...; returns read() and the
    accumulators.  arm() sizes the tables by the largest id it is given, so the ids outside the tables are handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    pm.arm(inside, cfg_.warmup_steps)
    pm.group.copy_(torch.from_numpy(group))
    for s in snaps:
        for k, a in s.items():
            getattr(B, k).copy_(torch.from_numpy(a))
        pm.accumulate()
    pm.disarm()
    res = pm.read()
    acc = {k: t.cpu().numpy() for k, t in pm.acc.items()}
    return res, acc


def state_name(k):
    return "env_map" if k == "map" else k


def one_nan(a):
    """`a` with every NaN replaced by one NaN: a float of the state may hold a NaN (px of a foot whose position is not finite), and IEEE 754
    leaves the sign and payload of a NaN that an operation makes to the hardware (an x86 host makes a negative one, the GPU a positive one);
    which words are NaN, and every other bit, are compared"""
    return np.where(np.isnan(a), a.dtype.type(np.nan), a) if a.dtype.kind == "f" else a


def same_as_the_model(res, acc, st, group, groups):
    """accumulators, state, map and both result tables against the model's state `st`, bit for bit"""
    N = st.N
    for k in ACCUMULATORS:
        assert acc[k].shape == (56, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in T.STATE:
        got, want = res[state_name(k)].view(getattr(st, k).dtype), getattr(st, k)
        assert got.shape == want.shape and bits(one_nan(got)) == bits(one_nan(want)), k
    want, want_cells = T.reduce(st, group, groups)
    rows = np.stack([res["metrics"][m] for m in T.METRICS], axis=2).reshape(groups, 56, 6)                   # (G, 4, 14, 6): row f * 14 + metric
    table = np.concatenate([rows, res["groups"][:, None, :]], axis=1)
    assert table.shape == want.shape == (groups, T.ROWS, 6)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and bits(table) == bits(want)
    assert res["map"].shape == (groups, 4, 8, 8) and bits(res["map"]) == bits(want_cells)
    return want, want_cells


def check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N):
    """the library's results against tests/place_ref.py, bit for bit; then that the script drove every kind of environment it was
    written to drive"""
    st, did = T.run(cfg_, snaps, N)
    want, want_cells = same_as_the_model(res, acc, st, group, groups)
    steps = len(snaps)
    row = lambda m: np.stack([st.count[f * T.M + m] for f in range(4)]).astype(np.int64)       # (4, N): the folded values of a row
    assert (res["steps"] == steps).all() and res["map_edges"][0] == pytest.approx(-0.12, abs=1e-8)
    assert (st.map.sum(axis=1) + st.map_outside == st.touchdowns).all() and (st.strides <= st.touchdowns).all() and (st.liftoffs <= st.touchdowns).all()
    stance, swing, sweeps = row(T.STANCE_ERR_X), row(T.SWING_ERR_X), row(T.STANCE_SWEEP)
    bad = st.nonfinite.reshape(4, T.M, N).sum(axis=(0, 1))
    walks = kind == 0
    # a clean walk: a trot of ten steps seen from step 2 on: FL and RR touch down at 10, 20, 30, FR and RL at 5, 15, 25, 35; every
    # stance seen from its touchdown is closed by a liftoff, every touchdown but the first closes a stride, every footprint is in the map
    assert walks.any() and (st.resets[walks] == 0).all() and bad[walks].sum() == 0
    assert (st.touchdowns[:, walks] == np.array([3, 4, 4, 3])[:, None]).all() and (st.strides[:, walks] == st.touchdowns[:, walks] - 1).all()
    assert (st.liftoffs[:, walks] == 3).all() and (sweeps[:, walks] == 3).all() and (st.map_outside[:, walks] == 0).all()
    assert ((stance + swing)[:, walks] == steps - cfg_.warmup_steps).all()
    assert np.isfinite(st.sum).all() and np.isfinite(st.sumsq).all()
    if N >= len(T.KINDS):
        _, resets, chatters, stands, threshold, odd, outside = (kind == k for k in range(len(T.KINDS)))
        # resets and the warm-up: fewer strides than a clean walk, and warm-up steps that are no resets
        assert (res["resets"][resets] >= 4).all() and snaps[0]["reset_buf"][resets].all() and (st.strides.sum(axis=0)[resets] < 10).all()
        assert any((~d["live"] & (s["reset_buf"] == 0)).any() for d, s in zip(did, snaps))
        assert ((stance + swing)[0, resets] < steps - cfg_.warmup_steps).all()
        # chatter: a bounce two steps after a touchdown is a touchdown and a stride of two steps
        assert (st.touchdowns[:, chatters] >= 5).all() and (st.touchdowns[:, chatters] > st.touchdowns[:, walks].max()).all()
        assert (st.strides[:, chatters] == st.touchdowns[:, chatters] - 1).all() and (st.liftoffs[:, chatters] >= 4).all()
        # a robot that stands: every folded step in stance, no event at all
        assert (stance[:, stands] == steps - cfg_.warmup_steps).all() and (swing[:, stands] == 0).all()
        assert (st.touchdowns[:, stands] == 0).all() and (st.liftoffs[:, stands] == 0).all() and (st.prev_contact[:, stands] == 1).all()
        # one ulp either side of the threshold gives both contact states
        assert (stance[:, threshold] > 0).all() and (swing[:, threshold] > 0).all()
        # +-inf and NaN in the forces and the positions and cmd[4] = 0 were met and entered no sum
        assert (bad[odd] > 0).all() and bad[~odd].sum() == 0
        assert any(np.isnan(s["contact_forces"][14::12][:, odd]).any() for s in snaps) and any(np.isinf(s["foot_positions"][:, odd]).any() for s in snaps)
        assert any(np.isnan(s["foot_positions"][:, odd]).any() for s in snaps) and any((s["commands"][4, odd] == 0).any() for s in snaps)
        # footprints outside the map
        assert (st.map_outside.sum(axis=0)[outside] > 0).all() and (st.map_outside[:, ~(outside | odd)] == 0).all()
    g = res["groups"]
    assert g[:, 0].sum() == np.isin(group, range(groups)).sum() and (g[:, 1] == steps * g[:, 0]).all() and g[1].tolist() == [0.0] * 6
    assert np.isnan(want[1, :56, 1:5]).all() and not want_cells[1].any()
    members = np.isin(group, range(groups))
    assert g[:, 3].sum() == st.touchdowns[:, members].sum() and g[:, 4].sum() == st.strides[:, members].sum() and g[:, 5].sum() == st.map_outside[:, members].sum()
    assert res["map"].sum() + g[:, 5].sum() == g[:, 3].sum()
    return st


# 1: one thread per foot; 64: one wavefront; 257: two blocks per foot with a ragged tail; 600: three terms per reduction thread and 38
# environments per map slice
SHAPES = [1, 64, 257, 600]


@pytest.mark.parametrize("N", SHAPES)
def test_emulated_place_kernels_follow_the_model(emu, N):
    groups = 3
    rng = np.random.default_rng(1100 + N)
    cfg_, snaps, kind = T.scripted_steps(rng, N)
    assert len(snaps) == T.SCRIPT_STEPS and (cfg_.warmup_steps, cfg_.num_commands) == (2, 15)
    assert N < len(T.KINDS) or set(kind.tolist()) == set(range(len(T.KINDS)))
    group = place_groups(rng, N, groups)
    pm, B = place_on("cpu", cfg_, N, lib=emu)
    res, acc = drive(pm, B, cfg_, snaps, group, groups)
    assert pm.cfg.num_groups == groups and (N < 3 or {-1, groups} <= set(group.tolist()))
    check_against_the_model(res, acc, cfg_, snaps, kind, group, groups, N)
    again = pm.read()                                                        # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ["groups", "map"] + [state_name(k) for k in T.STATE])
    assert all(bits(again["metrics"][m]) == bits(res["metrics"][m]) for m in T.METRICS)
    with pytest.raises(RuntimeError, match="go1place_accumulate failed: -12"):
        pm.cfg.map_cell = 0.0
        pm.accumulate()


def test_emulated_place_kernels_with_short_command_vectors(emu):
    """twelve and thirteen commands: the defaults stand in for the width and the length"""
    N, groups = 70, 3
    for num_commands in (12, 13):
        rng = np.random.default_rng(1200 + num_commands)
        cfg_, snaps, kind = T.scripted_steps(rng, N)
        cfg_.num_commands = num_commands
        group = place_groups(rng, N, groups)
        pm, B = place_on("cpu", cfg_, N, lib=emu)
        res, acc = drive(pm, B, cfg_, snaps, group, groups)
        st, _ = T.run(cfg_, snaps, N)
        same_as_the_model(res, acc, st, group, groups)
        assert st.map_outside.sum() > 0 and st.map.sum() > 0


# ---- 6. the environment hooks without a GPU -----------------------------------------------------------------------------------------------------
def test_placement_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    for module in ("go1eval_host", "go1place_host"):
        monkeypatch.delitem(sys.modules, module, raising=False)
    c = apply_train_config(make_cfg(), num_envs=16)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_placement_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_placement_metrics, env.read_placement_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert all(m not in sys.modules for m in ("go1eval_host", "go1place_host")) and env._place is None        # never measured: no host module
    env.step(torch.zeros(16, 12))                                             # and stepping goes on
    signature = inspect.signature(env.start_placement_metrics)
    assert {k: p.default for k, p in signature.parameters.items() if k != "groups"} == dict(warmup_steps=0, map_cell=0.03)
    families = [name for name, _ in env._STATE_FAMILIES]
    assert ("placement", "_place") in env._STATE_FAMILIES and families.index("gait") < families.index("spectrum") < families.index("rewards")
    assert len(set(families)) == len(families)


# ---- 7. the scenario of the GPU test, through the fp64 oracle here -----------------------------------------------------------------------------
TROT_STEPS, TROT_WARMUP = 100, 2


def trot_events(st):
    """what the GPU test relies on, per (foot, environment): touchdowns, closed strides, folded stance sweeps"""
    sweeps = np.stack([st.count[f * T.M + T.STANCE_SWEEP] for f in range(4)]).astype(np.int64)
    return st.touchdowns.astype(np.int64), st.strides.astype(np.int64), sweeps


def assert_trot_events(st, label, strict=True):
    """strict: at least 2 touchdowns, 1 closed stride and 1 folded stance sweep per (foot, environment); otherwise the weakest form the
    GPU's fp32 trot may be held to: at least 1 touchdown per foot and environment and 1 stride for some foot of every environment"""
    touchdowns, strides, sweeps = trot_events(st)
    print(f"\n{label}: resets {int(st.resets.sum())}; per (foot, environment) touchdowns {touchdowns.min()} to {touchdowns.max()}, closed strides {strides.min()} to "
          f"{strides.max()}, folded stance sweeps {sweeps.min()} to {sweeps.max()}, liftoffs {st.liftoffs.min()} to {st.liftoffs.max()}; touchdowns outside the map "
          f"{int(st.map_outside.sum())} of {int(touchdowns.sum())}")
    assert st.resets.sum() == 0
    assert (st.map.sum(axis=1) + st.map_outside == st.touchdowns).all()
    if strict:
        assert (touchdowns >= 2).all() and (strides >= 1).all() and (sweeps >= 1).all()
    else:
        assert (touchdowns >= 1).all() and (strides.max(axis=0) >= 1).all()


def test_the_trot_script_produces_placements_on_the_oracle(monkeypatch):
    """the scenario of test_gpu_place_metrics.test_placement_through_the_environment on the CPU oracle: under the foot family's trot script
    every foot of every environment touches down and lifts off at least three times in 100 steps, with no reset"""
    import fake_sim
    from test_foot_metrics import trot_action
    from test_gpu_response_trace import make_env
    fake_sim.install(monkeypatch)
    N = 64
    env = make_env(N, "plane", 20.0, seed=4)
    env.reset()
    cfg_ = T.config(warmup_steps=TROT_WARMUP, num_commands=int(env.sim_config.num_commands), map_cell=0.03)
    st = T.State(N)
    for step in range(TROT_STEPS):
        env.step(trot_action(step, N))
        T.accumulate(st, cfg_, {n: getattr(env.buffers, n).cpu().numpy().copy() for n in T.INPUTS})
    assert_trot_events(st, "oracle")
    assert st.touchdowns.min() >= 3 and st.liftoffs.min() >= 3


# ---- 8. the sweep's host pieces and the tool ------------------------------------------------------------------------------------------------------
def fixed_result():
    import go1place_host as G
    from go1_gym_learn.eval_metrics import behaviour
    cells = behaviour.behaviour_cells(dict(stance_width=[0.1, 0.3, 0.45]))
    commands = behaviour.behaviour_command_table(cells, 15, "cpu").numpy()
    row = lambda n, mean, std=0.0: np.array([[[n, mean, std, mean - std, mean + std, 0.0]] * 4] * 3)
    t = {m: row(40.0, 0.0) for m in T.METRICS}
    t["touchdown_x"], t["touchdown_y"] = row(40.0, 0.06, 0.01), row(40.0, -0.02, 0.005)
    t["touchdown_err_x"], t["touchdown_err_y"] = row(40.0, 0.015), row(40.0, -0.02)
    t["stance_err_x"], t["stance_err_y"], t["swing_err_x"], t["swing_err_y"] = row(900.0, 0.01), row(900.0, -0.015), row(900.0, -0.03), row(900.0, 0.004)
    t["stance_sweep"], t["stride_length"], t["stride_length_err"], t["track_width_err"] = row(36.0, 0.12, 0.02), row(32.0, 0.31, 0.02), row(32.0, -0.023), row(40.0, 0.05)
    t["liftoff_x"] = row(36.0, -0.06, 0.01)
    t["stride_length"][2, 3] = t["stride_length_err"][2, 3] = [0.0, NAN, NAN, NAN, NAN, 0.0]                 # RR of the widest cell closed no stride
    cells_map = np.zeros((3, 4, 8, 8))
    cells_map[:, :, 3, 6], cells_map[:, :, 4, 5], cells_map[2, 3] = 30.0, 8.0, 0.0
    counts = dict(touchdowns=np.full((3, 4), 40.0), strides=np.full((3, 4), 32.0), map_outside=np.full((3, 4), 2.0))
    counts["strides"][2, 3], counts["touchdowns"][2, 3], counts["map_outside"][2, 3] = 0.0, 0.0, 0.0
    return dict(preset="static_medium", cells=cells, commands=commands, placement=t, placement_groups=np.array([[8.0, 320.0, 0.0, 160.0, 128.0, 8.0]] * 3),
                map=cells_map, map_edges=G.map_edges(0.03), foot_counts=counts, metrics={"vel_x_err": np.zeros((3, 6))}, groups=np.zeros((3, 5)), map_cell=0.03,
                num_envs=24, steps=40, warmup_steps=5, seed=1, dt=0.02)


def test_placement_table_json_and_figure(tmp_path):
    from go1_gym_learn.eval_metrics import placement
    res = fixed_result()
    assert placement.commanded(res, 0) == dict(width=pytest.approx(0.1), length=pytest.approx(0.40), stride_length=pytest.approx(1.0 / 3.0))
    md = placement.placement_table(res).splitlines()
    assert md[0].startswith("| stance_width | foot | width / length | touchdown x | touchdown y | touchdown err x / y | stance err x / y | swing err x / y | stance sweep |")
    assert md[0].endswith("| stride real / cmd | track real / cmd | touchdowns | strides | outside map |")
    assert len(md) == 2 + 3 * 4 and len({line.count("|") for line in md}) == 1 and md[0].count("|") == 15
    assert md[2] == ("| 0.1 | FL | 0.100 / 0.400 | +0.060 ± 0.010 | -0.020 ± 0.005 | +0.015 / -0.020 | +0.010 / -0.015 | -0.030 / +0.004 | +0.120 ± 0.020 | "
                     "0.310 / 0.333 | 0.150 / 0.100 | 40 | 32 | 0.050 |")
    assert [line.split("|")[2].strip() for line in md[2:6]] == ["FL", "FR", "RL", "RR"] and md[6].startswith("| 0.3 | FL | 0.300 / 0.400 |")
    assert md[13].startswith("| 0.45 | RR |") and "| – / 0.333 | 0.500 / 0.450 | 0 | 0 | – |" in md[13]
    js = json.loads(json.dumps(placement.placement_to_json(res), allow_nan=False))
    assert js["cells"] == [dict(stance_width=w) for w in (0.1, 0.3, 0.45)] and js["group_fields"] == T.GROUP_FIELDS and js["feet"] == ["FL", "FR", "RL", "RR"]
    assert js["placement"]["stride_length"][2][3][1] is None and js["placement"]["touchdown_x"][0][0][1] == 0.06 and js["map"][0][0][3][6] == 30.0
    assert js["commanded"][2]["width"] == pytest.approx(0.45) and js["map_cell"] == 0.03 and len(js["map_edges"]) == 9 and js["foot_counts"]["strides"][2][3] == 0.0
    assert js["placement_groups"][0][3] == 160.0 and set(js["placement"]) == set(T.METRICS)
    path = tmp_path / "footprints.png"
    placement.plot_footprints(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000


def test_tool_accepts_a_placement_sweep(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import placement
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--placement", "--axis", "stance_width", "0.1", "0.3", "0.45", "--envs", "24", "--steps", "40", "--warmup-steps", "5",
                                      "--presets", "static_medium", "--map-cell", "0.02"])
    assert a.placement and not a.behaviour and not a.coordination and (a.envs, a.steps, a.map_cell) == (24, 40, 0.02)
    assert eval_sweep.behaviour_axes(a) == dict(stance_width=[0.1, 0.3, 0.45])
    plain = eval_sweep.parse_args(base + ["--placement", "--axis", "stance_length", "0.35", "--axis", "vx", "0.5", "1.0"])
    assert plain.map_cell == 0.03 and eval_sweep.behaviour_axes(plain) == dict(stance_length=[0.35], vx=[0.5, 1.0])
    assert not eval_sweep.parse_args(base).placement and eval_sweep.parse_args(base).map_cell is None
    assert eval_sweep.parse_args(base + ["--placement", "--terrain", "plane"]).terrain == "plane"
    for bad in (["--placement", "--terrain"], ["--placement", "--behaviour"], ["--placement", "--joints"], ["--placement", "--feet"], ["--placement", "--trunk"],
                ["--placement", "--rewards"], ["--placement", "--coordination"], ["--placement", "--spectrum"], ["--placement", "--response", "--switch", "vx", "0", "1"],
                ["--placement", "--push", "--magnitude", "1", "--direction", "0"], ["--map-cell", "0.03"], ["--feet", "--map-cell", "0.03"],
                ["--placement", "--map-cell", "0"], ["--placement", "--map-cell", "-0.01"], ["--placement", "--map-cell", "nan"], ["--placement", "--map-cell", "inf"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(base + bad)
    with pytest.raises(SystemExit, match="--placement needs at least one --axis"):
        eval_sweep.behaviour_axes(eval_sweep.parse_args(base + ["--placement"]))
    seen = {}

    def sweep_stub(policy, preset, axes, **kw):
        seen.update(kw, preset=preset, axes=axes)
        return fixed_result()
    monkeypatch.setattr(placement, "run_placement_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    eval_sweep.run_placement(a, None, eval_sweep.behaviour_axes(a))
    assert seen == dict(preset="static_medium", axes=dict(stance_width=[0.1, 0.3, 0.45]), num_envs=24, steps=40, warmup_steps=5, seed=1, terrain=None, map_cell=0.02)
    js = json.load(open(tmp_path / "eval" / "static_medium_placement.json"))
    assert js["preset"] == "static_medium" and js["cells"][1] == dict(stance_width=0.3)
    md = (tmp_path / "eval" / "static_medium_placement.md").read_text()
    assert "| 0.45 | RR |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_footprints.png").read_bytes()[:4] == b"\x89PNG"
