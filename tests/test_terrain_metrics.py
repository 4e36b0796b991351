"""CPU checks of terrain traversal (include/go1eval.h, fifth kernel family): the ctypes mirrors against the header, the refusals
without a GPU, the model of tests/terrain_ref.py on hand-computable cases, go1eval.hip itself under the SIMT emulator against that
model bit for bit (accumulators, state and result table), the environment hooks where there is no GPU, and the sweep's host pieces."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

import terrain_ref as T
from test_response_trace import C_TYPES, HEADER, REPO, eval_emu, bits, enum_order, struct_fields

NAN = float("nan")
f32 = np.float32
TYPES = dict(C_TYPES, uint32_t=ctypes.c_uint32)


# ---- 1. the mirrors against the header ---------------------------------------------------------------------------------------------
def test_terrain_mirrors_match_the_header():
    import go1eval_host as G
    src = open(HEADER).read()
    for macro, value in (("NUM_TERRAIN", G.NUM_TERRAIN), ("NUM_OUTCOME", G.NUM_OUTCOME), ("STUMBLE_RATIO", "5.0"), ("COLLISION_FORCE", "0.1"),
                         ("FOOT_RADIUS", "0.02")):
        assert f"#define GO1EVAL_{macro} {value}" in src
    want = struct_fields(src, "Go1TerrainConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1TerrainConfig._fields_] == [
        "num_envs", "warmup_steps", "num_groups", "hf_rows", "hf_cols", "penalised_body_mask", "dt", "hf_hscale", "hf_vscale", "hf_border",
        "tile_length", "tile_width"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1TerrainConfig._fields_):
        assert ctype is TYPES[ctext], field
    want = struct_fields(src, "Go1TerrainBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1TerrainBuffers._fields_]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1TerrainBuffers._fields_)
    assert [f for f, _ in want] == T.INPUTS + ["count", "sum", "sumsq", "min", "max", "nonfinite"] + T.STATE + ["group", "results"]
    assert dict(want)["height_samples"] == "const int16_t*" and dict(want)["status"] == "uint8_t*" and dict(want)["max_dist"] == "float*"
    assert G._TERRAIN_INPUTS == T.INPUTS and G._TERRAIN_STATE == T.STATE
    assert enum_order(src, "Go1TerrainMetric", "GO1TERRAIN_") == G.TERRAIN_NAMES == T.METRICS and len(T.METRICS) == G.NUM_TERRAIN == 5
    assert enum_order(src, "Go1TerrainStatus", "GO1TERRAIN_S_") == G.TERRAIN_STATUS == T.STATUS
    assert enum_order(src, "Go1TerrainOutcome", "GO1TERRAIN_O_") == G.TERRAIN_OUTCOMES == T.OUTCOMES and len(T.OUTCOMES) == G.NUM_OUTCOME
    assert enum_order(src, "Go1TerrainGroupField", "GO1TERRAIN_G_") == G.TERRAIN_GROUP_FIELDS == T.GROUP_FIELDS and len(T.GROUP_FIELDS) == G.NUM_FIELDS
    assert set(G.EXPORTED_SYMBOLS) >= {"go1eval_terrain_clear", "go1eval_terrain_accumulate", "go1eval_terrain_reduce"}
    # the existing layouts are as they were
    assert [ctypes.sizeof(s) for s in (G.Go1EvalConfig, G.Go1BehaviourConfig, G.Go1TraceConfig, G.Go1PushConfig, G.Go1RecoveryConfig)] == [20, 28, 20, 8, 36]
    assert ctypes.sizeof(G.Go1ResponseConfig) == 11 * 4 + G.MAX_SIGNALS * 16 and ctypes.sizeof(G.Go1TerrainConfig) == 48
    assert [ctypes.sizeof(s) // 8 for s in (G.Go1EvalBuffers, G.Go1BehaviourBuffers, G.Go1TraceBuffers, G.Go1ResponseBuffers, G.Go1PushBuffers,
                                            G.Go1RecoveryBuffers)] == [22, 24, 13, 5, 3, 5]


# ---- 2. the refusals without a GPU ---------------------------------------------------------------------------------------------------
def _terrain_cfg(G, **over):
    c = G.Go1TerrainConfig()
    c.num_envs, c.warmup_steps, c.num_groups, c.hf_rows, c.hf_cols, c.penalised_body_mask = 8, 0, 1, 7, 9, 1
    c.dt, c.hf_hscale, c.hf_vscale, c.hf_border, c.tile_length, c.tile_width = 0.02, 0.25, 0.005, 0.5, 1.0, 0.75
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_terrain_arguments_are_checked_before_any_launch():
    import __graft_entry__ as g
    import go1eval_host as G
    g.build_eval_hip()
    lib = G.load_library()
    ref = ctypes.byref
    anything = np.zeros(51 * 8, np.float64)
    calls = (lib.go1eval_terrain_clear, lib.go1eval_terrain_accumulate, lib.go1eval_terrain_reduce)
    buf = G.Go1TerrainBuffers()
    for fn in calls:
        assert fn(None, None, None) == -1
        assert fn(ref(_terrain_cfg(G, num_envs=0)), ref(buf), None) == -1
        assert fn(ref(_terrain_cfg(G)), ref(buf), None) == -2                      # no accumulators, no state
    for n in ["count", "sum", "sumsq", "min", "max", "nonfinite"] + G._TERRAIN_STATE[:-1]:
        setattr(buf, n, anything.ctypes.data)
    for fn in calls:
        assert fn(ref(_terrain_cfg(G)), ref(buf), None) == -2                      # max_dist is missing
    buf.max_dist = anything.ctypes.data
    assert lib.go1eval_terrain_accumulate(ref(_terrain_cfg(G)), ref(buf), None) == -3           # no inputs
    assert lib.go1eval_terrain_reduce(ref(_terrain_cfg(G)), ref(buf), None) == -5               # no group, no table
    buf.group = buf.results = anything.ctypes.data
    assert lib.go1eval_terrain_reduce(ref(_terrain_cfg(G, num_groups=0)), ref(buf), None) == -5
    for bad in (0.0, -0.02, NAN):
        assert lib.go1eval_terrain_reduce(ref(_terrain_cfg(G, dt=bad)), ref(buf), None) == -12
    for n in G._TERRAIN_INPUTS:
        if n not in ("height_samples", "env_origins"):
            setattr(buf, n, anything.ctypes.data)
    assert lib.go1eval_terrain_accumulate(ref(_terrain_cfg(G)), ref(buf), None) == -3           # env_origins is missing
    buf.env_origins = anything.ctypes.data
    refused = [dict(hf_hscale=0.0), dict(hf_hscale=-0.25), dict(hf_hscale=NAN), dict(tile_length=0.0), dict(tile_length=-1.0), dict(tile_width=0.0),
               dict(tile_width=NAN), dict(dt=0.0), dict(dt=-0.02)]
    for over in refused:                                                            # with the plane (no field) ...
        assert lib.go1eval_terrain_accumulate(ref(_terrain_cfg(G, **over)), ref(buf), None) == -12, over
    buf.height_samples = anything.ctypes.data
    for over in refused + [dict(hf_rows=1), dict(hf_cols=1), dict(hf_rows=0, hf_cols=0), dict(hf_cols=-9)]:           # ... and with a field
        assert lib.go1eval_terrain_accumulate(ref(_terrain_cfg(G, **over)), ref(buf), None) == -12, over
    assert not anything.any()


# ---- 3. the model by hand ---------------------------------------------------------------------------------------------------------------
#  the three samples of every cell differ, each of them is the lowest somewhere, and where the diagonal neighbour is lower still
#  (cells (0, 0) and (0, 2)) it must not be picked
FIELD = np.array([[5, 9, 2, 8],
                  [7, 1, 6, 3],
                  [4, 0, 11, 10]], np.int16)
LOWEST = [[5, 1, 2], [1, 0, 3]]                      # min(s[px][py], s[px + 1][py], s[px][py + 1]) of cell (px, py)


def test_model_height_sample_picks_the_cell_and_its_two_neighbours():
    geo = T.geometry(hf_hscale=0.5, hf_vscale=0.25, hf_border=0.0, height_samples=FIELD)
    for px in range(2):
        for py in range(3):
            h = T.height(geo, 0.5 * px + 0.25, 0.5 * py + 0.25)                         # the middle of the cell: x picks the row, y the column
            assert type(h) is f32 and h == 0.25 * LOWEST[px][py], (px, py)
    assert T.height(geo, 0.25, 1.25) == 0.5 and T.height(geo, 1.25, 0.25) == 0.25       # (0, 2) and, were x and y swapped, (1, 0)
    assert T.height(geo, 0.4999, 0.9999) == 0.25 and T.height(geo, 0.5, 1.0) == 0.75    # truncation: the cell starts AT its sample
    # the clamps: below 0 on either axis, and beyond the last cell (rows - 2 = 1, cols - 2 = 2)
    assert T.height(geo, -3.0, 0.25) == 1.25 and T.height(geo, -0.2, -7.0) == 1.25 and T.height(geo, 0.75, -1e30) == 0.25
    assert T.height(geo, 1.0, 0.25) == 0.25 and T.height(geo, 100.0, 0.75) == 0.0 and T.height(geo, 0.25, 1.5) == 0.5
    assert T.height(geo, 3.0e38, 3.0e38) == 0.75 and T.height(geo, 1e30, -1e30) == 0.25   # the quotient overflows: clamped, never converted
    shifted = T.geometry(hf_hscale=0.5, hf_vscale=0.25, hf_border=0.5, height_samples=FIELD)
    assert T.height(shifted, -0.25, 0.25) == 0.25 and T.height(shifted, -0.75, -0.25) == 1.25 and T.height(shifted, 0.25, 0.75) == 0.75
    for x, y in ((NAN, 0.25), (0.25, NAN), (np.inf, 0.25), (0.25, -np.inf)):
        assert np.isnan(T.height(geo, x, y)) and np.isnan(T.height(T.geometry(), x, y))
    assert T.height(T.geometry(), 0.3, 1e30) == 0.0 and not np.signbit(T.height(T.geometry(hf_vscale=-1.0), 0.0, 0.0))      # no field: +0


def snapshot(N=1, **over):
    """a quiet step of N robots on the tile around (1, 1): the base 0.5 m up, the feet 0.25 m up in a square around it, all four
    swinging (desired contact 0, swing phase 0), no force anywhere"""
    s = dict(root_states=np.zeros((13, N), f32), commands=np.zeros((15, N), f32), contact_forces=np.zeros((51, N), f32),
             foot_positions=np.zeros((12, N), f32), desired_contact_states=np.zeros((4, N), f32), foot_indices=np.full((4, N), 0.25, f32),
             env_origins=np.ones((3, N), f32), reset_buf=np.zeros(N, np.uint8), time_out_buf=np.zeros(N, np.uint8),
             episode_length_buf=np.full(N, 5, np.int32))
    s["root_states"][0:2], s["root_states"][2] = 1.0, 0.5
    for f, (ox, oy) in enumerate(((0.25, 0.125), (0.25, -0.125), (-0.25, 0.125), (-0.25, -0.125))):
        s["foot_positions"][3 * f], s["foot_positions"][3 * f + 1], s["foot_positions"][3 * f + 2] = 1.0 + ox, 1.0 + oy, 0.25
    for k, v in over.items():
        s[k] = v
    return s


def folded(st, e=0):
    """{metric: (count, nonfinite, min, max)} of environment e"""
    return {name: (int(st.count[m, e]), int(st.nonfinite[m, e]), float(st.min[m, e]), float(st.max[m, e])) for m, name in enumerate(T.METRICS)}


def test_model_quiet_step_on_the_plane_and_on_a_field():
    st, geo = T.State(1), T.geometry()
    T.accumulate(st, geo, snapshot())
    above = float(f32(0.25) - f32(0.02))
    miss = f32(0.0) * f32(0.0) + f32(0.02) - f32(0.25)
    clearance = float(f32(4 * float(miss * miss)))
    assert folded(st) == dict(base_height_terrain=(1, 0, 0.5, 0.5), feet_clearance_terrain=(1, 0, clearance, clearance),
                              swing_foot_height=(1, 0, above, above), stumble=(1, 0, 0.0, 0.0), collision=(1, 0, 0.0, 0.0))
    assert (st.status[0], st.steps[0], st.end_step[0], st.max_dist[0]) == (T.RUNNING, 1, 0, 0.0)
    assert st.sum[T.SWING, 0] == above and st.sumsq[T.SWING, 0] == above * above
    # on the 3 x 4 field (0.5 m samples from the world's origin, a quarter metre per unit): the base at (1, 1) is over cell (1, 2), 0.75 m
    # up; the feet at x = 1.25 / 0.75, y = 1.125 / 0.875 are over cells (1, 2), (1, 1), (1, 2), (1, 1): 0.75, 0, 0.75, 0 m of ground
    st, geo = T.State(1), T.geometry(hf_hscale=0.5, hf_vscale=0.25, hf_border=0.0, height_samples=FIELD)
    T.accumulate(st, geo, snapshot())
    got = folded(st)
    assert got["base_height_terrain"] == (1, 0, -0.25, -0.25)
    mean = float(f32((2 * float(f32(-0.5) - f32(0.02)) + 2 * float(f32(0.25) - f32(0.02))) / 4))
    assert got["swing_foot_height"] == (1, 0, mean, mean)
    low, high = f32(0.02) - f32(-0.5), f32(0.02) - f32(0.25)
    want = float(f32(float(low * low) + float(high * high) + float(low * low) + float(high * high)))
    assert got["feet_clearance_terrain"] == (1, 0, want, want)


def test_model_tile_edge_is_strict():
    geo = T.geometry(tile_length=1.0, tile_width=0.75)
    # the tile's origin is (1, 1).  One ulp beyond the edge on the far side; on the near side the next position whose DIFFERENCE from the
    # origin is beyond the edge (x - 1 has the ulp 2^-24 there, x itself half of it: one ulp of x rounds back onto the edge)
    step = f32(2.0 ** -24)
    for axis, edge, ulp in ((0, f32(1.5), np.nextafter(f32(1.5), f32(2.0))), (0, f32(0.5), f32(0.5) - step),
                            (1, f32(1.375), np.nextafter(f32(1.375), f32(2.0))), (1, f32(0.625), f32(0.625) - step)):
        st = T.State(2)
        s = snapshot(2)
        s["root_states"][axis] = [edge, ulp]                             # exactly on the edge, and one ulp beyond it
        T.accumulate(st, geo, s)
        assert st.status.tolist() == [T.RUNNING, T.TRAVERSED] and st.end_step.tolist() == [0, 1] and st.steps.tolist() == [1, 1], axis
        assert st.count[:, 0].tolist() == [1] * 5 and st.count[:, 1].tolist() == [0] * 5 and not st.nonfinite.any()
        assert st.max_dist[0] == abs(float(edge) - 1.0) and st.max_dist[1] > st.max_dist[0]
    st = T.State(3)                                                      # a position that is not finite does not traverse
    s = snapshot(3)
    s["root_states"][0], s["root_states"][1, 2] = [NAN, np.inf, 1.25], NAN
    T.accumulate(st, geo, s)
    assert st.status.tolist() == [T.RUNNING] * 3 and st.end_step.tolist() == [0] * 3 and st.max_dist.tolist() == [0.0, np.inf, 0.0]
    assert st.nonfinite[:, 0].tolist() == [1, 0, 0, 0, 0] and st.count[:, 0].tolist() == [0, 1, 1, 1, 1]     # the base has no ground; the feet do


def test_model_resets_first_episode_only():
    geo = T.geometry()
    st = T.State(3)
    s = snapshot(3, reset_buf=np.array([1, 2, 0], np.uint8), time_out_buf=np.array([0, 1, 1], np.uint8))     # a reset on the first step
    T.accumulate(st, geo, s)
    assert st.status.tolist() == [T.FELL, T.TIMED_OUT, T.RUNNING] and st.end_step.tolist() == [1, 1, 0] and st.steps.tolist() == [0, 0, 1]
    assert st.count[:, :2].sum() == 0 and st.count[:, 2].tolist() == [1] * 5                                  # time_out_buf alone means nothing
    moved = snapshot(3)
    moved["root_states"][0, 2] = 1.75
    T.accumulate(st, geo, moved)
    assert st.status.tolist() == [T.FELL, T.TIMED_OUT, T.TRAVERSED] and st.end_step.tolist() == [1, 1, 2] and st.max_dist.tolist() == [0.0, 0.0, 0.75]
    before = {k: v.copy() for k, v in st.arrays().items()}
    wild = snapshot(3, reset_buf=np.ones(3, np.uint8), time_out_buf=np.array([1, 0, 1], np.uint8))          # a reset after the traversal
    wild["root_states"][:] = 1e6
    T.accumulate(st, geo, wild)
    T.accumulate(st, geo, snapshot(3))
    assert all(bits(before[k]) == bits(v) for k, v in st.arrays().items())
    table = T.reduce(st, [0, 0, 0], 1, 0.02)
    assert table[0, 9].tolist() == [3.0, 0.0, 1.0, 1.0, 1.0, 1.0 / 3.0]
    third = 1.0 / 3.0
    assert table[0, 5].tolist() == [3.0, third, np.sqrt(third - third * third), 0.0, 1.0, 0.0] and table[0, 6, :2].tolist() == [3.0, third]
    assert table[0, 7, 3:5].tolist() == [0.0, 0.75] and table[0, 8, 3:5].tolist() == [float(f32(1) * f32(0.02)), float(f32(2) * f32(0.02))]


def test_model_warmup_swing_stumble_and_collision():
    geo = T.geometry(warmup_steps=5, penalised_body_mask=(1 << 0) | (1 << 5) | (1 << 6) | (1 << 17) | (1 << 31))
    st = T.State(1)
    s = snapshot()
    s["root_states"][0] = 1.25
    T.accumulate(st, geo, s)                                             # episode_length_buf = 5 = warmup_steps: the step counts, nothing is folded
    assert st.steps[0] == 1 and st.max_dist[0] == 0.25 and not st.count.any() and not st.nonfinite.any()
    s = snapshot(episode_length_buf=np.array([6], np.int32), desired_contact_states=np.full((4, 1), 0.75, f32))
    F = s["contact_forces"]
    F[0:3, 0] = [0.2, 0.0, 0.0]                                          # the trunk: 0.2 N > 0.1 N
    F[12:15, 0] = [50.0, 0.0, 50.0]                                      # foot 0 (body 4): not in the mask
    F[15:18, 0] = [0.05, 0.0, 0.0]                                       # body 5: in the mask, below the threshold
    F[18:21, 0] = [0.06, 0.06, 0.06]                                     # body 6: 0.104 N
    F[24:27, 0] = [3.0, 4.0, 1.0]                                        # foot 1: 5 N sideways on 1 N: exactly five times, no stumble
    T.accumulate(st, geo, s)
    got = folded(st)
    assert got["swing_foot_height"] == (0, 0, np.inf, -np.inf)           # a step with no swing foot: nothing is folded, nothing is counted
    assert got["stumble"] == (1, 0, 0.0, 0.0) and got["collision"] == (1, 0, 2.0, 2.0) and got["feet_clearance_terrain"][0] == 1
    F[26, 0] = 0.9375
    s["desired_contact_states"][2, 0] = 0.5                              # 0.5 is still a swing foot
    T.accumulate(st, geo, s)
    got = folded(st)
    above = float(f32(0.25) - f32(0.02))
    assert got["stumble"] == (2, 0, 0.0, 1.0) and got["swing_foot_height"] == (1, 0, above, above) and got["collision"] == (2, 0, 2.0, 2.0)
    table = T.reduce(st, [0], 2, 0.02)
    assert table[0, T.STUMBLE].tolist() == [2.0, 0.5, 0.5, 0.0, 1.0, 0.0] and table[0, 9].tolist()[:5] == [1.0, 1.0, 0.0, 0.0, 0.0] and np.isnan(table[0, 9, 5])
    assert table[0, 5].tolist()[0] == 0.0 and np.isnan(table[0, 5, 1:5]).all() and table[0, 5, 5] == 1.0 and table[0, 7, 1] == 0.25    # undecided
    assert table[1, 9].tolist()[:5] == [0.0] * 5 and np.isnan(table[1, 9, 5]) and table[1, :9, 0].tolist() == [0.0] * 9


# ---- 4. go1eval.hip under the SIMT emulator against the model -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import go1eval_host as G
    return G.load_library(eval_emu())


def terrain_on(device, geo, N, lib=None):
    """a go1eval_host.Go1Terrain on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1eval_host as G
    hs = geo.height_samples
    shapes = dict(root_states=13, commands=15, contact_forces=51, foot_positions=12, desired_contact_states=4, foot_indices=4, env_origins=3)
    tensors = {k: torch.zeros(r, N, device=device) for k, r in shapes.items()}
    tensors.update(reset_buf=torch.zeros(N, dtype=torch.uint8, device=device), time_out_buf=torch.zeros(N, dtype=torch.uint8, device=device),
                   episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device),
                   height_samples=None if hs is None else torch.from_numpy(hs).to(device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    S = types.SimpleNamespace(num_envs=N, penalised_body_mask=geo.penalised_body_mask, hf_hscale=geo.hf_hscale, hf_vscale=geo.hf_vscale, hf_border=geo.hf_border)
    ter = G.Go1Terrain(S, B, geo.dt, geo.tile_length, geo.tile_width, lib=lib)
    if torch.device(device).type == "cpu":
        ter._stream = lambda: None
    return ter, B


def drive(ter, B, geo, snaps, group, groups):
    """the scripted steps through the library: arm for `groups` groups, upload a snapshot, accumulate, ...; returns read() and the
    accumulators.  arm() sizes the table by the largest id it is given, so the ids outside the table are handed to the kernels
    afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    ter.arm(inside, geo.warmup_steps)
    ter.group.copy_(torch.from_numpy(group))
    for s in snaps:
        for k, a in s.items():
            getattr(B, k).copy_(torch.from_numpy(a))
        ter.accumulate()
    ter.disarm()
    res = ter.read()
    acc = {k: t.cpu().numpy() for k, t in ter.acc.items()}
    return res, acc


def scripted_groups(rng, N, groups):
    group = rng.integers(-1, groups + 1, N).astype(np.int32)             # includes -1 and an id outside the table ...
    group[group == 1] = 2                                                # ... and an empty group
    group[0], group[1], group[2] = groups - 1, groups, -1
    return group


def check_against_the_model(res, acc, geo, snaps, kind, group, groups, N):
    """accumulators, state and the whole result table against tests/terrain_ref.py, bit for bit; then what the script was written
    to drive: all four statuses, their end steps, the odd coordinates in nonfinite, the groups' bookkeeping"""
    st = T.run(geo, snaps, N)
    for k in ("count", "nonfinite", "sum", "sumsq", "min", "max"):
        assert acc[k].shape == (T.M, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in T.STATE:
        assert bits(res[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    want = T.reduce(st, group, groups, geo.dt)
    table = np.concatenate([np.stack([res["metrics"][m] for m in T.METRICS], axis=1), np.stack([res["outcomes"][o] for o in T.OUTCOMES], axis=1),
                            res["groups"][:, None, :]], axis=1)
    assert table.shape == want.shape == (groups, T.ROWS, 6)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and bits(table) == bits(want)
    status = res["status"]
    assert set(status.tolist()) == {0, 1, 2, 3} and (status[kind == 0] == T.RUNNING).all() and (status[kind == 1] == T.TRAVERSED).all()
    assert (status[kind == 2] == T.FELL).all() and (status[kind == 3] == T.TIMED_OUT).all() and (status[kind == 4] == T.FELL).all()
    assert (res["end_step"][kind == 4] == 1).all() and (res["steps"][kind == 4] == 0).all() and (res["end_step"][status == T.RUNNING] == 0).all()
    assert (res["end_step"][kind == 1] == res["steps"][kind == 1]).all() and (res["end_step"][np.isin(kind, (2, 3))] == res["steps"][np.isin(kind, (2, 3))] + 1).all()
    odd = kind == 5
    assert (status[odd] == T.RUNNING).all() and (res["steps"][odd] == len(snaps)).all() and (res["max_dist"][odd] >= 0.5).all()
    assert (acc["nonfinite"].view(np.uint32)[T.BASE_HEIGHT, odd] == 2).all() and (acc["nonfinite"].view(np.uint32)[T.SWING, odd] <= 1).all()
    assert (acc["count"].view(np.uint32)[T.STUMBLE, odd] == len(snaps) - geo.warmup_steps).all() and acc["nonfinite"].view(np.uint32)[T.STUMBLE:].sum() == 0
    assert (acc["count"].view(np.uint32)[T.SWING] < acc["count"].view(np.uint32)[T.STUMBLE]).any()                  # steps with no swing foot
    assert len(np.unique(acc["max"][T.COLLISION])) >= 4 and set(np.unique(acc["max"][T.STUMBLE]).tolist()) >= {0.0, 1.0}
    g = res["groups"]
    assert g[:, 0].sum() == np.isin(group, range(groups)).sum() and (g[:, 1:5].sum(axis=1) == g[:, 0]).all()
    assert g[1].tolist()[:5] == [0.0] * 5 and np.isnan(g[1, 5]) and np.isnan(want[1, :9, 1:5]).all()
    return st


@pytest.mark.parametrize("N", [70, 300])                                 # one ragged block; a full block and a ragged one
def test_emulated_terrain_kernels_follow_the_model(emu, N):
    groups = 4
    rng = np.random.default_rng(100 + N)
    geo, snaps, kind = T.scripted_steps(rng, N)
    assert geo.height_samples.shape == (7, 9) and len(snaps) == 12
    group = scripted_groups(rng, N, groups)
    ter, B = terrain_on("cpu", geo, N, lib=emu)
    res, acc = drive(ter, B, geo, snaps, group, groups)
    assert ter.cfg.num_groups == groups and {-1, groups} <= set(group.tolist())
    check_against_the_model(res, acc, geo, snaps, kind, group, groups, N)


def test_emulated_terrain_on_the_plane_has_no_field(emu):
    """height_samples = NULL is the plane: the same script over a ground of 0"""
    N, groups = 70, 3
    rng = np.random.default_rng(7)
    geo, snaps, kind = T.scripted_steps(rng, N)
    geo.height_samples = None
    group = scripted_groups(rng, N, groups)
    ter, B = terrain_on("cpu", geo, N, lib=emu)
    assert ter.buf.height_samples is None and ter.cfg.hf_rows == 0
    res, acc = drive(ter, B, geo, snaps, group, groups)
    st = T.run(geo, snaps, N)
    want = T.reduce(st, group, groups, geo.dt)
    table = np.concatenate([np.stack([res["metrics"][m] for m in T.METRICS], axis=1), np.stack([res["outcomes"][o] for o in T.OUTCOMES], axis=1),
                            res["groups"][:, None, :]], axis=1)
    assert bits(table) == bits(want) and res["groups"][:, 0].sum() == np.isin(group, range(groups)).sum() < N
    for k in T.STATE:
        assert bits(res[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    assert bits(ter.acc["sum"].numpy()) == bits(st.sum) and bits(ter.acc["min"].numpy()) == bits(st.min)
    with pytest.raises(RuntimeError, match="go1eval_terrain_accumulate failed: -12"):
        ter.cfg.tile_width = 0.0
        ter.accumulate()


# ---- 5. the environment hooks without a GPU, and place_on_terrain --------------------------------------------------------------------------------
def test_terrain_hooks_on_cpu_buffers(monkeypatch):
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
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_terrain_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_terrain_metrics, env.read_terrain_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    with pytest.raises(ValueError, match="has no tile grid"):
        env.place_on_terrain(0, 0)
    assert "go1eval_host" not in sys.modules and env._traversal is None       # an environment that never measures never imports the library
    env.step(torch.zeros(16, 12))                                             # and stepping goes on


def test_place_on_terrain_checks_its_arguments():
    from go1_gym.envs.base.legged_robot import LeggedRobot
    origins = torch.arange(18.0).reshape(2, 3, 3)
    resets = []
    env = types.SimpleNamespace(cfg=types.SimpleNamespace(terrain=types.SimpleNamespace(mesh_type="trimesh", num_rows=2, num_cols=3, terrain_origins=origins)),
                                num_train_envs=6, device="cpu", terrain_levels=torch.zeros(8, dtype=torch.long), terrain_types=torch.zeros(8, dtype=torch.long),
                                buffers=types.SimpleNamespace(env_origins=torch.zeros(3, 8)), reset_idx=lambda ids: resets.append(ids.tolist()))
    place = lambda *a: LeggedRobot.place_on_terrain(env, *a)
    bad = [([2, 0], [0, 0], [0, 1]), ([0, 0], [3, 0], [0, 1]), ([-1, 0], [0, 0], [0, 1]), ([0, 0], [0, -1], [0, 1]), ([0, 0], [0, 0], [0, 6]),
           ([0, 0], [0, 0], [-1, 0]), ([0, 0, 0], [0, 0], [0, 1]), ([0, 0], [0], [0, 1, 2]), ([0] * 5, [0] * 5, None)]
    for args in bad:
        with pytest.raises(ValueError):
            place(*args)
    assert not resets and not env.buffers.env_origins.any()
    place([1, 0], torch.tensor([2, 1]), [4, 0])
    assert resets == [[4, 0]] and env.buffers.env_origins[:, 4].tolist() == origins[1, 2].tolist() and env.buffers.env_origins[:, 0].tolist() == origins[0, 1].tolist()
    assert env.terrain_levels.tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and env.terrain_types.tolist() == [1, 0, 0, 0, 2, 0, 0, 0]
    place(1, 0)                                                               # one tile for every training environment
    assert resets[-1] == list(range(6)) and (env.buffers.env_origins[:, :6] == origins[1, 0][:, None]).all() and not env.buffers.env_origins[:, 6:].any()
    place([], [], [])
    assert len(resets) == 2
    env.cfg.terrain.mesh_type = "plane"
    with pytest.raises(ValueError, match="has no tile grid"):
        place(0, 0)


# ---- 6. the sweep's host pieces and the tool -----------------------------------------------------------------------------------------------------
def fixed_result():
    from go1_gym_learn.eval_metrics import terrain
    cells = terrain.terrain_cells(2, 3)
    metric = lambda mean: np.array([[40.0, mean, 0.5, 0.0, 1.0, 0.0]] * 5 + [[0.0, NAN, NAN, NAN, NAN, 0.0]])
    groups = np.array([[8.0, 0.0, 6.0, 2.0, 0.0, 0.75]] * 5 + [[8.0, 8.0, 0.0, 0.0, 0.0, NAN]])
    props = [0.1, 0.1, 0.35, 0.25, 0.2]
    return dict(preset="static_medium", cells=cells, terrain_type=[terrain.terrain_type_name(k, 3, props) for _, k in cells],
                difficulty=[terrain.cell_difficulty(lv, 2) for lv, _ in cells], metrics={m: metric(0.125) for m in T.METRICS},
                outcomes={o: metric(0.25) for o in T.OUTCOMES}, groups=groups, status=np.array([1] * 30 + [2] * 10 + [0] * 8), vx=1.0, num_envs=48,
                window=40, warmup=5, seed=1, num_rows=2, num_cols=3, mesh_type="trimesh", tile=(4.0, 4.0), dt=0.02)


def test_terrain_cells_names_grid_and_json():
    from go1_gym_learn.eval_metrics import terrain
    assert terrain.terrain_cells(2, 3) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)] and terrain.terrain_cells(1, 1) == [(0, 0)]
    props = [0.1, 0.1, 0.35, 0.25, 0.2]                                       # the training configuration's
    names = [terrain.terrain_type_name(k, 20, props) for k in range(20)]
    assert names == ["slope_down", "slope_up", "rough_slope", "rough_slope"] + ["stairs_down"] * 7 + ["stairs_up"] * 5 + ["discrete_obstacles"] * 4
    assert terrain.terrain_type_name(1, 2, [0.25]) == "rough_slope" and terrain.terrain_type_name(0, 2, [0.25]) == "slope_down"   # past the last proportion
    assert [terrain.terrain_type_name(k, 3, [0, 0, 0, 0, 0, 0, 0, 0, 1.0]) for k in range(3)] == ["noise"] * 3         # the training run's flat ground
    assert list(terrain.DEFAULT_PROPORTIONS) == props
    assert [terrain.cell_difficulty(lv, 4, 0.5) for lv in range(4)] == [0.0, 0.125, 0.25, 0.375]
    res = fixed_result()
    md = terrain.terrain_markdown_grid(res).splitlines()
    assert md[0] == "| difficulty | 0: slope_down | 1: stairs_down | 2: stairs_up |" and md[1] == "|---|---|---|---|" and len(md) == 4
    assert md[2] == "| 0.00 | 0.75 / 0.125 / 0.125 / 0.25 | 0.75 / 0.125 / 0.125 / 0.25 | 0.75 / 0.125 / 0.125 / 0.25 |"
    assert md[3] == "| 0.50 | 0.75 / 0.125 / 0.125 / 0.25 | 0.75 / 0.125 / 0.125 / 0.25 | – / – / – / – |"
    js = json.loads(json.dumps(terrain.terrain_to_json(res)))
    assert js["cells"][4] == dict(level=1, type=1, terrain_type="stairs_down", difficulty=0.5) and js["status_counts"] == [8, 30, 10, 0]
    assert js["group_fields"] == T.GROUP_FIELDS and js["groups"][0][5] == 0.75 and js["metrics"]["stumble"][0][1] == 0.125 and js["tile"] == [4.0, 4.0]


def test_tool_accepts_a_terrain_sweep(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import terrain
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--terrain", "--rows", "2", "--cols", "3", "--vx", "0.8", "--window", "40", "--envs", "48", "--presets", "static_medium"])
    assert a.tiles and (a.rows, a.cols, a.vx, a.window, a.mesh, a.terrain) == (2, 3, [0.8], 40, "trimesh", None)
    d = eval_sweep.parse_args(base + ["--terrain"])
    assert d.tiles and (d.rows, d.cols, d.vx, d.window) == (4, 5, [1.0], 500)
    plain = eval_sweep.parse_args(base + ["--terrain", "heightfield"])                      # the older meaning of the option is kept
    assert not plain.tiles and plain.terrain == "heightfield" and plain.vx == [0.5, 1.0, 1.5] and plain.rows is None
    assert not eval_sweep.parse_args(base).tiles and eval_sweep.parse_args(base).terrain is None
    for bad in (["--rows", "2"], ["--window", "40"], ["--terrain", "plane", "--cols", "3"], ["--terrain", "--vx", "0.5", "1.0"], ["--terrain", "--rows", "0"],
                ["--terrain", "--behaviour"], ["--terrain", "--push", "--magnitude", "1", "--direction", "0"], ["--terrain", "--mesh", "plane"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(base + bad)
    seen = {}

    def sweep_stub(policy, preset, **kw):
        seen.update(kw, preset=preset)
        return fixed_result()
    monkeypatch.setattr(terrain, "run_terrain_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    eval_sweep.run_terrain(a, None)
    assert seen == dict(preset="static_medium", vx=0.8, num_envs=48, window=40, warmup=25, seed=1, num_rows=2, num_cols=3, mesh_type="trimesh",
                        terrain_proportions=None)
    js = json.load(open(tmp_path / "eval" / "static_medium_terrain.json"))
    assert js["cells"][5]["terrain_type"] == "stairs_up" and js["status_counts"] == [8, 30, 10, 0]
    md = (tmp_path / "eval" / "static_medium_terrain.md").read_text()
    assert "| 0.50 | 0.75 / 0.125 / 0.125 / 0.25 | 0.75 / 0.125 / 0.125 / 0.25 | – / – / – / – |" in md and md in capsys.readouterr().out + "\n"
