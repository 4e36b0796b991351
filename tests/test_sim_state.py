"""Save, restore and branch of the simulator's state (include/go1state.h, go1state_host.py, LeggedRobot.save_state / load_state, the paired
push sweep), without a GPU: go1state.hip runs under the SIMT emulator (util.build_emu) against the numpy model of tests/state_ref.py, and the
environment's hooks run on CPU buffers stepped by the emulated simulator.  Every comparison is bit for bit.  The helpers here carry the
GPU tests of tests/test_gpu_sim_state.py as well: the same scripts on the compiled kernels."""
import ctypes
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import go1sim_abi as abi  # noqa: E402
import go1sim_host as H  # noqa: E402
import state_ref as R  # noqa: E402
from util import build_emu, make_sim  # noqa: E402


def G():
    import go1state_host
    return go1state_host


@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    return G().load_library(build_emu(g.state_sources(), "libgo1state_emu.so"))


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------
_BASE = {}


def base_sim():
    if not _BASE:
        _, S, meta, _ = make_sim("train", 16)
        _BASE.update(S=S, meta=meta)
    return _BASE["S"], _BASE["meta"]


def scripted_buffers(N, num_obs, lag, hist, device="cpu", salt=0, signature=True):
    """a SimBuffers of the train configuration with the four sizes replaced, the terrain and (signature) the contact record allocated, every word
    and byte a hash of where it is (state_ref.scripted)"""
    S0, meta = base_sim()
    S = abi.Go1SimConfig()
    ctypes.memmove(ctypes.byref(S), ctypes.byref(S0), ctypes.sizeof(S))
    S.num_envs, S.num_obs, S.lag_timesteps, S.num_obs_history = N, num_obs, lag, hist
    B = H.SimBuffers(S, meta, "cpu")
    B.tensors["height_samples"] = torch.zeros(5, 7, dtype=torch.int16)
    if signature:
        B.enable_contact_signature()
    R.scripted({k: t.numpy() for k, t in B.tensors.items() if t is not None}, salt)
    if torch.device(device).type != "cpu":
        B = B.clone_to(device)
    B.refresh_struct()
    return S, B


def host_copy(B):
    return {k: t.detach().cpu().numpy().copy() for k, t in B.tensors.items() if t is not None}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(a, b, skip=()):
    """the names whose bits differ between two host copies"""
    assert set(a) == set(b)
    return sorted(k for k in a if k not in skip and not same(a[k], b[k]))


def model_of(S):
    return R.Model(abi.BUFFER_FIELDS, G().PER_ENV, G().GLOBAL, S.num_obs, S.num_obs_history, S.lag_timesteps)


class Phase:
    """stands in for the simulator's handle: the counters a Go1State asks for"""

    def __init__(self, S, lag_head=0, hslot=0, counter=0):
        self.S, self.lag_head, self.hslot, self.counter = S, lag_head, hslot, counter

    def counters(self):
        return self.counter, self.lag_head

    def history_window_offset(self):
        return ((self.hslot + 1) % (self.S.num_obs_history + 1)) * self.S.num_obs


def stater(S, B, lib, lag_head=0, hslot=0):
    return G().Go1State(S, B, Phase(S, lag_head, hslot), lib=lib)


def snap_of(state):
    return dict(words=state.words.cpu().numpy().view(np.uint32), bytes=state.bytes.cpu().numpy(), rows=state.rows.cpu().numpy().view(np.uint32))


def check_scripted(N, num_obs, lag, hist, lib, device="cpu"):
    """the three cases of the scripted buffers, bit for bit against the model"""
    rng = np.random.default_rng(1000 * N + 100 * num_obs + 10 * lag + hist)
    S, B = scripted_buffers(N, num_obs, lag, hist, device, salt=1)
    M = model_of(S)
    src = host_copy(B)
    lag_n, Rr = lag + 1, hist + 1
    head, slot = int(rng.integers(lag_n)), int(rng.integers(Rr))
    st = stater(S, B, lib, head, slot)
    W, Bt, RW, Gw = M.sizes(src, N)
    L = st.layout
    assert (L["word_rows"], L["byte_rows"], L["row_words"], L["global_words"]) == (W, Bt, RW, Gw) and L["bytes_per_env"] == 4 * (W + RW) + Bt

    # 1. all environments, and the global section
    whole = st.capture(None)
    want = M.capture(src, None, head, slot)
    got = snap_of(whole)
    assert whole.whole and whole.num_rows == N and whole.env_ids is None
    for k in ("words", "bytes", "rows"):
        assert same(got[k], want[k]), k
    assert same(whole.glob.cpu().numpy().view(np.uint32), M.capture_global(src))
    # 2. an unsorted odd subset (with a repeat where there is room: a capture may name an environment twice)
    K = max(1, (N // 2) | 1) if N > 1 else 1
    ids = rng.permutation(N)[:K]
    if K >= 3:
        ids[-1] = ids[0]
    part = st.capture(ids)
    want_part = M.capture(src, ids, head, slot)
    got_part = snap_of(part)
    assert not part.whole and part.glob is None and part.num_rows == K and part.env_ids.cpu().tolist() == ids.tolist()
    for k in ("words", "bytes", "rows"):
        assert same(got_part[k], want_part[k]), k
    assert differing(host_copy(B), src) == [] and int(st.skipped.cpu()) == 0          # a capture writes no simulator buffer

    # 3. restores at other ring positions into other buffers: identity, a permutation, one row to all, rows into an odd subset
    head2, slot2 = (head + 1 + int(rng.integers(max(lag_n - 1, 1)))) % lag_n, (slot + 1 + int(rng.integers(max(Rr - 1, 1)))) % Rr
    assert (lag_n == 1 or head2 != head) and slot2 != slot
    perm = rng.permutation(N)
    odd = rng.permutation(N)[:K]
    cases = [("identity", whole, None, None), ("permutation", whole, None, perm), ("fan-out", whole, None, np.full(N, N // 2)),
             ("subset", whole, odd, rng.integers(0, N, K)), ("from a subset", part, odd, rng.integers(0, K, K))]
    for salt, (name, state, dst, rows) in enumerate(cases, 2):
        S2, B2 = scripted_buffers(N, num_obs, lag, hist, device, salt=salt)
        before = host_copy(B2)
        st2 = stater(S2, B2, lib, head2, slot2)
        st2.restore(state, dst, rows)
        want2 = {k: v.copy() for k, v in before.items()}
        snap = want if state is whole else want_part
        assert M.restore(want2, snap, dst, rows, head2, slot2) == 0
        after = host_copy(B2)
        assert differing(after, want2) == [], (name, differing(after, want2))
        # what was no destination is unchanged: the global and static tensors, the contact record, and every other environment
        for k in list(G().GLOBAL) + list(G().STATIC):
            assert same(after[k], before[k]), (name, k)
        if dst is not None:
            rest = np.setdiff1d(np.arange(N), dst)
            for k, kind in G().PER_ENV.items():
                a, b = (after[k], before[k]) if kind in ("rows", "history") else (after[k].reshape(-1, N).T, before[k].reshape(-1, N).T)
                assert same(a[rest], b[rest]), (name, k)
        else:
            changed = differing(after, before)
            assert set(changed) <= set(G().PER_ENV) and len(changed) > 40, name
        st2.restore(whole, None, None, restore_global=True)
        M.restore(want2, want, None, None, head2, slot2)
        M.restore_global(want2, M.capture_global(src))
        assert differing(host_copy(B2), want2) == [], name


# ---- 1. the classification ---------------------------------------------------------------------------------------------------------------------
def test_classification_is_total(emu):
    g = G()
    S, B = scripted_buffers(16, 70, 6, 30)
    names = set(B.tensors)
    assert names == set(H._buffer_specs(S)) | {"curriculum_nbr_ptr", "curriculum_nbr_idx", "height_samples", "contact_signature"}
    classes = [set(g.PER_ENV), set(g.GLOBAL), set(g.STATIC)]
    assert set.union(*classes) == names and sum(len(c) for c in classes) == len(names)          # each in exactly one
    assert set(g.STATIC) == {"curriculum_nbr_ptr", "curriculum_nbr_idx", "height_samples", "contact_signature"}
    assert names == set(abi.BUFFER_FIELDS)
    for out in ("obs_buf", "rew_buf", "reset_buf", "measured_heights", "privileged_obs_buf", "time_out_buf"):
        assert out in g.PER_ENV
    N = 16
    specs = H._buffer_specs(S)
    words = 0
    for name, kind in g.PER_ENV.items():
        _, shape = specs[name]
        if kind in ("words", "lag"):
            assert shape[-1] == N
            words += int(np.prod(shape)) // N                   # (the lag ring: all lag + 1 slots)
        elif kind == "rows":
            assert shape[0] == N
            words += shape[1]
        elif kind == "history":
            words += (S.num_obs_history + 1) * S.num_obs        # its logical size: every slot once
    L = g.layout_of(g.state_config(S), emu)
    nbytes = sum(int(np.prod(specs[n][1])) // N for n, k in g.PER_ENV.items() if k == "bytes")
    assert L["word_rows"] + L["row_words"] == words and L["byte_rows"] == nbytes == 7
    assert L["global_words"] == sum(int(np.prod(specs[n][1])) for n in g.GLOBAL)
    assert L["header"].tolist()[:2] == [0x53314F47, 1] and L["header"].tolist()[2:] == [70, S.num_privileged_obs, 30, 6, S.num_rewards, S.num_height_x * S.num_height_y,
                                                                                       abi.GO1_MAX_COMMANDS, S.num_categories, S.num_bins, max(S.curriculum_update_interval, 1)]
    print(f"\npacked state of the train configuration: {L['bytes_per_env']} bytes per environment ({L['word_rows']} SoA words, {L['byte_rows']} bytes, "
          f"{L['row_words']} row words), {4 * L['global_words']} bytes global")


def test_mirrors_match_the_header():
    import re
    g = G()
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "go1state.h")).read()
    for cls in (g.Go1StateConfig, g.Go1StateLayout, g.Go1StateSnapshot):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cls.__name__, cls.__name__), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.sub(r"[\*\s]|\[.*?\]", "", v) for decl in body.split(";") if decl.strip() for v in decl.strip().split(" ", 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], cls.__name__
    assert int(re.search(r"#define GO1STATE_HEADER_WORDS (\d+)", text).group(1)) == g.HEADER_WORDS == len(g.HEADER_NAMES)
    declared = re.findall(r"^(?:int|const char\*) (go1state_\w+)\(", text, re.M)
    assert declared == g.EXPORTED_SYMBOLS


def test_sources_flags_and_stamp():
    import inspect
    import __graft_entry__ as g
    assert [os.path.basename(p) for p in g.state_sources()] == ["go1state.hip", "go1state.h", "go1sim.h"]
    assert g.STATE_FLAGS[0] == "--offload-arch=gfx950" and "-shared" in g.STATE_FLAGS
    out = g.build_state_hip()
    assert os.path.basename(out) == "libgo1state.so" and g.library_stamp(out) == g.source_hash(g.state_sources(), g.STATE_FLAGS)
    assert "build_state_hip()" in inspect.getsource(g.build) and "libgo1state.so" in inspect.getsource(g.smoke)
    import subprocess
    symbols = subprocess.run(["nm", "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in symbols.splitlines() if " T " in line and "go1state_" in line and not line.split()[-1].startswith("_Z"))
    assert exported == sorted(G().EXPORTED_SYMBOLS)
    text = open(g.state_sources()[0]).read()
    assert "asm" not in text and "__shared__" not in text and text.count("atomicAdd") == 1      # no inline assembly, no LDS, one atomic: the skip count


def test_a_missing_library_fails_loudly(tmp_path):
    g = G()
    with pytest.raises(g.Go1StateLibraryMissing, match="no CPU fallback"):
        g.load_library(str(tmp_path / "libgo1state.so"))


# ---- 2. the scripted buffers ---------------------------------------------------------------------------------------------------------------------
CONFIGS = list(itertools.product([1, 16, 40, 257], [7, 70], [0, 6], [1, 30]))


@pytest.mark.parametrize("N,num_obs,lag,hist", CONFIGS)
def test_emulated_kernels_follow_the_model(emu, N, num_obs, lag, hist):
    check_scripted(N, num_obs, lag, hist, emu)


# ---- 3. the C functions' refusals ------------------------------------------------------------------------------------------------------------------
def test_return_codes_and_skipped_entries(emu):
    """every code of include/go1state.h but -20, which only a failed launch gives (the emulator's launches do not fail)"""
    g = G()
    N = 40
    S, B = scripted_buffers(N, 70, 6, 30, salt=1)
    st = stater(S, B, emu, 2, 5)
    state = st.capture(None)
    cfg, snap, buf = st.cfg, st._snapshot(state), B.struct
    st.restore(state)                                               # (the scripted history's two copies differ: from here on they agree)
    before = host_copy(B)
    ids = torch.arange(N, dtype=torch.int32)
    idp = ctypes.c_void_p(ids.data_ptr())
    c, b, s = ctypes.byref(cfg), ctypes.byref(buf), ctypes.byref(snap)

    def capture(c=c, b=b, ids=None, K=N, head=2, slot=5, s=s):
        return emu.go1state_capture(c, b, ids, K, head, slot, s, None)

    def restore(c=c, b=b, dst=None, rows=None, K=N, head=2, slot=5, s=s):
        return emu.go1state_restore(c, b, dst, rows, K, head, slot, s, None)

    def edited(obj, **kw):
        copy = type(obj)()
        ctypes.memmove(ctypes.byref(copy), ctypes.byref(obj), ctypes.sizeof(obj))
        for k, v in kw.items():
            setattr(copy, k, v)
        return ctypes.byref(copy)

    for call in (capture, restore):
        assert call() == 0
        assert call(c=None) == -1 and call(b=None) == -1 and call(c=edited(cfg, num_envs=0)) == -1 and call(K=0) == -1
        assert call(s=None) == -2 and call(s=edited(snap, words=None)) == -2 and call(s=edited(snap, bytes=None)) == -2
        assert call(s=edited(snap, rows=None)) == -2 and call(s=edited(snap, skipped=None)) == -2
        assert call(b=edited(buf, dof_pos=None)) == -3 and call(b=edited(buf, obs_history=None)) == -3 and call(b=edited(buf, reset_buf=None)) == -3
        assert call(b=edited(buf, measured_heights=None, episode_sums_eval=None)) == 0            # the two optional ones
        assert call(K=N - 1) == -8
        assert call(head=7) == -12 and call(head=-1) == -12 and call(slot=31) == -12 and call(slot=-1) == -12
        assert call(c=edited(cfg, num_obs=0)) == -12 and call(c=edited(cfg, lag_timesteps=abi.GO1_MAX_LAG)) == -12
        # the order of the codes
        assert call(c=edited(cfg, num_envs=0), s=None) == -1 and call(s=None, b=edited(buf, dof_pos=None)) == -2
        assert call(b=edited(buf, dof_pos=None), K=N - 1) == -3 and call(K=N - 1, head=7) == -8
    assert capture(ids=idp, K=5) == 0 and restore(dst=idp, K=5) == 0
    assert restore(dst=idp, K=N + 1) == -12                         # identity rows beyond the snapshot's
    assert emu.go1state_layout(None, None) == -1 and emu.go1state_layout(edited(cfg, num_bins=0), ctypes.byref(g.Go1StateLayout())) == -12
    assert emu.go1state_capture_global(c, b, edited(snap, **{"global": None}), None) == -2 and emu.go1state_capture_global(None, b, s, None) == -1
    assert emu.go1state_restore_global(c, edited(buf, episode_log=None), s, None) == -3
    assert emu.go1state_restore_global(c, edited(buf, contact_drop_counts=None), s, None) == 0
    assert differing(host_copy(B), before) == []                    # (every restore above put back what was there)

    # another layout: refused, and nothing is written
    S2, B2 = scripted_buffers(N, 70, 6, 29, salt=2)
    st2 = stater(S2, B2, emu, 0, 0)
    before2 = host_copy(B2)
    snap2 = st2._snapshot(state)
    assert emu.go1state_restore(ctypes.byref(st2.cfg), ctypes.byref(B2.struct), None, None, N, 0, 0, ctypes.byref(snap2), None) == -12
    assert emu.go1state_restore_global(ctypes.byref(st2.cfg), ctypes.byref(B2.struct), ctypes.byref(snap2), None) == -12
    assert differing(host_copy(B2), before2) == []
    with pytest.raises(RuntimeError, match="another layout"):
        st2.restore(state)

    # ids and rows out of range: skipped, counted, never written through; the rest is handled
    M = model_of(S)
    S3, B3 = scripted_buffers(N, 70, 6, 30, salt=3)
    st3 = stater(S3, B3, emu, 1, 9)
    bad_ids = torch.tensor([3, -1, N, 17, N + 5, 0, 2 ** 30, 39], dtype=torch.int32)
    part = g.SimState(st3.layout, 8, bad_ids, 0, False, torch.zeros(st3.layout["word_rows"], 8, dtype=torch.int32),
                      torch.zeros(st3.layout["byte_rows"], 8, dtype=torch.uint8), torch.zeros(st3.layout["row_words"] * 8, dtype=torch.int32))
    snap3 = st3._snapshot(part)
    assert emu.go1state_capture(ctypes.byref(st3.cfg), ctypes.byref(B3.struct), ctypes.c_void_p(bad_ids.data_ptr()), 8, 1, 9, ctypes.byref(snap3), None) == 0
    src3 = host_copy(B3)
    want = M.capture(src3, bad_ids.numpy(), 1, 9)
    assert want["skipped"] == 4 and int(st3.skipped) == 4
    for k, v in snap_of(part).items():
        assert same(v, want[k]), k
    dst = torch.tensor([5, N, 6, -3, 7, 8, 9], dtype=torch.int32)
    rows = torch.tensor([0, 0, 8, 3, -1, 5, 7], dtype=torch.int32)          # rows 1, 2, 4, 6 of the snapshot were never captured: zeros
    st3.skipped.zero_()
    part.num_rows = 8
    snap3 = st3._snapshot(part)
    assert emu.go1state_restore(ctypes.byref(st3.cfg), ctypes.byref(B3.struct), ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(rows.data_ptr()), 7, 4, 20,
                                ctypes.byref(snap3), None) == 0
    assert M.restore(src3, want, dst.numpy(), rows.numpy(), 4, 20) == 4 and int(st3.skipped) == 4
    assert differing(host_copy(B3), src3) == []


def test_host_checks_of_ids(emu):
    S, B = scripted_buffers(16, 7, 0, 1)
    st = stater(S, B, emu)
    state = st.capture([3, 1, 2])
    for bad, kw in (("named twice", dict(env_ids=[1, 1, 2])), ("lie in", dict(env_ids=[1, 16, 2])), ("lie in", dict(env_ids=[0, 1, 2], rows=[0, 1, 3])),
                    ("rows for", dict(env_ids=[0, 1], rows=[0, 1, 2])), ("name the rows", dict()), ("no entries", dict(env_ids=[])),
                    ("no global section", dict(env_ids=[0, 1, 2], restore_global=True))):
        with pytest.raises((ValueError, RuntimeError), match=bad):
            st.restore(state, **kw)
    with pytest.raises(ValueError, match="lie in"):
        st.capture([-1])


# ---- the environment on CPU buffers, stepped by the emulated simulator -----------------------------------------------------------------------------
def make_env(num_envs, device_str="cuda:0", configure=None, seed=0):
    """a HistoryWrapper environment of the train configuration: noise, randomisation and the training pushes on"""
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from go1_gym.envs.wrappers.history_wrapper import HistoryWrapper
    from scripts.train_config import apply_train_config
    c = apply_train_config(make_cfg(), num_envs=num_envs)
    c.terrain.mesh_type = "plane"
    c.noise.add_noise = True
    c.domain_rand.push_robots = True
    c.seed = seed
    if configure is not None:
        configure(c)
    torch.manual_seed(seed)
    np.random.seed(seed)
    return HistoryWrapper(VelocityTrackingEasyEnv(sim_device=device_str, headless=True, cfg=c))


def emulated(monkeypatch, emu):
    """make_env() builds its environment on CPU buffers stepped by the emulated simulator; inject(env) gives it the emulated state library"""
    import emu_sim
    import fake_sim
    fake_sim.install(monkeypatch)
    monkeypatch.setattr(H, "Go1Sim", emu_sim.EmuSim)

    def inject(env):
        base = env.env
        base._state = G().Go1State(base.sim_config, base.buffers, base.sim, lib=emu)
        return env
    return inject


def window(env):
    return env.obs_history.detach().cpu().numpy().copy()


def logical_copy(base):
    """host_copy() of an environment's buffers with the two rings read in logical order (the lag ring from its head, both copies of the history
    from the oldest slot, the spare last): what does not depend on where the rings stand"""
    S, c = base.sim_config, host_copy(base.buffers)
    M = model_of(S)
    _, head = base.sim.counters()
    slot = (base.sim.history_window_offset() // S.num_obs - 1) % (S.num_obs_history + 1)
    N = c["lag_buffer"].shape[-1]
    c["lag_buffer"] = c["lag_buffer"].reshape(-1, N)[M._lag_rows(head)]
    cols = M._hist_cols(slot)
    c["obs_history"] = np.concatenate([c["obs_history"][:, cols], c["obs_history"][:, cols + M.R * M.no]], axis=1)
    return c


def force_events(env, within=3):
    """write episode_length_buf so that on step `within` after now environment 3 times out, environment 7 resamples its commands and environment 11
    is pushed by the training push; returns {event: (environment, step index)}"""
    base = env.env
    S = base.sim_config
    assert S.push_robots and S.add_noise and base.num_envs >= 12
    L = base.buffers.episode_length_buf
    L[3] = S.max_episode_length - (within - 1)                       # ep_len = len + 1 > max_episode_length at that step
    L[7] = S.resample_interval - within                              # (len + 1) % resample_interval == 0 there
    L[11] = S.push_interval - within
    assert S.push_interval - within != S.resample_interval - within and S.push_interval < S.max_episode_length
    return dict(timeout=3, resample=7, push=11)


def scripted_actions(M, N, device, seed=0):
    return [torch.from_numpy((0.3 * np.random.default_rng(seed + i).standard_normal((N, 12))).astype(np.float32)).to(device) for i in range(M)]


def replay(env, M, within=3, seed=5):
    """the forced-event protocol: save, M scripted steps, load, the same M steps; bit-identical after the load and after every step in every
    tensor but episode_log, and in the history window.  Asserts that the three events happened inside the window."""
    base = env.env
    B, S = base.buffers, base.sim_config
    who = force_events(env, within)
    state = base.save_state()
    at_save, win_save, counter = logical_copy(base), window(env), base.common_step_counter
    acts = scripted_actions(M, base.num_envs, base.device, seed)
    first = []
    for a in acts:
        lens = B.episode_length_buf.cpu().numpy().copy()
        env.step(a)
        first.append((logical_copy(base), window(env), lens))
    # the events, from the buffers
    step = within - 1
    after, _, lens = first[step]
    prev = first[step - 1][0] if step > 0 else at_save
    e = who["timeout"]
    assert lens[e] + 1 > S.max_episode_length and after["time_out_buf"][e] == 1 and after["reset_buf"][e] == 1 and after["episode_length_buf"][e] == 0
    assert sum(int(f[0]["time_out_buf"][e]) for f in first) == 1
    e = who["resample"]
    assert (lens[e] + 1) % S.resample_interval == 0 and not after["reset_buf"][e] and not same(after["commands"][:, e], prev["commands"][:, e])
    assert same(first[step - 1][0]["commands"][:, e], at_save["commands"][:, e]) or step == 0
    e = who["push"]
    v = after["root_states"][7:9, e]
    assert (lens[e] + 1) % S.push_interval == 0 and not after["reset_buf"][e] and (np.abs(v) <= S.max_push_vel_xy).all() and (v != 0).all()
    assert base.common_step_counter == counter + M and base.sim.counters()[0] == state.counter + M

    base.load_state(state)
    assert base.common_step_counter == counter and base.sim.counters()[0] == state.counter
    assert differing(logical_copy(base), at_save) == [] and same(window(env), win_save)          # (episode_log too: nothing has stepped)
    for i, a in enumerate(acts):
        env.step(a)
        assert differing(logical_copy(base), first[i][0], skip=("episode_log",)) == [], i
        assert same(window(env), first[i][1]), i
    return state, first


def test_replay_through_the_emulated_simulator(monkeypatch, emu):
    inject = emulated(monkeypatch, emu)
    env = inject(make_env(16))
    env.reset()
    replay(env, 6)


# ---- 5. the host surface ---------------------------------------------------------------------------------------------------------------------------
def check_host_surface(env, tmp_path):
    g = G()
    base = env.env
    state = base.save_state()
    part = base.save_state([5, 2, 9])
    for s in (state, part):
        path = str(tmp_path / "state.npz")
        s.cpu().save(path)
        back = g.SimState.load(path)
        assert back.device.type == "cpu"
        back = back.to(base.device)
        assert back.device == s.device and back.num_rows == s.num_rows and back.counter == s.counter and back.whole == s.whole
        assert same(back.layout["header"], s.layout["header"]) and {k: v for k, v in back.layout.items() if k != "header"} == {k: v for k, v in s.layout.items() if k != "header"}
        assert (back.env_ids is None) == (s.env_ids is None) and (s.env_ids is None or back.env_ids.tolist() == s.env_ids.tolist())
        for k in g.SimState.SECTIONS:
            a, b = getattr(back, k), getattr(s, k)
            assert (a is None) == (b is None) and (a is None or (a.dtype == b.dtype and same(a.cpu().numpy(), b.cpu().numpy()))), k
    with np.load(str(tmp_path / "state.npz"), allow_pickle=False) as d:
        assert {"header", "sizes", "num_rows", "counter", "whole", "words", "bytes", "rows", "env_ids"} == set(d.files)
    before = host_copy(base.buffers)
    base.load_state(back, env_ids=[5, 2, 9])                              # the file's copy goes back where it came from: nothing changes
    assert differing(host_copy(base.buffers), before) == []
    # refusals
    base._trunk = types.SimpleNamespace(armed=True)
    base._trace = types.SimpleNamespace(armed=True)
    with pytest.raises(RuntimeError, match=r"load_state\(\): refused while trace, trunk are armed"):
        base.load_state(state)
    base._trace = None
    with pytest.raises(RuntimeError, match="refused while trunk is armed"):
        base.load_state(state)
    base._trunk = types.SimpleNamespace(armed=False)
    base.load_state(state)
    base._trunk = None
    with pytest.raises(ValueError, match="named twice"):
        base.load_state(part, env_ids=[1, 2, 1])
    foreign = g.SimState(dict(state.layout, header=state.layout["header"].copy()), state.num_rows, None, 0, True, state.words, state.bytes, state.rows, state.glob)
    foreign.layout["header"][4] += 1
    with pytest.raises(RuntimeError, match="another layout"):
        base.load_state(foreign)
    assert differing(host_copy(base.buffers), before) == []
    # the defaults of restore_clock
    count = base.common_step_counter
    env.step(torch.zeros(base.num_envs, 12, device=base.device))
    base.load_state(state, env_ids=list(range(base.num_envs)))            # ids given: a branch, the clock stays
    assert base.common_step_counter == count + 1 and base.sim.counters()[0] == state.counter + 1
    base.load_state(state)
    assert base.common_step_counter == count and base.sim.counters()[0] == state.counter
    base.load_state(state, restore_clock=False)
    with pytest.raises(RuntimeError, match="no global section"):
        base.load_state(part, env_ids=[0, 1, 2], restore_clock=True)


def test_host_surface(monkeypatch, emu, tmp_path):
    inject = emulated(monkeypatch, emu)
    module = G()
    monkeypatch.delitem(sys.modules, "go1state_host", raising=False)
    env = make_env(16)
    env.reset()
    env.step(torch.zeros(16, 12))
    for call in (env.env.save_state, lambda: env.env.load_state(None)):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert env.env._state is None and "go1state_host" not in sys.modules          # never saved: nothing imported
    monkeypatch.setitem(sys.modules, "go1state_host", module)                      # (the one the emulated library is bound to)
    import inspect
    assert list(inspect.signature(env.env.load_state).parameters) == ["state", "env_ids", "rows", "restore_clock"]
    assert list(inspect.signature(env.env.save_state).parameters) == ["env_ids"]
    check_host_surface(inject(env), tmp_path)


# ---- 6. the paired push sweep -------------------------------------------------------------------------------------------------------------------------
class StandStill:
    """zero actions: the robot holds its default pose"""

    def act_inference(self, obs):
        return torch.zeros(obs["obs"].shape[0], 12, device=obs["obs"].device)


PAIRED_KEYS = {"source", "paired_excess"}


def check_paired_result(res, N, cells):
    sources = N // cells
    src = res["source"]
    assert src.shape == (N,) and src[:sources * cells].tolist() == (np.arange(sources * cells) // cells).tolist() and (src[sources * cells:] == -1).all()
    ex = res["paired_excess"]
    assert ex.shape == (cells, 3)
    control = [g for g, (m, _) in enumerate(res["cells"]) if m == 0.0][0]
    both = (res["status"][:sources * cells].reshape(sources, cells) == 0)
    assert ex[control, 2] == both[:, control].sum() and (ex[control, 2] == 0 or (ex[control, 0] == 0.0 and ex[control, 1] == 0.0))
    for gi in range(cells):
        assert ex[gi, 2] == (both[:, gi] & both[:, control]).sum()
    assert res["groups"][:, 0].sum() == sources * cells                              # the remainder is in no group


def test_paired_push_sweep_on_the_emulator(monkeypatch, emu):
    import __graft_entry__ as ge
    import go1eval_host
    from go1_gym.envs.base.legged_robot import LeggedRobot
    from go1_gym_learn.eval_metrics import recovery
    inject = emulated(monkeypatch, emu)
    monkeypatch.setattr(go1eval_host, "_lib", go1eval_host.load_library(build_emu(ge.eval_sources(), "libgo1eval_emu.so")))
    monkeypatch.setattr(go1eval_host._Host, "_stream", lambda self: None)
    monkeypatch.setattr(LeggedRobot, "_need_gpu_metrics", lambda self, what: None)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)                   # (sweep.build_eval_env names the device by it)
    seen = {}
    real_load = LeggedRobot.load_state

    def first_use(self, what):                       # the environment is built inside run_push_sweep: hand it the emulated library there
        if self._state is None:
            self._state = G().Go1State(self.sim_config, self.buffers, self.sim, lib=emu)
        return self._state

    def load_and_look(self, state, env_ids=None, rows=None, restore_clock=None):
        real_load(self, state, env_ids, rows, restore_clock)
        seen.update(after=host_copy(self.buffers), rows=np.asarray(rows), counter=self.common_step_counter)
    monkeypatch.setattr(LeggedRobot, "_stater", first_use)
    monkeypatch.setattr(LeggedRobot, "load_state", load_and_look)
    N, kw = 70, dict(num_envs=70, settle_steps=4, pre=8, window=12, smooth=5, band=0.1, hold=5, seed=5, terrain="plane")
    res = recovery.run_push_sweep(StandStill(), "static_medium", (0, 1.0), (0, 90), paired=True, **kw)
    check_paired_result(res, N, 4)
    # immediately after the load the environments of one source hold identical bits in every per-environment tensor
    after = seen["after"]
    assert seen["rows"].tolist() == (np.arange(68) // 4).tolist()
    for k, kind in G().PER_ENV.items():
        a = after[k] if kind in ("rows", "history") else after[k].reshape(-1, N).T
        for s in range(17):
            assert all(same(a[4 * s], a[4 * s + j]) for j in range(1, 4)), (k, s)
    text = recovery.recovery_markdown_table(res)
    assert "paired excess peak error [m/s]" in text.splitlines()[0] and len(text.splitlines()) == 2 + 4
    js = recovery.recovery_to_json(res)
    assert js["paired"] and len(js["paired_excess"]) == 4 and js["paired_excess_fields"] == ["mean", "std", "count"] and len(js["source"]) == N
    monkeypatch.setattr(LeggedRobot, "load_state", real_load)
    plain = recovery.run_push_sweep(StandStill(), "static_medium", (0, 1.0), (0, 90), **kw)
    assert set(plain) == set(res) - PAIRED_KEYS == {"preset", "cells", "recovery", "groups", "values", "status", "num_envs", "settle_steps", "pre", "window",
                                                    "smooth", "band", "hold", "dt", "seed"}
    assert "paired" not in recovery.recovery_markdown_table(plain) and set(recovery.recovery_to_json(plain)) == set(js) - {"paired", "source", "paired_excess",
                                                                                                                         "paired_excess_fields"}


def test_paired_excess_and_the_tool(tmp_path, monkeypatch, capsys):
    from go1_gym_learn.eval_metrics import recovery
    cells = recovery.push_cells((0, 1.0), (0, 90))
    source = np.array([0] * 4 + [1] * 4 + [2] * 4 + [-1])
    peak = np.array([1, 1, 3, 4, 2, 2, 5, 9, 1, 7, 7, 7, 0], np.float32)
    status = np.array([0, 0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0])
    ex = recovery.paired_excess(cells, source, peak, status)
    assert ex[0].tolist() == [0.0, 0.0, 2.0] and ex[1].tolist() == [0.0, 0.0, 2.0] and ex[2].tolist() == [2.5, 0.5, 2.0] and ex[3].tolist() == [3.0, 0.0, 1.0]
    assert recovery.paired_excess(recovery.push_cells((0.5, 1.0), (0,)), source, peak, status) is None
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
    import eval_sweep
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--push", "--paired", "--magnitude", "0", "1", "--direction", "0"])
    assert a.paired and not eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--push", "--magnitude", "0", "1", "--direction", "0"]).paired
    with pytest.raises(SystemExit):
        eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--paired"])
    seen = []
    metric = np.array([[8.0, 0.25, 0.5, 0.0, 1.0, 0.0]] * 2)

    def sweep_stub(policy, preset, magnitudes, directions, **kw):
        seen.append(kw)
        out = dict(preset=preset, cells=recovery.push_cells(magnitudes, directions), recovery={m: metric for m in ("peak_vel_err", "recovery_time", "recovered")},
                   groups=np.array([[8.0, 8.0, 0.0, 0.0, 0.0]] * 2), status=np.zeros(16, np.int32), values={}, num_envs=16, settle_steps=100,
                   pre=25, window=150, smooth=17, band=0.1, hold=10, dt=0.02, seed=1)
        if kw.get("paired"):
            out.update(source=np.arange(16) // 2, paired_excess=np.array([[0.0, 0.0, 8.0], [0.5, 0.125, 8.0]]))
        return out
    monkeypatch.setattr(recovery, "run_push_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    common = ["--checkpoint", "c", "--out", str(tmp_path), "--presets", "static_medium", "--push", "--magnitude", "0", "1", "--direction", "90", "--envs", "16"]
    eval_sweep.run_push(eval_sweep.parse_args(common), None)
    assert "paired" not in seen[0] and "paired" not in capsys.readouterr().out             # the default path hands over what it handed over
    eval_sweep.run_push(eval_sweep.parse_args(common + ["--paired"]), None)
    assert seen[1]["paired"] is True and "| 0.5 ± 0.12 (8) |" in capsys.readouterr().out
    import json
    js = json.load(open(tmp_path / "eval" / "static_medium_push.json"))
    assert js["paired_excess"] == [[0.0, 0.0, 8.0], [0.5, 0.125, 8.0]]
