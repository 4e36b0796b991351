"""CPU checks of the renderer of recorded episodes: the library's C-ABI surface and stamp (include/go1render.h,
walk-these-ways_amd/csrc/go1render.hip), the fp64 reference renderer of tests/render_ref.py anchored to the physics and to
hand-computed camera cases, the no-op recording surface where the simulator's buffers are not on a GPU, and the animated-PNG
writer behind `logger.save_video`."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import render_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(REPO, "include", "go1render.h")


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(go1render_\w+)\s*\(", src)))


def exported_symbols(path):
    """defined dynamic symbols of a shared library (binutils or the ROCm LLVM nm)"""
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_render_library_exports_what_the_header_declares_with_the_source_stamp():
    import __graft_entry__ as g
    import go1render_host
    path = g.build_render_hip()
    assert path == go1render_host.LIB_PATH
    assert declared_functions() == sorted(go1render_host.EXPORTED_SYMBOLS)
    assert sorted(s for s in exported_symbols(path) if s.startswith("go1render")) == declared_functions()
    want = g.source_hash(g.render_sources(), g.RENDER_FLAGS)
    assert g.library_stamp(path) == want
    lib = go1render_host.load_library()
    v = lib.go1render_version()
    assert b"gfx950" in v and (g.STAMP + want.encode()) in v
    # argument validation happens before any launch: callable without a GPU
    cfg, buf = go1render_host.Go1RenderConfig(), go1render_host.Go1RenderBuffers()
    assert lib.go1render_record(None, None, None) == -1
    assert lib.go1render_record(ctypes.byref(cfg), ctypes.byref(buf), None) == -1          # num_envs = 0
    cfg.num_envs, cfg.num_cameras = 4, 3
    assert lib.go1render_image(ctypes.byref(cfg), ctypes.byref(buf), 0, None, None) == -1
    assert lib.go1render_note_reset(ctypes.byref(cfg), ctypes.byref(buf), None, 5, None) == -1


def test_render_library_is_separate_from_the_step_library():
    """the step kernel's sources, stamp and binary do not depend on the renderer"""
    import __graft_entry__ as g
    names = {os.path.basename(f) for f in g.sim_sources()} | {os.path.basename(f) for f in g.ppo_sources()}
    assert "go1render.hip" not in names and "go1render.h" not in names


def test_missing_render_library_fails_loudly(tmp_path):
    import go1render_host
    with pytest.raises(go1render_host.Go1RenderLibraryMissing, match="no CPU fallback"):
        go1render_host.load_library(str(tmp_path / "missing.so"))


def test_control_block_mirror_matches_the_header():
    import go1render_host as G
    assert ctypes.sizeof(G.Go1RecordControl) == 32 == 4 * G.CONTROL_WORDS
    src = open(HEADER).read()
    assert f"#define GO1RENDER_W {G.W}" in src and f"#define GO1RENDER_H {G.H}" in src
    assert [f for f, _ in G.Go1RenderConfig._fields_] == ["num_envs", "num_cameras", "terrain_type", "hf_rows", "hf_cols", "hf_hscale",
                                                          "hf_vscale", "hf_border", "hf_zmin", "hf_zmax"]


# ---- the reference renderer ---------------------------------------------------------------------------------------------------
def _fake_env(monkeypatch, N=16, record_video=True):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    cfg = apply_train_config(make_cfg(), num_envs=N)
    cfg.terrain.mesh_type = "plane"
    cfg.env.episode_length_s = 0.3
    cfg.env.record_video = record_video
    torch.manual_seed(0)
    return VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=cfg)


def test_reference_foot_spheres_sit_on_the_simulators_feet(monkeypatch):
    """forward kinematics of tests/render_ref.py == the oracle's foot_positions (the physics' own forward kinematics)"""
    env = _fake_env(monkeypatch)
    g = torch.Generator().manual_seed(3)
    worst, checked = 0.0, 0
    for k in range(25):
        env.step(0.8 * torch.randn(env.num_envs, 12, generator=g))
        fresh = env.reset_buf.numpy() == 0       # (an env reset by this step reports the feet of its pre-reset state, :112-115)
        if k % 4 != 3 or not fresh.any():
            continue
        root = env.root_states.double().numpy()
        dof = env.dof_pos.double().numpy()
        feet = env.foot_positions.double().numpy()
        checked += int(fresh.sum())
        for e in np.nonzero(fresh)[0]:
            worst = max(worst, float(np.abs(R.foot_centres(root[e], dof[e]) - feet[e]).max()))
    assert checked >= 3 * env.num_envs and worst < 1e-5, (checked, worst)


def test_reference_box_projects_to_the_pinhole_pixels():
    """a level camera at the origin looking along +y; the box's front face x, z in [-1, 1] at y = 4.9 covers exactly the pixels whose
    centres the pinhole model puts inside its projected rectangle: column (x / 4.9 + 1) * 180 - 0.5, row (1 - 1.5 z / 4.9) * 120 - 0.5"""
    eye, target = np.zeros(3), np.array([0.0, 10.0, 0.0])
    box = ("box", 3, (np.eye(3), np.array([0.0, 5.0, 0.0]), np.array([1.0, 0.1, 1.0])))
    _, ids = R.render_scene(eye, target, [box], terrain=None)
    c0, c1 = (-1 / 4.9 + 1) * 180 - 0.5, (1 / 4.9 + 1) * 180 - 0.5
    r0, r1 = (1 - 1.5 / 4.9) * 120 - 0.5, (1 + 1.5 / 4.9) * 120 - 0.5
    cols, rows = np.arange(R.W), np.arange(R.H)
    inside = ((rows >= r0) & (rows <= r1))[:, None] & ((cols >= c0) & (cols <= c1))[None, :]
    assert np.array_equal(ids == 3, inside)
    # and the model's own projection of the corners agrees with the hand-computed rectangle
    corners = np.array([[sx, 4.9, sz] for sx in (-1, 1) for sz in (-1, 1)])
    px = R.project(eye, target, corners)
    assert np.allclose(sorted(set(np.round(px[:, 0], 9))), [c0, c1]) and np.allclose(sorted(set(np.round(px[:, 1], 9))), [r0, r1])
    # a rotated box: its silhouette's extreme pixels are those of its projected corners (+-1 pixel)
    a = 0.4
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    half = np.array([0.5, 0.3, 0.4])
    c = np.array([0.7, 4.0, -0.2])
    _, ids = R.render_scene(eye, target, [("box", 3, (Rz, c, half))], terrain=None)
    pts = np.array([c + Rz @ (half * np.array([sx, sy, sz])) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    p = R.project(eye, target, pts)
    rr, cc = np.nonzero(ids == 3)
    assert abs(cc.min() - p[:, 0].min()) <= 1 and abs(cc.max() - p[:, 0].max()) <= 1
    assert abs(rr.min() - p[:, 1].min()) <= 1 and abs(rr.max() - p[:, 1].max()) <= 1


def test_reference_level_camera_sees_the_horizon_on_the_middle_row():
    _, ids = R.render_scene(np.array([0.0, 0.0, 1.0]), np.array([0.0, 10.0, 1.0]), [], terrain="plane", max_dist=1e7)
    assert (ids[:R.H // 2] == 0).all() and (ids[R.H // 2:] != 0).all()
    # the 1 m checker: straight below the camera's view the squares alternate along a row at x = +-1, +-2, ...
    row = ids[-1]
    assert set(np.unique(row)) == {1, 2}


def test_reference_height_field_of_constant_slope_is_a_plane():
    """a field whose samples rise linearly along x is the plane z = slope * x: same hits as the analytic plane tilted alike"""
    hs, vs, border = 0.1, 0.005, 5.0
    i = np.arange(200)[:, None] * np.ones((1, 200))
    samples = (i * 4).astype(np.int16)                       # 4 units of 5 mm per 10 cm cell: slope 0.2
    field = R.HeightField(samples, hs, vs, border)
    eye = np.array([3.0, 2.0, 4.0])
    d = R.camera_rays(eye, eye + np.array([0.0, 1.0, -1.0])).reshape(-1, 3)
    t, n, _ = field.intersect(eye, d, np.full(len(d), 30.0))
    # analytic: z = 0.2 (x + border)
    with np.errstate(divide="ignore"):
        ta = (0.2 * (eye[0] + border) - eye[2]) / (d[:, 2] - 0.2 * d[:, 0])
    hit = np.isfinite(t)
    assert hit.mean() > 0.9
    assert np.allclose(t[hit], ta[hit], atol=1e-9)
    assert np.allclose(n[hit], np.array([-0.2, 0.0, 1.0]) / np.sqrt(1.04), atol=1e-12)


# ---- recording surface where no GPU holds the buffers ----------------------------------------------------------------------------
def test_recording_is_a_no_op_off_the_gpu(monkeypatch):
    env = _fake_env(monkeypatch)
    assert env.start_recording() is None and env.get_complete_frames() == []
    for _ in range(40):
        env.step(torch.zeros(env.num_envs, 12))
    assert env.get_complete_frames() == [] and env.pause_recording() is None
    with pytest.raises(NotImplementedError):
        env.render()


# ---- logger.save_video: animated PNG ---------------------------------------------------------------------------------------------
def read_apng(path):
    """(frames as (H, W, 4) uint8 arrays, per-frame delays in seconds, acTL frame count), parsed with zlib and struct only"""
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        n, = struct.unpack(">I", blob[pos:pos + 4])
        kind, data = blob[pos + 4:pos + 8], blob[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + data) & 0xFFFFFFFF
        chunks.append((kind, data))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1][0] == b"IEND"
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[0][1][:10])
    assert (depth, ctype) == (8, 6)
    n_frames, = struct.unpack(">I", [d for k, d in chunks if k == b"acTL"][0][:4])
    frames, delays, seqs, cur = [], [], [], None
    for kind, data in chunks:
        if kind == b"fcTL":
            seqs.append(struct.unpack(">I", data[:4])[0])
            num, den = struct.unpack(">HH", data[20:24])
            delays.append(num / den)
            cur = []
            frames.append(cur)
        elif kind == b"IDAT":
            cur.append(data)
        elif kind == b"fdAT":
            seqs.append(struct.unpack(">I", data[:4])[0])
            cur.append(data[4:])
    assert seqs == list(range(len(seqs)))
    out = []
    for parts in frames:
        raw = np.frombuffer(zlib.decompress(b"".join(parts)), np.uint8).reshape(h, 1 + 4 * w)
        assert (raw[:, 0] == 0).all()
        out.append(raw[:, 1:].reshape(h, w, 4))
    return out, delays, n_frames


def test_save_video_writes_an_animated_png_that_decodes_to_the_frames(tmp_path):
    from ml_logger import logger
    logger.configure("run", root=str(tmp_path))
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (240, 360, 4), dtype=np.uint8) for _ in range(7)]
    dt = 0.02
    t = logger.save_video(frames, "videos/00012.mp4", fps=1 / dt)
    assert not t.daemon
    t.join()
    path = tmp_path / "run" / "videos" / "00012.png"
    assert path.exists() and not (tmp_path / "run" / "videos" / "00012.mp4").exists()
    got, delays, n = read_apng(str(path))
    assert n == len(got) == 7
    assert all(abs(d - dt) < 1e-12 for d in delays)
    for a, b in zip(frames, got):
        assert np.array_equal(a, b)
