"""CPU checks of the spectrum family (include/go1spectrum.h, libgo1spectrum.so): the ctypes mirrors and the exported symbols against the
header, the build's source list (as the compiler reads it), flags and stamp, the refusals without a GPU, the model of
tests/spectrum_ref.py against mathematics (an fp64 DFT, Parseval, the on-bin sine) within derived rounding bounds, the model's rules on
the scripted kinds, go1spectrum.hip itself under the SIMT emulator against that model bit for bit (accumulators, state, density sums and
the result tables), the environment hooks where there is no GPU, and the sweep's host pieces."""
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

import spectrum_ref as T
from test_eval_return_codes import Call, cfg, each, nobody, null
from test_response_trace import C_TYPES, REPO, bits, enum_order, struct_fields
from util import build_emu

HEADER = os.path.join(REPO, "include", "go1spectrum.h")
SOURCE = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1spectrum.hip")
TABLES = os.path.join(REPO, "walk-these-ways_amd", "csrc", "go1_tables.h")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]
DT = 0.02


# ---- 1. mirrors, symbols, sources, stamp ---------------------------------------------------------------------------------------------------
def test_spectrum_mirrors_match_the_header():
    import go1spectrum_host as G
    src = open(HEADER).read()
    for macro, value in (("GO1SPECTRUM_SIGNALS", G.NUM_SIGNALS), ("GO1SPECTRUM_NUM", G.NUM_SPECTRUM_METRICS), ("GO1SPECTRUM_MIN_SEGMENT", G.MIN_SEGMENT),
                         ("GO1SPECTRUM_MAX_SEGMENT", G.MAX_SEGMENT), ("GO1SPECTRUM_FOLD_THREADS", G.FOLD_THREADS), ("GO1SPECTRUM_NUM_FIELDS", 6),
                         ("GO1SPECTRUM_REDUCE_THREADS", 256)):
        assert re.search(rf"#define {macro} {value}\n", src), macro
    assert (G.NUM_SIGNALS, G.NUM_SPECTRUM_METRICS, G.MIN_SEGMENT, G.MAX_SEGMENT, G.FOLD_THREADS) == (40, 5, 8, 128, 64) and (T.S, T.NUM) == (40, 5)
    want = struct_fields(src, "Go1SpectrumConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1SpectrumConfig._fields_] == ["num_envs", "warmup_steps", "num_groups", "segment_steps", "high_bin", "bin_width"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1SpectrumConfig._fields_):
        assert ctype is C_TYPES[ctext], field
    assert ctypes.sizeof(G.Go1SpectrumConfig) == 24
    want = struct_fields(src, "Go1SpectrumBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1SpectrumBuffers._fields_] == \
        T.INPUTS + T.TABLES + ACCUMULATORS + T.STATE + ["group", "results", "psd_results", "psd_counts"]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1SpectrumBuffers._fields_)
    types_ = dict(want)
    assert types_["ring"] == "float*" and types_["valid"] == "uint8_t*" and types_["psd_sum"] == types_["psd_results"] == types_["psd_counts"] == "double*"
    assert types_["psd_segments"] == types_["segments"] == types_["segments_dropped"] == "uint32_t*" and types_["tw_re"] == types_["freq"] == "const float*"
    assert G._SPECTRUM_INPUTS == T.INPUTS and G._SPECTRUM_TABLES == T.TABLES and G._SPECTRUM_STATE == T.STATE
    assert set(G.Go1Spectrum.STATE) == set(T.STATE) - {"ring", "psd_sum"}                       # those two are sized by arm()
    assert enum_order(src, "Go1SpectrumMetric", "GO1SPECTRUM_") == G.SPECTRUM_NAMES == T.METRICS
    assert enum_order(src, "Go1SpectrumGroupField", "GO1SPECTRUM_G_") == G.SPECTRUM_GROUP_FIELDS == T.GROUP_FIELDS
    import go1eval_host as E
    assert enum_order(src, "Go1SpectrumField", "GO1SPECTRUM_F_") == E.FIELD_NAMES
    assert issubclass(G.Go1Spectrum, E._Table) and G.Go1Spectrum.ROWS == 200 and G.Go1Spectrum.TABLE_ROWS == 201
    assert len(G.SIGNAL_NAMES) == 40 == len(set(G.SIGNAL_NAMES)) and G.SIGNAL_NAMES[0] == "action_FL_hip" and G.SIGNAL_NAMES[14] == "torque_FL_calf"
    assert G.SIGNAL_NAMES[24 + 11] == "dof_vel_RR_calf" and G.SIGNAL_NAMES[36:] == ["roll_rate", "pitch_rate", "yaw_rate", "vertical_vel"]
    from go1_gym_learn.eval_metrics import spectrum
    assert spectrum.SPECTRUM_ROWS == G.SPECTRUM_NAMES and spectrum.NUM_SIGNALS == 40 and spectrum.TRUNK_SIGNALS == G.TRUNK_SIGNALS
    rows = spectrum.row_signals()
    assert len(rows) == 13 and sorted(s for _, _, signals in rows for s in signals) == list(range(40))
    assert rows[0] == ("action", "hip", [0, 3, 6, 9]) and rows[5] == ("torque", "calf", [14, 17, 20, 23]) and rows[12] == ("trunk", "vertical_vel", [39])
    for _, part, signals in rows[:9]:
        assert all(G.SIGNAL_NAMES[s].endswith("_" + part) for s in signals)
    # the host's tables are the model's, bit for bit
    for W in (8, 16, 100, 128):
        for taper in G.TAPERS:
            mine, theirs = T.tables(W, DT, taper), G.twiddle_tables(W, DT, taper)
            assert list(theirs) == T.TABLES and all(theirs[k].dtype == f32 and bits(theirs[k]) == bits(mine[k]) for k in T.TABLES), (W, taper)
    tb = G.twiddle_tables(100, DT)
    assert tb["tw_re"].shape == tb["tw_im"].shape == (51, 100) and tb["freq"][[0, 1, 50]].tolist() == [0.0, 0.5, 25.0] and tb["scale"][1] == 2 * tb["scale"][0] == 2 * tb["scale"][50]
    assert G.first_high_bin(tb["freq"], 10.0) == 20 and G.first_high_bin(tb["freq"], 9.9) == 20 and G.first_high_bin(tb["freq"], 25.0) == 50
    for bad in (0.0, -1.0, 25.1):
        with pytest.raises(ValueError):
            G.first_high_bin(tb["freq"], bad)
    for bad in (7, 6, 130, 99, 16.5):
        with pytest.raises(ValueError):
            G.check_segment(bad)
    with pytest.raises(ValueError):
        G.taper_weights(16, "hamming")


def test_exported_symbols_are_the_headers_declarations():
    import __graft_entry__ as g
    import go1spectrum_host as G
    declared = set(re.findall(r"\b(go1spectrum_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(G.EXPORTED_SYMBOLS) == {"go1spectrum_clear", "go1spectrum_record", "go1spectrum_fold", "go1spectrum_reduce", "go1spectrum_version"}
    out = g.build_spectrum_hip()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    dynamic = subprocess.run([nm, "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in dynamic.splitlines() if " T " in line and "go1spectrum_" in line} == declared
    assert not re.search(r"\bgo1(eval|feet|trunk|gait)_\w+", dynamic)


def test_sources_flags_and_stamp():
    import __graft_entry__ as g
    assert g.spectrum_sources() == [SOURCE, TABLES, HEADER] and g.SPECTRUM_FLAGS == g.EVAL_FLAGS and "-ffp-contract=off" in g.SPECTRUM_FLAGS
    assert g.SPECTRUM_FLAGS is not g.EVAL_FLAGS
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc] + g.SPECTRUM_FLAGS + ["--cuda-host-only", "-MM", SOURCE], cwd=g.CSRC, check=True, capture_output=True, text=True).stdout
    read = {os.path.normpath(os.path.join(g.CSRC, f)) for f in out.split(":", 1)[1].replace("\\\n", " ").split()}
    assert {f for f in read if not f.startswith("/opt/")} == {os.path.normpath(f) for f in g.spectrum_sources()}
    for others in (g.sim_sources(), g.ppo_sources(), g.render_sources(), g.state_sources()):
        assert not set(others) & set(g.spectrum_sources())
    for others in (g.eval_sources(), g.feet_sources(), g.trunk_sources(), g.gait_sources(), g.reward_sources()):      # one shared header, and nothing else
        assert set(others) & set(g.spectrum_sources()) == {TABLES}
    code = re.sub(r"//.*", "", open(SOURCE).read())
    assert not re.search(r"go1(eval|feet|trunk|gait)", code) and "GO1_TABLES_MATCH(GO1SPECTRUM)" in code
    assert "go1spectrum" not in re.sub(r"//.*", "", open(TABLES).read())    # the shared header names no library
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["../../include/go1spectrum.h", "go1_tables.h"]
    for banned in ("atomic", "sinf", "cosf", "sincosf", "__sinf", "__cosf", "fmaf", "__fmaf"):   # no atomics, no trigonometry, no fused multiply-add
        assert banned not in code, banned
    record = code[code.index("spectrum_record_kernel"):code.index("spectrum_fold_kernel")]
    assert "__shared__" not in record and "__syncthreads" not in record
    out = g.build_spectrum_hip()
    assert os.path.basename(out) == "libgo1spectrum.so" and g.library_stamp(out) == g.source_hash(g.spectrum_sources(), g.SPECTRUM_FLAGS)
    lib = ctypes.CDLL(out)                                                   # dlopen needs no GPU
    lib.go1spectrum_version.restype = ctypes.c_char_p
    assert lib.go1spectrum_version() == b"go1spectrum 0.1 (gfx950) go1-src:" + g.library_stamp(out).encode()
    assert "build_spectrum_hip()" in inspect.getsource(g.build) and "libgo1spectrum.so" in inspect.getsource(g.smoke)
    # the other table libraries' stamps are what their own sources give: this family changed none of them
    for name, sources, flags in (("eval", g.eval_sources(), g.EVAL_FLAGS), ("feet", g.feet_sources(), g.FEET_FLAGS), ("trunk", g.trunk_sources(), g.TRUNK_FLAGS),
                                 ("gait", g.gait_sources(), g.GAIT_FLAGS)):
        assert g.library_stamp(os.path.join(g.CSRC, f"libgo1{name}.so")) in (None, g.source_hash(sources, flags)), name


def test_a_missing_library_fails_loudly(tmp_path):
    import go1spectrum_host as G
    with pytest.raises(G.Go1SpectrumLibraryMissing, match="no CPU fallback"):
        G.load_library(str(tmp_path / "libgo1spectrum.so"))


# ---- 2. the refusals without a GPU (the helpers of tests/test_eval_return_codes.py) ----------------------------------------------------------
def spectrum_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.segment_steps, c.high_bin, c.bin_width = 70, 2, 3, 16, 4, 3.125


def slot(value):
    return lambda a: setattr(a, "row", value)


SPECTRUM_ACC = ACCUMULATORS + T.STATE
BAD_SEGMENT = [("segment_steps odd", -12, [cfg(segment_steps=15)]), ("segment_steps = 6", -12, [cfg(segment_steps=6)]),
               ("segment_steps = 130", -12, [cfg(segment_steps=130)]), ("segment_steps = 0", -12, [cfg(segment_steps=0)]), ("segment_steps < 0", -12, [cfg(segment_steps=-16)])]
CASES = {
    "go1spectrum_clear": nobody() + each(SPECTRUM_ACC, -2) + BAD_SEGMENT + [
        ("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")]),
        ("no psd_sum and segment_steps odd", -2, [null("psd_sum"), cfg(segment_steps=9)])],
    "go1spectrum_record": nobody() + each(SPECTRUM_ACC, -2) + each(T.INPUTS, -3) + BAD_SEGMENT[:3] + [
        ("segment_steps = 0: no slot is inside", -7, [cfg(segment_steps=0)]), ("segment_steps < 0: no slot is inside", -7, [cfg(segment_steps=-16)]),
        ("slot = W", -7, [slot(16)]), ("slot < 0", -7, [slot(-1)]), ("slot far outside", -7, [slot(2 ** 31 - 1)]),
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no ring and no actions", -2, [null("ring", "actions")]),
        ("no valid and slot = W", -2, [null("valid"), slot(16)]),
        ("no torques and slot = W", -3, [null("torques"), slot(16)]),
        ("no reset_buf and segment_steps odd", -3, [null("reset_buf"), cfg(segment_steps=9)]),
        ("slot = W and segment_steps odd", -7, [slot(9), cfg(segment_steps=9)]),
        ("a slot inside a segment that is too long", -12, [slot(129), cfg(segment_steps=130)])],
    "go1spectrum_fold": nobody() + each(SPECTRUM_ACC, -2) + each(T.TABLES, -3) + BAD_SEGMENT + [
        ("high_bin = 0", -12, [cfg(high_bin=0)]), ("high_bin < 0", -12, [cfg(high_bin=-1)]), ("high_bin = F", -12, [cfg(high_bin=9)]),
        ("bin_width = 0", -12, [cfg(bin_width=0.0)]), ("bin_width < 0", -12, [cfg(bin_width=-3.125)]), ("bin_width NaN", -12, [cfg(bin_width=NAN)]),
        ("bin_width inf", -12, [cfg(bin_width=INF)]),
        ("num_envs = 0 and no tw_re", -1, [cfg(num_envs=0), null("tw_re")]),
        ("no segments and no scale", -2, [null("segments", "scale")]),
        ("no tw_im and high_bin = 0", -3, [null("tw_im"), cfg(high_bin=0)]),
        ("no freq and segment_steps odd", -3, [null("freq"), cfg(segment_steps=9)]),
        ("no simulator input and high_bin = 0: the fold reads none", -12, [null(*T.INPUTS), cfg(high_bin=0)])],
    "go1spectrum_reduce": nobody() + each(SPECTRUM_ACC, -2) + BAD_SEGMENT + [
        ("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group", "results", "psd_results", "psd_counts"], -5) + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no resets and no psd_results", -2, [null("resets", "psd_results")]),
        ("no psd_counts and segment_steps odd", -5, [null("psd_counts"), cfg(segment_steps=9)]),
        ("no input, no table of the host and segment_steps odd: the reduction reads neither", -12, [null(*T.INPUTS, *T.TABLES), cfg(segment_steps=9)])],
}


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    """every case fails validation, so nothing is launched: there is no GPU.  The smallest and the largest good configuration are not
    refused: with an input missing they get as far as -3 (or -5)."""
    import __graft_entry__ as g
    import go1spectrum_host as G
    g.build_spectrum_hip()
    fn = getattr(G.load_library(), symbol)

    def call(a):
        extra = [ctypes.c_int32(a.row)] if symbol == "go1spectrum_record" else []
        return fn(None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b), *extra, None)
    assert len({label for label, _, _ in CASES[symbol]}) == len(CASES[symbol])
    assert sum(len(spoilers) > 1 for _, _, spoilers in CASES[symbol]) >= 2          # two conditions at once: precedence
    for label, code, spoilers in CASES[symbol]:
        a = Call(G.Go1SpectrumConfig, G.Go1SpectrumBuffers, spectrum_base)
        for spoil in spoilers:
            spoil(a)
        assert call(a) == code, (symbol, label)
    missing, short = {"go1spectrum_clear": ("count", -2), "go1spectrum_record": ("actions", -3), "go1spectrum_fold": ("freq", -3),
                      "go1spectrum_reduce": ("results", -5)}[symbol]
    for good in (cfg(segment_steps=8, high_bin=1), cfg(segment_steps=8, high_bin=4), cfg(segment_steps=128, high_bin=64), cfg(segment_steps=100, high_bin=20),
                 cfg(bin_width=1e-30)):
        a = Call(G.Go1SpectrumConfig, G.Go1SpectrumBuffers, spectrum_base)
        good(a)
        a.row = a.c.segment_steps - 1                                          # the last good slot
        null(missing)(a)
        assert call(a) == short


# ---- 3. the model against mathematics ----------------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def exact_tables(W, taper):
    """the tables in fp64, not rounded: (w, tw_re, tw_im, scale, freq)"""
    F, fs = W // 2 + 1, 1.0 / DT
    w = T.taper(W, taper)
    k, t = np.arange(F)[:, None], np.arange(W)[None, :]
    angle = 2.0 * np.pi * ((k * t) % W) / W
    scale = np.full(F, 2.0 / (fs * (w * w).sum()))
    scale[[0, F - 1]] *= 0.5
    return w, w * np.cos(angle), -w * np.sin(angle), scale, np.arange(F) * fs / W


def density_bound(E_re, E_im, re, im, scale):
    """|P32 - P| where P = (re^2 + im^2) scale in exact arithmetic on the exact re, im, and P32 the fp32 evaluation (two products, one sum,
    one product by the scale: each square carries one rounding, the sum one, the scaling one, so three in a chain: gamma_3) on values
    within E_re, E_im of them: |a32^2 - a^2| <= E (2 |a| + E)."""
    spread = E_re * (2.0 * np.abs(re) + E_re) + E_im * (2.0 * np.abs(im) + E_im)
    return scale * spread * (1.0 + gamma(3)) + gamma(3) * scale * (re * re + im * im)


@pytest.mark.parametrize("W,taper", [(8, "hann"), (16, "boxcar"), (100, "hann"), (128, "hann"), (100, "boxcar")])
def test_model_dft_within_the_sequential_dot_product_bound(W, taper):
    """The model's fp32 transform against an fp64 DFT of the model's own fp32 y with the fp32 tables promoted to fp64.

    The bound.  re is the fp32 evaluation of sum_t y_t c_t in ascending t, products rounded, then added: the standard result for a
    sequential dot product of n terms (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5)) is
        |fl(x . c) - x . c| <= gamma_n sum_t |x_t c_t|,  gamma_n = n u / (1 - n u),  u = 2^-24.
    Each term passes through one product and at most W - 1 additions, W roundings; the issue asks for gamma_{W+1} with a margin of 2,
    which is what is asserted: E = 2 gamma_{W+1} sum_t |y_t tw_t|.  The operands are the same fp32 numbers on both sides, so neither
    the tables' nor y's own rounding enters.  P = (re re + im im) scale then lies within density_bound() of its fp64 value, where the
    fp64 scale is the fp32 table value promoted.  The mean: W - 1 additions and one division, so |mean32 - mean64| <= gamma_W mean|x|.
    The fp64 DFT itself is np.fft.rfft-free: an explicit fp64 matrix product, whose own error (2^-53 W) is ten orders below the bound."""
    rng = np.random.default_rng(W)
    cfg_ = T.config(W, taper_name=taper, dt=DT)
    x = np.cumsum(rng.standard_normal((W, 3, 50)).astype(f32) * f32(0.1), axis=0, dtype=f32) + rng.standard_normal((1, 3, 50)).astype(f32) * f32(5.0)
    d = T.transform(x, cfg_)
    x64, y64 = x.astype(np.float64), d["y"].astype(np.float64)
    mean64 = x64.mean(axis=0)
    assert (np.abs(d["mean"].astype(np.float64) - mean64) <= gamma(W) * np.abs(x64).mean(axis=0)).all()
    assert bits(d["y"]) == bits(x - d["mean"])                              # y is the fp32 difference, one rounding
    tw_re, tw_im, scale = (cfg_.tables[k].astype(np.float64) for k in ("tw_re", "tw_im", "scale"))
    re64, im64 = np.einsum("kt,t...->k...", tw_re, y64), np.einsum("kt,t...->k...", tw_im, y64)
    E_re = 2.0 * gamma(W + 1) * np.einsum("kt,t...->k...", np.abs(tw_re), np.abs(y64))
    E_im = 2.0 * gamma(W + 1) * np.einsum("kt,t...->k...", np.abs(tw_im), np.abs(y64))
    err_re, err_im = np.abs(d["re"].astype(np.float64) - re64), np.abs(d["im"].astype(np.float64) - im64)
    assert (err_re <= E_re).all() and (err_im <= E_im).all()
    assert err_re.max() > 0 and E_re[1:].min() > 0                           # the comparison is not empty
    print(f"\nW {W} {taper}: worst |re32 - re64| / bound {np.max(err_re[1:] / E_re[1:]):.3f}, |im| {np.max(err_im[1:-1] / E_im[1:-1]):.3f}")
    sc = scale.reshape(-1, 1, 1)
    P64 = (re64 * re64 + im64 * im64) * sc
    assert (np.abs(d["P"].astype(np.float64) - P64) <= density_bound(E_re, E_im, re64, im64, sc)).all()

    # Parseval for the one-sided scale, against the EXACT taper: sum_k P_k bin_width = sum_t (w_t y_t)^2 / sum_t w_t^2, all bins k = 0 .. F - 1.
    # Against exact tables the fp32 table entries are one more rounding each (|fl(c) - c| <= u |c|: gamma_{W+2} in E), the fp32 scale and
    # bin_width one each (2 u relative on the whole), and the final sum over k is taken in fp64 here.
    w, xre, xim, xscale, _ = exact_tables(W, taper)
    re_x, im_x = np.einsum("kt,t...->k...", xre, y64), np.einsum("kt,t...->k...", xim, y64)
    E2_re = 2.0 * gamma(W + 2) * np.einsum("kt,t...->k...", np.abs(xre), np.abs(y64))
    E2_im = 2.0 * gamma(W + 2) * np.einsum("kt,t...->k...", np.abs(xim), np.abs(y64))
    xs = xscale.reshape(-1, 1, 1)
    width = 1.0 / DT / W
    rhs = ((w.reshape(-1, 1, 1) * y64) ** 2).sum(axis=0) / (w * w).sum()
    assert np.allclose(((re_x ** 2 + im_x ** 2) * xs).sum(axis=0) * width, rhs, rtol=1e-12, atol=0)          # the identity itself, in fp64
    lhs = d["P"].astype(np.float64).sum(axis=0) * float(cfg_.bin_width)
    tol = density_bound(E2_re, E2_im, re_x, im_x, xs).sum(axis=0) * width + 3.0 * U * rhs
    assert (np.abs(lhs - rhs) <= tol).all() and (tol < 1e-3 * rhs).all()        # (and the bound is no empty one)
    # and power is that sum without bin 0, summed in fp32 over F - 1 terms and scaled: gamma_F more
    power = (d["total"] * cfg_.bin_width).astype(np.float64)
    without_dc = rhs - (re_x[0] ** 2 + im_x[0] ** 2) * xs[0] * width
    assert (np.abs(power - without_dc) <= tol + gamma(W // 2 + 1) * rhs).all()


@pytest.mark.parametrize("W,taper,share", [(16, "hann", 2.0 / 3.0), (100, "hann", 2.0 / 3.0), (128, "hann", 2.0 / 3.0), (16, "boxcar", 1.0), (100, "boxcar", 1.0)])
def test_model_on_bin_sine(W, taper, share):
    """x_t = fl(sin(2 pi k0 t / W)) for every k0 in [2, W / 2 - 2]: peak_freq is freq[k0] exactly, and peak_share is 2/3 under Hann (the
    taper spreads an on-bin line over k0 - 1, k0, k0 + 1 with amplitudes 1/4, 1/2, 1/4: powers 1/16, 1/4, 1/16, so 4/6) and 1 under boxcar.

    The bound is the same kind as above, against the exact sine and exact tables: per bin E = 2 gamma_{W+2} sum_t |y_t c_t| for the
    arithmetic and the tables' rounding, plus (2 u + gamma_W) sum_t |c_t| for what the fp32 samples differ from the exact sine by
    (u for fl(sin), gamma_W for the fp32 mean of |x| <= 1 that is subtracted where the exact mean is 0, u for the subtraction).  With B_k
    = density_bound(E_k) and the fp32 total of F - 1 terms (gamma_F more) the share P_kp / total lies within
    (B_kp + share (sum_k B_k + gamma_F total)) / (total - sum_k B_k - gamma_F total) + u of the exact one."""
    cfg_ = T.config(W, taper_name=taper, dt=DT)
    k0 = np.arange(2, W // 2 - 1)
    t = np.arange(W)
    exact = np.sin(2.0 * np.pi * ((k0[None, :] * t[:, None]) % W) / W)     # (W, K)
    d = T.transform(exact.astype(f32), cfg_)
    assert d["kp"].tolist() == k0.tolist() and bits(cfg_.tables["freq"][d["kp"]]) == bits(cfg_.tables["freq"][k0])
    w, xre, xim, xscale, freq = exact_tables(W, taper)
    assert bits(cfg_.tables["freq"]) == bits(freq.astype(f32)) and (freq.astype(f32) == freq).all()          # k / 2 Hz and the like: exact in fp32
    re_x, im_x = xre @ exact, xim @ exact
    P_x = (re_x ** 2 + im_x ** 2) * xscale[:, None]
    total_x = P_x[1:].sum(axis=0)
    assert np.allclose(P_x[k0, np.arange(len(k0))] / total_x, share, rtol=1e-12, atol=0)                   # mathematics
    E_re = 2.0 * gamma(W + 2) * np.abs(xre) @ np.abs(exact) + (2.0 * U + gamma(W)) * np.abs(xre).sum(axis=1, keepdims=True)
    E_im = 2.0 * gamma(W + 2) * np.abs(xim) @ np.abs(exact) + (2.0 * U + gamma(W)) * np.abs(xim).sum(axis=1, keepdims=True)
    B = density_bound(E_re, E_im, re_x, im_x, xscale[:, None]) + U * P_x                                    # (+ the fp32 scale's own rounding)
    slack = B[1:].sum(axis=0) + gamma(W // 2 + 1) * total_x
    tol = (B[k0, np.arange(len(k0))] + share * slack) / (total_x - slack) + U
    got = (d["best"] / d["total"]).astype(np.float64)
    print(f"\nW {W} {taper}: peak_share {got.min():.9f} .. {got.max():.9f}, bound {tol.max():.2e}")
    assert (np.abs(got - share) <= tol).all() and tol.max() < 1e-4


# ---- 4. the model's rules on the scripted kinds -----------------------------------------------------------------------------------------------
def rows_of(st, s, e):
    """{row: (count, nonfinite)} of signal s of environment e"""
    return {name: (int(st.count[s * 5 + m, e]), int(st.nonfinite[s * 5 + m, e])) for m, name in enumerate(T.METRICS)}


def check_the_rules(st, folds, cfg_, snaps, kind, N):
    """what the script was written to drive, on the model's state `st` after it (every kind needs N >= len(KINDS))"""
    W = cfg_.segment_steps
    steps = len(snaps)
    assert steps == 3 * W + 2 and len(folds) == 3 and (st.steps == steps).all() and st.calls == steps
    assert (st.segments + st.segments_dropped == 3).all()                   # the open segment at the end is neither
    if N < len(T.KINDS):
        return
    of = lambda k: kind == k
    clean = np.isin(kind, (T.WALKS, T.SINES, T.NONFINITE, T.CONSTANT, T.HUGE, T.TIE))
    assert (st.segments[clean] == 3).all() and (st.resets[clean] == 0).all()
    # a spoiled segment is dropped and counted, and the next clean one is measured; a reset on a segment's last step spoils the next too
    assert (st.segments[of(T.RESETS)] == 2).all() and (st.segments_dropped[of(T.RESETS)] == 1).all() and (st.resets[of(T.RESETS)] == 3).all()
    assert (st.segments[of(T.LATE_RESET)] == 1).all() and (st.segments_dropped[of(T.LATE_RESET)] == 2).all() and (st.resets[of(T.LATE_RESET)] == 1).all()
    assert folds[0]["valid"].all() and (folds[1]["valid"] == ~np.isin(kind, (T.RESETS, T.LATE_RESET))).all() and (folds[2]["valid"] == ~of(T.LATE_RESET)).all()
    dead = [(~((s["reset_buf"] == 0) & (s["episode_length_buf"] > cfg_.warmup_steps)) & (s["reset_buf"] == 0)).any() for s in snaps]
    assert any(dead)                                                        # warm-up steps that are no resets
    for e in np.nonzero(of(T.RESETS) | of(T.LATE_RESET))[0]:
        assert all(rows_of(st, s, e)[m] == (int(st.segments[e]), 0) for s in (0, 39) for m in T.METRICS) and (st.psd_segments[:, e] == st.segments[e]).all()
    # a NaN or an infinite sample: exactly its own signal's five rows in nonfinite, its psd_sum as after two segments, every other signal whole
    bad = [s for s, _, _ in T.BAD_SAMPLES]
    for e in np.nonzero(of(T.NONFINITE))[0]:
        for s in range(T.S):
            want = (2, 1) if s in bad else (3, 0)
            assert all(rows_of(st, s, e)[m] == want for m in T.METRICS), (s, e)
            assert st.psd_segments[s, e] == want[0] and np.isfinite(st.psd_sum[s, :, e]).all()
        for s in bad:
            assert not folds[1]["enters"][s, e] and bits(st.psd_sum[s, :, e]) == bits(folds[0]["P"][:, s, e].astype(np.float64) + folds[2]["P"][:, s, e].astype(np.float64))
            assert not np.isfinite(folds[1]["rows"][:, s, e]).any()
    # the constant signal: power 0 and four non-finite rows, and a density sum of zeros that counts its segments
    for e in np.nonzero(of(T.CONSTANT))[0]:
        for s in range(T.S):
            got = rows_of(st, s, e)
            assert got["power"] == (3, 0) and all(got[m] == (0, 3) for m in T.METRICS[1:]) and st.max[s * 5, e] == 0.0 and st.min[s * 5, e] == 0.0
            assert st.psd_segments[s, e] == 3 and not st.psd_sum[s, :, e].any()
    # 1e20: the densities overflow, the total is infinite, all five rows are counted in nonfinite and nothing enters psd_sum
    for e in np.nonzero(of(T.HUGE))[0]:
        assert np.isinf(folds[1]["total"][:, e]).all() and not folds[1]["enters"][:, e].any()
        assert all(rows_of(st, s, e)[m] == (2, 1) for s in range(T.S) for m in T.METRICS) and (st.psd_segments[:, e] == 2).all() and np.isfinite(st.psd_sum[:, :, e]).all()
    # the tie goes to the lowest bin
    for e in np.nonzero(of(T.TIE))[0]:
        P = folds[1]["P"][:, :, e]
        assert (folds[1]["kp"][:, e] == 1).all() and (P[3] == P[1]).all() and (P[1] > 0).all() and (P[1:].max(axis=0) == P[1]).all()
        assert (folds[1]["rows"][T.PEAK_FREQ, :, e] == cfg_.tables["freq"][1]).all()
        if cfg_.taper == "boxcar":                                           # there only the odd bins carry power
            assert (P[2] < P[1] * 1e-10).all()
    # the sines: the peak is the signal's own bin in every segment
    for e in np.nonzero(of(T.SINES))[0]:
        for s in range(T.S):
            f = cfg_.tables["freq"][T.sine_bin(s, W)]
            assert st.min[s * 5 + T.PEAK_FREQ, e] == st.max[s * 5 + T.PEAK_FREQ, e] == f
    assert np.isfinite(st.sum).all() and np.isfinite(st.sumsq).all() and np.isfinite(st.psd_sum).all()


@pytest.mark.parametrize("W,taper", [(8, "hann"), (16, "boxcar"), (100, "hann")])
def test_model_rules_on_the_scripted_kinds(W, taper):
    N = 19
    rng = np.random.default_rng(W)
    cfg_ = T.config(W, warmup_steps=T.SCRIPT_WARMUP, taper_name=taper, dt=DT)
    snaps, kind = T.scripted_steps(rng, N, W)
    assert set(kind.tolist()) == set(range(len(T.KINDS)))
    st, folds = T.run(cfg_, snaps, N)
    check_the_rules(st, folds, cfg_, snaps, kind, N)
    # the open segment at the end changes nothing but the ring, the step counters and valid
    closed, _ = T.run(cfg_, snaps[:3 * W], N)
    for k, a in st.arrays().items():
        if k not in ("ring", "steps", "valid"):
            assert bits(a) == bits(closed.arrays()[k]), k
    assert (st.steps == closed.steps + 2).all() and bits(st.ring[2:]) == bits(closed.ring[2:]) and bits(st.ring[:2]) != bits(closed.ring[:2])
    table, psd, counts = T.reduce(st, np.zeros(N, np.int32), 2)
    assert table.shape == (2, 201, 6) and psd.shape == (2, 40, W // 2 + 1) and counts.shape == (2, 40)
    assert table[0, 200].tolist() == [N, N * (3 * W + 2), float(st.resets.sum()), float(st.segments.sum()), float(st.segments_dropped.sum()), 0.0]
    assert not table[1, 200].any() and np.isnan(table[1, :200, 1:5]).all() and not psd[1].any() and not counts[1].any()
    assert (counts[0] == st.psd_segments.sum(axis=1)).all()


# ---- 5. go1spectrum.hip under the SIMT emulator against the model ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as g
    import go1spectrum_host as G
    return G.load_library(build_emu(g.spectrum_sources(), "libgo1spectrum_emu.so"))


def spectrum_on(device, N, lib=None):
    """a go1spectrum_host.Go1Spectrum on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1spectrum_host as G
    tensors = {k: torch.zeros(rows, N, device=device) for k, rows in T.SHAPES_OF_INPUTS.items()}
    tensors.update(reset_buf=torch.zeros(N, dtype=torch.uint8, device=device), episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    sm = G.Go1Spectrum(types.SimpleNamespace(num_envs=N), B, DT, lib=lib)
    if torch.device(device).type == "cpu":
        sm._stream = lambda: None
    return sm, B


def spectrum_groups(rng, N, groups=3):
    """three groups of which group 1 is empty, some environments at -1 and (from three environments on) one id outside the tables"""
    assert groups == 3
    group = rng.integers(-1, groups, N).astype(np.int32)
    group[group == 1] = 2
    group[0] = groups - 1
    if N >= 3:
        group[1], group[2] = -1, groups
    return group


def drive(sm, B, cfg_, snaps, group, groups):
    """the scripted steps through the library: arm for `groups` groups, upload a snapshot, accumulate, ...; returns read() and the
    accumulators.  arm() sizes the tables by the largest id it is given, so the ids outside the tables are handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    sm.arm(inside, cfg_.warmup_steps, segment_steps=cfg_.segment_steps, high_freq=cfg_.high_freq, taper=cfg_.taper)
    sm.group.copy_(torch.from_numpy(group))
    for s in snaps:
        for k, a in s.items():
            getattr(B, k).copy_(torch.from_numpy(a))
        sm.accumulate()
    sm.disarm()
    res = sm.read()
    acc = {k: t.cpu().numpy() for k, t in sm.acc.items()}
    return res, acc


STATE_NAMES = dict(psd_sum="env_psd_sum", psd_segments="env_psd_segments")


def same_as_the_model(res, acc, ring, st, group, groups):
    """accumulators, state, ring, density sums and the result tables against the model's state `st`, bit for bit"""
    N, F = st.N, st.F
    for k in ACCUMULATORS:
        assert acc[k].shape == (200, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k in T.STATE:
        got = ring if k == "ring" else res[STATE_NAMES.get(k, k)]
        assert got.shape == getattr(st, k).shape and bits(got.view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    want, want_psd, want_counts = T.reduce(st, group, groups)
    table = np.zeros((groups, 201, 6))
    table[:, :200] = np.stack([res["metrics"][m] for m in T.METRICS], axis=2).reshape(groups, 200, 6)
    table[:, 200, :5] = res["groups"]
    assert all(res["metrics"][m].shape == (groups, 40, 6) for m in T.METRICS) and res["groups"].shape == (groups, 5)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and bits(table) == bits(want)
    assert res["psd_sum"].shape == (groups, 40, F) and bits(res["psd_sum"]) == bits(want_psd)
    assert res["psd_segments"].shape == (groups, 40) and bits(res["psd_segments"]) == bits(want_counts)
    with np.errstate(all="ignore"):
        mean = np.where(want_counts[:, :, None] > 0, want_psd / want_counts[:, :, None], np.nan)
    assert np.array_equal(np.isnan(res["psd"]), np.isnan(mean)) and bits(res["psd"]) == bits(mean)
    return want, want_psd, want_counts


def check_against_the_model(res, acc, ring, cfg_, snaps, kind, group, groups, N):
    """the library's results against tests/spectrum_ref.py, bit for bit; then that the script drove every rule it was written to drive"""
    st, folds = T.run(cfg_, snaps, N)
    want, want_psd, want_counts = same_as_the_model(res, acc, ring, st, group, groups)
    check_the_rules(st, folds, cfg_, snaps, kind, N)
    assert res["high_bin"] == cfg_.high_bin and res["segment_steps"] == cfg_.segment_steps and bits(f32(res["bin_width"])) == bits(cfg_.bin_width)
    assert bits(res["freq"].astype(f32)) == bits(cfg_.tables["freq"]) and len(res["signals"]) == 40
    g = res["groups"]
    assert g[:, 0].sum() == np.isin(group, range(groups)).sum() and (g[:, 1] == len(snaps) * g[:, 0]).all() and g[1].tolist() == [0.0] * 5
    assert np.isnan(want[1, :200, 1:5]).all() and not want_psd[1].any() and np.isnan(res["psd"][1]).all()
    return st


# (N, W, taper): one thread and the smallest window; one wavefront; two record blocks, five fold blocks and a ragged tail; three terms
# per reduction thread; a second window, on the boxcar taper (the tie's odd bins); the largest window: the whole of the fold's LDS
SHAPES = [(1, 8, "hann"), (64, 8, "hann"), (257, 8, "hann"), (600, 8, "hann"), (70, 16, "boxcar"), (3, 128, "hann")]


@pytest.mark.parametrize("N,W,taper", SHAPES)
def test_emulated_spectrum_kernels_follow_the_model(emu, N, W, taper):
    groups = 3
    rng = np.random.default_rng(1200 + N + W)
    cfg_ = T.config(W, warmup_steps=T.SCRIPT_WARMUP, taper_name=taper, dt=DT)
    snaps, kind = T.scripted_steps(rng, N, W)
    assert len(snaps) == 3 * W + 2 and (N < len(T.KINDS) or set(kind.tolist()) == set(range(len(T.KINDS))))
    group = spectrum_groups(rng, N, groups)
    sm, B = spectrum_on("cpu", N, lib=emu)
    res, acc = drive(sm, B, cfg_, snaps, group, groups)
    assert sm.cfg.num_groups == groups and (N < 3 or {-1, groups} <= set(group.tolist())) and sm.calls == 3 * W + 2
    check_against_the_model(res, acc, sm.ring.numpy(), cfg_, snaps, kind, group, groups, N)
    again = sm.read()                                                        # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ("groups", "psd", "psd_sum", "psd_segments", "env_psd_sum", "env_psd_segments", "segments", "valid"))
    assert all(bits(again["metrics"][m]) == bits(res["metrics"][m]) for m in T.METRICS)
    before = sm.ring.clone()
    assert sm.lib.go1spectrum_record(ctypes.byref(sm.cfg), ctypes.byref(sm.buf), W, None) == -7 and torch.equal(sm.ring, before)      # nothing written
    with pytest.raises(RuntimeError, match="go1spectrum_fold failed: -12"):
        sm.cfg.high_bin = 0
        sm.fold()


# ---- 6. the environment hooks without a GPU -----------------------------------------------------------------------------------------------------
def test_spectrum_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    for module in ("go1eval_host", "go1spectrum_host"):
        monkeypatch.delitem(sys.modules, module, raising=False)
    c = apply_train_config(make_cfg(), num_envs=16)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_spectrum_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_spectrum_metrics, env.read_spectrum_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert all(m not in sys.modules for m in ("go1eval_host", "go1spectrum_host")) and env._spectrum is None          # never measured: no host module
    env.step(torch.zeros(16, 12))                                             # and stepping goes on
    signature = inspect.signature(env.start_spectrum_metrics)
    assert {k: p.default for k, p in signature.parameters.items() if k != "groups"} == dict(warmup_steps=0, segment_steps=100, high_freq=10.0, taper="hann")
    families = [name for name, _ in env._STATE_FAMILIES]
    assert ("spectrum", "_spectrum") in env._STATE_FAMILIES and families.index("gait") < families.index("spectrum") < families.index("rewards")
    # the launch order of a step, by the calls themselves: the gait family's, then the spectrum's, then the reward family's
    calls = []
    armed = lambda name: types.SimpleNamespace(armed=True, accumulate=lambda *args: calls.append(name))
    env._gait, env._spectrum, env._reward = armed("gait"), armed("spectrum"), armed("rewards")
    env.step(torch.zeros(16, 12))
    assert calls == ["gait", "spectrum", "rewards"]


# ---- 7. the sweep's host pieces and the tool ------------------------------------------------------------------------------------------------------
def fixed_result():
    import go1spectrum_host as G
    from go1_gym_learn.eval_metrics import sweep
    F = 51
    freq = np.arange(F) * 0.5
    psd = np.zeros((2, 40, F))
    psd[:, :, 6], psd[:, :, 12], psd[:, :, 19], psd[:, :, 20] = 1.0, 0.5, 0.25, 0.25          # 3 Hz, 6 Hz, 9.5 Hz (next to the harmonic at 9), 10 Hz
    psd[1, 36:] = 0.0                                                        # cell 1: a trunk that does not move
    psd[1, 0, :] = 0.0
    psd[1, 0, 30] = 2.0                                                      # and a FL hip action that chatters at 15 Hz
    row = lambda mean: np.tile(np.array([10.0, mean, 0.0, mean, mean, 0.0]), (2, 40, 1))
    t = dict(power=row(0.04), peak_freq=row(3.0), peak_share=row(0.5), high_share=row(0.125), centroid=row(5.0))
    t["power"][1, 36:] = [10.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    for m in T.METRICS[1:]:
        t[m][1, 36:] = [0.0, NAN, NAN, NAN, NAN, 10.0]
    trot = sweep.GAITS["trotting"]
    return dict(preset="static_medium", cells=[(0.5, 0.0, trot), (1.0, 0.0, trot)], step_freq=[3.0, 3.0], spectrum=t,
                spectrum_groups=np.array([[12.0, 2400.0, 0.0, 10.0, 2.0]] * 2), psd=psd, psd_segments=np.full((2, 40), 10.0), freq=freq,
                signals=list(G.SIGNAL_NAMES), high_bin=20, metrics={}, groups=np.zeros((2, 5)), segment_steps=100, high_freq=10.0, taper="hann", num_envs=24,
                steps=200, warmup_steps=5, seed=1, dt=0.02)


def test_gait_locked_table_json_and_figure(tmp_path):
    from go1_gym_learn.eval_metrics import spectrum
    res = fixed_result()
    freq = res["freq"]
    assert spectrum.harmonic_bins(freq, 3.0) == sorted(k + d for k in (6, 12, 18, 24, 30, 36, 42, 48) for d in (-1, 0, 1))
    assert spectrum.harmonic_bins(freq, 25.0) == [49, 50] and spectrum.harmonic_bins(freq, 26.0) == [] and spectrum.harmonic_bins(freq, 0.0) == []
    assert spectrum.harmonic_bins(freq, 0.5) == list(range(1, 51)) and spectrum.harmonic_bins(freq, 12.4) == [24, 25, 26, 49, 50]
    assert spectrum.gait_locked(res["psd"][0, 0], freq, 3.0) == 0.875       # (1 + 0.5 + 0.25) / 2: the line at 10 Hz is not a harmonic's
    assert spectrum.gait_locked(res["psd"][0, 0], freq, 5.0) == 0.25 and np.isnan(spectrum.gait_locked(np.zeros(51), freq, 3.0))
    assert spectrum.gait_locked(res["psd"][1, 0], freq, 3.0) == 1.0 and spectrum.gait_locked(res["psd"][1, 0], freq, 4.0) == 0.0
    s = spectrum.cell_summary(res, 0)
    assert [(r["quantity"], r["part"]) for r in s[:4]] == [("action", "hip"), ("action", "thigh"), ("action", "calf"), ("torque", "hip")] and len(s) == 13
    assert s[0]["rms"] == pytest.approx(0.2) and s[0]["peak_freq"] == 3.0 and s[0]["peak_share"] == 0.5 and s[0]["high_share"] == 0.125
    assert s[0]["centroid"] == pytest.approx((3.0 + 3.0 + 9.5 * 0.25 + 2.5) / 2.0) and s[0]["gait_locked"] == 0.875
    chatter = spectrum.cell_summary(res, 1)[0]                               # one leg of four chatters: the mean density of the four hips
    assert chatter["peak_freq"] == 3.0 and chatter["high_share"] == pytest.approx((3 * 0.25 + 2.0) / (3 * 2.0 + 2.0)) and chatter["gait_locked"] == pytest.approx(7.25 / 8.0)
    still = spectrum.cell_summary(res, 1)[12]
    assert still["rms"] == 0.0 and all(np.isnan(still[k]) for k in ("peak_freq", "peak_share", "high_share", "centroid", "gait_locked"))
    md = spectrum.spectrum_markdown_table(res).splitlines()
    assert md[0] == "| vx | yaw | step Hz | quantity | part | rms | peak Hz | peak share | share >= 10 Hz | centroid Hz | gait_locked | segments | dropped |"
    assert len(md) == 2 + 2 * 13 and len({line.count("|") for line in md}) == 1
    assert md[2] == "| 0.5 | 0 | 3 | action | hip | 0.2 | 3.00 | 0.500 | 0.125 | 5.44 | 0.875 | 10 | 2 |"
    assert md[2 + 6].startswith("| 0.5 | 0 | 3 | joint speed | hip |") and md[2 + 9].startswith("| 0.5 | 0 | 3 | trunk | roll_rate |")
    assert md[-1] == "| 1 | 0 | 3 | trunk | vertical_vel | 0 | – | – | – | – | – | 10 | 2 |"
    js = json.loads(json.dumps(spectrum.spectrum_to_json(res), allow_nan=False))
    assert js["cells"][1] == dict(vx=1.0, yaw=0.0, gait=[0.5, 0.0, 0.0], step_freq=3.0) and js["group_fields"] == T.GROUP_FIELDS and len(js["signals"]) == 40
    assert js["spectrum"]["centroid"][1][39][1] is None and js["spectrum"]["power"][0][0][1] == 0.04 and js["psd"][0][0][6] == 1.0 and js["freq"][2] == 1.0
    assert js["summary"][1][12]["gait_locked"] is None and js["summary"][0][0]["gait_locked"] == 0.875 and len(js["summary"][0][0]["mean_psd"]) == 51
    assert (js["segment_steps"], js["high_freq"], js["high_bin"], js["taper"]) == (100, 10.0, 20, "hann") and js["spectrum_groups"][0][3] == 10.0
    path = tmp_path / "spectrum.png"
    spectrum.plot_spectrum(res, str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000


def test_tool_accepts_a_spectrum_sweep(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import spectrum, sweep
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--spectrum", "--vx", "0.5", "1.0", "--envs", "24", "--steps", "200", "--warmup-steps", "5", "--presets", "static_medium",
                                      "--segment-steps", "64", "--high-freq", "8", "--taper", "boxcar"])
    assert a.spectrum and not a.trunk and not a.coordination and (a.vx, a.envs, a.steps, a.segment_steps, a.high_freq, a.taper) == ([0.5, 1.0], 24, 200, 64, 8.0, "boxcar")
    plain = eval_sweep.parse_args(base + ["--spectrum"])
    assert (plain.segment_steps, plain.high_freq, plain.taper) == (100, 10.0, "hann") and not eval_sweep.parse_args(base).spectrum
    assert eval_sweep.parse_args(base + ["--spectrum", "--terrain", "plane"]).terrain == "plane"
    assert eval_sweep.parse_args(base + ["--trunk", "--segment-steps", "33"]).segment_steps == 33          # the trunk sweep's option keeps its meaning
    for bad in (["--spectrum", "--terrain"], ["--spectrum", "--behaviour"], ["--spectrum", "--joints"], ["--spectrum", "--feet"], ["--spectrum", "--trunk"],
                ["--spectrum", "--rewards"], ["--spectrum", "--coordination"], ["--spectrum", "--response", "--switch", "vx", "0", "1"],
                ["--spectrum", "--push", "--magnitude", "1", "--direction", "0"], ["--high-freq", "8"], ["--taper", "hann"], ["--trunk", "--taper", "hann"],
                ["--segment-steps", "64"], ["--spectrum", "--segment-steps", "63"], ["--spectrum", "--segment-steps", "6"], ["--spectrum", "--segment-steps", "130"],
                ["--spectrum", "--high-freq", "0"], ["--spectrum", "--taper", "hamming"], ["--spectrum", "--window", "64"], ["--spectrum", "--tilt-limit", "0.3"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(base + bad)
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(spectrum, "run_spectrum_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    grid = dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits])
    eval_sweep.run_spectrum(a, None, grid)
    assert seen == dict(preset="static_medium", grid=grid, num_envs=24, steps=200, warmup_steps=5, seed=1, terrain=None, segment_steps=64, high_freq=8.0, taper="boxcar")
    js = json.load(open(tmp_path / "eval" / "static_medium_spectrum.json"))
    assert js["preset"] == "static_medium" and js["summary"][0][0]["gait_locked"] == 0.875
    md = (tmp_path / "eval" / "static_medium_spectrum.md").read_text()
    assert "| 0.5 | 0 | 3 | action | hip | 0.2 | 3.00 | 0.500 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_spectrum.png").read_bytes()[:4] == b"\x89PNG"
