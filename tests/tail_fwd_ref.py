"""float64 / integer model of the policy's inference forward in libgo1ppo.so (csrc/go1ppo.hip): go1ppo_tail_fwd (tail_fwd_kernel<32>, the MLP
layers behind the first one with the activations kept on chip), its ELU-on-load path (elu_in: the first layer's ELU and the actor's latent
term latent Wz^T applied while the input rows are staged) and go1ppo_elu_fwd, which the header promises computes the same numbers in place.
Plain numpy on the CPU; bf16 travels as uint16 bit patterns, rounded to nearest even in integer arithmetic (ppo_rollout_ref.bf16_bits).

Two operations, each evaluated in float64 from the bits the kernel reads (products of two bf16 numbers are exact in float64, and a sum of at
most 512 of them errs by 512 * 2^-53 of the sum of magnitudes: eight orders below every bound here):

  elu_on_load   v = elu(s), s = x + sum_q latent[r, q] wz[c, q], stored as RNE_bf16(v)
  layer         v = act(z), z = in W^T + b, stored as RNE_bf16(v); act = elu or the identity (the head)

u = 2^-24 is the unit round-off of fp32.  No bound below is taken from what a kernel gives.

EXACT cases (zero bound, bit for bit).  Inputs are integers in -4 .. 4 times 2^-2, weights integers in -wmax .. wmax times 2^-3, biases
integers in -4 .. 4 times 2^-2 (plus a power of two where a layer's pre-activations have to be positive).  All of a layer's terms a_k w_k and
b are then integer multiples of one power of two, g, and the model asserts, per layer and net, in int64 arithmetic, that
(sum_k |a_k w_k| + |b|) / g < 2^24 for every output element: every partial sum of every pre-activation, in any order and grouping, is an
integer multiple of g below 2^24 g and so exactly representable in fp32; no addition rounds, whatever the matrix unit does inside one
instruction, and the kernel's fp32 accumulator holds z exactly.  The layer's output must be RNE_bf16(z).  Rounding to bf16 maps a multiple
of g to a multiple of g (it clears low bits of the integer z / g or leaves it), so the next layer starts on the grid g again and the chain
stays exact: g_l = g_{l-1} 2^-3.  A layer of an exact case has elu = 0, or the model asserts that all its pre-activations are >= 0, where
elu1 returns its argument (at 0: fma(0, 0, 0) = 0).  The integer magnitudes grow by about sqrt(k wmax^2) per layer, which is why the later
layers of the deep cases draw from -2 .. 2 and -1 .. 1.

ROUNDED cases (random normal data with production scaling: W ~ N(0, 1 / k), b ~ 0.1 N(0, 1), inputs ~ N(0, 1), all rounded to bf16).  Every
intermediate is stored, and the model of layer l + 1 starts from the stored output of layer l of whoever is under test, so errors do not
compound: one layer at a time is held against
    e_z = 2 (K + 2) u (sum_k |a_k w_k| + |b|)
on the pre-activation: (K + 2) u bounds K + 1 fp32 additions in any order ((1 + u)^(K+1) - 1 <= (K + 2) u for K <= 512), the products are
exact, and the factor 2 covers the matrix unit's undocumented order and rounding inside one instruction.  Through ELU, which is
1-Lipschitz, the error of the argument passes at most unchanged, and elu1 (csrc/go1ppo.hip) adds, at an argument t within e_z of z:
    t > 0                  nothing;
    -1e-3 < t <= 0         the series t + t^2 / 2 for expm1(t): the first omitted term |t|^3 / 6 (alternating series) plus two roundings,
                           2 u |t|;
    t <= -1e-3             __expf(t) - 1.  The ROCm documentation installed with the toolchain states no accuracy figure for __expf (no
                           document under the ROCm tree mentions it; the header declares __ocml_native_exp_f32 without a bound), so the
                           model is the fallback: 2 ulp of exp(t) (ulp(y) = 2^(floor(log2 y) - 23)) plus the rounding of the subtraction,
                           u |exp(t) - 1|.
Where t's branch is not decided (z within e_z of 0 or of -1e-3) the larger of the candidates is taken, evaluated at |z| + e_z.
The assertion is an interval on the rounded result, RNE_bf16(v - e) <= got <= RNE_bf16(v + e) as numbers; a NaN is outside every interval.
e is a worst case, so for many elements the interval admits the neighbouring bf16 value; therefore the share of elements with
got != RNE_bf16(v) is capped too.  The cap is measured on the reference, not on the kernel: `rounded_fp32` evaluates the same case with a
plain left-to-right fp32 accumulation of the same (exact) products, and the kernel's share over a case may be at most twice that
reference's share (the kernel adds 4 to 8 partial sums in an order nobody controls).

ELU-on-load and go1ppo_elu_fwd: the kernels evaluate s as a chain of npv fmaf's onto x.  Each rounds once, on a partial sum of magnitude at
most (|x| + sum |l w|)(1 + u)^npv:
    e_s = npv 2^-24 (|x| + sum_q |l_q w_q|)
(a factor (1 + u)^npv ~ 1 + 3e-7 below the count, which the elu1 term's own slack covers: it is counted at |s| + e_s) plus the elu1 bound
above, checked as an interval on the bf16 result as above.  e is far below a bf16 ulp here, so no share cap: instead the model asserts that
at most 1 % of a case's elements have an interval that holds two values (`two_valued`); the seeds (derived from the case names) satisfy
that, which tests/test_tail_fwd_ref.py checks without a GPU."""
from collections import namedtuple

import numpy as np

from ppo_rollout_ref import F32, F64, U, _rng, bf16_bits, bf16_is_nan, bf16_widen

ELU_SERIES_FROM = float(F32(-1e-3))             # elu1's branch point, as the kernel compares it
IN_GRID, W_GRID, B_GRID = 2.0 ** -2, 2.0 ** -3, 2.0 ** -2
JUNK = 0xC040                                   # -3.0: what the columns around an input block hold

# rows, dims = (k_in, n_1, ..., n_L), elu per layer, a power of two added to each layer's biases, the largest weight integer per layer,
# the input as columns [in_off, in_off + k_in) of a matrix with in_ld columns, every out with n_out + out_pad columns
Net = namedtuple("Net", "rows dims elu bias_base wmax in_off in_ld out_pad")
ExactCase = namedtuple("ExactCase", "name nets")
RoundedCase = namedtuple("RoundedCase", "name rows dims")
EluCase = namedtuple("EluCase", "name rows cols ld npv lat_cols lat_ld wz_ld")
# one net of an ELU-on-load launch: npv = 0: elu_in without a latent; lat_off / wz_off: elements past a 16-byte aligned place
LoadNet = namedtuple("LoadNet", "rows k npv lat_ld wz_ld lat_off wz_off")
LoadCase = namedtuple("LoadCase", "name nets")


def N(rows, *dims, elu=None, bias_base=None, wmax=None, in_off=0, in_ld=None, out_pad=0):
    L = len(dims) - 1
    return Net(rows, tuple(dims), tuple(elu or (0,) * L), tuple(bias_base or (0.0,) * L), tuple(wmax or (4, 4, 2, 1)[:L]), in_off,
               in_ld if in_ld is not None else dims[0] + in_off, out_pad)


# Which case covers which item of the kernel's structure (tests/test_tail_fwd_ref.py asserts the sets; profiles/tail_fwd_fp64.txt has the table):
#   k-steps 1, 2, 3, 4 (one fetch chunk)   k32-n16-r1, k64-n48-r31, k96-n64-r32, k128-n80-r33
#   k-steps 5, 8 (two chunks)              k160-n256-r65, k256-n272-r33         k-steps 9 (three): k288-n512-r31, k288-n80-r1
#   k-steps 16 (four chunks)               k512-n16-r65, k512-n512-r33
#   column tiles 1, 3 (idle waves)         k32-n16-r1, k64-n48-r31              4, 5 (a partly filled group): k96-n64-r32, k128-n80-r33
#   column tiles 16, 17, 32 (second pass)  k160-n256-r65, k256-n272-r33 (one tile in the second pass), k288-n512-r31 (sixteen)
#   rows 1, 31, 32, 33, 65                 the names say
#   2, 3, 4 layers                         l2-*, l3-*, l4-*                     ELU with pre-activations >= 0: elu-*
#   2 and 3 nets, shortest first / last    nets2-short-first, nets3-short-last, nets3-short-middle, nets2-equal
#   ld_in > k_in, column offset            in-block-*                           ld_out > n_out: out-pad-*
#   out == NULL on the intermediates       every case with more than one layer, in the GPU file's null-intermediates test
EXACT_CASES = [ExactCase(name, tuple(nets)) for name, nets in (
    ("k32-n16-r1", [N(1, 32, 16)]),
    ("k64-n48-r31", [N(31, 64, 48)]),
    ("k96-n64-r32", [N(32, 96, 64)]),
    ("k128-n80-r33", [N(33, 128, 80)]),
    ("k160-n256-r65", [N(65, 160, 256)]),
    ("k256-n272-r33", [N(33, 256, 272)]),
    ("k288-n512-r31", [N(31, 288, 512)]),
    ("k288-n80-r1", [N(1, 288, 80)]),
    ("k512-n16-r65", [N(65, 512, 16)]),
    ("k512-n512-r33", [N(33, 512, 512)]),
    ("k160-n48-r32", [N(32, 160, 48)]),
    ("k96-n272-r65", [N(65, 96, 272)]),
    ("l2-512-256-16-r33", [N(33, 512, 256, 16)]),
    ("l2-288-160-80-r31", [N(31, 288, 160, 80)]),
    ("l2-64-512-272-r32", [N(32, 64, 512, 272)]),
    ("l3-512-256-128-64-r65", [N(65, 512, 256, 128, 64)]),
    ("l3-160-96-288-48-r1", [N(1, 160, 96, 288, 48)]),
    ("l4-512-256-128-64-16-r33", [N(33, 512, 256, 128, 64, 16)]),
    ("l4-32-64-96-128-80-r65", [N(65, 32, 64, 96, 128, 80)]),
    ("elu-64-64-48-r33", [N(33, 64, 64, 48, elu=(1, 0), bias_base=(16.0, 0.0))]),
    ("elu-256-128-64-r65", [N(65, 256, 128, 64, elu=(1, 0), bias_base=(32.0, 0.0))]),
    ("elu-head-too-96-32-16-r31", [N(31, 96, 32, 16, elu=(1, 1), bias_base=(16.0, 512.0), wmax=(4, 2))]),
    ("nets2-short-first", [N(1, 32, 16), N(65, 128, 64, 48)]),
    ("nets3-short-last", [N(65, 256, 64, 32, 16), N(33, 96, 256, 80), N(31, 64, 16)]),
    ("nets3-short-middle", [N(33, 160, 272), N(1, 32, 48), N(65, 288, 64, 96, 16)]),
    ("nets2-equal", [N(33, 512, 256, 128, 64), N(33, 512, 256, 128, 64)]),
    ("in-block-off8-r33", [N(33, 128, 64, in_off=8, in_ld=160)]),
    ("in-block-off256-r65", [N(65, 512, 80, in_off=256, in_ld=1280), N(65, 512, 48, in_off=768, in_ld=1280)]),
    ("out-pad-3-r31", [N(31, 96, 64, 48, out_pad=3)]),
    ("out-pad-8-in-block-r32", [N(32, 64, 256, 272, in_off=16, in_ld=88, out_pad=8)]),
)]

# The fp32 reference differs from RNE_bf16(v) on about one element in 10^4, and twice its count is the kernel's cap: a case needs enough
# elements for that count to mean something.  So a rounded launch holds three nets of its shape (different data), and a case's name
# carries a seed suffix: the first of "", -s1, -s2, ... at which the REFERENCE's count is at least 4 (the kernel plays no part in it).
ROUNDED_CASES = [RoundedCase(f"rounded-{d[0]}-r{r}{s}", r, d) for d, r, s in (((512, 256, 128, 64), 33, ""), ((512, 256, 128, 64), 65, ""),
                                                                              ((256, 128, 64), 33, "-s2"), ((256, 128, 64), 65, "-s2"))]
ROUNDED_NETS = 3
ROUNDED_MIN_REFERENCE_COUNT = 4

# go1ppo_elu_fwd: rows {1, 63, 64, 65, 130} (64-row blocks), cols {8, 120, 128, 136} (128-column blocks) with ld > cols, npv {0 (no
# latent), 1, 2, 3, 5}, lat_cols {0, 8, half the columns (down to a multiple of 8), all}; npv == 2 needs even lat_ld / wz_ld here
ELU_CASES = [EluCase(f"elu-r{r}-c{c}-ld{ld}-npv{q}-lc{lc}", r, c, ld, q, lc, lat_ld, wz_ld) for r, c, ld, q, lc, lat_ld, wz_ld in (
    (1, 8, 16, 0, 0, 0, 0), (63, 120, 128, 1, 120, 1, 1), (64, 128, 136, 2, 64, 2, 2), (65, 136, 144, 3, 136, 3, 5),
    (130, 128, 1280, 2, 128, 64, 64), (130, 136, 144, 5, 64, 8, 5), (65, 120, 136, 2, 8, 4, 6), (63, 8, 24, 5, 8, 64, 64),
    (64, 136, 136 + 8, 1, 0, 3, 2), (1, 128, 256, 3, 64, 3, 3), (130, 120, 128, 0, 0, 0, 0), (65, 128, 136, 2, 56, 64, 2))]

# go1ppo_tail_fwd with elu_in: the lat2 dword path needs npv == 2, even lat_ld and wz_ld, 4-byte aligned latent and wz; anything else with a
# latent takes the general loop.  The first layer of every net is the identity (k x k, no bias, no ELU), whose stored output is the
# activated input itself; a random layer follows.
LOAD_CASES = [LoadCase(name, tuple(LoadNet(*n) for n in nets)) for name, nets in (
    ("lat2-r33-k128", [(33, 128, 2, 64, 64, 0, 0)]),
    ("lat2-r65-k32-tight", [(65, 32, 2, 2, 2, 0, 0)]),
    ("lat2-r1-k512", [(1, 512, 2, 64, 64, 2, 4)]),
    ("npv2-odd-lat-ld-r33-k64", [(33, 64, 2, 3, 64, 0, 0)]),
    ("npv2-odd-wz-ld-r65-k96", [(65, 96, 2, 64, 5, 0, 0)]),
    ("npv2-unaligned-latent-r31-k160", [(31, 160, 2, 64, 64, 1, 0)]),
    ("npv2-unaligned-wz-r32-k32", [(32, 32, 2, 4, 4, 0, 1)]),
    ("npv1-r63-k64", [(63, 64, 1, 1, 1, 0, 0)]),
    ("npv3-r64-k288", [(64, 288, 3, 64, 64, 0, 0)]),
    ("npv5-r65-k128", [(65, 128, 5, 5, 8, 0, 0)]),
    ("no-latent-r130-k256", [(130, 256, 0, 0, 0, 0, 0)]),
    ("latent-and-none-r33", [(33, 512, 2, 64, 64, 0, 0), (33, 512, 0, 0, 0, 0, 0)]),
    ("none-and-general-r65-r31", [(65, 64, 0, 0, 0, 0, 0), (31, 96, 3, 4, 3, 0, 0)]),
)]


def load_path(n):
    """the path tail_fwd_kernel takes for this net's latent term"""
    if n.npv == 0:
        return "none"
    return "lat2" if n.npv == 2 and n.lat_ld % 2 == 0 and n.wz_ld % 2 == 0 and n.lat_off % 2 == 0 and n.wz_off % 2 == 0 else "general"


# ------------------------------------------------------------------------------------------------------------------ bf16 helpers
def widen64(bits):
    return bf16_widen(bits).astype(F64)


def round_bf16(v):
    """float64 -> bf16 bit patterns.  The float64 -> fp32 step is exact for the exact cases (asserted by the caller) and rounds 29 bits
    below the bf16 rounding point otherwise: a double rounding only where v is within 2^-16 bf16 ulp of a tie, which the intervals absorb"""
    return bf16_bits(np.asarray(v, F64).astype(F32))


def ulp32(y):
    """2^(floor(log2 y) - 23) for y > 0"""
    return np.ldexp(1.0, np.frexp(y)[1] - 1 - 23)


# ------------------------------------------------------------------------------------------------------------------ the two operations
def elu64(x):
    x = np.asarray(x, F64)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))


def elu1_bound(z, e):
    """what elu1 may add to the error e of its argument z (see the module's docstring)"""
    z, e = np.asarray(z, F64), np.asarray(e, F64)
    t = np.abs(z) + e
    series = np.where((z + e > ELU_SERIES_FROM) & (z - e <= 0.0), t ** 3 / 6.0 + 2.0 * U * t, 0.0)
    lo = np.minimum(z + e, 0.0)                                    # the argument with the largest exp(t) among the candidates
    expo = np.where(z - e <= ELU_SERIES_FROM, 2.0 * ulp32(np.exp(lo)) + U * np.abs(np.expm1(z - e)), 0.0)
    return np.maximum(series, expo)


def layer(a_bits, W_bits, b_bits, elu):
    """act(a W^T + b) in float64 from bf16 bit patterns: (v, e), e the bound of the rounded family on v before its rounding to bf16"""
    a, W, b = widen64(a_bits), widen64(W_bits), widen64(b_bits)
    K = a.shape[1]
    assert W.shape[1] == K and b.shape == (W.shape[0],)
    z = a @ W.T + b
    mag = np.abs(a) @ np.abs(W).T + np.abs(b)
    e = 2.0 * (K + 2) * U * mag
    if not elu:
        return z, e
    return elu64(z), e + elu1_bound(z, e)


def elu_on_load(x_bits, lat_bits=None, wz_bits=None):
    """elu(x + latent wz^T) in float64: x [rows][k], latent [rows][npv], wz [k][npv] as bf16 bit patterns (latent None: plain ELU)"""
    x = widen64(x_bits)
    if lat_bits is None:
        s, e = x, np.zeros_like(x)
    else:
        lat, wz = widen64(lat_bits), widen64(wz_bits)
        npv = lat.shape[1]
        assert wz.shape == (x.shape[1], npv) and lat.shape[0] == x.shape[0]
        s = x + lat @ wz.T
        e = npv * U * (np.abs(x) + np.abs(lat) @ np.abs(wz).T)
    return elu64(s), e + elu1_bound(s, e)


# ------------------------------------------------------------------------------------------------------------------ comparing
def interval(v, e):
    """(lo, hi) as bf16 bit patterns"""
    return round_bf16(v - e), round_bf16(v + e)


def two_valued(v, e):
    """share of the elements whose interval holds more than one bf16 value"""
    lo, hi = interval(v, e)
    return float((bf16_widen(lo) != bf16_widen(hi)).mean())


def compare(got_bits, v, e):
    """(outside, mismatch): elements outside their interval (a NaN is outside), and elements that differ from RNE_bf16(v), as bool arrays"""
    got_bits = np.asarray(got_bits, np.uint16)
    assert got_bits.shape == v.shape, (got_bits.shape, v.shape)
    lo, hi = interval(v, e)
    g = bf16_widen(got_bits)
    with np.errstate(invalid="ignore"):
        inside = (bf16_widen(lo) <= g) & (g <= bf16_widen(hi)) & ~bf16_is_nan(got_bits)
        mismatch = ~(g == bf16_widen(round_bf16(v)))
    return ~inside, mismatch


def _towards(bits, up):
    """the neighbouring bf16 value (as bits), one step up or down in value; +0 and -0 are one value"""
    k = np.where(bits < 0x8000, bits.astype(np.int64), 0x8000 - bits.astype(np.int64))          # ordered like the values
    k = np.where(up, k + 1, k - 1)
    return np.where(k >= 0, k, 0x8000 - k).astype(np.uint16)


def ratio_to_bound(got_bits, v, e):
    """for the printed figures: the smallest error of the value before its rounding that explains `got`, over e.  0 where got is
    RNE_bf16(v); otherwise the distance from v to the edge of got's rounding cell (half way to got's neighbour on v's side); inf outside
    the interval"""
    got_bits = np.asarray(got_bits, np.uint16)
    outside, mismatch = compare(got_bits, v, e)
    if outside.any():
        return float("inf")
    g = widen64(got_bits)
    edge = 0.5 * (g + widen64(_towards(got_bits, g < v)))
    need = np.where(mismatch, np.abs(edge - v), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(need > 0, need / e, 0.0)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ exact cases
def _ints(g, lo, hi, shape, scale):
    return bf16_bits((g.integers(lo, hi + 1, shape) * scale).astype(F32))


def exact_inputs(c):
    """per net: the input matrix [rows][in_ld] (junk around the block), W_l, b_l as bf16 bit patterns"""
    nets = []
    for i, n in enumerate(c.nets):
        g = _rng(f"{c.name}/{i}")
        k0 = n.dims[0]
        assert n.in_off % 8 == 0 and n.in_ld % 8 == 0 and n.in_ld >= n.in_off + k0
        x = np.full((n.rows, n.in_ld), JUNK, np.uint16)
        x[:, n.in_off:n.in_off + k0] = _ints(g, -4, 4, (n.rows, k0), IN_GRID)
        W = [_ints(g, -m, m, (n.dims[l + 1], n.dims[l]), W_GRID) for l, m in enumerate(n.wmax)]
        b = [bf16_bits((g.integers(-4, 5, n.dims[l + 1]) * B_GRID + base).astype(F32)) for l, base in enumerate(n.bias_base)]
        nets.append(dict(net=n, x=x, W=W, b=b))
    return nets


def exact_layer(a_bits, W_bits, b_bits, elu, grid_in):
    """one layer of an exact case in int64: asserts the exactness condition, returns (out bits, the output's grid, max sum / 2^24)"""
    g = grid_in * W_GRID
    a, W, b = widen64(a_bits) / grid_in, widen64(W_bits) / W_GRID, widen64(b_bits) / g
    for t in (a, W, b):
        assert (t == np.rint(t)).all() and np.abs(t).max(initial=0) < 2.0 ** 53, "an operand is off the grid"
    a, W, b = a.astype(np.int64), W.astype(np.int64), b.astype(np.int64)
    mag = np.abs(a) @ np.abs(W).T + np.abs(b)
    assert mag.max() < 2 ** 24, f"sum |term| / grid = {mag.max()} >= 2^24: a partial sum may round"
    z = a @ W.T + b
    if elu:
        assert (z >= 0).all(), "an ELU layer of an exact case has a negative pre-activation"
    v = z.astype(F64) * g                                          # exact: |z| < 2^24
    assert (v.astype(F32).astype(F64) == v).all()
    out = round_bf16(v)
    assert (np.rint(widen64(out) / g) * g == widen64(out)).all()   # the rounded output stays on the grid
    return out, g, float(mag.max()) / 2 ** 24


def exact_model(d, variant=None):
    """outputs of every layer of one net (a dict of exact_inputs), as bf16 bit patterns.  `variant`: a deliberately wrong evaluation, in
    float64 on the same exact data: "drop_last_kstep" (the last 32 columns of every layer's input ignored) or "elu_on_head" (ELU on the last layer too)"""
    n = d["net"]
    a, grid = d["x"][:, n.in_off:n.in_off + n.dims[0]], IN_GRID
    outs = []
    for l in range(len(n.dims) - 1):
        want, grid_out, _ = exact_layer(a, d["W"][l], d["b"][l], n.elu[l], grid)
        if variant is None:
            out = want
        else:
            W = widen64(d["W"][l]).copy()
            if variant == "drop_last_kstep":
                W[:, -32:] = 0.0
            z = widen64(a) @ W.T + widen64(d["b"][l])
            last = l == len(n.dims) - 2
            out = round_bf16(elu64(z) if (n.elu[l] or (variant == "elu_on_head" and last)) else z)
        outs.append(out)
        a, grid = want, grid_out                                    # a wrong variant is judged layer by layer on right inputs
    return outs


# ------------------------------------------------------------------------------------------------------------------ rounded cases
def rounded_inputs(c):
    nets = []
    for i in range(ROUNDED_NETS):
        g = _rng(f"{c.name}/{i}")
        rnd = lambda *s, scale=1.0: bf16_bits((scale * g.standard_normal(s)).astype(F32))
        L = len(c.dims) - 1
        nets.append(dict(net=N(c.rows, *c.dims, elu=(1,) * (L - 1) + (0,)), x=rnd(c.rows, c.dims[0]),
                         W=[rnd(c.dims[l + 1], c.dims[l], scale=c.dims[l] ** -0.5) for l in range(L)],
                         b=[rnd(c.dims[l + 1], scale=0.1) for l in range(L)]))
    return nets


def elu1_fp32(x):
    """elu1 of csrc/go1ppo.hip in fp32 numpy (numpy's exp in place of the hardware's)"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        em = np.where(x > F32(-1e-3), (F32(0.5) * x * x).astype(F32) + x, np.exp(np.minimum(x, F32(0))).astype(F32) - F32(1))
    return np.where(x > 0, x, em).astype(F32)


def layer_fp32(a_bits, W_bits, b_bits, elu, variant=None):
    """the reference evaluation: the products (exact in fp32) added left to right in fp32, then the bias, elu1, RNE to bf16"""
    a, W, b = bf16_widen(a_bits), bf16_widen(W_bits), bf16_widen(b_bits)
    K = a.shape[1] - (32 if variant == "drop_last_kstep" else 0)
    acc = np.zeros((a.shape[0], W.shape[0]), F32)
    for k in range(K):
        acc += a[:, k:k + 1] * W[None, :, k]                       # fp32 product of two bf16 numbers: exact; the += rounds once
    z = acc + b
    return bf16_bits(elu1_fp32(z) if elu else z)


def chain_check(d, stored):
    """every layer of one net against the model, each from the stored output of the layer before: [(outside, mismatch, v, e)]"""
    n = d["net"]
    a = d["x"][:, n.in_off:n.in_off + n.dims[0]]
    res = []
    for l in range(len(n.dims) - 1):
        v, e = layer(a, d["W"][l], d["b"][l], n.elu[l])
        outside, mismatch = compare(stored[l], v, e)
        res.append((outside, mismatch, v, e))
        a = stored[l]
    return res


def rounded_fp32(d, variant=None):
    """the fp32 left-to-right chain of one net, every layer from its own stored output of the layer before.  `variant`:
    "drop_last_kstep" or "elu_on_head", as in exact_model"""
    n = d["net"]
    a, outs = d["x"], []
    L = len(n.dims) - 1
    for l in range(L):
        elu = n.elu[l] or (variant == "elu_on_head" and l == L - 1)
        outs.append(layer_fp32(a, d["W"][l], d["b"][l], elu, variant if variant == "drop_last_kstep" else None))
        a = outs[-1]
    return outs


def elements(nets):
    return sum(d["net"].rows * sum(d["net"].dims[1:]) for d in nets)


def shares(nets, stored):
    """over the nets of a case (stored[i][l]: net i's layer l as bf16 bits): (elements outside, mismatch share, largest ratio)"""
    outside = mism = total = 0
    worst = 0.0
    for d, st in zip(nets, stored):
        for (o, m, v, e), got in zip(chain_check(d, st), st):
            outside, mism, total = outside + int(o.sum()), mism + int(m.sum()), total + m.size
            worst = max(worst, ratio_to_bound(got, v, e))
    return outside, mism / total, worst


_REFERENCE_SHARE = {}


def reference_share(c):
    """the mismatch share of the fp32 left-to-right reference on a rounded case: the kernel's cap is twice this"""
    if c.name not in _REFERENCE_SHARE:
        nets = rounded_inputs(c)
        outside, share, _ = shares(nets, [rounded_fp32(d) for d in nets])
        assert outside == 0, "the fp32 reference itself leaves the bounds"
        _REFERENCE_SHARE[c.name] = share
    return _REFERENCE_SHARE[c.name]


# ------------------------------------------------------------------------------------------------------------------ ELU families
def _latent_data(g, rows, cols, npv, lat_ld, wz_ld):
    """latent [rows][lat_ld] and wz [cols][wz_ld]: the first npv columns are data (the latent of size 1, the weights 0.3), the rest junk"""
    lat = np.full((rows, max(lat_ld, 1)), JUNK, np.uint16)
    wz = np.full((cols, max(wz_ld, 1)), JUNK, np.uint16)
    lat[:, :npv] = bf16_bits(g.standard_normal((rows, npv)).astype(F32))
    wz[:, :npv] = bf16_bits((0.3 * g.standard_normal((cols, npv))).astype(F32))
    return lat, wz


def _preactivations(g, rows, cols):
    """N(0, 1.5^2) with a tenth of the elements inside the series branch's range (|x| below 1e-3, both signs) and a few exact zeros"""
    x = (1.5 * g.standard_normal((rows, cols))).astype(F32)
    k = g.random((rows, cols))
    x[k < 0.1] = (1e-3 * g.standard_normal((rows, cols))).astype(F32)[k < 0.1]
    x[k < 0.01] = 0.0
    return bf16_bits(x)


def elu_inputs(c):
    g = _rng(c.name)
    assert c.ld > c.cols and c.cols % 8 == 0 and c.ld % 8 == 0 and c.lat_cols % 8 == 0 and c.lat_cols <= c.cols
    assert c.npv == 0 or (c.lat_ld >= c.npv and c.wz_ld >= c.npv and (c.npv != 2 or (c.lat_ld % 2 == 0 and c.wz_ld % 2 == 0)))
    y = np.full((c.rows, c.ld), JUNK, np.uint16)
    y[:, :c.cols] = _preactivations(g, c.rows, c.cols)
    lat, wz = _latent_data(g, c.rows, c.cols, c.npv, c.lat_ld, c.wz_ld) if c.npv else (None, None)
    return dict(case=c, y=y, lat=lat, wz=wz)


def elu_model(d):
    """(v, e) over the [rows][cols] block: the latent term on the columns below lat_cols only"""
    c = d["case"]
    x = d["y"][:, :c.cols]
    v, e = elu_on_load(x)
    if c.npv and c.lat_cols:
        vl, el = elu_on_load(x[:, :c.lat_cols], d["lat"][:, :c.npv], d["wz"][:c.lat_cols, :c.npv])
        v, e = v.copy(), e.copy()
        v[:, :c.lat_cols], e[:, :c.lat_cols] = vl, el
    return v, e


def load_inputs(c):
    """per net: pre-activations x [rows][k + 8] (the block is the first k columns), latent, wz, and the random layer behind the identity"""
    nets = []
    for i, n in enumerate(c.nets):
        g = _rng(f"{c.name}/{i}")
        x = np.full((n.rows, n.k + 8), JUNK, np.uint16)
        x[:, :n.k] = _preactivations(g, n.rows, n.k)
        lat, wz = _latent_data(g, n.rows, n.k, n.npv, n.lat_ld, n.wz_ld) if n.npv else (None, None)
        eye = bf16_bits(np.eye(n.k, dtype=F32))
        W2 = bf16_bits((g.standard_normal((48, n.k)) * n.k ** -0.5).astype(F32))
        b2 = bf16_bits((0.1 * g.standard_normal(48)).astype(F32))
        nets.append(dict(net=n, x=x, lat=lat, wz=wz, W=[eye, W2], b=[np.zeros(n.k, np.uint16), b2]))
    return nets


def load_model(d):
    n = d["net"]
    x = d["x"][:, :n.k]
    return elu_on_load(x, d["lat"][:, :n.npv], d["wz"][:, :n.npv]) if n.npv else elu_on_load(x)


def elu_fp32(x_bits, lat_bits=None, wz_bits=None):
    """the kernels' statements in fp32 numpy: the fmaf chain evaluated in float64 and rounded to fp32 after every step (a product of two
    bf16 numbers plus an fp32 number is exact in float64 unless the exponents lie more than 29 bits apart), elu1, RNE to bf16"""
    s = bf16_widen(x_bits)
    if lat_bits is not None:
        lat, wz = widen64(lat_bits), widen64(wz_bits)
        for q in range(lat.shape[1]):
            s = (s.astype(F64) + lat[:, q:q + 1] * wz[None, :, q]).astype(F32)
    return bf16_bits(elu1_fp32(s))
