"""Cases, reference and criterion for K1, the colored-noise sampler every iCEM pool comes from (philox.h::box_muller, fused_dev.h::
row_normals / row_synth and their quad forms, the folded kernels of k_sample.hip, the generic thread and quad kernels of
generic_kernels.hip / generic_dev.h, and every fused carrier that promises sample_row's bits), shared by
test_noise_sensitivity_cpu.py and test_gpu_noise_probes.py (a plain module, no fixtures).

Why a table of its own.  test_philox_normals_match_oracle compares 37 rows of the stream's own draws at 4e-6 with the NumPy
float32 formula and samples them under a CONSTANT mean 0 / std 0.5; every other view of the sampler is a whole MPC step fed with
the device's own normals.  No draw there reaches the edges of the f32 formula (u1 next to 0, next to 1, exactly 1.0f, v == 1.0f,
angles next to a quarter turn), nothing compares the folded synthesis per sample, and a mean / std read at j h + t instead of
t d + j changes nothing a constant table can show.

Reference.  float64, from oracle/icem_oracle.py alone: the words of row (global trajectory, dim) from philox4x32 +
xoshiro128pp_words; the normals float64 Box-Muller ON THE DEVICE'S INPUTS (f32: u1 = fma(float(xa), 2^-32, 2^-33) and
v = float(xb) 2^-32, rounded as the kernel rounds them, then widened; f64: the f64 kernel text, oracle.box_muller); the samples
z_r @ Cr + z_i @ Ci with synthesis_matrices; the action clip(mean + std y) on the dtype-rounded mean, std, low, high.
test_noise_sensitivity_cpu.py holds it to colored_from_white (the irfft form, an independent path) at 1e-12 on the whole table.

Criterion, per entry, nothing left out (the clip is continuous), no NaN:
    f32 normals   |g_dev - g_ref| <= E_g,                                  E_g = min(8 x RESTATEMENT_DG_F32, 4e-6)
    f32 samples   |a_dev - a_ref| <= std[t, j] E_y + eps32 |a_ref|,        E_y = min(8 x RESTATEMENT_DY_F32, 1e-5)
    f64           normals 1e-12 absolute, samples 1e-11 max(1, |a_ref|)    (the project's existing bars)
The restatement below is NumPy float32, rounded wherever the device rounds, every transcendental CORRECTLY rounded (float64's,
rounded once); its samples run in the folded summation order (e0 / e1 / o0 / o1 as row_synth forms them).  Its worst distance
from the reference over THIS table, planted rows included (test_the_restatement_is_as_good_as_the_header_says):
    RESTATEMENT_DG_F32 = 4.27e-7  (measured 4.261e-7, on the planted xa = 181 row, |g| = 5.8: an ulp of a value in [4, 8) is 4.77e-7)
    RESTATEMENT_DY_F32 = 6.15e-7  (measured 6.149e-7 on 30x6x43-b3-open, in units of std, eps32 |a_ref| taken off first)
so E_g = 3.42e-6 and E_y = 4.92e-6.  4e-6 and 1e-5 are the bars of test_philox_normals_match_oracle and the most this check may
grant; 8 x is the allowance for the hardware's v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32 (about an ulp each where the
restatement's are half an ulp) and for the kernels' other summation orders (direct sum, generic quad form).
MI355X, this table, measured (EXPERIMENTS R21.1; for the record, nothing is asserted against a number taken from the device):
    normals f32   6.25e-7 at worst on the table's keys (0.18 of E_g); planted: xa < 2^10 4.26e-7 (the restatement's own figure),
                  xa >= 2^32 - 2^10 3.2e-11 (v_log_f32 next to 1 delivers the difference with relative accuracy), u1 == 1.0f
                  exactly +-0, v == 1.0f 6.0e-8, the quarter turns 3.2e-8 / 2.4e-8 / 5.9e-8 / 1.4e-7;  f64 4.4e-16
    samples f32   folded kernel 5.83e-7 (0.12 of E_y; the restatement's 6.15e-7 on the same case), generic thread form 1.01e-6
                  (h = 64: a direct sum of 64 terms), generic quad form 3.4e-7, every fused carrier at most 5.8e-7 and the
                  operator's bits;  f64 2.6e-15 of a std

Distributions.  Every (t, j) carries a value of its own in mean and in std, so t d + j read as j h + t, or a t off by one, moves
an entry; the boxes are asymmetric per dimension.  "open": bounds beyond +-100, no clip, every sample readable.  "tight": a
quarter of the samples clipped on each side.  row0_mean runs with first_index == 0 and with first_index > 0 (where it must not
apply).

Shapes (h, d, n): the smallest that reach each code path (SWG = WG = 256).
  folded sampler (f32, h in {30, 12, 13, 10}):
    (10, 1, 300)   d = 1, two workgroups                       (12, 6, 45)   42 rows / workgroup, four idle threads, a ragged
    (13, 3, 90)    odd H, h d = 39: scalar copy-out, an unused                second workgroup; H/2 even: the Q/2 row
                   second normal of the last pair              (30, 6, 43)
    (30, 17, 16)   h d = 510: scalar copy-out                  (30, 18, 15)  h d = 540 > 512: the staging tail loop
    (30, 64, 5)    the largest d the handle accepts, four rows per workgroup
  generic sampler (other horizons; f32 and f64; thread form and quad form, option gk_sample 0 / 1):
    (2, 1, 5)  (5, 3, 90)  (32, 4, 70)  (33, 2, 10): HMAX = 64  (64, 3, 7);  t_begin = h - 1 on (32, 4, 70)
beta: 0 (white), 0.25, 1, 3 on every folded horizon, 0.25 elsewhere; rng_rounds 7 on (30, 6, 43) and (5, 3, 90).
Stream keys: seed 0xDEADBEEFCAFE1234, offset (5 << 32) | 17, first_index 1000; first_index 3 000 000 017 (> 2^31) on (13, 3, 90)
and (5, 3, 90); first_index 0 where row0_mean has to apply.

Planted draws.  The device draws its own words, so the edges are coordinates whose stream has them: scan_planted() searches rows
with the oracle's integer side (18 s per 2^20 rows: run when the constants are made, not in the tests), PLANTED records what it
found at seed 11, offset 1, h = 30, d = 6 in the first 2^20 rows, the CPU test re-derives every one.  Each is drawn with
first_index = its row - 1, n = 3, at "open".
"""
from collections import namedtuple

import numpy as np

from oracle import icem_oracle as O

DTYPES = {"f32": np.float32, "f64": np.float64}
RESTATEMENT_DG_F32 = 4.27e-7   # the f32 restatement's worst |g - g_ref| over the table (measured 4.261e-7)
RESTATEMENT_DY_F32 = 6.15e-7   # ... worst (|a - a_ref| - eps32 |a_ref|) / std, folded order (measured 6.149e-7)
E_G_F32 = min(8 * RESTATEMENT_DG_F32, 4e-6)
E_Y_F32 = min(8 * RESTATEMENT_DY_F32, 1e-5)
E_G_F64, E_Y_F64 = 1e-12, 1e-11
DEVICE_DG_F32 = 6.25e-7        # MI355X, for the record (header): nothing is asserted against these
DEVICE_DY_F32 = 1.01e-6        # (the generic thread form at h = 64; the folded kernel 5.83e-7)
EPS32 = float(np.finfo(np.float32).eps)

SEED, OFFSET, FIRST = 0xDEADBEEFCAFE1234, (5 << 32) | 17, 1000
FIRST_HIGH = 3_000_000_017     # above 2^31 (and above 2^31 as a signed 32-bit value: negative)
FOLDED_H = (30, 12, 13, 10)    # ICEM_FAST_HORIZONS: the compiled horizons of the folded sampler
SWG = WG = 256
BETAS = (0.0, 0.25, 1.0, 3.0)

Case = namedtuple("Case", "name h d n beta rounds dist first row0 t_begin seed offset")


def _case(h, d, n, beta=0.25, rounds=10, dist="open", first=FIRST, row0=False, t_begin=0, seed=SEED, offset=OFFSET, tag=""):
    name = f"{h}x{d}x{n}-b{beta:g}-{dist}" + ("-r7" if rounds == 7 else "") + ("-row0" if row0 else "") + \
        (f"-first{first}" if first != FIRST else "") + (f"-t{t_begin}" if t_begin else "") + tag
    return Case(name, h, d, n, beta, rounds, dist, first, row0, t_begin, seed, offset)


FOLDED_SHAPES = [(10, 1, 300), (12, 6, 45), (13, 3, 90), (30, 6, 43), (30, 17, 16), (30, 18, 15), (30, 64, 5)]
GENERIC_SHAPES = [(2, 1, 5), (5, 3, 90), (32, 4, 70), (33, 2, 10), (64, 3, 7)]

FOLDED_CASES = [_case(h, d, n, dist=dist) for h, d, n in FOLDED_SHAPES for dist in ("open", "tight")]
FOLDED_CASES += [_case(h, d, n, beta=b) for h, d, n in FOLDED_SHAPES[:4] for b in BETAS if b != 0.25]
FOLDED_CASES += [
    _case(30, 6, 43, rounds=7),
    _case(12, 6, 45, first=0, row0=True), _case(12, 6, 45, row0=True),            # row0_mean applies / must not apply
    _case(30, 18, 15, first=0, row0=True, dist="tight"),                           # ... copied from the stage's tail as well
    _case(13, 3, 90, first=FIRST_HIGH),
]
GENERIC_CASES = [_case(h, d, n, dist=dist) for h, d, n in GENERIC_SHAPES for dist in ("open", "tight")]
GENERIC_CASES += [
    _case(5, 3, 90, rounds=7),
    _case(32, 4, 70, t_begin=31),                                                  # what shift_sample_batch_kernel shares
    _case(33, 2, 10, first=0, row0=True), _case(33, 2, 10, row0=True),
    _case(5, 3, 90, first=FIRST_HIGH),
]
# the generic kernels also serve the folded horizons in f64 (the strict-parity sampler): one case per HMAX is GENERIC's own
F64_FOLDED_H_CASES = [_case(30, 6, 43, tag="-f64"), _case(13, 3, 90, dist="tight", tag="-f64")]
CASES = FOLDED_CASES + GENERIC_CASES
BY_NAME = {c.name: c for c in CASES + F64_FOLDED_H_CASES}

# ---- planted draws -----------------------------------------------------------------------------------------------------------
P_SEED, P_OFFSET, P_H, P_D = 11, 1, 30, 6
QUARTERS = (0, 1 << 30, 1 << 31, 3 << 30)
# class -> [(global row, dim, pair, word)]: the word is xa of the pair for the xa / u1 classes, xb for the others
PLANTED = {
    "xa_small": [(98, 5, 4, 181), (12921, 0, 0, 791), (27324, 4, 12, 267)],            # u1 next to 0: |g| up to 5.8
    "xa_large": [(50490, 0, 12, 4294966612), (87326, 4, 8, 4294966544), (393670, 0, 0, 4294967133)],   # u1 next to 1
    "u1_one": [(62543, 2, 14, 4294967265), (64755, 1, 4, 4294967180), (516108, 5, 0, 4294967222),
               (561619, 0, 0, 4294967178)],                                            # xa >= 0xFFFFFF80: u1 == 1.0f, g = +-0
    "v_one": [(119010, 3, 8, 4294967267), (616667, 2, 14, 4294967273)],               # xb >= 0xFFFFFF80: v == 1.0f
    "quarter0": [(19722, 4, 7, 7), (86074, 2, 3, 4294966564), (98898, 1, 6, 683)],     # xb within 2^10 of a quarter turn
    "quarter1": [(42045, 0, 12, 1073742845), (59696, 2, 8, 1073742797), (70228, 3, 4, 1073742033)],
    "quarter2": [(20836, 4, 2, 2147483027), (37949, 3, 9, 2147482871), (44414, 3, 0, 2147483619)],
    "quarter3": [(14922, 1, 8, 3221225508), (32951, 0, 9, 3221224903), (70526, 1, 0, 3221224681)],
}
PLANTED_N = 3   # rows row - 1, row, row + 1


def planted_class(cls, xa, xb):
    """Is the pair (xa, xb) of class ``cls``?  (integers)"""
    if cls == "xa_small":
        return xa < 1 << 10
    if cls == "xa_large":
        return (1 << 32) - (1 << 10) <= xa < 0xFFFFFF80
    if cls == "u1_one":
        return xa >= 0xFFFFFF80
    if cls == "v_one":
        return xb >= 0xFFFFFF80
    c = QUARTERS[int(cls[-1])]
    dist = abs(xb - c) if c else min(xb, (1 << 32) - xb)
    return dist < 1 << 10 and xb < 0xFFFFFF80


def planted_cases():
    """One "open" case of PLANTED_N rows around every planted coordinate -> [(class, coordinate, Case)]."""
    out = []
    for cls, coords in PLANTED.items():
        for row, dim, pair, word in coords:
            c = _case(P_H, P_D, PLANTED_N, first=row - 1, seed=P_SEED, offset=P_OFFSET, tag=f"-{cls}")
            out.append((cls, (row, dim, pair, word), c))
    return out


def scan_planted(rows=1 << 20, seed=P_SEED, offset=P_OFFSET, h=P_H, d=P_D, chunk=1 << 16):
    """The search that made PLANTED: every pair of rows [0, rows) of the stream, by class -> {class: [(row, dim, pair, word)]}."""
    hits = {}
    for base in range(0, rows, chunk):
        w = stream_words(seed, offset, base, min(chunk, rows - base), d, h).astype(np.int64)
        xa, xb = w[..., 0::2], w[..., 1::2]
        near = [np.abs(xb - c) if c else np.minimum(xb, (1 << 32) - xb) for c in QUARTERS]
        masks = {"xa_small": (xa < 1 << 10, xa), "xa_large": ((xa >= (1 << 32) - (1 << 10)) & (xa < 0xFFFFFF80), xa),
                 "u1_one": (xa >= 0xFFFFFF80, xa), "v_one": (xb >= 0xFFFFFF80, xb)}
        masks.update({f"quarter{q}": ((near[q] < 1 << 10) & (xb < 0xFFFFFF80), xb) for q in range(4)})
        for cls, (mask, src) in masks.items():
            for r, j, p in zip(*np.nonzero(mask)):
                hits.setdefault(cls, []).append((base + int(r), int(j), int(p), int(src[r, j, p])))
    return hits


# ---- distributions -----------------------------------------------------------------------------------------------------------
def box(d, dist, dtype):
    j = np.arange(d)
    if dist == "open":
        return (-100.0 - j).astype(dtype), (100.0 + 0.5 * j).astype(dtype)
    return (-0.7 - 0.13 * j).astype(dtype), (0.9 + 0.07 * j).astype(dtype)


def distribution(case, dtype):
    """-> low, high [d], mean, std [h, d] of ``dtype``: every (t, j) its own value in mean and in std."""
    h, d = case.h, case.d
    low, high = box(d, case.dist, dtype)
    lo, hi = box(d, "tight", np.float64)
    lo, hi = lo[None], hi[None]
    e = np.arange(h * d, dtype=np.float64).reshape(h, d)
    wob, wob2 = np.sin(1.0 + e), np.cos(2.0 + 0.7 * e)
    mean = (lo + hi) / 2 + 0.05 * (hi - lo) / 2 * wob
    if case.dist == "open":
        std = (hi - lo) / 2 * 0.5 * (1 + 0.4 * wob2)          # 0.24 .. 0.9: the planner's own range (init_std 0.5)
    else:
        std = (hi - lo) / 2 / 0.6745 * (1 + 0.1 * wob2)       # the box's half width is the upper quartile of std |y|
    return low, high, np.ascontiguousarray(mean.astype(dtype)), np.ascontiguousarray(std.astype(dtype))


# ---- reference ---------------------------------------------------------------------------------------------------------------
def w64(x):
    return np.asarray(x).astype(np.float64)


def stream_words(seed, offset, first, n, d, h, rounds=10, count=None, dim_shift=16, swap_offset=False):
    """Words [n, d, count] (uint64 holding uint32) of rows first .. first + n: the oracle's integer side, keyed as the device
    keys it (the global row as an unsigned 32-bit counter word).  ``dim_shift`` / ``swap_offset``: the key faults of the
    sensitivity suite."""
    count = 2 * ((h + 1) // 2) if count is None else count
    gi = ((first + np.arange(n, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint64)
    n_idx = np.broadcast_to(gi[:, None], (n, d))
    j_idx = np.broadcast_to((np.arange(d, dtype=np.uint64) << np.uint64(dim_shift))[None, :], (n, d))
    o_lo, o_hi = offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF
    if swap_offset:
        o_lo, o_hi = o_hi, o_lo
    s = O.philox4x32(n_idx, j_idx, o_lo, o_hi, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, rounds)
    return np.stack(O.xoshiro128pp_words(*s, count), axis=-1)


def device_inputs_f32(xa, xb):
    """(u1, v) of the f32 box_muller as the kernel rounds them, widened: fma(float(xa), 2^-32, 2^-33) is exact in float64
    before its one rounding, float(xb) 2^-32 is a power-of-two scaling."""
    u1 = (xa.astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)
    v = xb.astype(np.float32) * np.float32(2.0 ** -32)
    return u1.astype(np.float64), v.astype(np.float64)


def reference_normals(words, h, dtype):
    """float64 normals [n, d, h] in draw order from the words [n, d, >= 2 ceil(h / 2)]."""
    npairs = (h + 1) // 2
    xa, xb = words[..., 0:2 * npairs:2], words[..., 1:2 * npairs:2]
    if dtype is np.float64:
        g0, g1 = O.box_muller(xa, xb, np.float64)
    else:
        u1, v = device_inputs_f32(xa, xb)
        r = np.sqrt(-2.0 * np.log(u1)) + 0.0      # (+ 0.0: u1 == 1 gives -0.0 under the root)
        g0, g1 = r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v)
    g = np.empty(xa.shape[:-1] + (2 * npairs,))
    g[..., 0::2], g[..., 1::2] = g0, g1
    return g[..., :h]


def split_normals(g, h):
    """Draw order [n, d, h] -> (z_r, z_i) [n, d, F] as icem_philox_normals returns them (unused imaginary slots 0)."""
    F = h // 2 + 1
    z_i = np.zeros(g.shape[:-1] + (F,), dtype=g.dtype)
    z_i[..., 1:1 + h - F] = g[..., F:]
    return np.ascontiguousarray(g[..., :F]), z_i


def reference_samples(g, h, beta):
    """y [n, h, d] in float64 from the float64 normals [n, d, h]: z_r @ Cr + z_i @ Ci (beta <= 0: the draws themselves)."""
    if beta <= 0:
        return np.ascontiguousarray(g.transpose(0, 2, 1))
    Cr, Ci = O.synthesis_matrices(h, beta)
    z_r, z_i = split_normals(g, h)
    return np.ascontiguousarray((z_r @ Cr + z_i @ Ci).transpose(0, 2, 1))


def reference_actions(y, mean, std, low, high, row0=False):
    a = np.clip(w64(mean)[None] + w64(std)[None] * y, w64(low)[None, None], w64(high)[None, None])
    if row0:
        a[0] = w64(mean)
    return a


def reference(case, dtype, tables=None):
    """-> dict(low, high, mean, std of ``dtype``; words; g [n, d, h], y, a [n, h, d] float64) of one case (``tables``: another
    (low, high, mean, std) than the case's own)."""
    low, high, mean, std = distribution(case, dtype) if tables is None else tables
    words = stream_words(case.seed, case.offset, case.first, case.n, case.d, case.h, case.rounds)
    g = reference_normals(words, case.h, dtype)
    y = reference_samples(g, case.h, case.beta)
    a = reference_actions(y, mean, std, low, high, case.row0 and case.first == 0)
    return dict(low=low, high=high, mean=mean, std=std, words=words, g=g, y=y, a=a)


# ---- criterion ---------------------------------------------------------------------------------------------------------------
def normals_miss(g_dev, g_ref, dtype, bound=None):
    """By what factor the worst normal misses its bound (<= 1: accepted); inf for a NaN or an infinity."""
    g_dev = w64(g_dev)
    if g_dev.shape != g_ref.shape or not np.isfinite(g_dev).all():
        return np.inf
    e = bound if bound is not None else (E_G_F64 if dtype is np.float64 else E_G_F32)
    return float((np.abs(g_dev - g_ref) / e).max())


def samples_miss(a_dev, a_ref, std, dtype):
    """By what factor the worst sample / action misses its bound (<= 1: accepted); inf for a NaN or an infinity."""
    a_dev = w64(a_dev)
    if a_dev.shape != a_ref.shape or not np.isfinite(a_dev).all():
        return np.inf
    if dtype is np.float64:
        return float((np.abs(a_dev - a_ref) / (E_Y_F64 * np.maximum(1.0, np.abs(a_ref)))).max())
    tiny = np.finfo(np.float64).tiny
    return float((np.abs(a_dev - a_ref) / (w64(std)[None] * E_Y_F32 + EPS32 * np.abs(a_ref) + tiny)).max())


def samples_error(a_dev, a_ref, std, eps=EPS32):
    """The worst (|a_dev - a_ref| - eps |a_ref|) / std: the error in units of y, for the record and for the restatement (eps:
    the one rounding of the closing multiply-add; 0 for f64, whose bar is not of this form)."""
    s = w64(std)[None] + 0 * a_ref
    err = np.abs(w64(a_dev) - a_ref) - eps * np.abs(a_ref)
    on = s > 0
    return float((err[on] / s[on]).max())


# ---- the restatement: the kernels' text in NumPy float32, rounded where the device rounds; every keyword is one fault -------------
F32 = np.float32


def fma32(a, b, c):
    """round(a b + c) once: the product of two f32 is exact in float64, the sum's float64 rounding comes first (2^-29 ulp)."""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
            + np.asarray(c, F32).astype(np.float64)).astype(F32)


def normals_standin(words, h, swap_ab=False, second="own", shift_last_odd=False, no_half=False):
    """row_normals -> f32 normals [n, d, 2 ceil(h / 2)] in slot order (pair i -> slots 2 i, 2 i + 1; an odd h leaves the last
    slot unused).  log2, sqrt, sin, cos are float64's rounded once.  ``second``: "own" | "dropped" (pair i fills slot i alone:
    the row runs through h pairs) | "duplicated" (slot 2 i + 1 repeats slot 2 i)."""
    npairs = (h + 1) // 2
    use = h if second == "dropped" else npairs
    assert words.shape[-1] >= 2 * use + (1 if shift_last_odd else 0)
    xa, xb = words[..., 0:2 * use:2].copy(), words[..., 1:2 * use:2].copy()
    if shift_last_odd and h % 2:     # the last pair of an odd h starts one word late
        xa[..., npairs - 1], xb[..., npairs - 1] = words[..., 2 * npairs - 1], words[..., 2 * npairs]
    if swap_ab:
        xa, xb = xb, xa
    xa32 = xa.astype(F32)
    u1 = (xa32 * F32(2.0 ** -32)).astype(F32) if no_half else \
        (xa32.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(F32)
    v = xb.astype(F32) * F32(2.0 ** -32)
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.log2(u1.astype(np.float64)).astype(F32)
        r = np.sqrt((F32(-1.3862943611198906) * lg).astype(np.float64)).astype(F32)
        c = np.cos(2.0 * np.pi * v.astype(np.float64)).astype(F32)
        s = np.sin(2.0 * np.pi * v.astype(np.float64)).astype(F32)
        g0, g1 = (r * c).astype(F32), (r * s).astype(F32)
    if second == "dropped":
        g = np.zeros(xa.shape[:-1] + (2 * npairs,), F32)
        g[..., :h] = g0
        return g
    g = np.empty(xa.shape[:-1] + (2 * npairs,), F32)
    g[..., 0::2], g[..., 1::2] = g0, (g0 if second == "duplicated" else g1)
    return g


def quad_pair_lane(pair):
    """row_normals_quad: pair 4 k + q of group k is transformed by lane q."""
    return pair % 4


def table(h, beta, hmax=None, dtype=F32, sigma_of="own", beta_full=False, nyquist2=False, dc2=False, imag_shift=0, scale=None):
    """The synthesis table W[t][m] [h, HMAX] of ``dtype`` (icem_create): m < F the real part of bin m, F <= m < h the imaginary
    part of bin m - F + 1; beta <= 0: the identity.  Faults: ``sigma_of`` "even" / "odd" (the Nyquist bin's share of sigma taken
    as an even / odd horizon's; "odd" at an even h is what keeping the Nyquist bin's imaginary draw comes to: its weight
    sin(pi t) is zero, its power is not), ``beta_full`` (f^-beta for f^-beta/2), ``nyquist2`` / ``dc2`` (weight 2 for 1),
    ``imag_shift`` (bin m - F + 1 + shift), ``scale`` ((t, m, factor))."""
    hmax = (32 if h <= 32 else 64) if hmax is None else hmax
    F = h // 2 + 1
    W = np.zeros((h, hmax))
    if beta <= 0:
        W[np.arange(h), np.arange(h)] = 1.0
    else:
        f = np.fft.rfftfreq(h)
        s = f.copy()
        s[0] = s[1]
        s = s ** (-beta if beta_full else -beta / 2.0)
        wgt = s[1:].copy()
        odd = {"own": h % 2, "even": 0, "odd": 1}[sigma_of]
        wgt[-1] *= (1 + odd) / 2.0
        sigma = 2.0 * np.sqrt(np.sum(wgt ** 2)) / h
        k, t = np.arange(F, dtype=np.float64)[:, None], np.arange(h, dtype=np.float64)[None, :]
        ang = 2.0 * np.pi * k * t / h
        mult = np.full((F, 1), 2.0)
        mult[0, 0] = 2.0 if dc2 else 1.0
        if h % 2 == 0:
            mult[F - 1, 0] = 2.0 if nyquist2 else 1.0
        amp = mult * s[:, None] / (h * sigma)
        Cr, Ci = amp * np.cos(ang), -amp * np.sin(ang)
        Ci[0] = 0.0
        if h % 2 == 0:
            Ci[F - 1] = 0.0
        W[:, :F] = Cr.T
        for m in range(F, h):
            kk = m - F + 1 + imag_shift
            W[:, m] = Ci[kk] if 0 <= kk < F else 0.0
    if scale is not None:
        W[scale[0], scale[1]] *= scale[2]
    return np.ascontiguousarray(W.astype(dtype))


def folded_rows(h, lane=None, lane_takes=None):
    """The table rows row_synth runs, in order: [(tp, four)].  ``lane`` = q: the rows row_synth_quad deals to lane q
    ("zero": t = 0 is lane 3's); ``lane_takes`` = (q, q'): lane q runs lane q''s rows instead of its own."""
    Q = h // 2
    if h % 2 == 0:
        rows = [(tp, True) for tp in range(1, (Q - 1) // 2 + 1)]
        if Q % 2 == 0:
            rows.append((Q // 2, False))
    else:
        rows = [(tp, False) for tp in range(1, h // 2 + 1)]
    if lane is None:
        return rows

    def of(q):
        if h % 2 == 0:
            mine = [(tp, True) for tp in range(q + 1, (Q - 1) // 2 + 1, 4)]
            if Q % 2 == 0 and q == ((Q - 1) // 2) % 4:
                mine.append((Q // 2, False))
            return mine
        return [(tp, False) for tp in range(q + 1, h // 2 + 1, 4)]
    return of(lane_takes[1] if lane_takes is not None and lane == lane_takes[0] else lane)


def synth_folded(g, W, h, white=False, stride=None, swap_q=False, od_sign=1, dd_sign=1, q2="once", quad=False, lane_takes=None):
    """row_synth (``quad``: row_synth_quad, the same operations dealt over four lanes) -> y [..., h] f32 from the slots
    g [..., >= h] and the table W (flat reads at tp * stride + m).  Faults: ``stride`` (H for HMAX), ``swap_q`` (the outputs
    Q - tp and Q + tp exchanged), ``od_sign`` / ``dd_sign``, ``q2`` "skipped" / "four" (the Q/2 row left out / run as a
    four-output row: the latter is NOT a fault, the extra outputs are its own), ``lane_takes`` (quad form)."""
    g = np.asarray(g, F32)
    y = np.zeros(g.shape[:-1] + (h,), F32)      # an output nobody writes stays 0 (the quad form's tile is not pre-set)
    if white:
        y[...] = g[..., :h]
        return y
    F, Q = h // 2 + 1, h // 2
    hmax = W.shape[1]
    stride = hmax if stride is None else stride
    flat = np.concatenate([W.reshape(-1), np.zeros(hmax, F32)])

    def sums(tp):
        w = flat[tp * stride: tp * stride + h]
        acc = [np.zeros(g.shape[:-1], F32) for _ in range(4)]      # e0, e1, o0, o1
        for m in range(0, F):
            acc[m % 2] = fma32(g[..., m], w[m], acc[m % 2])
        for m in range(F, h):
            i = 2 + (m - F) % 2
            acc[i] = fma32(g[..., m], w[m], acc[i])
        return acc

    def zero_row():
        e0, e1, _, _ = sums(0)
        y[..., 0] = e0 + e1
        if h % 2 == 0:
            y[..., Q] = e0 - e1

    def row(tp, four):
        e0, e1, o0, o1 = sums(tp)
        e, od = e0 + e1, F32(od_sign) * (o0 + o1)
        y[..., tp] = e + od
        if h - tp != tp:
            y[..., h - tp] = e - od
        if four:
            ed, dd = e0 - e1, F32(dd_sign) * (o0 - o1)
            a, b = (Q + tp, Q - tp) if swap_q else (Q - tp, Q + tp)
            y[..., a] = ed + dd
            y[..., b] = ed - dd

    lanes = range(4) if quad else [None]
    for q in lanes:
        if q is None or q == 3:
            zero_row()
        for tp, four in folded_rows(h, q, lane_takes):
            if h % 2 == 0 and Q % 2 == 0 and tp == Q // 2 and not four:
                if q2 == "skipped":
                    continue
                four = q2 == "four"
            row(tp, four)
    return y


def synth_direct(g, W, h, white=False, t_begin=0):
    """sample_clip_body: acc = fma(g[m], w[m], acc) over m = 0 .. HMAX - 1 (slots past the horizon are zero)."""
    g = np.asarray(g, F32)
    hmax = W.shape[1]
    gz = np.zeros(g.shape[:-1] + (hmax,), F32)
    gz[..., :h] = g[..., :h]
    y = np.zeros(g.shape[:-1] + (h,), F32)
    for t in range(t_begin, h):
        acc = np.zeros(g.shape[:-1], F32)
        for m in range(hmax):
            acc = fma32(gz[..., m], W[t, m], acc)
        y[..., t] = acc
    return y


def synth_generic_quad(g, W, h, t_begin=0):
    """sample_clip_quad_body: lane q sums its slots m = 8 i + 2 q, 8 i + 2 q + 1 in order, the quad adds lanes (0 + 1) + (2 + 3)."""
    g = np.asarray(g, F32)
    hmax = W.shape[1]
    gz = np.zeros(g.shape[:-1] + (hmax,), F32)
    gz[..., :h] = g[..., :h]
    y = np.zeros(g.shape[:-1] + (h,), F32)
    for t in range(t_begin, h):
        part = []
        for q in range(4):
            acc = np.zeros(g.shape[:-1], F32)
            for i in range(hmax // 8):
                for u in range(2):
                    m = 8 * i + 2 * q + u
                    acc = fma32(gz[..., m], W[t, m], acc)
            part.append(acc)
        y[..., t] = (part[0] + part[1]) + (part[2] + part[3])
    return y


def affine_clip(y, mean, std, low, high, row0=False, transposed=False, t_shift=0, j_shift=0, stale_from=None):
    """v = fma(y, std[t, j], mean[t, j]) clipped to [low[j], high[j]] -> [n, h, d] f32 from y [n, h, d].  Faults: ``transposed``
    (the tables read at j h + t), ``t_shift`` (at t + shift, the last kept), ``j_shift`` (the box of dim j + shift),
    ``stale_from`` (the LDS stage's entries e >= stale_from hold what entry e - stale_from holds)."""
    h, d = mean.shape
    mean, std = np.asarray(mean, F32), np.asarray(std, F32)
    mean_row = mean
    if transposed:
        at = np.arange(d)[None] * h + np.arange(h)[:, None]
        mean, std = mean.reshape(-1)[at], std.reshape(-1)[at]
    if t_shift:
        at = np.clip(np.arange(h) + t_shift, 0, h - 1)
        mean, std = mean[at], std[at]
    if stale_from is not None:
        e = np.arange(h * d)
        at = np.where(e >= stale_from, e - stale_from, e)
        mean, std = mean.reshape(-1)[at].reshape(h, d), std.reshape(-1)[at].reshape(h, d)
    low, high = np.roll(np.asarray(low, F32), -j_shift), np.roll(np.asarray(high, F32), -j_shift)
    v = fma32(y, std[None], mean[None])
    a = np.minimum(np.maximum(v, low[None, None]), high[None, None])
    if row0:
        a[0] = mean_row
    return a


STREAM_FAULTS = ("dim_shift", "swap_offset", "ignore_first", "rounds")
NORMAL_FAULTS = ("swap_ab", "second", "shift_last_odd", "no_half")
TABLE_FAULTS = ("sigma_of", "beta_full", "nyquist2", "dc2", "imag_shift", "scale")
SYNTH_FAULTS = ("stride", "swap_q", "od_sign", "dd_sign", "q2", "lane_takes")
AFFINE_FAULTS = ("transposed", "t_shift", "j_shift", "stale_from", "row0_always")


def form_of(case, dtype=F32, gk_quad=True):
    """Which kernel serves sample_clip on this case: "folded" | "quad" | "thread"."""
    if dtype is F32 and case.h in FOLDED_H and case.t_begin == 0:
        return "folded"
    return "quad" if gk_quad else "thread"


def standin(case, form=None, tables=None, **faults):
    """The f32 restatement of one case -> dict(g slots [n, d, 2 ceil(h / 2)], y, a [n, h, d]) under the named faults
    (``rounds``: "other" = 7 for 10 and 10 for 7)."""
    unknown = set(faults) - set(STREAM_FAULTS + NORMAL_FAULTS + TABLE_FAULTS + SYNTH_FAULTS + AFFINE_FAULTS)
    assert not unknown, unknown
    form = form_of(case) if form is None else form
    low, high, mean, std = distribution(case, F32) if tables is None else tables
    h = case.h
    rounds = (17 - case.rounds) if faults.get("rounds") == "other" else case.rounds
    words = stream_words(case.seed, case.offset, 0 if faults.get("ignore_first") else case.first, case.n, case.d, h,
                         rounds, count=2 * h + 2, dim_shift=faults.get("dim_shift", 16),
                         swap_offset=faults.get("swap_offset", False))
    g = normals_standin(words, h, **{k: v for k, v in faults.items() if k in NORMAL_FAULTS})
    W = table(h, case.beta, **{k: v for k, v in faults.items() if k in TABLE_FAULTS})
    sf = {k: v for k, v in faults.items() if k in SYNTH_FAULTS}
    if form in ("folded", "folded-quad"):
        y = synth_folded(g, W, h, white=case.beta <= 0, quad=form == "folded-quad", **sf)
    elif form == "quad":
        y = synth_generic_quad(g, W, h, case.t_begin)
    else:
        y = synth_direct(g, W, h, t_begin=case.t_begin)
    y = np.ascontiguousarray(np.swapaxes(y, 1, 2))
    af = {k: v for k, v in faults.items() if k in AFFINE_FAULTS and k != "row0_always"}
    row0 = case.row0 and (case.first == 0 or faults.get("row0_always", False))
    a = affine_clip(y, mean, std, low, high, row0=row0, **af)
    return dict(g=g, y=y, a=a, low=low, high=high, mean=mean, std=std)


def time_slice(a, t_begin):
    """What a t_begin > 0 call is held to: the steps it writes."""
    return a[:, t_begin:]
