"""Cases, reference and criterion for the truncated-normal sampler of the CEM baseline (cem_dev.h::truncnorm_quantile and
cem_bounds_element: the text of sample_truncnorm_kernel, cem_bounds_kernel and of every sampler of icem_plan_step_cem*), shared
by test_truncnorm_sensitivity_cpu.py and test_gpu_truncnorm_probes.py (a plain module, no fixtures).

Why a table of its own.  The fused and batched tests hold the step's kernels to the operators bit for bit -- they share this text,
so a fault in it passes all of them -- and the goldens run on beginning_of_rollout's distribution (lower / upper about -2 / +2) at
3e-5.  Nothing held the quantile where a CEM run takes it after a few iterations on saturating controls: the mean on an action
bound, a shrunken std, a uniform next to 0 or 1.  There the formula as first written, Phi^-1(pa + u pd), is one-sided: f32 holds
p to 6e-8 next to 1, and at lower = 0, upper = 300 a uniform within 2^-24 of 1 came back as ``upper`` (295 sigma off).

Reference.  oracle.truncnorm_quantile_f64: two-sided (the lower half through p, the upper half through the complement q),
float64, on the DEVICE's inputs -- mean, std, lower, upper and u as the kernel reads them (planner dtype), widened; the action is
mean + std z in float64.  It agrees with mpmath at 50 digits to 1e-13 (test_truncnorm_sensitivity_cpu.py, which also records
why scipy.stats.truncnorm.ppf, the reference project's call and oracle.truncnorm_from_uniform's, is not the yardstick).

Criterion, per entry, nothing left out (the quantile is continuous in everything it reads):
    |a_dev - a_ref| <= E_z std + eps |a_ref|                                          (accuracy)
    mean + std lower - eps |.| <= a_dev <= mean + std upper + eps |.|                  (the clamp: z lies in [lower, upper];
                                                                                        both ends rounded once, as the device's)
and no NaN.  eps is the planner dtype's (2^-23 / 2^-52): the one rounding of the closing multiply-add.
    f64   E_z = 1e-10 max(1, |z_ref|): the project's strict-parity bar (F64_RTOL of test_gpu_parity.py)
    f32   E_z = min(8 x RESTATEMENT_DZ_F32, 2e-6).  The f32 restatement below (NumPy, rounded wherever the device rounds, Phi
          and Phi^-1 CORRECTLY rounded) is at most RESTATEMENT_DZ_F32 = 2.54e-7 from the reference in z over this table
          (measured 2.537e-7 on 30x6x43-ulp-plain at the planted 1 - 2^-24, z = 5.4: half an ulp of a z in [4, 8) is 2.38e-7;
          test_the_restatement_is_as_good_as_the_header_says).  The device's normcdff / normcdfinvf are a few ulp each; a
          relative error r in p or q moves z by at most 1.26 r on the half where each is used; 8 x is the allowance for that.
          8 x 2.54e-7 = 2.03e-6 is held down to 2e-6, the project's F32_ATOL for std <= 1 and the most this check may grant.
          MI355X, this table, measured (EXPERIMENTS R17.1): the device's worst (|a_dev - a_ref| - eps |a_ref|) / std is 5.5e-7 in
          f32 (40x6x7-bound-plain, planted; 2.2 x the restatement), 0.50 of the bound at worst; 7.8e-13 in f64.  The one-sided
          text it replaced: up to 6.4e-3 on the device's own stream, ``upper`` itself at the planted 1 - 2^-24.
Bounds (cem_bounds_element): lower / upper within 4 eps |value| of the float64 expression on the dtype-rounded inputs (three
correctly rounded operations); like_levine's std within 2 eps relative of its float64 value, the 1e-8 floor and -2 / +2 exact.

Cases.  Every (t, j) has values of its own in every table, so an index t d + j read as j h + t, or a t off by one, moves an entry.
Shapes (h, d, n), every action box asymmetric per dimension (low_j = -0.7 - 0.13 j, high_j = 0.9 + 0.07 j):
    (2, 1, 5)      the smallest
    (13, 3, 86)    258 (row, dim) threads: two of them in a second workgroup of 256
    (30, 6, 43)    258 again
    (12, 17, 16)   272
    (40, 6, 7)     the long horizon (in f64 the LDS bound, not 256 / d, sets the fused sampler's rows per workgroup)
Distributions: "init" (beginning_of_rollout's, every entry moved a little), "bound" (the mean ON the low bound for even j and on
the high bound for odd j, std log-spaced 1e-3 .. 0.5 over t: lower = 0, upper up to 2.4e3), "ulp" (the mean one ulp inside the
bound), "zero" (std == 0 and std == 1e-8 at two entries in three: the output is the mean), "wide" (std = 1e3: the interval a
sliver around 0).  Each under _update_bounds ("plain") and under like_levine ("levine") -- on the GPU the device makes those
bounds, here bounds_standin does --, and "direct": lower / upper given, (-2, 2), (-1, 5), (-0.5, 8), (-5, 1), (0, 300),
(-300, 0), (-1e-3, 1e-3) in turn over the entries, each scaled by 1 + 1e-3 k on its k-th use.
Uniforms [n, h, d]: the device's own Philox stream (oracle.philox_uniforms) with planted values 2^-33, 1e-7, 0.5, 1 - 2^-12,
1 - 2^-20, 1 - 2^-24, 1.0 (f64 also 1e-300, 1 - 1e-12, 1 - 2^-53) -- every entry (t, j) meets min(n, 9 or 12) of 9 (12) slots,
planted ones and the stream's, in turn over the rows.  "stream" is the unplanted stream: what the device draws itself (u = NULL).
"""
from collections import namedtuple

import numpy as np

from oracle import icem_oracle as O

DTYPES = {"f32": np.float32, "f64": np.float64}
RESTATEMENT_DZ_F32 = 2.54e-7    # the f32 restatement's worst |z - z_ref| over the table (measured 2.537e-7)
E_Z_F32 = min(8 * RESTATEMENT_DZ_F32, 2e-6)
DEVICE_DZ_F32 = 5.5e-7         # MI355X, for the record (header): nothing is asserted against it
E_Z_F64 = 1e-10
SEED = 11

SHAPES = [(2, 1, 5), (13, 3, 86), (30, 6, 43), (12, 17, 16), (40, 6, 7)]
DISTS = ["init", "bound", "ulp", "zero", "wide"]
PAIRS = [(-2.0, 2.0), (-1.0, 5.0), (-0.5, 8.0), (-5.0, 1.0), (0.0, 300.0), (-300.0, 0.0), (-1e-3, 1e-3)]
PLANTED = [2.0 ** -33, 1e-7, 0.5, 1 - 2.0 ** -12, 1 - 2.0 ** -20, 1 - 2.0 ** -24, 1.0]
PLANTED_F64 = [1e-300, 1 - 1e-12, 1 - 2.0 ** -53]

Case = namedtuple("Case", "name h d n dist bounds")   # bounds: "plain" | "levine" | "direct"
CASES = [Case(f"{h}x{d}x{n}-{dist}-{b}", h, d, n, dist, b) for h, d, n in SHAPES for dist in DISTS for b in ("plain", "levine")]
CASES += [Case(f"{h}x{d}x{n}-init-direct", h, d, n, "init", "direct") for h, d, n in SHAPES]
EDGE_DISTS = ("bound", "ulp", "zero", "wide")


def box(d, dtype):
    j = np.arange(d)
    return (-0.7 - 0.13 * j).astype(dtype), (0.9 + 0.07 * j).astype(dtype)


def distribution(case, dtype):
    """-> low, high [d], mean, std [h, d] of ``dtype``."""
    h, d = case.h, case.d
    low, high = box(d, dtype)
    lo, hi = low.astype(np.float64)[None], high.astype(np.float64)[None]
    e = np.arange(h * d, dtype=np.float64).reshape(h, d)
    t, j = np.divmod(np.arange(h * d), d)
    t, j = t.reshape(h, d), j.reshape(h, d)
    wob, wob2 = np.sin(1.0 + e), np.cos(2.0 + 0.7 * e)
    mean = (lo + hi) / 2 + 0.05 * (hi - lo) * wob
    std = (hi - lo) / 2 * 0.5 * (1 + 0.1 * wob2)
    if case.dist == "bound":
        mean = np.where(j % 2 == 0, lo, hi) + 0 * e
        std = np.logspace(-3, np.log10(0.5), h)[:, None] * (1 + 0.01 * j)
    elif case.dist == "ulp":
        lo_in, hi_in = np.nextafter(low, dtype(np.inf)), np.nextafter(high, dtype(-np.inf))
        mean = np.where(j % 2 == 0, lo_in.astype(np.float64)[None], hi_in.astype(np.float64)[None]) + 0 * e
        std = 0.05 * (1 + 0.5 * wob2)
    elif case.dist == "zero":
        k = (t + 2 * j) % 3
        mean = np.where(k != 2, mean, np.where(e % 5 == 0, lo, np.where(e % 5 == 1, hi, mean)))
        std = np.where(k == 0, 0.0, np.where(k == 1, 1e-8, std))
    elif case.dist == "wide":
        std = 1e3 * (1 + 0.01 * e)
    return low, high, np.ascontiguousarray(mean.astype(dtype)), np.ascontiguousarray(std.astype(dtype))


def direct_bounds(case, dtype):
    e = np.arange(case.h * case.d)
    pair, use = e % len(PAIRS), e // len(PAIRS)
    scale = 1 + 1e-3 * use
    lower = np.array([PAIRS[p][0] for p in pair]) * scale
    upper = np.array([PAIRS[p][1] for p in pair]) * scale
    return lower.reshape(case.h, case.d).astype(dtype), upper.reshape(case.h, case.d).astype(dtype)


def stream(case, dtype, rounds=10, offset=0, seed=SEED, n=None):
    """The uniforms the device draws itself: planner seed ``seed``, stream offset ``offset``."""
    return O.philox_uniforms(seed, offset, case.n if n is None else n, case.d, case.h, rounds=rounds, dtype=dtype)


def planted(dtype):
    return np.array(PLANTED + (PLANTED_F64 if dtype is np.float64 else []), dtype=dtype)


def uniforms(case, dtype):
    """The stream with the planted values: slot (row + n (t d + j)) mod M of entry (row, t, j), slots below P planted."""
    u = stream(case, dtype)
    vals = planted(dtype)
    m = max(case.n, len(vals) + 2)
    r, e = np.arange(case.n)[:, None, None], np.arange(case.h * case.d).reshape(1, case.h, case.d)
    slot = (r + case.n * e) % m
    return np.ascontiguousarray(np.where(slot < len(vals), vals[np.minimum(slot, len(vals) - 1)], u).astype(dtype))


# ---- reference ------------------------------------------------------------------------------------------------------------------
def w(x):
    return np.asarray(x).astype(np.float64)


def fma64(a, b, c):
    """a b + c of float64 arrays rounded ONCE (to a part in 2^100): the product split exactly (Veltkamp / Dekker), the sum's
    error carried (Knuth) -- what the device's closing multiply-add gives, which a product rounded on its own misses by an ulp."""
    a, b, c = np.broadcast_arrays(w(a), w(b), w(c))
    p = a * b
    ah, bh = 134217729.0 * a, 134217729.0 * b
    ah, bh = ah - (ah - a), bh - (bh - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    v = s - p
    t = (p - (s - v)) + (c - v)
    return s + (t + e)


def reference(mean, std, lower, upper, u):
    """-> (a_ref, z_ref) [n, h, d] in float64 from the device's inputs (arrays of the planner dtype)."""
    z = O.truncnorm_quantile_f64(w(u), w(lower)[None], w(upper)[None])
    return w(mean)[None] + w(std)[None] * z, z


def bounds_reference(mean, std, low, high, like_levine):
    """-> (std, lower, upper) in float64 from the dtype-rounded inputs."""
    return O.cem_bounds(w(mean), w(std), w(low)[None], w(high)[None], like_levine)


# ---- criterion ------------------------------------------------------------------------------------------------------------------
def e_z(dtype, z_ref):
    return E_Z_F64 * np.maximum(1.0, np.abs(z_ref)) if dtype is np.float64 else np.full(z_ref.shape, E_Z_F32)


def miss(a_dev, mean, std, lower, upper, u, dtype):
    """By what factor the worst entry misses the criterion (<= 1: accepted), the larger of the accuracy part and the clamp part;
    inf for a NaN or an infinity."""
    a_dev = w(a_dev)
    if not np.isfinite(a_dev).all():
        return np.inf
    eps = float(np.finfo(dtype).eps)
    a_ref, z_ref = reference(mean, std, lower, upper, u)
    tiny = np.finfo(np.float64).tiny
    acc = np.abs(a_dev - a_ref) / (e_z(dtype, z_ref) * w(std)[None] + eps * np.abs(a_ref) + tiny)
    a_lo, a_hi = fma64(std, lower, mean)[None], fma64(std, upper, mean)[None]
    out = np.maximum(a_lo - a_dev, a_dev - a_hi)             # > 0: outside
    slack = eps * np.maximum(np.abs(a_lo), np.abs(a_hi)) + tiny
    return float(max(acc.max(), (1 + (out - slack) / slack).max()))   # (the clamp part: 1 at the edge of the slack)


def accuracy(a_dev, mean, std, lower, upper, u, dtype=np.float32):
    """The worst |a_dev - a_ref| - eps |a_ref| over std (entries with std > 0): the device's error in units of z, for the
    record."""
    a_ref, _ = reference(mean, std, lower, upper, u)
    s = w(std)[None] + 0 * a_ref
    on = s > 0
    err = np.abs(w(a_dev) - a_ref) - float(np.finfo(dtype).eps) * np.abs(a_ref)
    return float((err[on] / s[on]).max()) if on.any() else 0.0


def bounds_miss(std_dev, lower_dev, upper_dev, mean, std, low, high, like_levine, dtype):
    eps = float(np.finfo(dtype).eps)
    s, lo, up = bounds_reference(mean, std, low, high, like_levine)
    if not all(np.isfinite(w(x)).all() for x in (std_dev, lower_dev, upper_dev)):
        return np.inf
    if like_levine:
        exact = np.array_equal(w(lower_dev), lo) and np.array_equal(w(upper_dev), up)
        floor = np.array_equal(w(std_dev)[s == 1e-8], np.full((s == 1e-8).sum(), w(dtype(1e-8))))
        on = s != 1e-8
        rel = (np.abs(w(std_dev) - s)[on] / (2 * eps * np.abs(s[on]))).max() if on.any() else 0.0
        return float(rel) if exact and floor else np.inf
    tiny = np.finfo(np.float64).tiny
    if not np.array_equal(w(std_dev), w(std)):   # (untouched)
        return np.inf
    return float(max((np.abs(w(lower_dev) - lo) / (4 * eps * np.abs(lo) + tiny)).max(),
                     (np.abs(w(upper_dev) - up) / (4 * eps * np.abs(up) + tiny)).max()))


# ---- the restatement: the device's text in NumPy, rounded where the device rounds; every keyword is one fault ---------------------
def _fma(a, b, c, dtype):
    """round(a b + c) once (f32: float64's own rounding of the sum comes first, 2^-29 of an f32 ulp)."""
    return fma64(a, b, c).astype(dtype)


def bounds_standin(mean, std, low, high, like_levine, dtype, no_eps=False, two_terms=False, no_floor=False, three=False):
    """cem_bounds_element -> (std, lower, upper) of ``dtype``."""
    f = dtype
    mean, std, low, high = (np.asarray(x, dtype=f) for x in (mean, std, low[None], high[None]))
    if like_levine:
        lb, ub = (mean - low) / f(2), (high - mean) / f(2)
        s = np.minimum(lb, ub)
        s = s if two_terms else np.minimum(s, std)
        s = s if no_floor else np.maximum(s, f(1e-8))
        c = f(3) if three else f(2)
        return s.astype(f), np.full(mean.shape, -c, dtype=f), np.full(mean.shape, c, dtype=f)
    den = std if no_eps else std + f(1e-8)
    with np.errstate(divide="ignore", invalid="ignore"):
        return std, ((low - mean) / den).astype(f), ((high - mean) / den).astype(f)


def word_uniform(u_stream, dtype, no_half=False):
    """word_uniform of the words behind oracle.philox_uniforms' float64 stream."""
    words = np.rint(w(u_stream) * 2.0 ** 32 - 0.5)
    x = words.astype(dtype)
    return ((x if no_half else x + dtype(0.5)) * dtype(2.0 ** -32)).astype(dtype)


def quantile_standin(mean, std, lower, upper, u, dtype, one_sided=False, pd_is_pb=False, transposed=False, next_u=False,
                     no_clamp_lo=False, no_clamp_hi=False, swapped=False, std_neighbour=False, mean_neighbour=False,
                     complement_u=False):
    """sample_truncnorm_kernel / cem_sample_body -> (actions, z) [n, h, d] of ``dtype``.  Phi and Phi^-1 are float64's, rounded
    once: correctly rounded for f32."""
    from scipy.special import ndtr, ndtri
    f = dtype
    h, d = mean.shape
    mean, std, lower, upper, u = (np.asarray(x, dtype=f) for x in (mean, std, lower, upper, u))
    if transposed:   # the tables read at j h + t
        at = np.arange(d)[None] * h + np.arange(h)[:, None]
        lower, upper = lower.reshape(-1)[at], upper.reshape(-1)[at]
    if swapped:
        lower, upper = upper, lower
    if next_u:
        u = np.roll(u, -1, axis=1)
    if std_neighbour:
        std = np.roll(std.reshape(-1), -1).reshape(h, d)
    if mean_neighbour:
        mean = np.roll(mean.reshape(-1), -1).reshape(h, d)
    pa, pb, qb = (ndtr(w(x)).astype(f) for x in (lower, upper, -upper))
    pd = pb if pd_is_pb else (pb - pa).astype(f)
    pa, qb, pd, lo, hi = pa[None], qb[None], pd[None], lower[None], upper[None]
    p = _fma(u, pd, pa, f)
    with np.errstate(divide="ignore", invalid="ignore"):
        if one_sided:   # the text of the parent commit
            z = ndtri(w(p)).astype(f)
        else:
            v = u if complement_u else (f(1) - u).astype(f)
            q = _fma(v, pd, qb, f)
            low_half = p <= q
            z = ndtri(w(np.where(low_half, p, q))).astype(f)
            z = np.where(low_half, z, -z)
        if not no_clamp_lo:
            z = np.where(z < lo, lo, z)
        if not no_clamp_hi:
            z = np.where(z > hi, hi, z)
        if not one_sided:
            z = np.where(u < f(1), z, np.broadcast_to(hi, z.shape))   # ppf(1) = upper
        a = _fma(z, std[None], mean[None], f)
    return a, z.astype(f)


def case_inputs(case, dtype, **bounds_faults):
    """-> dict(low, high, mean, std, lower, upper, u) with the stand-in's bounds (on the GPU the device makes them)."""
    low, high, mean, std = distribution(case, dtype)
    if case.bounds == "direct":
        lower, upper = direct_bounds(case, dtype)
    else:
        std, lower, upper = bounds_standin(mean, std, low, high, case.bounds == "levine", dtype, **bounds_faults)
    return dict(low=low, high=high, mean=mean, std=std, lower=lower, upper=upper, u=uniforms(case, dtype))
