"""The test of the colored-noise sampler's tests (no GPU): the float64 reference of noise_cases.py against colored_from_white (the
irfft form), the planted coordinates re-derived from the oracle's integer side, the criterion on the NumPy restatement of the
kernels' text (accepted on every case, in every summation order the kernels use), and on single-fault mutants of it: each one
REJECTED on some case of the table.  Which of them the criteria in force before this table accepted -- constant mean 0 / std 0.5,
37 rows, atol 1e-5, and the stream's own normals at 4e-6 (test_philox_normals_match_oracle) -- is recorded in the last field of
every MUTANTS entry, checked and printed."""
import numpy as np
import pytest

import noise_cases as NC
from oracle import icem_oracle as O

F32 = np.float32
_ref, _std = {}, {}


def ref(case):
    if case.name not in _ref:
        _ref[case.name] = NC.reference(case, F32)
    return _ref[case.name]


def std(case, form=None):
    key = (case.name, form)
    if key not in _std:
        _std[key] = NC.standin(case, form)
    return _std[key]


def draw_order(g, h):
    return g[..., :h]


def misses(case, out, r=None):
    """(normals' miss, samples' miss) of a restatement's output under the table's criterion."""
    r = ref(case) if r is None else r
    tb = case.t_begin
    return (NC.normals_miss(draw_order(out["g"], case.h), r["g"], F32),
            NC.samples_miss(NC.time_slice(out["a"], tb), NC.time_slice(r["a"], tb), r["std"][tb:], F32))


PLANTED_CASES = NC.planted_cases()
ALL_CASES = NC.CASES + [c for _, _, c in PLANTED_CASES]


# ---- the reference -----------------------------------------------------------------------------------------------------------
def test_the_reference_agrees_with_the_irfft_form():
    """z_r @ Cr + z_i @ Ci against colored_from_white on the whole table, f32-input and f64 normals: 1e-12."""
    worst = 0.0
    for case in ALL_CASES + NC.F64_FOLDED_H_CASES:
        if case.beta <= 0:
            continue
        for dtype in (np.float32, np.float64):
            words = NC.stream_words(case.seed, case.offset, case.first, case.n, case.d, case.h, case.rounds)
            g = NC.reference_normals(words, case.h, dtype)
            z_r, z_i = NC.split_normals(g, case.h)
            want = O.colored_from_white(case.beta, case.h, z_r.copy(), z_i.copy()).transpose(0, 2, 1)
            worst = max(worst, float(np.abs(NC.reference_samples(g, case.h, case.beta) - want).max()))
    print("reference vs irfft form: worst", worst)
    assert worst <= 1e-12


def test_the_reference_normals_are_the_oracles_in_f64_and_near_them_in_f32():
    """f64: the oracle's philox_white_noise itself.  f32 inputs: within 4e-6 of the oracle's float32 formula (the existing test's
    yardstick), so the two references do not contradict each other on the stream's own draws."""
    for case in (NC.BY_NAME["30x6x43-b0.25-open"], NC.BY_NAME["13x3x90-b0.25-open"], NC.BY_NAME["33x2x10-b0.25-open"]):
        words = NC.stream_words(case.seed, case.offset, case.first, case.n, case.d, case.h)
        for dtype, atol in ((np.float64, 0.0), (np.float32, 4e-6)):
            z_r, z_i = NC.split_normals(NC.reference_normals(words, case.h, dtype), case.h)
            o_r, o_i = O.philox_white_noise(case.seed, case.offset, case.n, case.d, case.h, case.first, 10, dtype)
            assert np.abs(z_r - o_r).max() <= atol and np.abs(z_i - o_i).max() <= atol


def test_the_planted_coordinates_rederive():
    """Every recorded (row, dim, pair, word) is what the stream has there, is of its class, and sits in its case's middle row."""
    assert set(NC.PLANTED) == {"xa_small", "xa_large", "u1_one", "v_one", "quarter0", "quarter1", "quarter2", "quarter3"}
    for cls, (row, dim, pair, word), case in PLANTED_CASES:
        w = NC.stream_words(NC.P_SEED, NC.P_OFFSET, row, 1, NC.P_D, NC.P_H)[0, dim]
        xa, xb = int(w[2 * pair]), int(w[2 * pair + 1])
        assert NC.planted_class(cls, xa, xb), (cls, row, dim, pair, xa, xb)
        assert word == (xa if cls in ("xa_small", "xa_large", "u1_one") else xb)
        cw = NC.stream_words(case.seed, case.offset, case.first, case.n, case.d, case.h)
        assert np.array_equal(cw[1, dim], w) and case.first == row - 1 and case.n == 3
        u1, v = NC.device_inputs_f32(np.array([xa], dtype=np.uint64), np.array([xb], dtype=np.uint64))
        g = NC.reference_normals(cw, case.h, F32)[1, dim, 2 * pair:2 * pair + 2]
        if cls == "u1_one":
            assert u1[0] == 1.0 and (g == 0).all()
        if cls == "v_one":
            assert v[0] == 1.0
        if cls == "xa_small":
            assert np.hypot(*g) > 5.4
        if cls == "xa_large":
            assert 0 < np.hypot(*g) < 1e-3 and u1[0] < 1.0


def test_the_distributions_are_what_the_header_says():
    for case in NC.CASES:
        low, high, mean, sd = NC.distribution(case, F32)
        assert len(np.unique(mean)) == mean.size and len(np.unique(sd)) == sd.size, case.name     # every (t, j) its own
        if case.d > 1:
            assert len(np.unique(low)) == case.d and len(np.unique(high)) == case.d and not np.array_equal(-low, high)
        a, y = ref(case)["a"], ref(case)["y"]
        raw = NC.w64(mean)[None] + NC.w64(sd)[None] * y
        if case.dist == "open":
            assert np.array_equal(a[1:], raw[1:])                                                 # nothing clipped
        elif case.n * case.h * case.d >= 2000 and case.beta == 0.25:
            lo_share, hi_share = (raw < NC.w64(low)).mean(), (raw > NC.w64(high)).mean()
            assert 0.17 <= lo_share <= 0.33 and 0.17 <= hi_share <= 0.33, (case.name, lo_share, hi_share)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_the_criterion_accepts_the_restatement(case):
    forms = ["folded", "folded-quad"] if NC.form_of(case) == "folded" else ["thread", "quad"]
    for form in forms:
        mg, ma = misses(case, std(case, form))
        assert mg <= 1.0 and ma <= 1.0, (form, mg, ma)


def test_the_restatement_builds_the_oracles_table():
    """table() without a fault is synthesis_matrices in the layout W[t][m]: m < F real, else imaginary k = m - F + 1."""
    for h in (2, 5, 10, 12, 13, 30, 32, 33, 64):
        for beta in (0.25, 1.0, 3.0):
            Cr, Ci = O.synthesis_matrices(h, beta)
            W, F = NC.table(h, beta, dtype=np.float64), h // 2 + 1
            assert W.shape == (h, 32 if h <= 32 else 64) and np.array_equal(W[:, :F], Cr.T)
            assert np.array_equal(W[:, F:h], Ci[1:h - F + 1].T) and not W[:, h:].any()
    assert np.array_equal(NC.table(13, 0.0), np.eye(13, 32, dtype=F32))


def test_the_quad_deal_changes_no_bit():
    """row_synth_quad's deal of rows over four lanes writes every output once, with row_synth's bits."""
    for h in range(2, 65):
        got = sorted(tp for q in range(4) for tp, _ in NC.folded_rows(h, q))
        assert got == sorted(tp for tp, _ in NC.folded_rows(h)), h
    for case in NC.FOLDED_CASES:
        assert np.array_equal(std(case, "folded")["a"], std(case, "folded-quad")["a"]), case.name
    assert [NC.quad_pair_lane(p) for p in range(7)] == [0, 1, 2, 3, 0, 1, 2]


def test_the_q2_row_as_a_four_output_row_is_no_fault():
    """The Q/2 row "run twice" -- as a four-output row, its extra outputs Q - tp = tp and Q + tp = H - tp written again -- is not a
    fault a test could reject: at t = H/4 the odd cosines and the even sines are zero (1e-17 in the table), so e1 and o1 vanish
    and ed + dd IS e + od.  The restatement's samples move by less than an ulp of the sums; the mutant list leaves it out."""
    case = NC.BY_NAME["12x6x45-b0.25-open"]
    a, b = std(case, "folded")["y"], NC.standin(case, "folded", q2="four")["y"]
    assert np.abs(NC.w64(a) - NC.w64(b)).max() <= 2 * NC.EPS32 * np.abs(a).max()
    assert misses(case, NC.standin(case, "folded", q2="four"))[1] <= 1.0


def test_the_restatement_is_as_good_as_the_header_says():
    """The f32 restatement's worst |g - g_ref| and worst sample error in units of std (folded order) over the table, planted rows
    included: what E_g and E_y are eight times of."""
    dg, dy, where_g, where_y = 0.0, 0.0, None, None
    for case in ALL_CASES:
        out, r = std(case, "folded"), ref(case)
        g = float(np.abs(NC.w64(draw_order(out["g"], case.h)) - r["g"]).max())
        rows = slice(1, None) if case.row0 and case.first == 0 else slice(None)
        y = NC.samples_error(out["a"][rows], r["a"][rows], r["std"])
        if g > dg:
            dg, where_g = g, case.name
        if y > dy:
            dy, where_y = y, case.name
    print("f32 restatement: worst |dg|", dg, where_g, " worst dy", dy, where_y)
    assert 0.9 * NC.RESTATEMENT_DG_F32 <= dg <= NC.RESTATEMENT_DG_F32
    assert 0.9 * NC.RESTATEMENT_DY_F32 <= dy <= NC.RESTATEMENT_DY_F32
    assert NC.E_G_F32 == min(8 * NC.RESTATEMENT_DG_F32, 4e-6) and NC.E_Y_F32 == min(8 * NC.RESTATEMENT_DY_F32, 1e-5)


# ---- mutants -----------------------------------------------------------------------------------------------------------------
def names(*ns):
    return [NC.BY_NAME[n] for n in ns]


PLANTED_OF = {cls: [c for k, _, c in PLANTED_CASES if k == cls] for cls in NC.PLANTED}
STREAMS = names("30x6x43-b0.25-open", "13x3x90-b0.25-open", "5x3x90-b0.25-open", "64x3x7-b0.25-open")
EVEN = names("30x6x43-b0.25-open", "12x6x45-b0.25-open", "10x1x300-b0.25-open", "30x6x43-b3-open")
ODD = names("13x3x90-b0.25-open", "13x3x90-b3-open")
FOLDED_OPEN = EVEN + ODD
TIGHT = names("30x6x43-b0.25-tight", "12x6x45-b0.25-tight", "13x3x90-b0.25-tight", "30x17x16-b0.25-tight", "5x3x90-b0.25-tight")
INDEXED = names("30x6x43-b0.25-open", "12x6x45-b0.25-open", "13x3x90-b0.25-open", "30x17x16-b0.25-open", "30x18x15-b0.25-open",
                "33x2x10-b0.25-open")

# name -> (cases, form or None, faults, accepted by the criteria in force before this table)
MUTANTS = {
    # Box-Muller and streams
    "xa / xb swapped": (STREAMS, None, dict(swap_ab=True), False),
    "second normal dropped": (STREAMS, None, dict(second="dropped"), False),
    "second normal duplicated": (STREAMS, None, dict(second="duplicated"), False),
    "last odd-H pair shifted": (ODD + names("5x3x90-b0.25-open", "33x2x10-b0.25-open"), None, dict(shift_last_odd=True), False),
    "dim << 16 dropped": (STREAMS, None, dict(dim_shift=0), False),
    "offset words swapped": (STREAMS, None, dict(swap_offset=True), False),
    "first_index ignored": (STREAMS, None, dict(ignore_first=True), False),
    "7 rounds for 10": (STREAMS, None, dict(rounds="other"), False),
    "u1 without its 2^-33": (PLANTED_OF["xa_small"], None, dict(no_half=True), True),
    # synthesis
    "Q - tp and Q + tp swapped": (EVEN, "folded", dict(swap_q=True), False),
    "od's sign flipped": (FOLDED_OPEN, "folded", dict(od_sign=-1), False),
    "dd's sign flipped": (EVEN, "folded", dict(dd_sign=-1), False),
    "Q/2 row skipped": (names("12x6x45-b0.25-open"), "folded", dict(q2="skipped"), False),
    "Nyquist weight 2 for 1": (EVEN, None, dict(nyquist2=True), False),
    "DC weight 2 for 1": (FOLDED_OPEN, None, dict(dc2=True), False),
    "Nyquist imaginary draw not dropped (its power kept in sigma)": (EVEN, None, dict(sigma_of="odd"), False),
    "imaginary index off by one (down)": (FOLDED_OPEN, None, dict(imag_shift=-1), False),
    "imaginary index off by one (up)": (FOLDED_OPEN, None, dict(imag_shift=1), False),
    "sigma of even h at odd h": (ODD, None, dict(sigma_of="even"), False),
    "beta / 2 -> beta": (FOLDED_OPEN, None, dict(beta_full=True), False),
    "row stride HMAX -> H": (FOLDED_OPEN, "folded", dict(stride="H"), False),
    "quad form: lane 1 runs lane 0's rows": (FOLDED_OPEN, "folded-quad", dict(lane_takes=(1, 0)), False),
    "quad form: lane 3 runs lane 2's rows": (names("30x6x43-b0.25-open", "13x3x90-b0.25-open"), "folded-quad",
                                             dict(lane_takes=(3, 2)), False),
    # distribution and clip
    "mean / std transposed": (INDEXED, None, dict(transposed=True), True),
    "t off by one (up)": (INDEXED, None, dict(t_shift=1), True),
    "t off by one (down)": (INDEXED, None, dict(t_shift=-1), True),
    "low / high of dim j + 1": (TIGHT, None, dict(j_shift=1), True),
    "low / high of dim j - 1": (TIGHT, None, dict(j_shift=-1), True),
    "row0_mean applied at first_index > 0": (names("12x6x45-b0.25-open-row0", "33x2x10-b0.25-open-row0"), None,
                                             dict(row0_always=True), True),
    "the stage's tail entries (e >= 512) stale": (names("30x18x15-b0.25-open", "30x18x15-b0.25-tight-row0-first0"), None,
                                                  dict(stale_from=512), True),
}
# one table entry x 1.01 in every class of (t, m): (case, t, m) -- the t = 0 row's DC, odd real, last real (Nyquist) entries; a
# four-output row's real even / odd and imaginary first / second / last; the Q/2 row; an odd H's rows; the generic kernels' rows
# beyond H/2 and columns beyond 32
ENTRIES = [("30x6x43-b0.25-open", 0, 0), ("30x6x43-b0.25-open", 0, 1), ("30x6x43-b0.25-open", 0, 15),
           ("30x6x43-b0.25-open", 1, 2), ("30x6x43-b0.25-open", 7, 3), ("30x6x43-b0.25-open", 1, 16),
           ("30x6x43-b0.25-open", 4, 17), ("30x6x43-b0.25-open", 7, 29),
           ("12x6x45-b0.25-open", 3, 2), ("12x6x45-b0.25-open", 3, 7), ("12x6x45-b0.25-open", 2, 11), ("12x6x45-b0.25-open", 0, 6),
           ("10x1x300-b0.25-open", 2, 5), ("10x1x300-b0.25-open", 1, 9),
           ("13x3x90-b0.25-open", 6, 12), ("13x3x90-b0.25-open", 1, 6), ("13x3x90-b0.25-open", 0, 0),
           ("64x3x7-b0.25-open", 63, 63), ("33x2x10-b0.25-open", 32, 5), ("33x2x10-b0.25-open", 1, 32), ("5x3x90-b0.25-open", 4, 4),
           ("2x1x5-b0.25-open", 1, 1), ("32x4x70-b0.25-open-t31", 31, 30)]
for _name, _t, _m in ENTRIES:
    # (the old comparisons ran at h = 30, 12, 13, 64 and 2: an entry of another horizon's table is none of theirs)
    MUTANTS[f"table entry ({_t}, {_m}) x 1.01 at {_name.split('-')[0]}"] = (
        names(_name), None, dict(scale=(_t, _m, 1.01)), NC.BY_NAME[_name].h not in (30, 12, 13, 64, 2))


def run_mutant(cases, form, faults, tables=None):
    worst = (0.0, 0.0, None)
    for case in cases:
        f = dict(faults)
        if f.get("stride") == "H":
            f["stride"] = case.h
        r = ref(case) if tables is None else NC.reference(case, F32, tables(case))
        out = NC.standin(case, form, None if tables is None else tables(case), **f)
        mg, ma = misses(case, out, r)
        if max(mg, ma) > max(worst[:2]):
            worst = (mg, ma, case.name)
    return worst


@pytest.mark.parametrize("name", list(MUTANTS), ids=lambda n: n.replace(" ", "_"))
def test_the_criterion_rejects_the_mutant(name):
    cases, form, faults, _ = MUTANTS[name]
    unfaulted = max(max(misses(c, std(c, form))) for c in cases)
    mg, ma, where = run_mutant(cases, form, faults)
    print(f"{name}: normals miss {mg:.3g}, samples miss {ma:.3g} at {where} (unfaulted {unfaulted:.3g})")
    assert unfaulted <= 1.0
    assert max(mg, ma) > 1.0, (name, mg, ma)


# ---- what the criteria in force before this table accepted ----------------------------------------------------------------------
OLD_SHAPES = [(30, 6), (12, 6), (13, 4), (30, 17), (64, 3), (2, 1)]


def old_case(h, d, rounds):
    return NC._case(h, d, 37, rounds=rounds, tag="-old")


def old_tables(case):
    d, h = case.d, case.h
    return (-np.ones(d, F32), np.ones(d, F32), np.zeros((h, d), F32), np.full((h, d), 0.5, F32))


def old_criteria_accept(form, faults, cases=()):
    """test_philox_normals_match_oracle's two comparisons on the restatement: the normals at 4e-6, the samples under a constant
    mean 0 / std 0.5 in the box [-1, 1] at atol 1e-5; 37 rows of the stream's own draws at its six shapes and both round counts.
    (A fault of one form alone is tried on the shapes that form serves.)"""
    for h, d in OLD_SHAPES:
        for rounds in (10, 7):
            case = old_case(h, d, rounds)
            f = dict(faults)
            if f.get("stride") == "H":
                f["stride"] = h
            if form in ("folded", "folded-quad") and h not in NC.FOLDED_H:
                continue
            if (f.get("swap_q") or "dd_sign" in f) and h % 2:
                continue
            if "scale" in f and h != cases[0].h:
                continue
            r = NC.reference(case, F32, old_tables(case))
            out = NC.standin(case, form, old_tables(case), **f)
            if np.abs(NC.w64(draw_order(out["g"], h)) - r["g"]).max() > 4e-6 or not np.isfinite(out["a"]).all():
                return False
            if np.abs(NC.w64(out["a"]) - r["a"]).max() > 1e-5:
                return False
    return True


def test_what_the_criteria_in_force_accepted():
    """The old comparisons accept the unfaulted restatement, and of the mutants above exactly those whose entry says so: every fault
    of the distribution's indexing and of the clip's, the one Box-Muller fault only a planted draw shows, and the table entries of
    horizons they never ran."""
    assert old_criteria_accept(None, {})
    accepted = []
    for name, (cases, form, faults, expected) in MUTANTS.items():
        got = old_criteria_accept(form, faults, cases)
        accepted += [name] if got else []
        assert got == expected, (name, got)
    print(f"{len(accepted)} of {len(MUTANTS)} mutants accepted by the criteria in force before this table:")
    for name in accepted:
        print("   ", name)
