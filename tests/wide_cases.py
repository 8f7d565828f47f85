"""Cases for the wide GEMM rollout kernels (32 < o <= 384: rollout_wide_split_kernel on the fp16 and on the bf16 planes,
k_rollout_wide_split.hip / wide_split_body.h, and rollout_wide_kernel, the exact-f32 kernel of k_rollout_wide.hip), shared by
test_wide_sensitivity_cpu.py and test_gpu_wide_probes.py (a plain module, no fixtures).  The criterion, the reference and the
helpers are cost_term_cases.py's: row error against the float64 oracle over the row's per-mode magnitude, every row that is not
near a threshold within ROW_BOUND, the median within MEDIAN_BOUND, no share allowance.  What is new is the table.

Why a table of its own.  The kernels were held by HalfCheetah's cost on the dense benchmark model (one state column read, an
off-diagonal entry 0.0026 at o = 378: a fault off that column arrives at second order) and by cost_term_cases.py at o = 39 (one
column tile per wave, NT = 4).  On that model pack_wide_model_split's per-entry scales are trivial (every observation row 2^0,
every action row 2^-1, every column 2^0), so nothing read ``ksc`` / ``csc`` at an index that mattered.  Here every unit of
every shape is read out, sparse models give single entries of [A ; B] a readout of their own, and the scale groups run under
models whose row and column scales differ between every pair of neighbours the index arithmetic can confuse.

Shapes (o, d), from the kernels' tiling functions restated below (split_kb, split_nct, exact_kb, exact_nt, split_fits):
    (33, 4)     the narrowest wide shape: NT = 4, two 32-blocks (KB = 2, the only EVEN block count below: the m0 / m1 operand
                sets end where they began) -- (180, 12) is the second even one
    (64, 6) (65, 3)      NT 4 -> 8
    (128, 8) (129, 3)    NCT 1 -> 2, NT 8 -> 16
    (180, 12)   o + d = 192: KB = 6, even at NCT = 2, and NO padded contraction row in the last block
    (200, 64)   the largest d: a four-tile batch's actions are no longer held ahead in registers (held_ahead); KB = 9, odd
    (256, 17) (257, 6)   NCT 2 -> 3, NT 16 -> 24
    (378, 17)   the shipped shape (HumanoidStandup): KB = 13, the last column tile ragged (columns 378 .. 383 padded)
    (384, 32)   o + d = 416 = SPLIT_KMAX: every column live, the largest shape the plane kernel holds; a five-tile batch's
                actions are not held ahead (80 x 32 > 2048)
    (384, 64)   past split_fits: a handle asked for "f16x2" or "bf16x3" reports "f32" and is served by the exact kernel at 448
                contraction entries
Row counts: 35 (2 tiles + 3: the regular instantiation, a partly empty batch), 67 (5 tiles, ragged: FIVE, one operand set),
83 (4 + 2 tiles in one workgroup: a second batch through the same workgroup), 531 for the flip cases (34 tiles on 8 workgroups,
two of them with five: FIVE; 1 % of the rows is five of them), one 1-row case per shape (is_five restates the launch rule).

The reference pair (test_wide_sensitivity_cpu.py::test_reference_pair_agrees; kernel_standin: f32 with model entries and
per-step states rounded to 22 bits, a superset of the bf16 form's and the exact kernel's error), worst over the table (one seed: the seed perturbs
square roots only, and no cost of this table takes one):
    row error     1.7e-6   (1.68e-6 o384d64-unit-dense209-k1-final; unit-make 1.27e-6, scale 6.2e-7, long 8.7e-7, flip 5.4e-7,
                            entry 4.5e-7, action 1.5e-7, control 1.2e-7)
    median        4e-7     (3.93e-7 o378d17-shiftA1-lo3-unit0: B = 0, every row is the same trajectory and the median IS the row
                            error; unit-make 3.29e-7, scale 2.73e-7, every other group <= 1.8e-7)
    state error   4.6e-6   of the row's largest |state entry| (4.54e-6 o378d17-h30-flip2-lin2-k0-best: thirty steps of the
                            linear model; every h <= 12 group <= 2.7e-6)
The row error stays within cost_term_cases.MEASURED_ROW (1.8e-6), the median and the state error leave that module's
MEASURED_MEDIAN / _STATE (3.5e-7 / 3.4e-6), so this table has constants of its own, the values above x 4 (the factor and the
reason of cost_term_cases.py): ROW_BOUND 6.8e-6 (below the 1e-5 the wide kernels' tests claim), MEDIAN_BOUND 1.6e-6, NEAR 1.84e-5
-- BOUNDS below, handed to cost_term_cases.errors / violations / agree / rejection / near.  No bound is taken from a kernel.

The table (every launch <= 1100 rows; h = 3 for the dense readouts -- an entry fault arrives at first order --, h = 12 for the
sparse cycles, h = 4 for the flip cases, one h = 30 group at (378, 17)):
  unit-make-*   SyntheticModel.make, cost = state unit k: every k, kind 0 at 35 rows and kind 1 at 67, final and sum; one best
                and one 1-row case
  unit-dense-*  a fully dense model, A = N(0, 1) / sqrt(o), B = 0.3 N(0, 1) (every entry distinct, all of one order), tanh,
                83 rows: every k, final and sum.  Together with unit-make: every position of [A ; B] feeds a unit that is read
                one step later -- the claim for GROSS faults
  action-*      A = 0, B one-hot [j, k] = 0.75, cost = unit k at the tiling's edges (edge_units), j = 0, d - 1 and either side of
                a multiple of 4, 8 and 32 in the contraction index o + j
  control-*     A = B = 0, obs0 = 0, ctrl_weight 0.1, row r has the single action entry (t, j) = divmod(r, d): n = h d
  flip-*        flip on the edge units, flip_idx == lin_idx and !=, thresholds from the float64 rollout (both signs fire on
                10-90 % of the rows)
  entry-*       linear, sparse.  shiftA s: A[i][(i + s) % o] = w_i, B = 0; shiftB s: B[j][(j + s) % o] = v_j beside A = diag(w);
                weights distinct, alternating in sign, in +-[0.9, 1.0), exact in fp16.  Not every shift is affordable at o = 378:
                entry_shifts are chosen so that every CLASS of the two index decompositions (plane_classes, exact_classes) is met
                by an entry that alone carries a readout (test_every_class_is_claimed, from the sparsity pattern alone).  "lo"
                variants for shiftA 1 and shiftB o - d, read in 'final': lo = 1 adds 7 x 2^-15 to every |weight| (a low fp16
                plane that is not zero), lo = 2 adds 3 x 2^-19 (below bf16's 16 leading bits: the third bf16 plane); the residue
                is added to the MAGNITUDE of every weight, so a dropped plane shrinks every factor of the cycle's product and the
                per-step errors add up along it
  scale-*       models in other units, D^-1 A D with obs0 D and B D under action-row scales of their own (``units``): the
                exponents follow 3 (index % 5), under which any two indices that differ by 1, 4, 8, 16, 32, 48 or 128 differ
                (none is a multiple of 5), so that ksc and csc differ between every pair of neighbours the kernels' index
                arithmetic could confuse (asserted from pack_wide_model_split's rule restated in numpy: pack_scales); "pow2"
                powers of two, "odd" the same times non-powers.  A similarity transform because the planes promise accuracy
                relative to a row's largest CONTRIBUTION (absolute below 2^-13 of it: header of k_rollout_wide_split.hip,
                tile_cases._scale_cases): the same dynamics in other units keep every contribution balanced, D1 M D2 with
                unrelated D1, D2 would not (a power of two on all action rows, seam_shift, separates the pairs across the obs | action
                seam too); the dense scale models are linear (a tanh saturates the units of large scale, and a
                saturated unit shows no wrong scale).  Every unit read out under pow2, the edge units under odd, shiftA 1 and shiftB
                o - d under pow2; "graded": actions x 2^-(2 (row % 4) + 3 (tile % 2)) with B x 10 and a small observation under the LINEAR model, so
                that the per-row, per-step plane scale S differs between neighbouring rows and tiles; observations x 1e-4 and
                x 30, action bounds 0.01 and 50 (the bound at the observation's scale where B = 0, as in tile_cases.py)
                What the scale readouts do NOT test: the criterion's magnitude is taken from the row's largest |state entry|, which
                lives in the units of scale 2^12, so the four units in five with k % 5 != 4 are bounded 8 to 4096 times more loosely
                than their own magnitude.  Gross wrong-scale faults are still seen there (the mutants); the plane kernel's promise
                of accuracy relative to each output column's OWN scale is held only on the units of the largest scale
  long-*        (378, 17) at h = 30: edge units, both kinds, sum / final / best, and two flip cases
What the table cannot see is listed in test_wide_sensitivity_cpu.py.
"""
import dataclasses
import functools
import math

import numpy as np

import cost_term_cases as CC
from oracle import icem_oracle as O
from tile_cases import _read_units, forget, reaches, uncovered_claims  # noqa: F401  (the coverage helpers are pattern-only)

SHAPES = ((33, 4), (64, 6), (65, 3), (128, 8), (129, 3), (180, 12), (200, 64), (256, 17), (257, 6), (378, 17), (384, 32), (384, 64))
ROWS, ROWS_FIVE, ROWS_TWO, ROWS_FLIP = 35, 67, 83, 531
H_DENSE, H_SPARSE, H_FLIP, H_LONG = 3, 12, 4, 30

# the reference pair's worst values over THIS table (module docstring) and the bounds: each x 4, the project's factor for the
# matrix instruction's accumulation order (cost_term_cases.py)
MEASURED_ROW, MEASURED_MEDIAN, MEASURED_STATE = 1.7e-6, 4e-7, 4.6e-6
BOUNDS = CC.Bounds(row=4 * MEASURED_ROW, median=4 * MEASURED_MEDIAN, near=4 * MEASURED_STATE)

# ---- the kernels' tiling and launch rules, restated ---------------------------------------------------------------------
SPLIT_TT, SPLIT_WAVES, SPLIT_KMAX, FAST_MAX_LISTS, SPLIT_PLANE_BYTES = 5, 8, 416, 256, 24 * 1024


def split_kb(o, d):
    """wide_split_kb: 32-deep contraction blocks of the plane kernel."""
    return (o + d + 31) // 32


def split_nct(o):
    """wide_split_nct: column tiles per wave of the plane kernel."""
    nt = (o + 15) // 16
    return 1 if nt <= 8 else 2 if nt <= 16 else 3


def split_fits(o, d):
    """wide_split_fits: the workgroup's rows and planes in 160 KB of LDS and the contraction inside SPLIT_KMAX."""
    xs = 32 * split_kb(o, d) + 4
    return 16 * SPLIT_TT * xs * 4 + SPLIT_PLANE_BYTES + 4608 <= 160 * 1024 and 32 * split_kb(o, d) <= SPLIT_KMAX


def exact_kb(o, d):
    """wide_kb: 4-deep contraction blocks of the exact kernel, padded to a multiple of three."""
    return ((o + d + 3) // 4 + 2) // 3 * 3


def exact_nt(o):
    """wide_nt: column tiles of the exact kernel."""
    nt = (o + 15) // 16
    return 4 if nt <= 4 else 8 if nt <= 8 else 16 if nt <= 16 else 24


def is_five(n):
    """launch_rollout_wide_split's rule: does some workgroup of an n-row launch hold a batch of five tiles?"""
    tiles = (n + 15) // 16
    grid = min(max(1, tiles // (SPLIT_TT - 1)), FAST_MAX_LISTS)
    base, extra = divmod(tiles, grid)
    return (base >= SPLIT_TT and base % (SPLIT_TT - 1) == 1) or (extra > 0 and base + 1 >= SPLIT_TT and (base + 1) % (SPLIT_TT - 1) == 1)


def held_ahead(tiles, d):
    """split_batch's ``ahead``: are the next step's actions of a batch of ``tiles`` tiles held in registers?"""
    return 16 * tiles * d <= 64 * SPLIT_WAVES * 4


def tag(shape):
    return "o%dd%d" % tuple(shape)


def edge_units(o):
    """The units at the wide tiling's edges: 16- and 32-block edges, the first wave boundary at NCT = 2 (128) and the last
    column of the first 8 NCT tiles, the last live column."""
    return sorted({u for u in (0, 15, 16, 31, 32, 127, 128, 16 * 8 * split_nct(o) - 1, o - 1) if u < o})


def edge_actions(o, d):
    """Action entries 0, d - 1 and those on either side of a multiple of 4, 8 and 32 in the contraction index o + j."""
    js = {0, d - 1}
    for j in range(1, d):
        if any((o + j) % m == 0 for m in (4, 8, 32)):
            js |= {j - 1, j}
    return sorted(js)


# ---- the two index decompositions ---------------------------------------------------------------------------------------
def plane_classes(k, c, o, d):
    """The classes of entry M[k][c] (M = [A ; B], k the contraction index) in the plane kernel: contraction index = 32 kb + 8
    (lane / 16) + v, column = 16 (NCT wave + ct) + lane % 16."""
    nct, kb = split_nct(o), k // 32
    out = {f"p:g{(k % 32) // 8}", f"p:v{k % 8}", f"p:wave{(c // 16) // nct}", f"p:ct{(c // 16) % nct}"}
    out.add("p:kb-first" if kb == 0 else "p:kb-middle")
    if kb == o // 32:
        out.add("p:kb-seam")          # the block that holds the first action row (and, o % 32 != 0, the last observation rows)
    if kb == (o + d - 1) // 32:
        out.add("p:kb-last")          # partly padded unless (o + d) % 32 == 0
    if c == o - 1:
        out.add("p:last-live-column")
    return out


def exact_classes(k, c, o, d):
    """... in the exact kernel: contraction index = 4 kb + lane / 16, column = 16 (4 q + v) + lane % 16."""
    kb = k // 4
    out = {f"x:g{k % 4}", f"x:q{c // 64}", f"x:v{(c // 16) % 4}"}
    out.add("x:kb-first" if kb == 0 else "x:kb-middle")
    if kb == o // 4:
        out.add("x:kb-seam")
    if kb == (o + d - 1) // 4:
        out.add("x:kb-last")
    return out


def entry_index(entry, o):
    """(contraction index, column) of ("A", i, j) / ("B", j, c)."""
    return (entry[1] if entry[0] == "A" else o + entry[1]), entry[2]


def classes_of(entry, o, d):
    k, c = entry_index(entry, o)
    return plane_classes(k, c, o, d) | exact_classes(k, c, o, d)


def all_classes(o, d):
    """Every class some position of [A ; B] belongs to (the first padded column, o % 16 != 0, holds no entry: a mutant reads
    it as non-zero instead)."""
    out = set()
    for k in range(o + d):
        for c in (list(range(0, o, 16)) + [o - 1]):
            out |= plane_classes(k, c, o, d) | exact_classes(k, c, o, d)
    return out


# ---- models -------------------------------------------------------------------------------------------------------------
def shift_weights(n, lo=0, offset=0):
    """n distinct weights alternating in sign, magnitudes (1844 + offset + i // 2) / 2048 in [0.9, 1.0): exact in fp16 (11 bits);
    ``lo`` = 1: 7 x 2^-15 more in magnitude (a low fp16 plane that is not zero), 2: 3 x 2^-19 more (24 significant bits, the
    residue below the 16 bits two bf16 planes hold; rounding to 16 bits rounds it DOWN)."""
    i = np.arange(n)
    mag = (1844 + offset + i // 2) / 2048.0 + {0: 0.0, 1: 7.0 / 32768.0, 2: 3.0 / 524288.0}[lo]
    assert mag.max() < 1.0
    return np.where(i % 2 == 1, -1.0, 1.0) * mag


UNIT_STEP, UNIT_MOD = 3, 5   # exponent 3 (index % 5): differences of 3 and more survive the +-1 a dense line's largest weight moves


def unit_scales(n, units, first=0):
    """D[first .. first + n): 2^(3 (index % 5)), times a non-power of two in [1, 1.4) per index under "odd"."""
    i = np.arange(first, first + n)
    D = np.ldexp(1.0, UNIT_STEP * (i % UNIT_MOD))
    return D * (1.0 + 0.057 * (i % 7)) if units == "odd" else D


def pack_scales(A, B):
    """pack_wide_model_split's rule for the fp16 form, restated: (e [o + d], f [o]) -- 2^e_k the power of two of row k's largest
    |weight| (frexp: the row scaled by 2^-e_k peaks in [0.5, 1); a zero row is dead: e = 0 and takes no part), 2^f_j that of
    column j's largest row-scaled |weight|.  ksc[k] = 2^e_k, csc[j] = 2^f_j."""
    M = np.concatenate([A, B]).astype(np.float32).astype(np.float64)
    live = (M != 0).any(axis=1)
    e = np.where(live, np.frexp(np.abs(M).max(axis=1))[1], 0)
    Ms = np.where(live[:, None], np.ldexp(M, -e[:, None]), 0.0)
    cmax = np.abs(Ms).max(axis=0)
    f = np.where(cmax > 0, np.frexp(cmax)[1], 0)
    return e, f


@dataclasses.dataclass(eq=False)
class Case(CC.Case):
    """cost_term_cases.Case with the model forms of this table: "make", ("make-b", g) = make with B x g, ("dense", seed) = A =
    N(0, 1) / sqrt(o), B = 0.3 N(0, 1), ("onehot", j, k, w), "zero", ("shiftA", s, lo), ("shiftB", s, lo) (module docstring).
    ``units``: "" / "pow2" / "odd" -- the model in other units (D^-1 A D, B D under action-row scales; the case's obs_set
    carries obs0 D).  ``claims``: the entries (("A", i, j) / ("B", j, c)) an entry case puts on a path into the unit it scores."""
    claims: tuple = ()
    units: str = ""

    def matrices(self):
        o, d, m = self.o, self.d, self.model
        A, B = np.zeros((o, o)), np.zeros((d, o))
        if m == "make" or m[0] == "make-b":
            sm = O.SyntheticModel.make(o, d, self.kind)
            A, B = sm.A.copy(), sm.B * (1.0 if m == "make" else m[1])
        elif m[0] == "dense":
            rs = np.random.RandomState(m[1])
            A, B = rs.randn(o, o) / math.sqrt(o), 0.3 * rs.randn(d, o)
        elif m[0] == "onehot":
            B[m[1], m[2]] = m[3]
        elif m[0] == "shiftA":
            A[np.arange(o), (np.arange(o) + m[1]) % o] = shift_weights(o, m[2])
        elif m[0] == "shiftB":
            A[np.arange(o), np.arange(o)] = shift_weights(o, m[2])
            B[np.arange(d), (np.arange(d) + m[1]) % o] = shift_weights(d, m[2], offset=3)
        else:
            assert m == "zero", m
        if self.units:
            D = unit_scales(o, self.units)
            A = A * D[None, :] / D[:, None]
            B = B * D[None, :] / unit_scales(d, self.units, first=o)[:, None]
            if m[0] == "dense":
                B = B * 2.0 ** seam_shift(o, d, self.units, m[1])
        return A, B


@functools.lru_cache(maxsize=None)
def seam_shift(o, d, units, seed):
    """The power of two on ALL action rows of a dense scale model under which the pairs of contraction entries 1, 8 and 32 apart
    ACROSS the obs | action seam have different e_k as well: B's weights are of another order than A's, so the pattern alone
    (which separates each block among itself) leaves some seam pairs equal; the smallest |shift| that separates them all."""
    rs = np.random.RandomState(seed)
    A, B = rs.randn(o, o) / math.sqrt(o), 0.3 * rs.randn(d, o)
    D = unit_scales(o, units)
    e, _ = pack_scales(A * D[None, :] / D[:, None], B * D[None, :] / unit_scales(d, units, first=o)[:, None])
    for g in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        ee = e.copy()
        ee[o:] += g
        if all(ee[k] != ee[k + dk] for dk in (1, 8, 32) for k in range(max(0, o - dk), o) if k + dk < o + d):
            return g
    raise AssertionError((o, d, units))


def shape_of(case):
    return (case.o, case.d)


def _unit_spec(k):
    return CC._spec(lin_idx=k, lin_weight=1.0)


@functools.lru_cache(maxsize=None)
def _start(o, scale=0.2, units=""):
    """Start entries of ONE magnitude, signs mixed (no unit's readout is dwarfed by the row's largest entry), in the case's units."""
    D = unit_scales(o, units) if units else np.ones(o)
    return tuple((i, float(scale * (1.0 if (7 * i) % 5 < 3 else -1.0) * D[i])) for i in range(o))


@functools.lru_cache(maxsize=None)
def _random_start(o, units, seed, scale=0.2):
    D = unit_scales(o, units)
    x = scale * np.random.RandomState(seed).randn(o)
    return tuple((i, float(x[i] * D[i])) for i in range(o))


def _unit_cases(sh):
    o, d = sh
    g, out = f"unit-make-{tag(sh)}", []
    for mode in ("final", "sum"):
        for kind, n in ((0, ROWS), (1, ROWS_FIVE)):
            for k in range(o):
                out.append(Case(f"{tag(sh)}-unit{k}-k{kind}-{mode}", g, o, d, H_DENSE, kind, mode, n, _unit_spec(k), seed=7,
                                what=f"state unit {k}, benchmark model kind {kind}, {mode}, {n} rows"))
    k = o - 1
    out.append(Case(f"{tag(sh)}-unit{k}-k1-best", g, o, d, H_DENSE, 1, "best", ROWS_FIVE, _unit_spec(k), seed=7,
                    what=f"state unit {k}, benchmark model kind 1, best"))
    out.append(Case(f"{tag(sh)}-unit32-k0-sum-1row", g, o, d, H_DENSE, 0, "sum", 1, _unit_spec(32), seed=7, what="state unit 32, one row"))
    g = f"unit-dense-{tag(sh)}"
    for mode in ("final", "sum"):
        for k in range(o):
            out.append(Case(f"{tag(sh)}-unit-dense{k}-k1-{mode}", g, o, d, H_DENSE, 1, mode, ROWS_TWO, _unit_spec(k), seed=7, model=("dense", 5),
                            what=f"state unit {k}, dense model N(0, 1) / sqrt(o), {mode}, {ROWS_TWO} rows"))
    return out


FLIP_THRESH = {}   # case name -> threshold, from the float64 rollout


def _flip_cases(sh, h=H_FLIP, group=None, units=None):
    """Flip and linear parts on the edge units; threshold = the median over the rows of max_t |x_u| of the float64 rollout, to
    three digits (x_u starts at 0: neither sign fires at step 0, each fires later on about a quarter of the rows)."""
    o, d = sh
    units = edge_units(o) if units is None else units
    group = group or f"flip-{tag(sh)}"
    out = []
    for i, u in enumerate(units):
        kind = i % 2
        probe = Case(f"{tag(sh)}-h{h}-flip{u}-probe", "probe", o, d, h, kind, "sum", ROWS_FLIP, CC._spec(), seed=12 + i, obs_set=((u, 0.0),))
        x = O.rollout_observations(*CC.inputs(probe))[:, :, u]   # (the float64 rollout alone: the flip case below shares the inputs)
        th = float(f"{np.median(np.abs(x).max(axis=1)):.3g}")
        lin, mode = (u, ("sum", "best")[i == 0]) if i % 2 == 0 else (units[(i + 1) % len(units)], ("sum", "final")[i == 1])
        name = f"{tag(sh)}-h{h}-flip{u}-lin{lin}-k{kind}-{mode}"
        FLIP_THRESH[name] = th
        out.append(Case(name, group, o, d, h, kind, mode, ROWS_FLIP, O.CostSpec(0.1, lin, -1.0, u, 10.0, th), seed=12 + i,
                        obs_set=((u, 0.0),), what=f"flip on unit {u} at +-{th}, linear term on unit {lin}"))
    return out


def _action_cases(sh):
    o, d = sh
    units, out = edge_units(o), []
    for mode in ("final", "sum"):
        for n, j in enumerate(edge_actions(o, d)):
            for k in (units[n % len(units)], units[(n + 3) % len(units)]):
                out.append(Case(f"{tag(sh)}-act{j}-unit{k}-{mode}", f"action-{tag(sh)}", o, d, H_DENSE, 0, mode, ROWS, _unit_spec(k), seed=8,
                                model=("onehot", j, k, 0.75), what=f"action entry {j} (contraction index {o + j}) into state unit {k}, {mode}"))
    return out


def _control_cases(sh):
    o, d = sh
    return [Case(f"{tag(sh)}-ctrl-{mode}", f"control-{tag(sh)}", o, d, H_DENSE, 0, mode, H_DENSE * d, CC._spec(ctrl_weight=0.1, lin_idx=0, lin_weight=1.0),
                 seed=9, obs_scale=0.0, model="zero", acts="single", what="row r: action entry (t, j) = divmod(r, d)")
            for mode in ("sum", "final")]


def entry_shifts(o, d):
    """(shifts of shiftA, shifts of shiftB).  shiftA 1 claims A[i][i + 1] for EVERY i: every contraction class of the observation
    rows and every column class; 16 NCT + 1 and 33 move the pairing of row class and column class (another wave / ct for
    the same lane group, another block); o - 1 the other diagonal.  shiftB o - d claims every action row (the seam block, the
    last block) into the last columns, the last live one among them; 0 and 15 pair them with the first tiles."""
    a = sorted({s for s in (1, 16 * split_nct(o) + 1, 33, o - 1) if 0 < s < o})
    b = sorted({s % o for s in (0, 15, o - d)})
    return a, b


def _entry_cases(sh, **kw):
    o, d = sh
    h = H_SPARSE
    suffix, group = kw.pop("suffix", ""), kw.pop("group", f"entry-{tag(sh)}")
    sa, sb = entry_shifts(o, d)
    shifts_a, shifts_b, los = kw.pop("shifts_a", sa), kw.pop("shifts_b", sb), kw.pop("los", (0, 1, 2))
    units, scale = kw.get("units", ""), kw.pop("start_scale", 0.2)
    out = []
    for lo in los:
        mode = "final" if lo else "sum"
        tg = ("", "-lo", "-lo3")[lo]
        for n_s, s in enumerate(shifts_a):
            if lo and s != 1:
                continue
            for n_k, (k, entries) in enumerate(_read_units(h, o, s)):
                n = (ROWS, ROWS_FIVE)[(n_s + n_k + lo) % 2]   # (B = 0: every row is the same trajectory)
                out.append(Case(f"{tag(sh)}-shiftA{s}{tg}-unit{k}{suffix}", group, o, d, h, 0, mode, n, _unit_spec(k), seed=21,
                                model=("shiftA", s, lo), obs_set=_start(o, scale, units), claims=tuple(("A", i, j) for i, j in entries),
                                what=f"A[i][(i + {s}) % {o}] on the cycle into unit {k}", **kw))
        for n_s, s in enumerate(shifts_b):
            if lo and s != (o - d) % o:
                continue
            for j in range(d):
                c = (j + s) % o
                n = (ROWS, ROWS_FIVE)[(n_s + j + lo) % 2]
                extra = dict(obs_set=_random_start(o, units, 22)) if units else {}
                out.append(Case(f"{tag(sh)}-shiftB{s}{tg}-act{j}{suffix}", group, o, d, h, 0, mode, n, _unit_spec(c), seed=22,
                                model=("shiftB", s, lo), claims=(("B", j, c), ("A", c, c)),
                                what=f"B[{j}][{c}] (action {j}, contraction index {o + j}, into unit {c}) and A[{c}][{c}]", **extra, **kw))
    return out


GRADED = {}   # case name -> (row factors), for the mutants that need them


def _graded_inputs(case):
    """Actions graded per row and per tile by powers of two under B x 10 and a small observation: the plane scale S (a power of
    two per trajectory row and step, from the row's largest contribution) differs between neighbouring rows and between the
    same rows of neighbouring tiles.  Handed over through cost_term_cases.give_inputs."""
    A, B = case.matrices()
    f = lambda x: np.asarray(x).astype(np.float32).astype(np.float64)  # noqa: E731
    rs = np.random.RandomState(case.seed)
    obs0 = 0.01 * rs.randn(case.o)
    r = np.arange(case.n)
    grade = np.ldexp(1.0, -(2 * (r % 4) + 3 * ((r // 16) % 2)))
    acts = rs.uniform(-1, 1, (case.n, case.h, case.d)) * grade[:, None, None]
    GRADED[case.name] = grade
    CC.give_inputs(case, O.SyntheticModel(f(A), f(B), case.kind), f(obs0), f(acts))


def _scale_cases(sh):
    o, d = sh
    g, out = f"scale-{tag(sh)}", []
    # every unit under the dense model in power-of-two units (regular and FIVE by parity of k); the edge units under "odd".  The
    # LINEAR model: D^-1 A D is the same dynamics in other units only without the tanh, which would saturate the units of large
    # scale -- and a saturated unit does not show a wrong csc
    for units, ks in (("pow2", range(o)), ("odd", edge_units(o))):
        for k in ks:
            n, mode = ((ROWS, "final"), (ROWS_FIVE, "sum"))[k % 2]
            out.append(Case(f"{tag(sh)}-scale-{units}-unit{k}", g, o, d, H_DENSE, 0, mode, n, _unit_spec(k), seed=7, model=("dense", 6), units=units,
                            obs_set=_random_start(o, units, 31), what=f"state unit {k}, dense model in {units} units, {mode}, {n} rows"))
    out += _entry_cases(sh, suffix="-pow2", group=g, shifts_a=(1,), shifts_b=((o - d) % o,), los=(0, 1), units="pow2")
    # S differs between neighbouring rows and tiles.  The LINEAR model: the kernel scans the state for S at every step; under tanh it
    # takes the state's bound (sbound) from step 1 on, and every row whose actions stay below it would share one S
    for k in edge_units(o):
        for n, mode in ((ROWS_FIVE, "final"), (ROWS_TWO, "sum")):
            c = Case(f"{tag(sh)}-scale-graded-unit{k}-{mode}", g, o, d, H_DENSE, 0, mode, n, _unit_spec(k), seed=33, model=("make-b", 10.0),
                     what=f"state unit {k}, actions graded by powers of two per row and tile, {mode}, {n} rows")
            _graded_inputs(c)
            out.append(c)
    variants = {"obs1e-4": dict(obs_scale=2e-5), "obs30": dict(obs_scale=6.0), "bound0.01": dict(act_scale=0.01, high=0.01),
                "bound50": dict(act_scale=50.0, high=50.0)}
    for name, kw in variants.items():
        for i, k in enumerate(edge_units(o)):
            out.append(Case(f"{tag(sh)}-scale-{name}-unit{k}", g, o, d, H_DENSE, 0, "sum", (ROWS_TWO, ROWS_FIVE)[i % 2], _unit_spec(k), seed=7,
                            what=f"state unit {k} under {name}", **kw))
        if name.startswith("obs"):
            # B = 0: only the start observation sets the state's scale.  The planes' accuracy is ABSOLUTE below 2^-13 of the
            # row's largest contribution: an action bound 5e4 above a state it never reaches is outside what they promise
            # (tile_cases._scale_cases), so the bound follows the observation where it is the smaller one
            bound = dict(act_scale=2e-5, high=2e-5) if name == "obs1e-4" else {}
            out += _entry_cases(sh, suffix=f"-{name}", group=g, shifts_a=(1,), shifts_b=(), los=(0,), start_scale=kw["obs_scale"], **kw, **bound)
        else:
            out += _entry_cases(sh, suffix=f"-{name}", group=g, shifts_a=(), shifts_b=((o - d) % o,), los=(0,), **kw)
    return out


LONG_SHAPE = (378, 17)


def _long_cases():
    """The shipped shape at the shipped horizon: edge units under the benchmark model, and the flip on two of them."""
    o, d = LONG_SHAPE
    g, out = f"long-{tag(LONG_SHAPE)}", []
    for i, k in enumerate(edge_units(o)):
        for kind, mode, n in ((0, "sum", ROWS_TWO), (1, "final", ROWS_FIVE), (1, ("best", "sum")[i % 2], ROWS)):
            out.append(Case(f"{tag(LONG_SHAPE)}-h30-unit{k}-k{kind}-{mode}", g, o, d, H_LONG, kind, mode, n, _unit_spec(k), seed=7,
                            what=f"state unit {k} at h = 30, benchmark model kind {kind}, {mode}, {n} rows"))
    return out + _flip_cases(LONG_SHAPE, h=H_LONG, group=g, units=[2, o - 1])


def _table():
    out = []
    for sh in SHAPES:
        out += _unit_cases(sh) + _flip_cases(sh) + _action_cases(sh) + _control_cases(sh) + _entry_cases(sh) + _scale_cases(sh)
    return out + _long_cases()


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GROUPS = sorted({c.group for c in CASES})
_BY_GROUP = {}
for _c in CASES:
    _BY_GROUP.setdefault(_c.group, []).append(_c)


def by_group(group):
    return _BY_GROUP[group]


def groups_of(shape):
    return [g for g in GROUPS if g.endswith("-" + tag(shape))]
