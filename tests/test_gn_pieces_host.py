"""The pieces of csrc/pf_gn.hpp on the host, one at a time: gn_sincos, gn_factor + gn_solve and gn_exp_apply behind the
C wrappers of tests/gn_pieces.cpp, built with g++ (-ffp-contract=off, as the library's host side) and loaded with
ctypes.  No GPU.

A refinement near the truth takes rotation steps far below pi/4 and factors matrices whose pivot order hardly varies,
so whole refinements never reach the quarter-turn cases of gn_sincos, its range reduction above 1e5 rad, most of the
pivot exchanges of gn_sym_swap or a zero pivot.  Here each piece meets inputs chosen to reach them, against
  * mpmath at 60 digits (sin, cos, the closed form of the exponential map), and
  * exact rational arithmetic (fractions.Fraction) for the linear solve and the inverse.

Bounds and where they come from:
  * gn_sincos, th <= 1e5: |error| <= 2^-53, the header's "within 1 ulp" written as an absolute error (an ulp of a value
    in [0.5, 1] is 2^-53; relative ulps mean nothing next to a zero of sin).  The bound and the figure 8.0e-17 are the ones the sweep was
    specified with, from a CPU run; this module's angles give 7.7e-17.
  * gn_sincos, 1e5 < th <= 1e9: th * 2^-53 + 2^-53, the header's own statement (the angle is taken modulo the double
    nearest 2 pi, which is 2.4e-16 away from 2 pi: the error grows with th).  Measured: 3.9e-8 at most.
  * the solve: 1e-13 relative to max |x| (specified with the sweep, where a CPU run gave 5.8e-16; here 5.3e-16; the matrices have condition numbers near 1e5 but are
    strongly graded, and an LDL^T with diagonal pivoting solves such systems to a few ulps of the largest component);
    the inverse, column by column, under the same bound: a column is the solve of a unit vector.
  * gn_exp_apply: 1e-14 plus the gn_sincos bound as it reaches the entry, on entries of magnitude up to 4.  With
    e = 2^-53 the bound on s and on c: R = I + O s / th + O^2 (1 - c) / th^2 has |dR/ds|, |dR/dc| <= 1, so a rotation
    entry gets 1e-14 + e.  V = I + (1 - c) / th^2 O + (th - s) / th^3 O^2 has |dV/dc|, |dV/ds| <= 1 / th, so an entry
    of the translation V upsilon gets 1e-14 + e (1 + 2 |upsilon| / th).  That term is the reference's formula, not
    this code: exponentialMap forms 1 - cos(th) by subtraction, which is 0 below th = 1e-8, so with |upsilon| of order
    1 the translation is off by th |upsilon| / 2 there (measured 5.2e-13 at th = 1e-12 and 5.0e-11 at th = 1e-6; a flat
    1e-14 + e holds from th = 0.1 on and for th = 0).  A Gauss-Newton step that small has an upsilon as small.
    Orthonormality of R: 1e-14.
"""
import ctypes as C
import itertools
import math
import os
import subprocess
from fractions import Fraction

import mpmath
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
EPS = 2.0 ** -53
N_ANGLES = 3000

mpmath.mp.dps = 60


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("gn_pieces") / "libgn_pieces.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "gn_pieces.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.gnp_sincos.restype = None
    lib.gnp_sincos.argtypes = [DP, C.c_int, DP, DP]
    lib.gnp_factor_solve.restype = C.c_int
    lib.gnp_factor_solve.argtypes = [DP, DP, DP, IP, DP, DP]
    lib.gnp_exp_apply.restype = None
    lib.gnp_exp_apply.argtypes = [DP, DP]
    return lib


def _dp(a):
    return a.ctypes.data_as(DP)


# ------------------------------------------------------------------------------------------------- gn_sincos
def sincos(lib, th):
    th = np.ascontiguousarray(th, dtype=np.float64)
    s, c = np.zeros_like(th), np.zeros_like(th)
    lib.gnp_sincos(_dp(th), len(th), _dp(s), _dp(c))
    return s, c


def residue(th):
    """The quarter-turn case gn_sincos takes: its own first three operations, in the same double arithmetic."""
    x = math.fmod(th, 6.283185307179586) if th > 1e5 else th
    return int(math.floor(x * 6.36619772367581382433e-01 + 0.5)) & 3


def sincos_error(lib, th):
    """Largest |error| of sin and of cos over the angles, and the per-angle errors."""
    s, c = sincos(lib, th)
    err = np.zeros(len(th))
    for i, t in enumerate(th):
        x = mpmath.mpf(float(t))
        err[i] = max(abs(float(mpmath.mpf(float(s[i])) - mpmath.sin(x))), abs(float(mpmath.mpf(float(c[i])) - mpmath.cos(x))))
    return err


def quarter_turn_neighbours():
    out = []
    for k in range(1, 60):
        at = float(mpmath.pi * k / 2)
        lo = hi = at
        out.append(at)
        for _ in range(10):
            lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
            out += [lo, hi]
    return np.array(out)


def angle_set(name):
    rng = np.random.default_rng(20)
    if name == "tiny":
        return 10.0 ** rng.uniform(-30.0, -3.0, N_ANGLES), {0}
    if name == "turn":
        return rng.uniform(0.0, 2.0 * math.pi, N_ANGLES), {0, 1, 2, 3}
    if name == "large":
        return rng.uniform(1e2, 1e5, N_ANGLES), {0, 1, 2, 3}
    if name == "quarter-turns":
        return quarter_turn_neighbours(), {0, 1, 2, 3}
    raise KeyError(name)


@pytest.mark.parametrize("name", ["tiny", "turn", "large", "quarter-turns"])
def test_sincos_within_an_ulp(lib, name):
    th, reachable = angle_set(name)
    assert th.max() <= 1e5
    seen = {residue(float(t)) for t in th}
    err = sincos_error(lib, th)
    worst = int(np.argmax(err))
    print(f"gn_sincos {name}: {len(th)} angles, residues {sorted(seen)}, max |error| {err[worst]:.3e} at {th[worst]!r} "
          f"(bound {EPS:.3e})")
    assert seen == reachable, (name, seen)
    assert err[worst] <= EPS, (name, float(th[worst]), err[worst])


def test_sincos_above_1e5(lib):
    th = np.random.default_rng(21).uniform(1e5, 1e9, N_ANGLES)
    th[0], th[1] = math.nextafter(1e5, math.inf), 1e9
    seen = {residue(float(t)) for t in th}
    err = sincos_error(lib, th)
    bound = th * EPS + EPS
    k = int(np.argmax(err / bound))
    print(f"gn_sincos above 1e5: residues {sorted(seen)}, max |error| {err.max():.3e}, largest error / bound "
          f"{err[k] / bound[k]:.3f} at {th[k]!r}")
    assert seen == {0, 1, 2, 3}
    assert np.all(err <= bound), (float(th[k]), err[k], bound[k])
    s, c = sincos(lib, th)
    assert np.all(np.abs(s) <= 1.0) and np.all(np.abs(c) <= 1.0)


def test_sincos_specials(lib):
    s, c = sincos(lib, np.array([np.nan, np.inf, -np.inf]))
    assert np.all(np.isnan(s)) and np.all(np.isnan(c))
    s, c = sincos(lib, np.array([0.0]))
    assert s[0] == 0.0 and c[0] == 1.0 and not np.signbit(s[0])


# ------------------------------------------------------------------------------------- gn_factor / gn_solve
def factor_solve(lib, A, b):
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    fac, x, inv = np.zeros(21), np.zeros(6), np.zeros((6, 6))
    pv = np.zeros(6, dtype=np.int32)
    ok = lib.gnp_factor_solve(_dp(A), _dp(b), _dp(fac), pv.ctypes.data_as(IP), _dp(x), _dp(inv))
    return bool(ok), fac, [int(p) for p in pv], x, inv


def rational_solve(A, b):
    """(x, A^-1) of the doubles of A and b in exact rational arithmetic: Gauss-Jordan on [A | b | I]."""
    n = 6
    rows = [[Fraction(float(A[i, j])) for j in range(n)] + [Fraction(float(b[i]))] +
            [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for k in range(n):
        p = next(i for i in range(k, n) if rows[i][k] != 0)
        rows[k], rows[p] = rows[p], rows[k]
        d = rows[k][k]
        rows[k] = [v / d for v in rows[k]]
        for i in range(n):
            if i != k and rows[i][k] != 0:
                f = rows[i][k]
                rows[i] = [vi - f * vk for vi, vk in zip(rows[i], rows[k])]
    x = [rows[i][n] for i in range(n)]
    inv = [[rows[i][n + 1 + j] for j in range(n)] for i in range(n)]
    return x, inv


def predicted_pivots(diag):
    """The exchanges of a diagonal pivot search on fixed diagonal values (a matrix whose Schur updates do not change
    their order): the largest remaining one, the first among equals."""
    d = list(diag)
    pv = []
    for k in range(6):
        p = k
        for i in range(k + 1, 6):
            if d[i] > d[p]:
                p = i
        pv.append(p)
        d[k], d[p] = d[p], d[k]
    return pv


def rel_to_max(got, want_fractions):
    """max |got - want| / max |want|, the difference formed exactly."""
    want = list(want_fractions)
    top = max(abs(w) for w in want)
    return float(max(abs(Fraction(float(g)) - w) for g, w in zip(got, want)) / top)


def spd_part(rng):
    """A random symmetric positive definite matrix with eigenvalues in [1, 2]."""
    q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    return (q * rng.uniform(1.0, 2.0, 6)) @ q.T


SOLVE_RTOL = 1e-13


def test_every_pivot_exchange(lib):
    """One graded SPD matrix per permutation of the diagonal's order: 0.05 x a well-conditioned SPD part plus
    diag(10^(5 - rank)).  The Schur updates change a diagonal by at most 1e-3 of the gap to the next one, so the
    pivot order is the prescribed one and the exchanges can be predicted; every one of the 21 (k, pv[k]) occurs."""
    rng = np.random.default_rng(22)
    seen = set()
    worst_x = worst_inv = 0.0
    for perm in itertools.permutations(range(6)):
        S = 0.05 * spd_part(rng)
        A = S + np.diag([10.0 ** (5 - r) for r in perm])
        A = 0.5 * (A + A.T)
        b = rng.normal(size=6)
        ok, fac, pv, x, inv = factor_solve(lib, A, b)
        assert ok, perm
        assert pv == predicted_pivots([10.0 ** (5 - r) for r in perm]), (perm, pv)
        assert all(pv[k] >= k for k in range(6))
        seen.update((k, pv[k]) for k in range(6))
        # D of the factorisation: the prescribed order, largest first
        d = [fac[i * (i + 1) // 2 + i] for i in range(6)]
        assert all(d[i] > d[i + 1] > 0.0 for i in range(5)), (perm, d)
        xr, invr = rational_solve(A, b)
        ex = rel_to_max(x, xr)
        worst_x = max(worst_x, ex)
        assert ex <= SOLVE_RTOL, (perm, ex)
        for c in range(6):
            ei = rel_to_max(inv[:, c], [invr[r][c] for r in range(6)])
            worst_inv = max(worst_inv, ei)
            assert ei <= SOLVE_RTOL, (perm, c, ei)
    print(f"gn_factor / gn_solve over 720 pivot orders: {len(seen)} exchanges seen, max relative error of x {worst_x:.3e}, "
          f"of a column of the inverse {worst_inv:.3e} (bound {SOLVE_RTOL:.0e})")
    assert seen == {(k, p) for k in range(6) for p in range(k, 6)}


def test_first_among_equal_diagonals(lib):
    rng = np.random.default_rng(23)
    # diagonal matrices: the Schur updates leave the remaining diagonal as it is, so every search meets its ties
    for diag in ([2.0] * 6, [0.5] * 6, [3.0, 3.0, 2.0, 2.0, 1.0, 1.0], [1.0, 3.0, 2.0, 3.0, 1.0, 2.0],
                 [1.0, 1.0, 1.0, 4.0, 4.0, 4.0], [2.0, 7.0, 7.0, 2.0, 7.0, 2.0]):
        A = np.diag(diag)
        b = rng.normal(size=6)
        ok, fac, pv, x, inv = factor_solve(lib, A, b)
        assert ok and pv == predicted_pivots(diag), (diag, pv)
        if len(set(diag)) == 1:
            assert pv == list(range(6))
        assert np.array_equal(x, b / np.array(diag)), diag
        assert np.array_equal(inv, np.diag(1.0 / np.array(diag))), diag
    # equal diagonals with couplings: the first search must stay at row 0, and the solution is still right
    for _ in range(20):
        S = 0.05 * spd_part(rng)
        np.fill_diagonal(S, 0.0)
        A = 0.5 * (S + S.T) + 2.0 * np.eye(6)
        b = rng.normal(size=6)
        ok, fac, pv, x, inv = factor_solve(lib, A, b)
        assert ok and pv[0] == 0, pv
        xr, invr = rational_solve(A, b)
        assert rel_to_max(x, xr) <= SOLVE_RTOL
    # -2 beside 2: the search compares magnitudes, the first of the two wins
    ok, fac, pv, x, inv = factor_solve(lib, np.diag([1.0, -2.0, 2.0, 1.0, 1.0, 1.0]), np.ones(6))
    assert ok and pv[0] == 1 and np.array_equal(x, [1.0, -0.5, 0.5, 1.0, 1.0, 1.0])


def test_zero_pivot_is_reported(lib):
    b = np.ones(6)
    # a zero on the diagonal from the start, in every place
    for z in range(6):
        d = np.ones(6)
        d[z] = 0.0
        assert not factor_solve(lib, np.diag(d), b)[0], z
    assert not factor_solve(lib, np.zeros((6, 6)), b)[0]
    # a zero that the elimination makes: rows 4 and 5 are the same (3 - 3 * 3 / 3 is exactly 0)
    A = np.diag([6.0, 5.0, 4.0, 3.5, 3.0, 3.0])
    A[5, 4] = A[4, 5] = 3.0
    assert not factor_solve(lib, A, b)[0]
    # the same matrix nudged off singular factors
    A[5, 5] = 3.25
    ok, fac, pv, x, inv = factor_solve(lib, A, b)
    xr, _ = rational_solve(A, b)
    assert ok and rel_to_max(x, xr) <= SOLVE_RTOL


# ---------------------------------------------------------------------------------------------- gn_exp_apply
def exp_apply(lib, xi, P):
    xi = np.ascontiguousarray(xi, dtype=np.float64)
    out = np.array(P, dtype=np.float64).reshape(12).copy()
    lib.gnp_exp_apply(_dp(xi), _dp(out))
    return out


def exp_apply_mp(xi, P):
    """exponentialMap(xi) * P in 60 digits: Rodrigues' formula and the V matrix in closed form."""
    m = mpmath
    u = m.matrix([m.mpf(float(v)) for v in xi[:3]])
    w = [m.mpf(float(v)) for v in xi[3:]]
    th = m.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = m.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    O2 = O * O
    I = m.eye(3)
    if th == 0:
        R, V = I, I
    else:
        R = I + (m.sin(th) / th) * O + ((1 - m.cos(th)) / th ** 2) * O2
        V = I + ((1 - m.cos(th)) / th ** 2) * O + ((th - m.sin(th)) / th ** 3) * O2
    Pm = m.matrix(3, 4)
    for i in range(3):
        for j in range(4):
            Pm[i, j] = m.mpf(float(P[4 * i + j]))
    N = R * Pm
    t = V * u
    for i in range(3):
        N[i, 3] += t[i]
    return N


def random_pose(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    P = np.zeros((3, 4))
    P[:, :3] = q
    P[:, 3] = [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(1, 3)]
    return P.reshape(12)


EXP_NORMS = [0.0, 1e-12, 1e-6, 0.1, 1.0, math.pi - 1e-9, math.pi, 4.0, 10.0]
EXP_ATOL = 1e-14 + EPS  # a rotation entry; a translation entry: see exp_bounds


def exp_bounds(xi):
    """(rotation entries, translation entries): the bounds of the module docstring."""
    th = float(np.linalg.norm(xi[3:]))
    if th == 0.0:
        return EXP_ATOL, EXP_ATOL
    return EXP_ATOL, 1e-14 + EPS * (1.0 + 2.0 * float(np.linalg.norm(xi[:3])) / th)


def test_exp_apply_against_the_closed_form(lib):
    rng = np.random.default_rng(24)
    identity = np.eye(3, 4).reshape(12)
    for norm in EXP_NORMS:
        worst_r = worst_t = ratio = ortho = 0.0
        quarters = set()
        for _ in range(24):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            xi = np.concatenate([rng.uniform(-1, 1, 3), norm * axis])
            P = random_pose(rng)
            got = exp_apply(lib, xi, P)
            want = exp_apply_mp(xi, P)
            th = math.sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5])
            quarters.add(residue(th))
            bar_r, bar_t = exp_bounds(xi)
            for i in range(3):
                for j in range(4):
                    err = abs(float(mpmath.mpf(float(got[4 * i + j])) - want[i, j]))
                    if j < 3:
                        worst_r = max(worst_r, err)
                    else:
                        worst_t = max(worst_t, err)
                    ratio = max(ratio, err / (bar_r if j < 3 else bar_t))
            R = exp_apply(lib, xi, identity).reshape(3, 4)[:, :3]
            ortho = max(ortho, float(np.abs(R @ R.T - np.eye(3)).max()), abs(float(np.linalg.det(R)) - 1.0))
            if norm == 0.0:  # no rotation: the translation is added, nothing else changes, to the bit
                want0 = P.copy()
                want0[[3, 7, 11]] += xi[:3]
                assert got.tobytes() == want0.tobytes()
        print(f"gn_exp_apply |omega| = {norm!r}: quarter-turn cases {sorted(quarters)}, max |error| rotation {worst_r:.3e}, "
              f"translation {worst_t:.3e}, largest error / bound {ratio:.3f}, orthonormality {ortho:.3e}")
        assert ratio <= 1.0, (norm, worst_r, worst_t, ratio)
        if norm == 0.0 or norm >= 0.1:  # the flat bound, where 1 - cos(th) is formed without cancellation
            assert max(worst_r, worst_t) <= EXP_ATOL, (norm, worst_r, worst_t)
        assert ortho <= 1e-14, (norm, ortho)
