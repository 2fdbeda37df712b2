"""The pieces of csrc/pf_p3p.hpp and csrc/pf_init_index.hpp on the host, one at a time, behind the C wrappers of
tests/p3p_pieces.cpp: built with g++ (the oracle's flags: -O2 -ffp-contract=off) and loaded with ctypes.  No GPU.

The kernels of pfmpe_init.hip reach the P3P solver only through integer histograms and four initialisations; here
every piece meets the reference's own arithmetic directly.

  * The complex operations against std::complex<double> (libstdc++ operators, libgcc's division, glibc's csqrt / clog,
    libstdc++'s pow), compiled into the pieces file itself.  Bar: bit-equal, NaN matching NaN.  1,200,000 random values
    with magnitudes 2^-30 .. 2^30 and the edges of every branch (Im = +-0, Re = 0, negative reals, the larger
    component exactly 0.5, 1 and 2 and one ulp on either side, the smaller component around DBL_EPSILON and
    DBL_EPSILON / 2, x^2 + y^2 on either side of 0.5, subnormal components), and clog and the division once more on
    subnormal, huge, infinite, NaN and zero operands, where glibc and libgcc rescale or take special cases.
  * setup + solution against the oracle's p3p (which uses std::complex as the reference does), 20,000 problems from the
    16-LED model, a quarter true projections and the rest random float32 pixels.  Bar: bit-equal, NaN matching NaN.
    The same sweep with the header's device form (-DPFP3P_DEVICE_ARITHMETIC: log(hypot), Smith's division alone,
    pow(x, 2.0) as the compiler folds it), which the kernels keep for its speed: 117 of the 20,000 differ in some bit,
    by 3.81e-9 at most in a finite entry, with the oracle's finite / non-finite pattern.  Bar: that pattern, and
    16 x 3.81e-9.  That form operation by operation: all but clog and the powers built on it bit-equal to std::complex
    where no operand and no component of the result is subnormal; clog's imaginary part bit-equal, its real part
    within 2^-52 + 2 ulp (157,601 of 1,206,602 differ, by 2.2e-16 at most).
  * inverse34 and project against the oracle's inverse44 / project44, bit-equal (project: -0.0 == +0.0, see there).
  * A check that does not rest on the oracle: 5,000 exact projections of random poses (depth 0.6 - 5 m, rotations up
    to 1 rad about each axis); the best finite solution equals the inverse of the true pose within 1e-8 in every
    entry, in all but 2 % of the cases at most.  Measured with this module's generator: the oracle misses 0.64 % at
    1e-8 (0.08 % at 1e-6; median error 2.4e-13), the header the same 0.64 % and 0.08 % (its solutions are the
    oracle's): Kneip's parametrisation loses digits near its singular configurations, it does not fail.
  * The index maps: unrank3 inverts the colex rank (every rank below C(64, 3); at 1024 blobs both neighbours of every
    boundary C(c, 3) and C(c, 3) + C(b, 2)), perm3 is a bijection onto the ordered distinct triples and unused_markers
    the ascending complement, for every M from 3 to 16.
"""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import pforacle as orc
from pf_monocular_pose_estimator_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
LP = C.POINTER(C.c_int64)
EPS = 2.0 ** -52  # DBL_EPSILON
MEASURED_DEVICE_MATH = 3.81e-9  # measured with g++ 11.4, glibc 2.35: 117 of the 20,000 problems differ in some bit

OPS = {"div": 0, "div_scalar": 1, "scalar_div": 2, "scalar_mul": 3, "scalar_add": 4, "scalar_sub": 5, "add": 6,
       "sub": 7, "neg": 8, "csqrt": 9, "clog": 10, "cpow2": 11, "cpow3": 12, "cpow_third": 13}


def build_pieces(tmp_path_factory, name, *defines):
    so = tmp_path_factory.mktemp(name) / f"lib{name}.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra",
                    "-Wno-unknown-pragmas", *defines, os.path.join(ROOT, "tests", "p3p_pieces.cpp"), "-o", str(so)],
                   check=True)
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def lib_device_math(tmp_path_factory):
    """The header with the device's complex arithmetic (log(hypot), Smith's division alone), on the host's libm."""
    lib = build_pieces(tmp_path_factory, "p3p_pieces_device_math", "-DPFP3P_DEVICE_ARITHMETIC")
    lib.p3_cx_op.restype = C.c_int
    lib.p3_cx_op.argtypes = [C.c_int, C.c_int, DP, DP, DP, DP, DP, DP]
    lib.p3_p3p_n.restype = None
    lib.p3_p3p_n.argtypes = [C.c_int, DP, DP, DP, IP]
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_pieces(tmp_path_factory, "p3p_pieces")
    lib.p3_cx_op.restype = C.c_int
    lib.p3_cx_op.argtypes = [C.c_int, C.c_int, DP, DP, DP, DP, DP, DP]
    lib.p3_p3p.restype = C.c_int
    lib.p3_p3p.argtypes = [DP, DP, DP, DP]
    lib.p3_p3p_n.restype = None
    lib.p3_p3p_n.argtypes = [C.c_int, DP, DP, DP, IP]
    lib.p3_finite12.restype = C.c_int
    lib.p3_finite12.argtypes = [DP]
    lib.p3_inverse34.restype = None
    lib.p3_inverse34.argtypes = [DP, DP]
    lib.p3_project.restype = None
    lib.p3_project.argtypes = [DP, DP, DP, DP]
    lib.p3_unrank3.restype = None
    lib.p3_unrank3.argtypes = [C.c_int, LP, IP]
    lib.p3_c3.restype = C.c_int64
    lib.p3_c3.argtypes = [C.c_int64]
    lib.p3_c2.restype = C.c_int64
    lib.p3_c2.argtypes = [C.c_int64]
    lib.p3_perm3_all.restype = None
    lib.p3_perm3_all.argtypes = [C.c_int, IP]
    lib.p3_unused.restype = C.c_int
    lib.p3_unused.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, IP]
    return lib


def _dp(a):
    return a.ctypes.data_as(DP)


def same_bits(a, b):
    """Entry for entry: the same bit pattern, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------------------------------- complex operations
def _around(v):
    """v, and one and two ulps on either side."""
    out = [v]
    lo = hi = v
    for _ in range(2):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


def edge_values():
    """(re, im) pairs on and next to every branch of csqrt, clog and pow."""
    big = []  # the larger component: the clog branch limits and points inside each branch
    for v in (0.5, 1.0, 2.0):
        big += _around(v)
    big += [0.5625, 0.7, 0.75, 0.999, 1.001, 1.25, 1.5, 1.999, 0.25, 0.499, 2.5, 3.0]
    small = [0.0, 5e-324, 1e-300, 1e-20]  # the smaller one: around DBL_EPSILON / 2, DBL_EPSILON, 1, and up to the larger
    for v in (EPS / 2, EPS, 1.0):
        small += _around(v)
    small += [1e-9, 1e-3, 0.1, 0.25, 0.37, 0.38, 0.4, 0.49, 0.5, 0.6, 0.7, 0.9, 1.2, 1.9]
    pairs = []
    for a in big:
        for b in small:
            if b <= a:
                for sa, sb in itertools.product((1.0, -1.0), repeat=2):
                    pairs.append((sa * a, sb * b))
                    pairs.append((sb * b, sa * a))
        # x^2 + y^2 on either side of 0.5 for 0.5 <= a < 0.7072
        if 0.5 <= a < math.sqrt(0.5):
            y = math.sqrt(0.5 - a * a)
            for yy in _around(y):
                pairs += [(a, yy), (-yy, a)]
    # Im = +-0 and Re = +-0 at many magnitudes, negative reals among them
    for e in range(-30, 31, 3):
        for m in (1.0, 1.3, 1.7):
            v = math.ldexp(m, e)
            for s in (1.0, -1.0):
                pairs += [(s * v, 0.0), (s * v, -0.0), (0.0, s * v), (-0.0, s * v)]
    return np.array(pairs)


@pytest.fixture(scope="module")
def cx_inputs():
    """z and w: 1,200,000 random values with magnitudes 2^-30 .. 2^30 (a third at magnitude one, where clog's branches
    lie; a fifth of z real), then the edge values."""
    rng = np.random.default_rng(41)
    n = 1_200_000
    i = np.arange(n)
    s1 = np.where(i % 3 == 0, 1.0, np.ldexp(1.0, rng.integers(-30, 31, n)))
    s2 = np.where(i % 3 == 0, 1.0, np.ldexp(1.0, rng.integers(-30, 31, n)))
    zr = rng.uniform(-1, 1, n) * 2 * s1
    zi = np.where(i % 5 == 0, 0.0, rng.uniform(-1, 1, n) * 2 * s2)
    wr = rng.uniform(-1, 1, n) * s2
    wi = rng.uniform(-1, 1, n) * s1
    e = edge_values()
    we = np.roll(e, 7, axis=0)
    we = np.where(we == 0.0, 0.75, we)  # divisors: not zero
    zr, zi = np.concatenate([zr, e[:, 0]]), np.concatenate([zi, e[:, 1]])
    wr, wi = np.concatenate([wr, we[:, 0]]), np.concatenate([wi, we[:, 1]])
    assert np.all(wr != 0.0) and np.all(np.isfinite(wr)) and np.all(np.isfinite(wi))
    return tuple(np.ascontiguousarray(a) for a in (zr, zi, wr, wi))


def test_edge_values_reach_every_clog_branch():
    """The inputs, not the code: each of glibc's clog branches has edge values inside it."""
    e = np.abs(edge_values())
    ax, ay = e.max(axis=1), e.min(axis=1)
    near = (ax >= 0.5) & (ax < 2.0)
    branches = {
        "one": ax == 1.0,
        "above one, small": (ax > 1.0) & near & (ay < 1.0) & (ay < EPS),
        "above one": (ax > 1.0) & near & (ay < 1.0) & (ay >= EPS),
        "below one, tiny": (ax < 1.0) & near & (ay < EPS / 2),
        "below one, exact sum": (ax < 1.0) & near & (ay >= EPS / 2) & (ax * ax + ay * ay >= 0.5),
        "below one, small sum": (ax < 1.0) & near & (ay >= EPS / 2) & (ax * ax + ay * ay < 0.5),
        "both above one": (ax > 1.0) & near & (ay >= 1.0),
        "far below": ax < 0.5,
        "far above": ax >= 2.0,
    }
    for name, m in branches.items():
        assert m.sum() >= 4, name


@pytest.mark.parametrize("op", sorted(OPS, key=OPS.get))
def test_complex_operation_equals_std_complex(lib, cx_inputs, op):
    zr, zi, wr, wi = cx_inputs
    n = len(zr)
    hdr, ref = np.zeros((n, 2)), np.zeros((n, 2))
    assert lib.p3_cx_op(OPS[op], n, _dp(zr), _dp(zi), _dp(wr), _dp(wi), _dp(hdr), _dp(ref)) == 0
    ok = same_bits(hdr, ref).all(axis=1)
    bad = np.flatnonzero(~ok)
    print(f"{op}: {len(bad)} of {n} differ")
    assert len(bad) == 0, [(zr[k], zi[k], wr[k], wi[k], hdr[k].tolist(), ref[k].tolist()) for k in bad[:5]]


DEVICE_EXACT_OPS = [op for op in sorted(OPS, key=OPS.get) if op not in ("clog", "cpow2", "cpow3", "cpow_third")]


@pytest.mark.parametrize("op", DEVICE_EXACT_OPS)
def test_device_form_operation_equals_std_complex(lib_device_math, cx_inputs, op):
    """The form the kernels compile (PFP3P_DEVICE_MATH), operation by operation: everything but clog and what is built on
    it equals std::complex bit for bit as long as no operand and no component of the result is subnormal: Smith's
    division alone is libgcc 12's __divdc3 there (its scalings are by powers of two, and its other order of operations
    is for a subnormal ratio)."""
    zr, zi, wr, wi = cx_inputs
    tiny = 2.2250738585072014e-308
    keep = np.ones(len(zr), dtype=bool)
    for a in (zr, zi, wr, wi):
        keep &= (a == 0.0) | (np.abs(a) >= tiny)
    assert (~keep).sum() < 1000  # only edge values with a subnormal component go
    zr, zi, wr, wi = (np.ascontiguousarray(a[keep]) for a in (zr, zi, wr, wi))
    n = len(zr)
    hdr, ref = np.zeros((n, 2)), np.zeros((n, 2))
    assert lib_device_math.p3_cx_op(OPS[op], n, _dp(zr), _dp(zi), _dp(wr), _dp(wi), _dp(hdr), _dp(ref)) == 0
    normal = ((ref == 0.0) | ~(np.abs(ref) < tiny)).all(axis=1)  # libgcc's scaling also keeps bits of a subnormal quotient
    assert (~normal).sum() < 1000
    bad = np.flatnonzero(~same_bits(hdr, ref).all(axis=1) & normal)
    assert len(bad) == 0, [(zr[k], zi[k], wr[k], wi[k], hdr[k].tolist(), ref[k].tolist()) for k in bad[:5]]


def test_device_form_clog_is_log_hypot(lib_device_math, cx_inputs):
    """The kernels' clog: the imaginary part is glibc's bit for bit; the real part is log(hypot), within
    2^-52 + 2 ulp of glibc's: hypot is within an ulp of |z| (a relative 2^-52, which log turns into that much
    absolute error), and each side rounds its own result once.  Next to |z| = 1 that is many ulps of a small result:
    what glibc's log1p branches are for, and what the solver's bound of 16 x 3.81e-9 absorbs."""
    zr, zi, wr, wi = cx_inputs
    n = len(zr)
    hdr, ref = np.zeros((n, 2)), np.zeros((n, 2))
    assert lib_device_math.p3_cx_op(OPS["clog"], n, _dp(zr), _dp(zi), _dp(wr), _dp(wi), _dp(hdr), _dp(ref)) == 0
    assert same_bits(hdr[:, 1], ref[:, 1]).all()
    fin = np.isfinite(ref[:, 0])
    assert np.array_equal(fin, np.isfinite(hdr[:, 0])) and same_bits(hdr[~fin, 0], ref[~fin, 0]).all()
    d = np.abs(hdr[fin, 0] - ref[fin, 0])
    differ = (~same_bits(hdr[:, 0], ref[:, 0])).sum()
    print(f"device clog: {differ} of {n} real parts differ, by {d.max():.3g} at most")
    assert differ > 0  # the two forms are not the same function
    assert (d <= 2.0 ** -52 + 2 * np.spacing(np.abs(ref[fin, 0]))).all()


END_VALUES = [0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 4.450147717014403e-308, 1e-300, 2.0 ** -53,
              2.0 ** -52, 1.0, -1.0, 0.7, 1.9958403095347196e292, 1e300, 8.988465674311579e307,
              math.nextafter(8.988465674311579e307, math.inf), -1.2e308, 1.7976931348623157e308, math.inf, -math.inf,
              math.nan]


def test_clog_at_the_ends_of_the_range(lib):
    """clog where glibc rescales or takes a special case: subnormal, huge, infinite, NaN and zero operands."""
    z = np.array(list(itertools.product(END_VALUES, repeat=2)))
    zr, zi = np.ascontiguousarray(z[:, 0]), np.ascontiguousarray(z[:, 1])
    n = len(zr)
    hdr, ref = np.zeros((n, 2)), np.zeros((n, 2))
    assert lib.p3_cx_op(OPS["clog"], n, _dp(zr), _dp(zi), _dp(zr), _dp(zi), _dp(hdr), _dp(ref)) == 0
    bad = np.flatnonzero(~same_bits(hdr, ref).all(axis=1))
    assert len(bad) == 0, [(zr[k], zi[k], hdr[k].tolist(), ref[k].tolist()) for k in bad[:5]]


def test_division_at_the_ends_of_the_range(lib):
    """z / w and x / z where libgcc halves or scales the operands, takes the other order for a subnormal ratio, or
    recovers an infinity or a zero from NaN + i NaN: every combination of four of the end values, and 200,000 random
    ones with exponents over the whole double range."""
    q = np.array(list(itertools.product(END_VALUES, repeat=4)))
    rng = np.random.default_rng(43)
    r = rng.uniform(-2, 2, (200_000, 4)) * np.ldexp(1.0, rng.integers(-1070, 1023, (200_000, 4)))
    q = np.concatenate([q, r])
    zr, zi, wr, wi = (np.ascontiguousarray(q[:, k]) for k in range(4))
    n = len(zr)
    for op in ("div", "scalar_div"):
        hdr, ref = np.zeros((n, 2)), np.zeros((n, 2))
        assert lib.p3_cx_op(OPS[op], n, _dp(zr), _dp(zi), _dp(wr), _dp(wi), _dp(hdr), _dp(ref)) == 0
        bad = np.flatnonzero(~same_bits(hdr, ref).all(axis=1))
        assert len(bad) == 0, (op, len(bad), [(q[k].tolist(), hdr[k].tolist(), ref[k].tolist()) for k in bad[:5]])


# --------------------------------------------------------------------------------------------------- the solver
def image_vectors(K, uv):
    """calculateImageVectors (PE:1072-1085) in numpy: the operations of prep_blob, in its order."""
    v = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(uv))], axis=1)
    n = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return v / n[:, None]


def solve_n(lib, fv, wp):
    n = len(fv)
    fv, wp = np.ascontiguousarray(fv, dtype=np.float64), np.ascontiguousarray(wp, dtype=np.float64)
    sol, rc = np.zeros((n, 4, 12)), np.zeros(n, dtype=np.int32)
    lib.p3_p3p_n(n, _dp(fv), _dp(wp), _dp(sol), rc.ctypes.data_as(IP))
    return rc, sol


def oracle_n(fv, wp):
    n = len(fv)
    sol, rc = np.zeros((n, 4, 12)), np.zeros(n, dtype=np.int32)
    for i in range(n):
        rc[i], sol[i] = orc.p3p(fv[i], wp[i])
    return rc, sol


@pytest.fixture(scope="module")
def sweep():
    """20,000 three-point problems from the 16-LED model: (fv, wp), n x 3 x 3 each."""
    rng = np.random.default_rng(0)
    K = syn.K_README
    mk = syn.markers_for(16)
    n = 20_000
    fv, wp = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    for it in range(n):
        w = mk[rng.choice(16, 3, replace=False)]
        if it % 4 == 0:  # a true projection, every other one with 0.3 px of noise
            T = syn.se3_exp(np.r_[rng.normal(size=3) * 0.3, rng.normal(size=3) * 0.5])
            T[:3, 3] += [0, 0, 2]
            uv = syn.project(K, T, w) + (rng.normal(size=(3, 2)) * 0.3 if it % 8 == 0 else 0)
        else:
            uv = np.c_[rng.uniform(0, 752, 3), rng.uniform(0, 480, 3)]
        uv = uv.astype(np.float32).astype(np.float64)
        fv[it], wp[it] = orc.image_vectors(K, uv), w
    return fv, wp


@pytest.fixture(scope="module")
def sweep_solutions(lib, sweep):
    fv, wp = sweep
    return solve_n(lib, fv, wp), oracle_n(fv, wp)


def test_image_vectors_generator_equals_oracle(sweep):
    """This module's numpy image vectors (used where the oracle must stay out) are the oracle's, bit for bit."""
    rng = np.random.default_rng(3)
    uv = np.c_[rng.uniform(-50, 800, 500), rng.uniform(-50, 530, 500)].astype(np.float32).astype(np.float64)
    assert same_bits(image_vectors(syn.K_README, uv), orc.image_vectors(syn.K_README, uv)).all()


def test_solver_equals_oracle_bit_for_bit(sweep_solutions):
    (rc, sol), (rc_o, sol_o) = sweep_solutions
    assert np.array_equal(rc, rc_o)
    assert (rc == 0).all()
    ok = same_bits(sol, sol_o).reshape(len(sol), -1).all(axis=1)
    finite = np.isfinite(sol).all(axis=2)
    with_nan = (~np.isfinite(sol_o).all(axis=2)).any(axis=1)
    diff = np.abs(sol - sol_o)[finite & np.isfinite(sol_o).all(axis=2)]
    print(f"{(~ok).sum()} of {len(sol)} problems differ; largest difference of a finite entry "
          f"{diff.max() if diff.size else 0.0:.3g}; {with_nan.sum()} problems have a non-finite solution")
    assert with_nan.sum() >= len(sol) // 10  # the non-finite roots do occur
    assert np.array_equal(finite, np.isfinite(sol_o).all(axis=2))
    assert ok.all(), np.flatnonzero(~ok)[:10].tolist()


# 16 x the largest difference of a finite entry measured over the sweep with the device's arithmetic on the host
DEVICE_MATH_BOUND = 16 * MEASURED_DEVICE_MATH


def test_solver_with_device_arithmetic_stays_near_oracle(lib_device_math, sweep, sweep_solutions):
    """The kernels keep log(hypot) for clog and Smith's division without safeguards (the restated glibc / libgcc
    forms cost 13 % of k_p3p_hist's time).  Built that way for the host, the solver is not bit-equal to
    the oracle: the finite / non-finite pattern is the oracle's, and finite entries stay within 16 x the largest
    difference measured over this sweep."""
    fv, wp = sweep
    rc, sol = solve_n(lib_device_math, fv, wp)
    _, (rc_o, sol_o) = sweep_solutions
    assert np.array_equal(rc, rc_o)
    fin, fin_o = np.isfinite(sol).all(axis=2), np.isfinite(sol_o).all(axis=2)
    differ = (~same_bits(sol, sol_o).reshape(len(sol), -1).all(axis=1)).sum()
    d = np.abs(sol - sol_o)[fin & fin_o]
    print(f"device arithmetic: {differ} of {len(sol)} problems differ in some bit; largest difference {d.max():.3g}")
    assert np.array_equal(fin, fin_o)
    assert d.max() <= DEVICE_MATH_BOUND


def test_collinear_world_points_return_false(lib):
    fv = orc.image_vectors(syn.K_README, np.array([[100.0, 120.0], [300.0, 200.0], [420.0, 310.0]]))
    for w in ([[0, 0, 0], [0.125, 0, 0], [0.25, 0, 0]],
              [[0.5, 0.25, -0.125], [0.75, 0.5, 0.0], [1.0, 0.75, 0.125]],
              [[0.25, 0.5, 1.0], [0.25, 0.5, 1.0], [0.0, 0.125, 0.5]]):  # two points equal
        w = np.array(w, dtype=np.float64)
        rc, _ = solve_n(lib, fv[None], w[None])
        assert rc[0] == -1
        assert orc.p3p(fv, w)[0] == -1


def test_identical_feature_vectors_give_nan(lib):
    fv = orc.image_vectors(syn.K_README, np.array([[100.0, 120.0], [100.0, 120.0], [420.0, 310.0]]))
    w = syn.markers_for(16)[[0, 5, 9]]
    rc, sol = solve_n(lib, fv[None], w[None])
    rc_o, sol_o = orc.p3p(fv, w)
    assert rc[0] == 0 and rc_o == 0
    assert np.isnan(sol).all() and np.isnan(sol_o).all()
    assert lib.p3_finite12(_dp(np.ascontiguousarray(sol[0, 0]))) == 0


def test_finite12(lib):
    a = np.arange(12, dtype=np.float64)
    assert lib.p3_finite12(_dp(a)) == 1
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 5, 11):
            b = a.copy()
            b[k] = bad
            assert lib.p3_finite12(_dp(b)) == 0


def test_inverse34_equals_oracle(lib, sweep_solutions):
    _, (_, sol_o) = sweep_solutions
    poses = sol_o[np.isfinite(sol_o).all(axis=2)][:4000]
    assert len(poses) == 4000
    inv = np.zeros(12)
    for p in poses:
        p = np.ascontiguousarray(p)
        lib.p3_inverse34(_dp(p), _dp(inv))
        assert same_bits(inv, orc.inverse44(p)[:3].reshape(12)).all()


def project_pair(lib, K, T44, X):
    uv = np.zeros(2)
    K, T44, X = (np.ascontiguousarray(a, dtype=np.float64) for a in (K, T44, X))
    lib.p3_project(_dp(K.reshape(9)), _dp(T44.reshape(16)[:12].copy()), _dp(X), _dp(uv))
    return uv, orc.project44(K, T44, X)


def same_projection(a, b):
    """Bit-equal but for the sign of a zero: the header drops the oracle's "+ 0.0 * T(3, j)" (pf_p3p.hpp, project)."""
    return bool((same_bits(a, b) | ((a == 0.0) & (b == 0.0))).all())


def test_project_equals_oracle(lib, sweep_solutions):
    _, (_, sol_o) = sweep_solutions
    poses = sol_o[np.isfinite(sol_o).all(axis=2)][:1500]
    mk = syn.markers_for(16)
    K2 = np.array([[612.25, 0.0, 301.5], [0.0, 587.75, 255.125], [0.0, 0.0, 1.0]])
    n = 0
    for i, p in enumerate(poses):
        T = orc.inverse44(p)
        for K in (syn.K_README, K2):
            for X in mk[[i % 16, (i * 7 + 3) % 16]]:
                a, b = project_pair(lib, K, T, X)
                assert same_projection(a, b), (i, a, b)
                n += 1
    assert n == 6000


def test_project_on_and_behind_the_camera_plane(lib):
    K = syn.K_README
    for R in (np.eye(3), syn.rot_z(0.4) @ syn.rot_x(-0.3), -np.eye(3)):
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = [0.25, -0.125, 0.0]
        Rt = R.T
        # camera-frame points (x, y, z) with z = 0 exactly (on the plane) and z < 0 (behind)
        for cam in ([0.5, 0.25, 0.0], [-0.5, 0.125, 0.0], [0.0, 0.0, 0.0], [0.25, -0.5, -1.0], [0.0, 0.0, -2.0]):
            X = Rt @ (np.array(cam) - T[:3, 3])
            a, b = project_pair(lib, K, T, X)
            assert same_projection(a, b), (cam, a, b)
    # z exactly zero through exact arithmetic: identity rotation, dyadic numbers
    T = np.eye(4)
    T[:3, 3] = [0.25, -0.125, -1.5]
    for X in ([0.5, 0.25, 1.5], [-0.5, 0.125, 1.5], [-0.25, 0.125, 1.5], [0.5, 0.5, 0.5]):
        a, b = project_pair(lib, K, T, np.array(X))
        assert same_projection(a, b), (X, a, b)
        if X[2] == 1.5:
            assert not np.isfinite(a).any()  # x / 0 or 0 / 0
        else:
            want = syn.project(K, T, np.array([X]))[0]  # behind the camera: the mirrored pixel, finite
            assert np.allclose(a, want, rtol=1e-12, atol=1e-9)


# ------------------------------------------------------------------ a check that does not rest on the oracle
def true_pose_problems(n=5000, seed=7):
    rng = np.random.default_rng(seed)
    mk = syn.markers_for(16)
    K = syn.K_README
    fv, wp, truth = np.zeros((n, 3, 3)), np.zeros((n, 3, 3)), np.zeros((n, 12))
    for it in range(n):
        w = mk[rng.choice(16, 3, replace=False)]
        a = rng.uniform(-1.0, 1.0, 3)
        T = np.eye(4)
        T[:3, :3] = syn.rot_z(a[2]) @ syn.rot_y(a[1]) @ syn.rot_x(a[0])
        T[:3, 3] = [rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4), rng.uniform(0.6, 5.0)]
        fv[it], wp[it] = image_vectors(K, syn.project(K, T, w)), w  # exact double projections: no rounding to float32
        truth[it] = syn.rigid_inv(T)[:3].reshape(12)  # the solver returns [R | C]: camera in the object's frame
    return fv, wp, truth


def best_errors(sol, truth):
    """Per problem: the smallest, over the finite solutions, of the largest entry difference to the truth."""
    finite = np.isfinite(sol).all(axis=2)
    err = np.where(finite, np.abs(np.where(finite[:, :, None], sol, 0.0) - truth[:, None, :]).max(axis=2), np.inf)
    return err.min(axis=1)


def test_true_poses_are_recovered(lib):
    fv, wp, truth = true_pose_problems()
    rc, sol = solve_n(lib, fv, wp)
    assert (rc == 0).all()
    err = best_errors(sol, truth)
    rc_o, sol_o = oracle_n(fv, wp)
    err_o = best_errors(sol_o, truth)
    for name, e in (("header", err), ("oracle", err_o)):
        print(f"{name}: misses {100 * (e > 1e-8).mean():.2f} % at 1e-8, {100 * (e > 1e-6).mean():.2f} % at 1e-6, "
              f"median {np.median(e):.2g}")
    assert (err > 1e-8).mean() <= 0.02


# ---------------------------------------------------------------------------------------------- the index maps
def unrank(lib, r):
    r = np.ascontiguousarray(r, dtype=np.int64)
    out = np.zeros((len(r), 3), dtype=np.int32)
    lib.p3_unrank3(len(r), r.ctypes.data_as(LP), out.ctypes.data_as(IP))
    return out


def test_c3_c2(lib):
    for n in range(0, 1030):
        assert lib.p3_c3(n) == math.comb(n, 3)
        assert lib.p3_c2(n) == math.comb(n, 2)


def test_unrank3_inverts_the_colex_rank_up_to_64_blobs(lib):
    want = np.array([(a, b, c) for c in range(64) for b in range(c) for a in range(b)], dtype=np.int32)
    assert len(want) == math.comb(64, 3)
    got = unrank(lib, np.arange(len(want)))
    assert np.array_equal(got, want)  # colex order: sorted by c, then b, then a; B only cuts the list off


def test_unrank3_at_every_boundary_of_1024_blobs(lib):
    c = np.repeat(np.arange(2, 1024), np.arange(2, 1024) - 1)  # every (b, c) with 1 <= b < c
    b = np.concatenate([np.arange(1, k) for k in range(2, 1024)])
    c, b = c.astype(np.int64), b.astype(np.int64)
    first = c * (c - 1) * (c - 2) // 6 + b * (b - 1) // 2  # rank of (0, b, c): the first of its (b, c) run
    got = unrank(lib, first)
    assert np.array_equal(got, np.stack([np.zeros_like(b), b, c], axis=1))
    last = unrank(lib, first + b - 1)  # (b - 1, b, c): the last of the run, the rank before the next boundary
    assert np.array_equal(last, np.stack([b - 1, b, c], axis=1))
    before = unrank(lib, first[1:] - 1)  # the neighbour below each boundary is the last of the run before
    assert np.array_equal(before, last[:-1])
    assert first[-1] + b[-1] == math.comb(1024, 3)
    assert np.array_equal(unrank(lib, [math.comb(1024, 3) - 1])[0], [1021, 1022, 1023])


@pytest.mark.parametrize("M", range(3, 17))
def test_perm3_is_a_bijection(lib, M):
    n = M * (M - 1) * (M - 2)
    out = np.full((n, 3), -1, dtype=np.int32)
    lib.p3_perm3_all(M, out.ctypes.data_as(IP))
    assert set(map(tuple, out.tolist())) == set(itertools.permutations(range(M), 3))


@pytest.mark.parametrize("M", range(3, 17))
def test_unused_markers_is_the_ascending_complement(lib, M):
    maxu = 2 if M <= 5 else 9 if M <= 12 else 13  # the kernel instance that serves M
    un = np.zeros(maxu, dtype=np.int32)
    for t in itertools.permutations(range(M), 3):
        assert lib.p3_unused(maxu, t[0], t[1], t[2], un.ctypes.data_as(IP)) == 0
        assert un[:M - 3].tolist() == [m for m in range(M) if m not in t]
