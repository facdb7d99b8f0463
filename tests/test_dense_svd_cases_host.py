"""The fixtures and checks of the dense SVD tests (tests/dense_svd_cases.py), on the CPU: the builders are what they claim; every
check accepts LAPACK's own factors of every case, so the reference passes each bound before the device is asked to; a check
rejects factors that the older tests (S, reconstruction, V^T V) cannot tell from converged ones; the scalar model of the kernel's
acceptance rule reaches the contract's bound to within its constant."""
import numpy as np
import pytest

import dense_svd_cases as C

EPS = C.EPS


# ------------------------------------------------------------------------------------------------------------- builders
def test_edge_shapes_cover_the_block_and_chunk_edges():
    assert len(C.EDGE_SHAPES) == 77 and all(m >= n for m, n in C.EDGE_SHAPES)
    nblocks = {n: -(-n // 16) for n in C.EDGE_N}
    assert {1, 2, 3, 4, 5} == set(nblocks.values())                                  # odd real block counts get a padding block
    assert {n % 16 for n in C.EDGE_N} == {15, 0, 1}                                  # a short block, full blocks, one live column
    assert {-(-m // 128) for m in C.EDGE_M} == {1, 2, 3} and {-(-m // 256) for m in C.EDGE_M} == {1, 2}
    assert all((n, m) in C.EDGE_SHAPES and m < n for m, n in C.WIDE_SHAPES) and len(C.WIDE_SHAPES) == 5


@pytest.mark.parametrize("name,smallest", [("graded300_1e-6", 1e-6), ("graded300_1e-10", 1e-10), ("graded300_1e-14", 1e-14)])
def test_graded_has_its_singular_values(name, smallest):
    A = C.named(name)
    S = np.linalg.svd(A, compute_uv=False)
    assert A.shape == (300, 300)
    assert np.max(np.abs(S - np.geomspace(1.0, smallest, 300))) <= 300 * EPS
    assert (3 * 300 * EPS * S[0] / S[-1] < 1e-6) == C.NAMED[name][1] or smallest < 1e-12
    rng = np.random.default_rng(9)                                                    # `_graded(300, 9, smallest)` of test_gpu_direct.py
    Q1 = np.linalg.qr(rng.standard_normal((300, 300)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((300, 300)))[0]
    assert np.array_equal(A, (Q1 * np.geomspace(1.0, smallest, 300)) @ Q2.T)


def test_structured_builders():
    assert not np.any(C.zero()) and max(C.zero().shape) <= 64
    R = C.rank_one()
    assert R.shape == (64, 48) and np.linalg.matrix_rank(R) == 1
    S = np.linalg.svd(C.repeated(), compute_uv=False)
    assert C.repeated().shape == (64, 48) and np.max(np.abs(S - C.REPEATED_SIGMA)) <= 64 * EPS * 3
    d = C.diag_entries()
    D = C.diag_top()
    assert D.shape == (50, 33) and np.array_equal(D[:33], np.diag(d)) and not np.any(D[33:])
    assert np.sum(d < 0) == 1 and np.sum(d == 0) == 1 and np.unique(np.abs(d)).size == 32 and np.any(np.diff(np.abs(d)) < 0)
    assert C.blur576().shape == (576, 576)


def test_sqrt_of_a_rounded_square_is_exact():
    """What makes S of the diagonal case exact: sqrt(fl(d^2)) == |d| for float64 away from the ends of the range."""
    rng = np.random.default_rng(0)
    d = np.ldexp(rng.uniform(0.5, 1.0, 200_000), rng.integers(-400, 400, 200_000))
    assert np.array_equal(np.sqrt(d * d), d)


@pytest.mark.parametrize("name", C.SCALE_CASES)
@pytest.mark.parametrize("k", [-600, -300, -60, 60, 300, 600])
def test_power_of_two_scaling_is_exact(name, k):
    A = C.named(name)
    B = C.scaled(A, k)
    assert np.all(np.isfinite(B)) and np.array_equal(np.ldexp(B, -k), A)
    assert np.all(np.abs(B[B != 0]) > np.finfo(np.float64).tiny)
    if abs(k) <= 300:
        # no product of two entries is subnormal or overflows: the unscaled iteration sees the same roundings at every k
        lo, hi = np.min(np.abs(B[B != 0])), np.max(np.abs(B))
        assert lo * lo > 1e-250 and hi * hi < 1e250
    else:
        with np.errstate(over="ignore", under="ignore"):
            assert np.max(np.abs(B)) ** 2 in (0.0, np.inf)                            # out of the range in which entries can be squared
    # LAPACK is right at every scale: the reference of the device tests
    S0, S = np.linalg.svd(A, compute_uv=False), np.linalg.svd(B, compute_uv=False)
    assert np.max(np.abs(np.ldexp(S, -k) - S0)) <= 8 * max(A.shape) * EPS * S0[0]


# ------------------------------------------------------------------------------------------ the checks on LAPACK's factors
def _all_cases():
    for name in C.NAMED:
        yield name, (lambda nm=name: C.named(nm)), C.NAMED[name][1], C.NAMED[name][2]
    for m, n in C.EDGE_SHAPES + C.WIDE_SHAPES:
        yield f"gauss{m}x{n}", (lambda mm=m, nn=n: C.gaussian(mm, nn)), True, True
    for name in C.SCALE_CASES:
        for k in (-600, 600):
            yield f"{name}@2^{k}", (lambda nm=name, kk=k: C.scaled(C.named(nm), kk)), C.NAMED[name][1], True


CASES = list(_all_cases())


@pytest.mark.parametrize("name,build,bound_utu,vectors", CASES, ids=[c[0] for c in CASES])
def test_lapack_factors_pass_every_check(name, build, bound_utu, vectors):
    A = build()
    U, S, Vh = C.lapack_factors(A)
    C.check_against_lapack(A, U, S, Vh, vectors=vectors)
    C.check_reconstruction(A, U, S, Vh)
    C.check_rotation_orthogonal(A, U, Vh)
    r_g, r_diag, r_utu = C.check_contract(A, U, S, Vh, bound_utu)
    assert (r_utu is not None) == bound_utu


def test_diagonal_case_check_accepts_the_exact_factors():
    """LAPACK may put the sign of a negative diagonal entry in either factor; what the Jacobi iteration must return is the one
    answer that rotates nothing: V a permutation, the sign in U."""
    d = C.diag_entries()
    order = np.argsort(-np.abs(d), kind="stable")
    S = np.abs(d)[order]
    Vh = np.eye(33)[order]
    U = np.zeros((50, 33))
    U[order, np.arange(33)] = np.sign(d[order])
    assert np.array_equal((U * S) @ Vh, C.diag_top())
    C.check_diag_top(U, S, Vh)
    C.check_contract(C.diag_top(), U, S, Vh, False)
    with pytest.raises(AssertionError):
        C.check_diag_top(-U, S, -Vh)                                                  # the sign in V
    G, sweeps = C.jacobi_model(C.diag_top(), 64 * EPS)
    assert sweeps == 1


# ------------------------------------------------------------------------------------------- the checks reject wrong factors
def test_contract_rejects_an_unconverged_u_that_the_older_checks_accept():
    """Rotate two columns of G = U S against one another by 1e-8 and V along with them: A = U S V^T and V^T V = I hold as before
    and S moves by 1e-16 (second order), but u_i . u_j is 1e-8."""
    A = C.named("gauss257x100")
    U, S, Vh = C.lapack_factors(A)
    t = 1e-8
    c, s = np.cos(t), np.sin(t)
    G, V = U * S, Vh.T.copy()
    i, j = 0, 99
    for X in (G, V):
        X[:, i], X[:, j] = c * X[:, i] - s * X[:, j], s * X[:, i] + c * X[:, j]
    S2 = np.linalg.norm(G, axis=0)
    U2, Vh2 = G / S2, V.T
    C.check_against_lapack(A, U2, S2, Vh2)
    with pytest.raises(AssertionError):
        C.check_contract(A, U2, S2, Vh2, True)
    with pytest.raises(AssertionError):
        C.check_contract(A, U2, S2, Vh2, False)                                       # the g form alone sees it too


def test_contract_rejects_a_vector_beside_a_zero_singular_value():
    A = C.zero()
    U, S, Vh = np.linalg.svd(A, full_matrices=False)
    with pytest.raises(AssertionError):
        C.check_contract(A, U, S, Vh, False)


def test_checks_are_not_fooled_by_overflow():
    """At 2^600 the norms of the older check are Inf <= Inf; these must still reject a wrong S."""
    A = C.scaled(C.named("gauss257x100"), 600)
    U, S, Vh = C.lapack_factors(A)
    with pytest.raises(AssertionError):
        C.check_reconstruction(A, U, S * (1 + 1e-9), Vh)
    with pytest.raises(AssertionError):
        C.check_against_lapack(A, U, np.zeros_like(S), Vh)


# ----------------------------------------------------------------------------------------------------- the scalar model
@pytest.mark.parametrize("smallest", [None, 1e-6, 1e-10, 1e-14])
def test_model_reaches_the_contract_bound(smallest):
    """Why the constant is 3 and not 30: the acceptance rule alone (no Gram rounding of a blocked kernel, G not formed again from
    U and S) already leaves |u_i . u_j| at 0.97 tol sigma_big / sigma_small."""
    A = C.gaussian(70, 40, 7040) if smallest is None else C.graded(70, 40, 7040, smallest)
    ratio, sweeps = C.model_ratio(A)
    print(f"model 70 x 40 {'gaussian' if smallest is None else f'graded to {smallest:g}'}: {sweeps} sweeps, "
          f"max |u_i . u_j| / (tol sigma_big / sigma_small) = {ratio:.3f}")
    assert 0.0 < ratio <= 1.5


# ------------------------------------------------------------------------------------------------------------------ gemv
def test_gemv_reference_and_bound():
    A, x, d, y0 = C.gemv_operands(257, 40, True, 1)
    ref, bound = C.gemv_reference(True, A, x, d, -0.5, 2.0, y0)
    got = 2.0 * y0 - 0.5 * (A.T @ (d * x))
    assert ref.dtype == np.longdouble and ref.shape == (40,) and np.all(np.abs(got - ref) <= bound) and np.all(bound > 0)
    assert np.all(bound < 1e-10)
    ref0, bound0 = C.gemv_reference(False, A, y0, None, 1.0, 0.0, np.full(257, np.nan))
    assert np.all(np.isfinite(ref0.astype(np.float64))) and np.all(np.abs(A @ y0 - ref0) <= bound0)
    wrong = got.copy()
    wrong[3] += 1e-10
    assert not np.all(np.abs(wrong - ref) <= bound)
