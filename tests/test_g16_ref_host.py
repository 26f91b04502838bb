"""The plain-integer references of tests/_g16_ref.py against each other, before tests/test_gpu_g16_kernels.py lets them judge the decider's kernels: the
radix-2 recursion against the O(n²) definition, the quotient step by step on the coset against the schoolbook product, the quotient's defining identity
at random points, the closed form of the multi-scalar sum against the sum point by point.  No GPU."""
import random

import pytest

from tests import _g16_ref as G
from tests._pairing import G2, R, g2_add, g2_mul, g2_on_curve


@pytest.mark.parametrize("logn", range(1, G.DFT_MAX_LOGN + 1))
def test_ntt_is_the_dft(logn):
    w = G.omega(logn)
    assert pow(w, 1 << logn, R) == 1 and pow(w, 1 << (logn - 1), R) == R - 1
    for name, v in G.transform_cases(logn).items():
        if logn > 6 and name not in ("random", "e_1", "e_last"):
            continue
        for root in (w, pow(w, -1, R)):
            assert G.ntt(v, root) == G.dft(v, root), name
    v = G.transform_cases(logn)["random"]
    assert G.ntt(G.ntt(v, w), pow(w, -1, R)) == [(x << logn) % R for x in v]


@pytest.mark.parametrize("logn", [1, 2, 3, 5, 6])
def test_quotient_pipeline_is_the_schoolbook_quotient(logn):
    n = 1 << logn
    cases = G.quotient_cases(logn)
    assert sum(sat for _, _, _, sat in cases.values()) == len(cases) - 1 >= 5
    for name, (a, b, c, sat) in cases.items():
        h = G.quotient_pipeline(a, b, c, logn)
        if not sat:
            with pytest.raises(AssertionError):
                G.quotient_schoolbook(a, b, c, logn)
            continue
        assert h == G.quotient_schoolbook(a, b, c, logn), name
        assert len(h) == n and h[n - 1] == 0, name
    assert not any(G.quotient_pipeline(*cases["constant"][:3], logn))
    assert G.quotient_pipeline(*cases["top_degree"][:3], logn) == G.unit(n, n - 2)


def test_quotient_identity_at_random_points():
    logn = 10
    points = G.identity_points(logn)
    assert len(points) == 2
    for name, (a, b, c, sat) in G.quotient_cases(logn).items():
        h = G.quotient_pipeline(a, b, c, logn)
        for x in points:
            assert G.quotient_identity_holds(a, b, c, h, logn, x) == sat, name
        if sat:
            assert h[-1] == 0
            wrong = list(h)
            wrong[0] = (wrong[0] + 1) % R
            assert not G.quotient_identity_holds(a, b, c, wrong, logn, points[0]), name


def test_barycentric_weights_evaluate_a_polynomial():
    logn = 4
    rng = random.Random("g16/host/barycentric")
    coef = [rng.randrange(R) for _ in range(1 << logn)]
    values = G.dft(coef, G.omega(logn))
    x = rng.randrange(2, R)
    assert G.dot(G.barycentric_weights(x, logn), values) == G.horner(coef, x)
    assert G.interpolate(values, logn) == coef
    assert G.coset_extend(values, logn) == [G.horner(coef, G.GEN * pow(G.omega(logn), i, R) % R) for i in range(1 << logn)]


def test_msm_closed_form_is_the_explicit_sum():
    rng = random.Random("g16/host/msm")
    k = [rng.randrange(1, R) for _ in range(5)]
    pts = [g2_mul(G2, x) for x in k]
    assert all(g2_on_curve(p) for p in pts)
    case = {"bases": [1, -2, 3, 0, 5], "scalars": [rng.randrange(R) for _ in range(5)], "form": 1}
    want = G.msm_explicit(case, pts)
    assert want is not None and want == g2_mul(G2, G.msm_multiplier(case, k))
    acc = None
    for s, p, sign in zip(case["scalars"], pts, (1, -1, 1, 0, 1)):
        acc = g2_add(acc, g2_mul(p, sign * s % R))
    assert acc == want
    assert g2_mul(G2, R - 1) == G.g2_neg(G2) and g2_mul(G2, R) is None
    assert G.g2_from_words(G.g2_words(want)) == want and G.g2_words(None) == [0, 0, 0, 0]


def test_case_lists():
    for logn in G.TRANSFORM_LOGN:
        if logn > 10:
            continue
        n = 1 << logn
        tc, qc = G.transform_cases(logn), G.quotient_cases(logn)
        assert len(tc) == 8 and len(qc) == 6
        for v in list(tc.values()) + [v for a, b, c, _ in qc.values() for v in (a, b, c)]:
            assert len(v) == n and all(0 <= x < R for x in v)
    sp = G.fixed_special_scalars()
    assert len(sp) == 83 and sp[:6] == [0, 1, 2, 15, 16, 17] and (3 << 252) in sp and (3 << 252) < R < (4 << 252)
    for n in G.FIXED_N:
        s = G.fixed_scalars(n)
        assert len(s) == n and all(0 <= x < R for x in s)
    assert G.fixed_scalars(129)[:83] == sp and G.fixed_scalars(1)[0] != 0
    pool, cases = G.msm_pool_scalars(), G.msm_cases()
    assert len(pool) == G.MSM_POOL and all(0 < x < R for x in pool)
    assert len(cases) == len(G.MSM_N) + 1 + 6 * len(G.MSM_EDGE_N) + 5 + 3 and G.MSM_REPEAT in cases
    for name, c in cases.items():
        n = len(c["scalars"])
        assert 0 < n == len(c["bases"]) <= G.MSM_POOL and all(0 <= s < R for s in c["scalars"]) and all(abs(b) <= G.MSM_POOL for b in c["bases"]), name
        wires, idx = G.msm_layout(c)
        assert len(wires) == 2 * n + 3 and [wires[i] for i in idx] == c["scalars"] and max(idx) < len(wires), name
    top = cases["top_plane/65"]["scalars"]
    assert top[0] == 1 << 253 < R
    assert G.msm_multiplier(cases["cancel_restart"], pool) == 64 * pool[0] % R and G.msm_multiplier(cases["same_base"], pool) == G.MSM_POOL * pool[0] % R
    assert G.msm_multiplier(cases["tree_cancel"], pool) == 32 * pool[1] % R and G.msm_multiplier(cases["horner_cancel"], pool) == 0
    d = cases["density/4160"]["scalars"]
    assert d[0] == d[64] == 0 and bin(d[63]).count("1") > 200 > 64 > bin(d[8]).count("1") > 0
