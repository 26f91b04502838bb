"""tests/_mlkzg_ref.py checked against the definitions it restates (no GPU, no library): the fold against the multilinear evaluation by brute force, every fold
equation of the verifier on the prover's evaluations, the remainder rule of the three divisions, the chunked division's carries against the plain recurrence, and the
pairing equation in the exponent — with tau known, e(L, G2) = e(Rr, [tau]G2) is L = tau·Rr, on scalars and on the points pairing_sides forms."""
import random

import pytest

from tests import _mlkzg_ref as M
from tests._pairing import G1, R, g1_mul

CASES = [(logn, n) for logn in (1, 2, 3, 5) for n in sorted({1, 2, (1 << logn) - 1, 1 << logn}) if 1 <= n <= 1 << logn]


def _case(logn, n, edge=False):
    rng = random.Random(f"mlkzg/ref/{logn}/{n}/{edge}")
    v = [rng.randrange(R) for _ in range(n)]
    x = [rng.randrange(R) for _ in range(logn)]
    if edge:
        x = [(0, 1, R - 1)[k % 3] for k in range(logn)]
        v[0] = R - 1
    return rng.randrange(1, R), v, x


@pytest.mark.parametrize("logn,n", CASES)
@pytest.mark.parametrize("edge", (False, True))
def test_the_fold_is_the_multilinear_evaluation(logn, n, edge):
    _, v, x = _case(logn, n, edge)
    P = M.fold_levels(v + [0] * ((1 << logn) - n), x)
    assert [len(p) for p in P] == [1 << (logn - k) for k in range(logn + 1)]
    assert P[logn] == [M.mle_eval(v, x)]


@pytest.mark.parametrize("logn,n", CASES)
def test_fold_equations_remainders_and_the_pairing_equation_in_the_exponent(logn, n):
    tau, v, x = _case(logn, n)
    pr = M.prove(tau, v, logn, x)
    assert pr["eval"] == M.mle_eval(v, x) and len(pr["proof"]) == M.proof_words(logn)
    assert M.point_of(pr["comm"]) == g1_mul(G1, M.horner(v, tau))
    r, q, d = pr["r"], pr["q"], pr["d"]
    assert 0 < r < 1 << 128 and q < 1 << 128 and d < 1 << 128
    assert M.fold_equations(x, pr["eval"], pr["E"], r) == [True] * logn
    bad = [row[:] for row in pr["E"]]
    bad[0][logn - 1] = (bad[0][logn - 1] + 1) % R
    assert M.fold_equations(x, pr["eval"], bad, r)[logn - 1] is False
    us = [r, -r % R, r * r % R]
    cb = sum(pow(q, k, R) * M.horner(pr["levels"][k], tau) for k in range(logn)) % R
    assert cb == M.horner(pr["B"], tau)
    L = Rr = 0
    for j, u in enumerate(us):
        quot, rem = M.divide(pr["B"], u)
        assert rem == M.horner(pr["B"], u) == M.horner(pr["E"][j], q) == pr["remainders"][j]
        # Q·(X − u) + rem = B, coefficient by coefficient
        back = [(-u * c) % R for c in quot] + [0]
        for i, c in enumerate(quot):
            back[i + 1] = (back[i + 1] + c) % R
        back[0] = (back[0] + rem) % R
        assert back == pr["B"]
        w = M.horner(quot, tau)
        L = (L + pow(d, j, R) * (cb - rem + u * w)) % R
        Rr = (Rr + pow(d, j, R) * w) % R
    assert L == tau * Rr % R
    P = M.parse([0] * 16, pr["comm"], logn, pr["point_words"], M.words_of(pr["eval"]), pr["proof"])
    Lp, Rp = M.pairing_sides(P, r, q, d)
    assert Lp == g1_mul(G1, L) and Rp == g1_mul(G1, Rr) and Lp == (g1_mul(Rp, tau) if Rp else None)


@pytest.mark.parametrize("n", (1, 2, 7, 8, 9, 31, 32, 33))
@pytest.mark.parametrize("u", (0, 1, R - 1, 0x1234567890ABCDEF1234567890ABCDEF))
def test_the_chunked_division_s_carries(n, u):
    rng = random.Random(f"mlkzg/carries/{n}")
    b = [rng.randrange(R) for _ in range(n)]
    quot, rem = M.divide(b, u)
    out, cin = M.division_carries(b, u, 4)
    full = [rem] + quot + [0]                                    # s_0 .. s_n of the recurrence
    for t in range(len(out)):
        assert cin[t] == full[min(4 * (t + 1), n)]
        assert (out[t] + pow(u, 4, R) * cin[t]) % R == full[4 * t]
    assert M.eval3(b, u) == [M.horner(b, u), M.horner(b, R - u if u else 0), M.horner(b, u * u % R)]
