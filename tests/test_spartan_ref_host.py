"""The integer prover of tests/_spartan_ref.py — what tests/test_gpu_spartan_kernels.py measures the compressed proof's kernels against — checked on the CPU
against definitions it does not share code with: the eq table against the product formula, the sum-check messages against brute-force sums over the hypercube,
the bound values against multilinear extensions evaluated by definition, the folded bases against the CPU oracle's curve arithmetic, and every instance case's
bytes against the independent verifier of tests/_spartan.py (accepted as written, rejected with one bit flipped in each part of the argument).

Cases skipped here: none — (513, 512) runs on both curves."""
import itertools
import random

import pytest

from tests import _oracle
from tests import _spartan_ref as S


@pytest.fixture(scope="module")
def orc():
    return _oracle.load()


def eq_by_definition(pt, i, p):
    k, acc = len(pt), 1
    for q, r in enumerate(pt):
        acc = acc * (r if (i >> (k - 1 - q)) & 1 else 1 - r) % p
    return acc


def mle(v, pt, p):
    """the multilinear extension of v at pt, by definition"""
    return sum(x * eq_by_definition(pt, i, p) for i, x in enumerate(v) if x) % p


@pytest.mark.parametrize("fid", [0, 1])
def test_eq_table_is_the_product_formula(fid):
    p = S.FIELD[fid]
    for k in (1, 2, 3, 8):
        for name in S.small_case_names("eq"):
            pt = S.small_case("eq", fid, k, name)["vecs"][0]
            tab = S.eq_table(pt, p)
            assert len(tab) == 1 << k and sum(tab) % p == 1
            for i, t in enumerate(tab):
                assert t == eq_by_definition(pt, i, p), (k, name, i)


def _partial_sums(vecs, u, fixed, k, p, term):
    """sum over the unbound variables of term(values at the point (fixed ‖ X ‖ x)) for X = 0, 1, 2, 3 — by the multilinear extensions' definition"""
    free = k - len(fixed) - 1
    out = []
    for X in range(4):
        acc = 0
        for bits in itertools.product((0, 1), repeat=free):
            pt = list(fixed) + [X] + list(bits)
            acc += term([mle(v, pt, p) for v in vecs], u)
        out.append(acc % p)
    return out


@pytest.mark.parametrize("fid", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_sumcheck_messages_against_brute_force(fid, k):
    p = S.FIELD[fid]
    rng = random.Random(f"host/sc/{fid}/{k}")
    n = 1 << k
    for has_e in (True, False):
        vecs = [[rng.randrange(p) for _ in range(n)] for _ in range(5 if has_e else 4)]
        u = rng.randrange(p)
        chal = [rng.randrange(p) for _ in range(k)]
        outer = lambda v, u_: v[0] * (v[1] * v[2] - u_ * v[3] - (v[4] if has_e else 0))      # noqa: E731
        msgs, fin = S.outer_rounds(*vecs[:4], vecs[4] if has_e else None, u, S.from_list(chal), p)
        claim = sum(outer([v[i] for v in vecs], u) for i in range(n)) % p
        for j, (s0, s2, s3) in enumerate(msgs):
            want = _partial_sums(vecs, u, chal[:j], k, p, outer)
            assert (s0, s2, s3) == (want[0], want[2], want[3]), (j, has_e)
            assert (want[0] + want[1]) % p == claim                        # s(0) + s(1) = claim
            claim = S.interp([s0, (claim - s0) % p, s2, s3], chal[j], p)
        assert fin[:len(vecs)] == [mle(v, chal, p) for v in vecs] and (has_e or fin[4] == 0)
        assert claim == outer(fin, u) % p
    m, z = ([rng.randrange(p) for _ in range(n)] for _ in range(2))
    chal = [rng.randrange(p) for _ in range(k)]
    inner = lambda v, u_: v[0] * v[1]      # noqa: E731
    msgs, fin = S.inner_rounds(m, z, S.from_list(chal), p)
    claim = sum(a * b for a, b in zip(m, z)) % p
    for j, (s0, s2) in enumerate(msgs):
        want = _partial_sums([m, z], None, chal[:j], k, p, inner)
        assert (s0, s2) == (want[0], want[2]) and (want[0] + want[1]) % p == claim
        claim = S.interp([s0, (claim - s0) % p, s2], chal[j], p)
    assert fin == [mle(m, chal, p), mle(z, chal, p)] and claim == fin[0] * fin[1] % p


@pytest.mark.parametrize("fid", [0, 1])
def test_every_small_case_is_consistent(fid):
    """at every case the GPU test runs (k <= 8 here; 9 and 10 are the same code on longer lists): the claims chain and the finals are the extensions' values"""
    p = S.FIELD[fid]
    for k in (1, 2, 3, 8):
        for name in S.small_case_names("outer"):
            c = S.small_case("outer", fid, k, name)
            eq, a, b, cc, e = c["vecs"]
            msgs, fin = S.outer_rounds(eq, a, b, cc, e, c["u"], S.from_list(c["chal"]), p)
            ez = e if e is not None else [0] * len(eq)
            claim = sum(q * (x * y - c["u"] * w - v) for q, x, y, w, v in zip(eq, a, b, cc, ez)) % p
            for (s0, s2, s3), r in zip(msgs, c["chal"]):
                claim = S.interp([s0, (claim - s0) % p, s2, s3], r, p)
            assert claim == fin[0] * (fin[1] * fin[2] - c["u"] * fin[3] - fin[4]) % p, (k, name)
            if k <= 3:
                assert fin == [mle(v, c["chal"], p) if v is not None else 0 for v in c["vecs"]]
        for name in S.small_case_names("inner"):
            c = S.small_case("inner", fid, k, name)
            msgs, fin = S.inner_rounds(*c["vecs"], S.from_list(c["chal"]), p)
            claim = sum(x * y for x, y in zip(*c["vecs"])) % p
            for (s0, s2), r in zip(msgs, c["chal"]):
                claim = S.interp([s0, (claim - s0) % p, s2], r, p)
            assert claim == fin[0] * fin[1] % p, (k, name)


@pytest.mark.parametrize("fid", [0, 1])
def test_ipa_vector_rounds_end_in_the_folded_claim(fid):
    p = S.FIELD[fid]
    for k in (1, 2, 3, 8):
        for name in S.small_case_names("ipa"):
            c = S.small_case("ipa", fid, k, name)
            a, b = c["vecs"]
            dots, (af, bf) = S.ipa_vec_rounds(a, b, S.from_list(c["chal"]), p)
            claim = sum(x * y for x, y in zip(a, b)) % p
            for (cl, cr), x in zip(dots, c["chal"]):
                claim = (cr + x * claim + x * x * cl) % p                 # <a', b'> = <a_R,b_L> + x·<a,b> + x²·<a_L,b_R>
            assert af * bf % p == claim, (k, name)
            # the final b is <s, b> for s_i = the product of the challenges of the rounds in which i sat in the right half (what the verifier computes)
            s = [1]
            for x in reversed(c["chal"]):
                s = s + [v * x % p for v in s]
            assert bf == sum(u * v for u, v in zip(s, b)) % p


def _orc_pt(P):
    return (0, 0) if P is None else P


@pytest.mark.parametrize("cid", [0, 1])
def test_fold_bases_against_the_oracle(orc, cid):
    p = S.CURVES[cid][0]
    assert all(S.on_curve(P, cid) for P in S.fold_pool(cid)) and len(set(S.fold_pool(cid))) == S.FOLD_POOL
    for name in S.fold_case_names():
        pts, x = S.fold_case(cid, name)
        half = len(pts) // 2
        got = S.fold_bases(cid, pts, x)
        assert len(got) == half and all(S.on_curve(P, cid) for P in got)
        for i in range(half):
            want = orc.curve_add(cid, _orc_pt(pts[i]), orc.curve_mul(cid, _orc_pt(pts[i + half]), x))
            assert _orc_pt(got[i]) == want, (name, i)
    # the planted pairs are what they are named for
    pts, x = S.fold_case(cid, "planted/64")
    got, at = S.fold_bases(cid, pts, x), S.PLANT
    hi = lambda i: pts[i + 64]      # noqa: E731
    assert pts[at["lo_identity"]] is None and got[at["lo_identity"]] == S.ec_mul(hi(at["lo_identity"]), x, p) is not None
    assert hi(at["hi_identity"]) is None and got[at["hi_identity"]] == pts[at["hi_identity"]] is not None
    assert pts[at["both_identity"]] is None and hi(at["both_identity"]) is None and got[at["both_identity"]] is None
    assert pts[at["doubling"]] == S.ec_mul(hi(at["doubling"]), x, p) and got[at["doubling"]] == S.ec_add(pts[at["doubling"]], pts[at["doubling"]], p) is not None
    assert got[at["cancel"]] is None and pts[at["cancel"]] is not None and S.pt_words(got[at["cancel"]]) == [0, 0]
    pts, x = S.fold_case(cid, "hi_is_lo_x=1/64")
    i = at["hi_is_lo"]
    assert x == 1 and pts[i] == pts[i + 64] and S.fold_bases(cid, pts, x)[i] == S.ec_mul(pts[i], 2, p)
    for xv in S.FOLD_X_AT_65:
        assert S.fold_case(cid, f"x={xv:#x}/65")[1] == xv
    assert S.fold_bases(cid, *S.fold_case(cid, "x=0x0/65")) == S.fold_case(cid, "x=0x0/65")[0][:65]


def test_instance_cases_have_the_shapes_they_are_named_for():
    for name in S.instance_names():
        c = S.instance_case(name)
        n_w, n_c = c["n_w"], c["n_c"]
        p = S.FIELD[_oracle.CURVE_SCALAR[c["cid"]]]
        az, bz, cz = S.products(c)
        e = c["E"] if c["E"] is not None else [0] * n_c
        assert all((x * y - c["Z"][0] * w - v) % p == 0 for x, y, w, v in zip(az, bz, cz, e)), name          # satisfied by construction
        assert (c["E"] is None) == name.endswith("strict") and (c["E"] is not None or c["Z"][0] == 1)
        for m in "ABC":
            cols = {col for _, col, v in c[m] if v}
            assert n_w - 2 in cols and n_w - 1 in cols, name                                                  # X0 and X1 are used
            assert all(0 <= r < n_c and 0 <= col < n_w and 0 < v < p for r, col, v in c[m])
            if (n_w, n_c) in S.DENSE_SHAPES:
                per_col, per_row, rows_of = [0] * n_w, [0] * n_c, [set() for _ in range(n_w)]
                for r, col, _ in c[m]:
                    per_col[col] += 1; per_row[r] += 1; rows_of[col].add(r)
                assert per_col[0] > 32 and per_col[n_w // 2] > 32 and 7 <= len(rows_of[n_w // 3]) <= 32 and 7 <= per_col[n_w // 3] <= 32, name
                assert any(7 <= x <= 32 for x in per_row) and any(x > 32 for x in per_row), name
                if n_c > 32:
                    assert len(rows_of[0]) > 32 and len(rows_of[n_w // 2]) > 32


@pytest.mark.parametrize("name", S.instance_names())
def test_instance_bytes_convince_the_independent_verifier(orc, name):
    case = S.instance_case(name)
    blob = S.prove_instance(orc, case)
    assert len(blob) == 128 + S.argument_size(case)
    assert S.verify_bytes(orc, case, blob) is None
    lay = S.argument_layout(case)
    assert len(lay) == (7 if case["E"] is not None else 6)          # (a strict instance has no E opening)
    for what, off in lay.items():
        assert S.verify_bytes(orc, case, S.flip(blob, 128 + off)) is not None, f"{name}: a flipped bit in the {what} was accepted"
    assert S.verify_bytes(orc, case, blob, X0_delta=1) is not None
    assert S.prove_instance(orc, case) == blob
