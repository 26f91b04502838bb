"""The decider's kernels (vimz_amd/csrc/groth16.hip: k_pow_table, k_bitrev, k_ntt_stage, k_scale_pow, k_quotient, k_fixed_mul over Fq and Fq2, k_g2_canon,
k_g2_planes, k_g2_plane_tree) against plain Python integers (tests/_g16_ref.py, checked on the CPU by tests/test_g16_ref_host.py), through hooks that call
the set-up's and the prover's own functions.  Every comparison is exact equality of words.

Transforms and quotients at domains of 2, 4, 8 points, at n/2 = 128, 256 and 512 (half a block, one block, two blocks of k_ntt_stage) and at 2^13, on random,
extreme, constant and unit vectors; key points for scalars that put one digit in every window, the largest digit in the top window, r − 1 and its
neighbours, at n around the block of 128; the G2 sum at n around a wave and around the 2048 threads of a plane, on planes that are full, empty, nearly
full and of graded density, the top plane alone, and on bases that make the accumulators double, cancel and restart."""
import functools
import json
import os
import subprocess
import sys

import pytest

from tests import _g16_kernels_gpu as P
from tests import _g16_ref as G
from tests._pairing import G1, G2, Q, R, g1_mul, g2_mul, g2_on_curve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = tmp_path_factory.mktemp("g16_kernels") / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._g16_kernels_gpu", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


def same(got_hex, want, what):
    """exact equality of a vector's words with the integers expected; names the first element that differs"""
    want_hex = P.ints_hex(want)
    if got_hex != want_hex:
        assert len(got_hex) == len(want_hex), f"{what}: {len(got_hex) // 64} elements, expected {len(want)}"
        k = next(i for i in range(len(want)) if got_hex[64 * i:64 * i + 64] != want_hex[64 * i:64 * i + 64])
        raise AssertionError(f"{what}: element {k} of {len(want)} is {int.from_bytes(bytes.fromhex(got_hex[64 * k:64 * k + 64]), 'little')}, expected {want[k]}")


@pytest.mark.parametrize("logn", G.TRANSFORM_LOGN)
def test_transforms(probe, logn):
    n, w = 1 << logn, G.omega(logn)
    winv = pow(w, -1, R)
    for name, v in G.transform_cases(logn).items():
        got = probe["transform"][f"{logn}/{name}"]
        fwd = G.transform(v, w)
        same(got["fwd"], fwd, f"forward NTT of {name} at 2^{logn}")
        same(got["inv"], G.transform(v, winv), f"inverse NTT of {name} at 2^{logn}")
        same(got["inv_of_fwd"], [x * n % R for x in v], f"inverse of forward of {name} at 2^{logn}")
        same(got["coset"], G.coset_extend(v, logn), f"coset extension of {name} at 2^{logn}")
        if name == "e_1":            # a row of the DFT matrix, in so many words
            assert fwd == [pow(w, i, R) for i in range(n)]


@pytest.mark.parametrize("logn", G.TRANSFORM_LOGN)
def test_quotient(probe, logn):
    n = 1 << logn
    points = G.identity_points(logn) if logn == max(G.TRANSFORM_LOGN) else []
    weights = [G.barycentric_weights(x, logn) for x in points]
    for name, (a, b, c, satisfied) in G.quotient_cases(logn).items():
        got = probe["quotient"][f"{logn}/{name}"]
        h = G.quotient_pipeline(a, b, c, logn)
        same(got, h, f"quotient of {name} at 2^{logn}")
        if not satisfied:
            continue
        assert h[n - 1] == 0
        if logn <= 6:
            same(got, G.quotient_schoolbook(a, b, c, logn), f"quotient of {name} at 2^{logn} (schoolbook)")
        hg = P.hex_ints(got)
        for x, u in zip(points, weights):      # A(x)·B(x) − C(x) = h(x)·(x^n − 1), on the device's words
            assert (G.dot(u, a) * G.dot(u, b) - G.dot(u, c) - G.horner(hg, x) * (pow(x, n, R) - 1)) % R == 0, name
    if logn == 3:
        a, b, c, _ = G.quotient_cases(3)["random"]
        same(probe["quotient_montgomery/3"], [x * P.MONT % R for x in G.quotient_pipeline(a, b, c, 3)], "quotient in Montgomery form")
    if n > 2:
        assert G.quotient_pipeline(*G.quotient_cases(logn)["top_degree"][:3], logn)[n - 2] != 0


def test_bad_arguments_are_refused(probe):
    assert set(probe["refused"]) == {"logn_0", "logn_27", "not_reduced", "msm_n_0", "msm_n_above_m", "msm_idx_not_below_m"}
    assert all(rc == probe["invalid"] for rc in probe["refused"].values()), probe["refused"]
    assert probe["accepted"] == 0


@functools.lru_cache(maxsize=None)
def multiples(group):
    """k·G of the fixed-base scalars in G1 / G2, once"""
    mul, gen = (g1_mul, G1) if group == 1 else (g2_mul, G2)
    return {k: mul(gen, k) for k in G.fixed_scalars(max(G.FIXED_N)) + G.fixed_scalars(1)}


@pytest.mark.parametrize("n", G.FIXED_N)
@pytest.mark.parametrize("group", [1, 2])
def test_fixed_base_multiplication(probe, group, n):
    sc = G.fixed_scalars(n)
    want = []
    for k in sc:
        p = multiples(group)[k]
        want += ([0, 0] if p is None else list(p)) if group == 1 else G.g2_words(p)
        assert group == 1 or g2_on_curve(p)
    same(probe["fixed"][f"{group}/{n}"], want, f"multiples of the generator of G{group}, n = {n}")
    if n > 1:
        per = 2 * group
        assert sc[0] == 0 and not any(want[:per])                                    # 0·G: all words zero
        at = sc.index(R - 1)
        neg = [1, Q - 2] if group == 1 else G.g2_words(G.g2_neg(G2))
        assert want[per * at:per * at + per] == neg                                  # (r − 1)·G = −G


def test_g2_msm_bases_are_multiples_of_the_generator(probe):
    assert probe["pool_off_curve"] == []
    assert len(probe["pool_spot"]) == P.SPOT and probe["pool_spot_wrong"] == []


def _msm_names(pred):
    return sorted(k for k, c in G.msm_cases().items() if pred(k, c))


@pytest.mark.parametrize("name", _msm_names(lambda k, c: True))
def test_g2_msm(probe, name):
    case, pool_k = G.msm_cases()[name], G.msm_pool_scalars()
    want = g2_mul(G2, G.msm_multiplier(case, pool_k))
    same(probe["msm"][name], G.g2_words(want), f"G2 sum {name}")
    n = len(case["scalars"])
    if n <= 8:
        pts = [g2_mul(G2, pool_k[j]) for j in range(max(abs(b) for b in case["bases"]))]
        assert G.msm_explicit(case, pts) == want
    kind = name.split("/")[0]
    if kind in ("zero", "horner_cancel"):
        assert want is None and probe["msm"][name] == "00" * 128                      # the identity: 16 zero words
    else:
        assert want is not None and g2_on_curve(want)


def test_g2_msm_special_bases_are_what_they_are_meant_to_be():
    cases, pool_k = G.msm_cases(), G.msm_pool_scalars()
    m = lambda name: G.msm_multiplier(cases[name], pool_k)      # noqa: E731
    t = cases["same_base_scaled"]["scalars"][0]
    assert t not in (0, 1) and m("same_base") == G.MSM_POOL * pool_k[0] % R and m("cancel_restart") == 64 * pool_k[0] % R
    assert m("same_base_scaled") == t * G.MSM_POOL * pool_k[0] % R and m("cancel_restart_scaled") == t * 64 * pool_k[0] % R
    assert cases["identity_every_tenth"]["bases"][:11] == [0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0]


def test_g2_msm_repeats(probe):
    assert probe["msm_repeat"][0] == probe["msm_repeat"][1] == probe["msm"][G.MSM_REPEAT]
