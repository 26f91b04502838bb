"""The MSM's signed scalar loader (VIMZ_TUNE=signed_scalars, on by default): a scalar above (p - 1)/2 goes through every digit producer as
p - s with its signs flipped.  The commitment must be the very same point with the switch on and off, on every path (the large pipeline
with the LDS sort, with the global-atomics sort, over window tables with one shared bucket set, with the unit split; the fused small
kernel; the tables of multiples), on every curve, and equal to the CPU oracle's — and the switch must actually remove the entries it
is there to remove.  Folds must give the same proof either way."""
import json
import os
import subprocess
import sys

import pytest

from tests import _signed_scalars as S
from tests._oracle import to_limbs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _probe(tmp_path_factory, flag):
    out = tmp_path_factory.mktemp(f"signed{flag}") / "points.json"
    r = subprocess.run([sys.executable, "-m", "tests._signed_scalars", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=840,
                       env={**os.environ, "VIMZ_TUNE": f"signed_scalars={flag}"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    """what a process with the switch on and one with it off computed: {"curve/vector": {path: point or entry count}}"""
    return {1: _probe(tmp_path_factory, 1), 0: _probe(tmp_path_factory, 0)}


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", S.VECTORS)
def test_commitments_equal_the_oracle_with_the_switch_on_and_off(probes, oracle, cid, kind):
    sc = S.vector(cid, kind)
    bases = oracle.seq_bases(cid, S.N_LARGE)
    want = {n: [int(x) for x in oracle.msm(cid, bases[:n], to_limbs(sc[:n]), threads=8)] for n in (S.N_LARGE, S.N_SMALL, S.N_FIXED)}
    size = {"large": S.N_LARGE, "large_canonical_input": S.N_LARGE, "large_c15": S.N_LARGE, "large_tables15": S.N_LARGE, "large_tables15_split_ones": S.N_LARGE,
            "small": S.N_SMALL, "small_canonical_input": S.N_SMALL, "fixed_plain": S.N_FIXED, "fixed_tables": S.N_FIXED}
    on, off = probes[1][f"{cid}/{kind}"], probes[0][f"{cid}/{kind}"]
    for path, n in size.items():
        assert on[path] == off[path], (path, "the switch changed a commitment")        # limb for limb
        assert on[path] == want[n], (path, "differs from the oracle")


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_negative_small_scalars_cost_the_digits_of_the_small_value(probes, cid):
    """All p - (139-bit) at c = 15: at most ten entries a scalar (windows 0..9) with the switch on — over tables and without.  Off, on
    the BN254 fields, every one of the 17 windows holds a digit (the upper windows spell the upper part of p)."""
    n = S.N_LARGE
    for kind in ("neg_small", "one_x"):
        on, off = probes[1][f"{cid}/{kind}"], probes[0][f"{cid}/{kind}"]
        for path in ("large_c15_entries", "large_tables15_entries"):
            print(f"curve {cid} {kind} {path}: on {on[path]} off {off[path]} (n = {n})")
            assert 0 < on[path] <= 10 * n
            if cid in (0, 1):
                assert off[path] == 17 * n
    # every count exactly, against the digits of the same scalars in Python integers (c = 15 has K = 17 windows on BN254, 18 on the Pasta fields)
    p = S.MODULI[S.SCALAR_FIELD[cid]]
    for kind in S.VECTORS:
        sc = S.vector(cid, kind)
        for flag in (1, 0):
            want = S.entries(sc, 15, p, bool(flag))
            for path in ("large_c15_entries", "large_tables15_entries"):
                assert probes[flag][f"{cid}/{kind}"][path] == want, (kind, flag, path)
    # (the Pasta moduli are 2^254 + a 126-bit tail: there p - small is sparse under the plain recoding too, and nothing is claimed about "off")
    # the mixed and the boolean-row-like vectors lose their negative-small scalars' upper digits as well
    if cid in (0, 1):
        for kind in ("mixed", "bufm"):
            for path in ("large_entries", "large_c15_entries", "large_tables15_entries"):
                assert probes[1][f"{cid}/{kind}"][path] < probes[0][f"{cid}/{kind}"][path]


def test_folds_give_the_same_proof_with_the_switch_off():
    """tools/ivc_digest.py (the schedule-independence test's probe) under the default and under signed_scalars=0: with window tables of the
    key and without, in the boolean-row form of the step rows' commitment and with the plain vector, with and without the fused small MSM."""
    variants = [{}, {"VIMZ_TUNE": "signed_scalars=0"},
                {"VIMZ_DIGEST_TABLES": "15"}, {"VIMZ_DIGEST_TABLES": "15", "VIMZ_TUNE": "signed_scalars=0"},
                {"VIMZ_IVC_BOOL_ROWS": "0"}, {"VIMZ_IVC_BOOL_ROWS": "0", "VIMZ_TUNE": "signed_scalars=0"},
                {"VIMZ_DEBUG_NO_SMALL_MSM": "1"}, {"VIMZ_DEBUG_NO_SMALL_MSM": "1", "VIMZ_TUNE": "signed_scalars=0"},
                {"VIMZ_IVC_MULT_TABLES": "1", "VIMZ_TUNE": "signed_scalars=0"},
                {"VIMZ_TUNE": "signed_scalars=0,sort_blocks=40,combine_lane_bits=2", "VIMZ_DEBUG_CHECK_MSM": "1"}]
    lines = []
    for env in variants:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ivc_digest.py"), "grayscale", "2", "8"], capture_output=True, text=True,
                             timeout=600, env={**os.environ, **env})
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("digest ")][-1]
        assert " verify 0 " in line, (env, line)
        lines.append(line)
    assert len(set(lines)) == 1, list(zip(variants, lines))
