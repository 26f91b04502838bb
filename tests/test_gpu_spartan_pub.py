"""The compressed proof's argument for an instance with n_pub public elements at the tail of Z (vimz_amd/csrc/spartan.hip: k_committed_part, k_mask_public, the
evalW correction, the verifier's Z(ry)) — what a CycleFold instance (n_pub = 7) needs — against the integer prover and verifier of tests/_spartan_pub_ref.py
(checked on the CPU by tests/test_spartan_pub_ref_host.py), through the hooks vimz_test_spartan_instance_pub / _pub_verify.  Shapes (n_c, n_w, n_pub): (2, 9, 7)
one committed wire and seven padding slots; (4, 16, 7) no padding; (3, 17, 7) the publics straddle index 16, the top variable of ry; (2, 3, 1); (5, 12, 2) — on
both curves (scalar fields BN254 Fr and Fq), relaxed and strict.  Equality is of words; there is no tolerance anywhere."""
import json
import os
import subprocess
import sys

import pytest

from tests import _oracle
from tests import _spartan_pub_ref as P
from tests import _spartan_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = tmp_path_factory.mktemp("spartan_pub") / "words.json"
    r = subprocess.run([sys.executable, "-m", "tests._spartan_pub_gpu", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    with open(out) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def orc():
    return _oracle.load()


def test_every_case_is_in_the_probe(probe):
    assert sorted(probe["case"]) == sorted(P.case_names())
    assert {tuple(int(x) for x in n.split("/")[1].split("x")) for n in probe["case"]} == {(2, 9, 7), (4, 16, 7), (3, 17, 7), (2, 3, 1), (5, 12, 2)}


@pytest.mark.parametrize("name", P.case_names())
def test_instance(probe, orc, name):
    c = P.case(name)
    got = probe["case"][name]
    blob = bytes.fromhex(got["blob"])
    inst, want = P.prove(orc, c)
    # 1. the integer prover's bytes, word for word
    assert len(blob) == len(want) == 128 + S.argument_size(c)
    if blob != want:
        lay = sorted((off + 128, what) for what, off in S.argument_layout(c).items())
        k = next(i for i in range(0, len(want), 32) if blob[i:i + 32] != want[i:i + 32])
        near = [w for off, w in lay if off <= k]
        raise AssertionError(f"{name}: the element at byte {k} ({'the commitments' if k < 128 else 'at or after the ' + near[-1] if near else 'the outer messages'}) is "
                             f"{int.from_bytes(blob[k:k + 32], 'little')}, expected {int.from_bytes(want[k:k + 32], 'little')}")
    # 2. at two public elements, the bytes of the hook that has always had two
    if c["n_pub"] == 2:
        assert got["old_hook"] == got["blob"]
    else:
        assert "old_hook" not in got
    # 3. both verifiers accept
    assert got["verify"] == 1
    assert P.verify_bytes(orc, c, blob) is None
    # 4. the product's verifier rejects every X_k + 1 and u + 1 ...
    assert got["x_plus_1"] == [0] * c["n_pub"], f"{name}: accepted with a public element + 1: {got['x_plus_1']}"
    assert got["u_plus_1"] == 0
    # 5. ... and every forged argument: a correction of X_k hidden under the generator of its slot, and a -1 in a padding slot
    assert sorted(int(i) for i in got["forged"]) == P.forge_indices(c)
    assert all(v == 0 for v in got["forged"].values()), f"{name}: a forged argument was accepted: {got['forged']}"


def test_shapes_without_a_committed_wire_or_a_public_element_are_refused(probe):
    assert set(probe["refused"]) == {"prove_n_w_is_n_pub_plus_1", "prove_n_pub_0", "verify_n_w_is_n_pub_plus_1", "verify_n_pub_0", "prove_n_w_8_n_pub_7"}
    assert all(rc == probe["invalid"] for rc in probe["refused"].values()), probe["refused"]
    assert probe["accepted_after"]["rc"] > 0 and probe["accepted_after"]["same"]
