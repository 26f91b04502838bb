"""iden3.write_ptau and iden3.new_powers without a GPU: the writer is the exact inverse of the reader at powers 1–3, its bytes are the bytes the existing test helper
(tests/_decider_powers_gpu.ptau_bytes) writes for the same points, and the new string reads back as generators that the reference verdict accepts."""
import numpy as np
import pytest

from tests import _g16_powers_ref as P
from tests import _powers_contrib_ref as K
from tests import _powers_verify_ref as V
from tests._decider_powers_gpu import ptau_bytes
from tests._pairing import G1, G2, Q
from vimz_amd import iden3

MONT = 1 << 256
NAMES = ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")


def canon_arrays(power):
    """the string of (TAU0, ALPHA0, BETA0) as canonical uint64 rows"""
    pts = V.string_points(P.string_scalars(K.TAU0, K.ALPHA0, K.BETA0, power))
    return {name: np.frombuffer(b"".join(c.to_bytes(32, "little") for p in pts[name] for c in V.flat(V.GROUP[name], p)), dtype="<u8").reshape(len(pts[name]), -1) for name in NAMES}


def ints(a):
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


@pytest.mark.parametrize("power", (1, 2, 3))
def test_the_writer_is_the_readers_inverse(power):
    data = ptau_bytes(power, canon_arrays(power))
    p = iden3.read_ptau(data)
    again = iden3.write_ptau(p)
    assert again == data                                                       # the helper's bytes, byte for byte
    q = iden3.read_ptau(again)
    assert (q["power"], q["ceremony_power"]) == (power, power)
    for name in NAMES:
        assert q[name].shape == p[name].shape and np.array_equal(q[name], p[name]), name
    p2 = dict(p, ceremony_power=28)
    assert iden3.read_ptau(iden3.write_ptau(p2))["ceremony_power"] == 28
    assert iden3.write_ptau({k: v for k, v in p.items() if k != "ceremony_power"}) == data


def test_the_writer_refuses_shapes_that_do_not_match_the_power():
    p = iden3.read_ptau(ptau_bytes(2, canon_arrays(2)))
    with pytest.raises(ValueError, match="section 2 .tau_g1."):
        iden3.write_ptau(dict(p, tau_g1=p["tau_g1"][:-1]))
    with pytest.raises(ValueError, match="section 6 .beta_g2."):
        iden3.write_ptau(dict(p, beta_g2=np.concatenate([p["beta_g2"], p["beta_g2"]])))
    with pytest.raises(ValueError, match="power outside"):
        iden3.write_ptau(dict(p, power=27))
    with pytest.raises(ValueError, match="power outside"):
        iden3.new_powers(0)


@pytest.mark.parametrize("power", (1, 3))
def test_the_new_string_is_generators_and_a_string(power):
    p = iden3.read_ptau(iden3.write_ptau(iden3.new_powers(power)))
    n2 = 1 << power
    assert [p[name].shape for name in NAMES] == [(2 * n2 - 1, 8), (n2, 16), (n2, 8), (n2, 8), (1, 16)]
    g1 = [c * MONT % Q for c in G1]
    g2 = [c * MONT % Q for c in G2[0] + G2[1]]
    for name in NAMES:
        want = g1 if V.GROUP[name] == 1 else g2
        assert ints(p[name]) == want * p[name].shape[0], name
    if power == 1:
        minv = pow(MONT, -1, Q)
        pts = {}
        for name in NAMES:
            c = [x * minv % Q for x in ints(p[name])]
            per = 2 * V.GROUP[name]
            rows = [c[i:i + per] for i in range(0, len(c), per)]
            pts[name] = [tuple(r) if per == 2 else ((r[0], r[1]), (r[2], r[3])) for r in rows]
        assert pts == V.string_points(P.string_scalars(1, 1, 1, 1))
        assert K.verify(K.base_points(pts), pts, b"") == (0, 0, (0, 0))
