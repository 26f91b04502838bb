"""vimz_amd.iden3.read_ptau on `.ptau` containers written here (no GPU): a string of a known (tau, alpha, beta) round-trips point by point; another prime, a wrong
header, a short, a long and a missing section, a file cut inside its section table or inside a section are refused with ValueError.  The writer restates the
same published layout the reader does: the pair is consistent, not pinned on a real ceremony file."""
import struct

import numpy as np
import pytest

from tests._pairing import G1, G2, Q, R, g1_mul, g2_mul
from vimz_amd import iden3

TAU, ALPHA, BETA = 0x1234567890ABCDEF1234567, 0xFEDCBA987654321, 0x55AA55AA55AA77


def string_of(power):
    n2 = 1 << power
    pw = [pow(TAU, k, R) for k in range(2 * n2 - 1)]
    return {"tau_g1": [g1_mul(G1, k) for k in pw], "tau_g2": [g2_mul(G2, k) for k in pw[:n2]], "alpha_g1": [g1_mul(G1, ALPHA * k % R) for k in pw[:n2]],
            "beta_g1": [g1_mul(G1, BETA * k % R) for k in pw[:n2]], "beta_g2": [g2_mul(G2, BETA)]}


@pytest.fixture(scope="module")
def strings():
    return {1: string_of(1), 2: string_of(2)}


def mont(x):
    return x * (1 << 256) % Q


def coords(p):
    return list(p) if isinstance(p[0], int) else [p[0][0], p[0][1], p[1][0], p[1][1]]


def point_bytes(p):
    return b"".join(mont(c).to_bytes(32, "little") for c in coords(p))


NAMES = {2: "tau_g1", 3: "tau_g2", 4: "alpha_g1", 5: "beta_g1", 6: "beta_g2"}


def write_ptau(power, srs, prime=Q, ceremony_power=None, resize=None, drop=None, header=None):
    """snarkjs's container: "ptau", version, section count, then (type u32, size u64, body) per section.  resize = (section, delta bytes); drop = a section left out."""
    secs = {1: struct.pack("<I", 32) + prime.to_bytes(32, "little") + struct.pack("<II", power, power if ceremony_power is None else ceremony_power)}
    if header is not None:
        secs[1] = header
    for t, name in NAMES.items():
        secs[t] = b"".join(point_bytes(p) for p in srs[name])
    if resize:
        t, d = resize
        secs[t] = secs[t][:d] if d < 0 else secs[t] + bytes(d)
    order = [t for t in (1, 6, 2, 3, 4, 5) if t != drop]      # (sections may come in any order)
    out = b"ptau" + struct.pack("<II", 1, len(order))
    for t in order:
        out += struct.pack("<IQ", t, len(secs[t])) + secs[t]
    return out


def ints(a):
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


@pytest.mark.parametrize("power", [1, 2])
def test_ptau_round_trip(strings, power):
    srs = strings[power]
    got = iden3.read_ptau(write_ptau(power, srs, ceremony_power=28))
    assert got["power"] == power and got["ceremony_power"] == 28
    n2 = 1 << power
    for name, count, per in (("tau_g1", 2 * n2 - 1, 2), ("tau_g2", n2, 4), ("alpha_g1", n2, 2), ("beta_g1", n2, 2), ("beta_g2", 1, 4)):
        a = got[name]
        assert a.dtype == np.dtype("<u8") and a.shape == (count, 4 * per)
        assert ints(a) == [mont(c) for p in srs[name] for c in coords(p)], name
    assert ints(got["tau_g1"][0]) == [mont(1), mont(2)]            # the generator first


def test_ptau_refusals(strings):
    srs, good = strings[1], write_ptau(1, strings[1])
    iden3.read_ptau(good)
    with pytest.raises(ValueError, match="prime"):
        iden3.read_ptau(write_ptau(1, srs, prime=R))
    for sec in NAMES:
        for delta in (-32, 64):
            with pytest.raises(ValueError, match=f"section {sec} .{NAMES[sec]}.: "):
                iden3.read_ptau(write_ptau(1, srs, resize=(sec, delta)))
        with pytest.raises(ValueError, match=f"section {sec} .{NAMES[sec]}. is missing"):
            iden3.read_ptau(write_ptau(1, srs, drop=sec))
    with pytest.raises(ValueError, match="no header"):
        iden3.read_ptau(write_ptau(1, srs, drop=1))
    with pytest.raises(ValueError, match="section 2"):
        iden3.read_ptau(write_ptau(2, srs))                           # the header's power does not match the sections
    with pytest.raises(ValueError, match="power outside"):
        iden3.read_ptau(write_ptau(27, srs))
    with pytest.raises(ValueError, match="32-byte"):
        iden3.read_ptau(write_ptau(1, srs, header=struct.pack("<I", 48) + bytes(48) + struct.pack("<II", 1, 1)))
    with pytest.raises(ValueError, match="expected 44"):
        iden3.read_ptau(write_ptau(1, srs, header=struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<I", 1)))
    with pytest.raises(ValueError, match="not a ptau file"):
        iden3.read_ptau(b"r1cs" + good[4:])
    with pytest.raises(ValueError, match="inside its section table"):
        iden3.read_ptau(good[:12 + 56 + 5])                           # the header section, then five bytes of the next entry
    with pytest.raises(ValueError, match="inside a section"):
        iden3.read_ptau(good[:-10])
