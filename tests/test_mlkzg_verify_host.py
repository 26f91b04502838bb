"""hip.mlkzg_verify (vimz_mlkzg_verify: host only, no context, no GPU; vimz_amd/csrc/mlkzg_verify.hpp) on the proofs tests/_mlkzg_ref.py makes with a known tau: it
accepts them at ℓ = 1, 2, 3, 10 and n = 1, 2^ℓ − 1, 2^ℓ, and every row of a tamper table gives exactly the bit that stage of the verifier owns.  A change that
reaches the transcript before r (the commitment, the point, the evaluation, a C_k that stays on the curve) moves r and so fails a FOLD equation before the pairing is
asked; E_(r²)[0] stands in no fold equation, a doubled W is absorbed after q, and a key of another tau changes no challenge: those three reach the PAIRING bit.
The Python verifier agrees on one accepted proof and on one refusal per bit (it is slow: no more than those)."""
import ctypes
import random

import numpy as np
import pytest

from tests import _mlkzg_ref as M
from tests._pairing import Q, R, g1_add
from vimz_amd import _lib, hip

TAU = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543210A1B2C3D4E5F607 % R


def _statement(logn, n):
    rng = random.Random(f"mlkzg/verify/{logn}/{n}")
    v = [rng.randrange(R) for _ in range(n)]
    x = [rng.randrange(R) for _ in range(logn)]
    return v, x, M.prove(TAU, v, logn, x)


def _native(vk, comm, x, y, proof):
    return hip.mlkzg_verify(np.array(vk, dtype=np.uint64), np.array(comm, dtype=np.uint64), x, y, np.array(proof, dtype=np.uint64))


@pytest.fixture(scope="module")
def vk():
    return M.vk_words(TAU)


@pytest.mark.parametrize("logn", (1, 2, 3, 10))
def test_proofs_of_the_reference_are_accepted(vk, logn):
    for n in sorted({1, (1 << logn) - 1, 1 << logn}):
        v, x, pr = _statement(logn, n)
        assert _native(vk, pr["comm"], x, pr["eval"], pr["proof"]) == 0, (logn, n)


def _bump(words, at):
    out = list(words)
    out[at] = (out[at] + 1) & M.M64
    return out


def _put(words, at, value):
    out = list(words)
    out[at:at + 4] = M.words_of(value)
    return out


def _doubled(words, at):
    p = M.point_of(words[at:at + 8])
    out = list(words)
    out[at:at + 8] = M.point_words(g1_add(p, p))
    return out


def tamper_table(logn, vk, pr, x):
    """name -> (vk, comm, x, eval, proof, the expected verdict)"""
    comm, y, proof = pr["comm"], pr["eval"], pr["proof"]
    e, w = 8 * (logn - 1), 8 * (logn - 1) + 12 * logn
    t = {"a C_k + 1": (vk, comm, x, y, _bump(proof, 0), M.OFF_CURVE),
         "E_r + 1": (vk, comm, x, y, _bump(proof, e), M.FOLD),
         "E_-r + 1": (vk, comm, x, y, _bump(proof, e + 4 * logn), M.FOLD),
         "E_r2[0] + 1": (vk, comm, x, y, _bump(proof, e + 8 * logn), M.PAIRING),
         "E_r2[1] + 1": (vk, comm, x, y, _bump(proof, e + 8 * logn + 4), M.FOLD),
         "eval + 1": (vk, comm, x, (y + 1) % R, proof, M.FOLD),
         "C -> 2C": (vk, _doubled(comm, 0), x, y, proof, M.FOLD),
         "a C_k -> 2 C_k": (vk, comm, x, y, _doubled(proof, 0), M.FOLD),
         "W_r -> 2 W_r": (vk, comm, x, y, _doubled(proof, w), M.PAIRING),
         "eval = r": (vk, comm, x, R, proof, M.MALFORMED),
         "E = r": (vk, comm, x, y, _put(proof, e + 4, R), M.MALFORMED),
         "C.x = q": (vk, _put(comm, 0, Q), x, y, proof, M.MALFORMED),
         "C_k.y = q": (vk, comm, x, y, _put(proof, 4, Q), M.MALFORMED),
         "W.x = q": (vk, comm, x, y, _put(proof, w + 16, Q), M.MALFORMED),
         "vk coordinate = q": (_put(vk, 8, Q), comm, x, y, proof, M.MALFORMED),
         "a C_k off the curve": (vk, comm, x, y, _put(_put(proof, 0, 1), 4, 3), M.OFF_CURVE),
         "C off the curve": (vk, _put(_put(comm, 0, 1), 4, 3), x, y, proof, M.OFF_CURVE),
         "one word short": (vk, comm, x, y, proof[:-1], M.MALFORMED),
         "one word long": (vk, comm, x, y, proof + [0], M.MALFORMED),
         "another tau": (M.vk_words(TAU + 1), comm, x, y, proof, M.PAIRING)}
    for k in range(3):
        t[f"W[{k}] + 1"] = (vk, comm, x, y, _bump(proof, w + 8 * k), M.OFF_CURVE)
    for k in range(logn):
        t[f"x_{k} + 1"] = (vk, comm, x[:k] + [(x[k] + 1) % R] + x[k + 1:], y, proof, M.FOLD)
        t[f"x_{k} = r"] = (vk, comm, x[:k] + [R] + x[k + 1:], y, proof, M.MALFORMED)
    return t


def test_every_tampering_gives_exactly_its_bit(vk):
    logn = 3
    v, x, pr = _statement(logn, 7)
    assert _native(vk, pr["comm"], x, pr["eval"], pr["proof"]) == 0
    table = tamper_table(logn, vk, pr, x)
    got = {name: _native(*row[:5]) for name, row in table.items()}
    assert got == {name: row[5] for name, row in table.items()}
    assert set(got.values()) == set(hip.MLKZG_PROBLEMS)


def test_the_python_verifier_agrees_on_an_accept_and_on_one_refusal_per_bit(vk):
    logn = 2
    v, x, pr = _statement(logn, 3)
    table = tamper_table(logn, vk, pr, x)
    rows = {"untouched": (vk, pr["comm"], x, pr["eval"], pr["proof"], 0)}
    rows.update({name: table[name] for name in ("one word short", "W[1] + 1", "eval + 1", "another tau")})
    assert sorted(r[5] for r in rows.values()) == [0, 1, 2, 4, 8]
    for name, (k, c, xs, y, p, want) in rows.items():
        point_w = [w for xk in xs for w in M.words_of(xk)]
        assert M.verify(k, c, logn, point_w, M.words_of(y), p) == want, name
        assert _native(k, c, xs, y, p) == want, name


@pytest.mark.parametrize("label,tag,n", [(b"vimz-mlkzg-v1", b"logn", 8), (b"vimz-mlkzg-v1", b"Ck", 0), (b"x", b"E", 135), (b"y" * 40, b"W", 136), (b"z", b"eightchr9", 137),
                                         (b"vimz-cf-compressed-v1", b"x", 1000)])
def test_the_restated_chain_is_the_proof_objects_transcript(label, tag, n):
    """mlkzg_verify.hpp restates proof_io.hpp's Transcript without HIP: both, and the reference's, give the same challenges after the same absorptions, at lengths on
    each side of the sponge's rate and with a tag longer than its eight bytes"""
    T = _lib.testing_lib()
    T.vimz_test_mlkzg_chains.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    data = bytes((7 * i + n) & 0xFF for i in range(n))
    out = np.zeros(4, dtype=np.uint64)
    assert T.vimz_test_mlkzg_chains(label, tag, data, n, out.ctypes.data_as(ctypes.c_void_p)) == 0
    t = M.Transcript(label)
    for _ in range(2):
        t.absorb(tag, data)
        want = t.challenge()
    assert [int(out[0]) | int(out[1]) << 64, int(out[2]) | int(out[3]) << 64] == [want, want]


def test_bad_arguments_are_errors_not_verdicts(vk):
    v, x, pr = _statement(1, 1)
    with pytest.raises(_lib.VimzError) as e:
        _native(vk, pr["comm"], [], pr["eval"], pr["proof"])
    assert e.value.code == _lib.ERR_INVALID
    lib = _lib.lib()
    lib.vimz_mlkzg_proof_words.argtypes, lib.vimz_mlkzg_proof_words.restype = [ctypes.c_uint32], ctypes.c_size_t
    assert [lib.vimz_mlkzg_proof_words(k) for k in (0, 1, 10, 26, 27)] == [0, 36, 216, 536, 0]
    # logn above the limit with a proof of "its" length: a verdict, MALFORMED
    assert _native(vk, pr["comm"], [1] * 27, pr["eval"], [0] * (20 * 27 + 16)) == M.MALFORMED
