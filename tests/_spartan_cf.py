"""ORACLE — TEST INFRASTRUCTURE ONLY.  An independent verifier of the two compressed Nova + CycleFold proofs (vimz_cf_compress, vimz_cf_merged_compress),
written from the layout in vimz_amd/csrc/cf_compressed_parse.hpp and the protocol text of vimz_amd/csrc/spartan.hip and sharing no code with them: the
argument verifier of tests/_spartan_pub_ref.py (n_pub public elements), the hashes and the replay of the merged records of tests/_cyclefold.py, shapes from
CycleFoldIVC.r1cs and export.  Pure-Python loops over the shapes: meant for the small circuits of the tests."""
import numpy as np

from tests import _cyclefold as cfo
from tests import _spartan_pub_ref as P
from tests._oracle import ck_derive
from tests._spartan import Reader, Transcript

CHAIN_MAGIC = 0x314E534643565A
MERGED_MAGIC = 0x31474D4346565A
CF_IO = cfo.CF_IO


def _log2(n):
    return (n - 1).bit_length()


def _shapes(cf):
    info = cf.info()
    return (info["main_wires"], info["main_constraints"]), (info["cyclefold_wires"], info["cyclefold_constraints"]), info["len_z"]


def _arguments(orc, cf, tr, rd, key1, key2, dg, todo):
    """todo: (name, cid, instance, side tag, has_E).  Returns the failed checks (stops at the first argument that fails, as the product does)."""
    n1, n2, _ = _shapes(cf)
    tabs = {0: cf.r1cs(0), 1: cf.r1cs(1)}
    Ug = {0: ck_derive(0, b"vimz-ipa-u", 0), 1: ck_derive(1, b"vimz-ipa-u", 0)}
    for name, cid, inst, tag, has_E in todo:
        n = n1 if cid == 0 else n2
        try:
            why = P.spartan_verify(orc, cid, tr, dg, inst, tabs[cid], n[0], n[1], key1 if cid == 0 else key2, Ug[cid], tag, rd, has_E)
        except ValueError as e:
            why = str(e)
        if why:
            return [f"{name}: {why}"]
    return [] if rd.pos == len(rd.b) else ["trailing bytes"]


def verify_chain(orc, cf, blob, num_steps, z0, key1, key2):
    """(failed checks, z_n).  cf: a CycleFoldIVC for the same circuit and keys (shapes only); key1 / key2: (n, 8) canonical affine limbs."""
    pr, pq = orc.modulus[0], orc.modulus[1]
    n1, n2, len_z = _shapes(cf)
    rd = Reader(bytes(blob))
    head = [rd.word() for _ in range(8)]
    if head != [CHAIN_MAGIC, head[1], len_z, _log2(n1[1]), _log2(n1[0]), _log2(n2[1]), _log2(n2[0]), 0]:
        return ["header"], None
    steps = head[1]
    failed = []
    try:
        z0p = [rd.fe(pr) for _ in range(len_z)]
        zn = [rd.fe(pr) for _ in range(len_z)]
        lo = rd.pos
        U = [rd.fe(pq) for _ in range(4)] + [rd.fe(pr) for _ in range(3)]
        u = [rd.fe(pq), rd.fe(pq), rd.fe(pr), rd.fe(pr)]
        cfU = [rd.fe(pr) for _ in range(5)] + [rd.fe(pq) for _ in range(CF_IO)]
    except ValueError as e:
        return [str(e)], None
    inst_bytes = rd.b[lo:rd.pos]
    if steps != num_steps or steps == 0 or z0p != [int(x) for x in z0]:
        failed.append("statement")
    dg = cfo.shape_digest(cf)
    if cfo.hash_main(orc, dg, steps, [int(x) for x in z0], zn, U) != u[2]:
        failed.append("hash of the main running instance")
    if cfo.hash_cf(orc, dg, cfU) != u[3]:
        failed.append("hash of the CycleFold running instance")
    tr = Transcript(b"vimz-cf-compressed-v1")
    tr.absorb(b"steps", steps.to_bytes(8, "little"))
    for z in z0p:
        tr.fe(b"z0", z)
    for z in zn:
        tr.fe(b"zn", z)
    tr.absorb(b"inst", inst_bytes)
    todo = (("U_n", 0, ((U[0], U[1]), (U[2], U[3]), U[4], [U[5], U[6]]), 1, True),
            ("u_n", 0, ((u[0], u[1]), (0, 0), 1, [u[2], u[3]]), 3, False),
            ("cfU_n", 1, ((cfU[0], cfU[1]), (cfU[2], cfU[3]), cfU[4], list(cfU[5:])), 2, True))
    return failed + _arguments(orc, cf, tr, rd, key1, key2, dg, todo), zn


def verify_merged(orc, cf, blob, num_steps, z0, key1, key2):
    """(failed checks, z_end)"""
    _, _, len_z = _shapes(cf)
    b = bytes(blob)
    if len(b) < 16 or len(b) % 8:
        return ["header"], None
    words = np.frombuffer(b, dtype="<u8")
    rw = int(words[1])
    if int(words[0]) != MERGED_MAGIC or rw > len(words) - 2:
        return ["header"], None
    try:
        rec = cfo.parse_merged_records(words[2:2 + rw], len_z)
    except (AssertionError, IndexError):
        return ["records"], None
    info = cf.info()
    if rec["shape"] != (info["main_wires"], info["main_constraints"], info["cyclefold_wires"], info["cyclefold_constraints"]):
        return ["records: another circuit"], None
    dg = cfo.shape_digest(cf)
    failed, acc = cfo.replay_merged(orc, rec, dg, len_z)
    if acc["n"] != num_steps or acc["zs"] != [int(x) for x in z0]:
        failed.append("statement")
    tr = Transcript(b"vimz-cf-merged-compressed-v1")
    tr.absorb(b"records", b[16:16 + 8 * rw])
    rd = Reader(b[16 + 8 * rw:])
    Pm, Q = acc["P"], acc["Q"]
    todo = (("main", 0, (tuple(Pm[0]), tuple(Pm[1]), Pm[2], [Pm[3], Pm[4]]), 1, True),
            ("cyclefold", 1, (tuple(Q[0]), tuple(Q[1]), Q[2], list(Q[3])), 2, True))
    return failed + _arguments(orc, cf, tr, rd, key1, key2, dg, todo), acc["ze"]
