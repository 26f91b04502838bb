"""The witness kernels (vimz_amd/csrc/witness.hpp) against the oracle's executor, bit for bit, at the edges of the step relations:
partial lane blocks (160, 480, 90, 270 and crop's 1..160 lanes against blocks of 64), the clamp branches and the zero-padded border
reads, rows exactly on and just past a relation's tolerance, the factor ceilings, range checks, Poseidon chains on all-0xff and
all-zero rows from states of p - 1 in both chain arithmetics, a failure in the middle of a batch, and the refusal of row widths
whose hasher needs a permutation the chain kernel does not have.  The rows are those of tests/_witness_edges.py, validated on the
CPU by tests/test_witness_edges_host.py."""
import numpy as np
import pytest

from tests import _witness_edges as we
from tests._oracle import from_limbs
from tests.test_witness_edges_host import KEYS, circuit, executed
from vimz_amd import _lib

pytestmark = pytest.mark.gpu

WIT_UNSAT = 1
BOTH_ARITHMETICS = ("hash", "sharpness", "redact")
PASSES = [(k, a) for k in KEYS for a in (("radix29", "standard") if we.CIRCUITS[k][0] in BOTH_ARITHMETICS else ("radix29",))]


@pytest.fixture(scope="module")
def ctx():
    from vimz_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ck(ctx):
    b = ctx.bases_generate(_lib.CURVE_BN254_G1, 1 << 16)
    yield b
    b.free()


# the executor's rows of one circuit at a time (its wires are what takes the room), the state chains of all of them
_rows = {}
_states = {}


def reference(oracle, key):
    if key not in _rows:
        _rows.clear()
        _rows[key] = list(executed(oracle, key))
        _states[key] = {run.name: ([st for st, _, _, _ in rows], [rows[0][2]] + [z_out for _, _, _, z_out in rows]) for run, rows in _rows[key]}
    return _rows[key]


def states(oracle, key, name):
    """(the executor's status per row, its chained states z_0..z_n) of a run."""
    if key not in _states:
        reference(oracle, key)
    return _states[key][name]


def test_the_passes_cover_every_circuit():
    assert [k for k, a in PASSES if a == "radix29"] == KEYS == list(we.cases())
    assert sorted(k for k, a in PASSES if a == "standard") == sorted(["hash-8", "hash-9", "hash-16", "sharpness-16", "sharpness-9", "redact-16"])


@pytest.mark.parametrize("key,arithmetic", PASSES)
def test_wires_states_and_status_match_the_executor(ctx, ck, oracle, monkeypatch, key, arithmetic):
    """Every run of the circuit on ONE prover (max_batch 8), reset between runs: the states, the status (zero or not, bit 0 where
    the executor says 1) and, for every row the executor does not flag, all wires — crop's rows with x past the row included, whose
    wires violate the R1CS in the same way on both sides.  A prover's buffers hold the previous run's rows (an all-255 image comes
    before the all-zero one), so a wire that a run leaves unwritten shows as a difference.  `standard` is the chain kernels' plain
    Montgomery twin (VIMZ_DEBUG_POSEIDON_STD, read when the prover is created)."""
    from vimz_amd import hip
    c = circuit(key)
    if arithmetic == "standard":
        monkeypatch.setenv("VIMZ_DEBUG_POSEIDON_STD", "1")
    else:
        monkeypatch.delenv("VIMZ_DEBUG_POSEIDON_STD", raising=False)
    P = hip.Prover(ctx, c, ck, max_batch=8)
    compared = exact = 0
    try:
        for run, rows in reference(oracle, key):
            P.reset(run.z0)
            zw, zs, st = P.witness(np.stack(run.rows))
            for i, (status, wires, z_in, z_out) in enumerate(rows):
                where = f"{key} / {run.name} / row {i}"
                assert from_limbs(zs[i]) == z_in and from_limbs(zs[i + 1]) == z_out, f"{where}: states differ"
                assert (st[i] != 0) == (status != 0), f"{where}: status {st[i]}, the executor's {status}"
                if status == 1:
                    assert st[i] & WIT_UNSAT, f"{where}: status {st[i]}"
                if status == 0:
                    diff = np.nonzero((zw[i] != wires).any(axis=1))[0]
                    assert diff.size == 0, f"{where}: {diff.size} of {c.n_wires} wires differ, first {diff[:5]}"
                    exact += 1
                compared += 1
            if run.name == "mid-batch":
                assert [int(x != 0) for x in st] == [0, 0, 1, 0, 0]
    finally:
        P.close()
    runs = we.cases()[key][1]
    assert compared == sum(len(r.rows) for r in runs) > 0
    assert exact >= sum(1 for r in runs for i in range(len(r.rows)) if we.expect_of(r, i) != "unsat") > 0


@pytest.mark.parametrize("key", [k for k in KEYS if we.CIRCUITS[k][0] in ("hash", "blur", "resize", "crop")])
def test_hash_only_pass_gives_the_same_states(ctx, ck, oracle, key):
    """vimz_prover_state_chain (the phase-A chains without wires, then the host's chain; crop: the ahead-of-time pass of
    fold_prepare) against the states of the full witness, which the test above holds equal to the executor's."""
    from vimz_amd import hip
    c = circuit(key)
    P = hip.Prover(ctx, c, ck, max_batch=8)
    n = 0
    try:
        for run in we.cases()[key][1]:
            if run.expect != "sat":
                continue
            status, zs = states(oracle, key, run.name)
            assert not any(status)
            got = P.state_chain(run.z0, np.stack(run.rows))
            assert [from_limbs(z) for z in got] == zs, f"{key} / {run.name}"
            n += 1
    finally:
        P.close()
    assert n == sum(1 for r in we.cases()[key][1] if r.expect == "sat") >= 6


FOLDS = [("sharpness-16", "checker"), ("contrast-16", "extremes-f22"), ("crop-16", "three-rows")]


@pytest.mark.parametrize("head_rows", [0, 6])
@pytest.mark.parametrize("key,name", FOLDS)
def test_folds_of_edge_rows_verify(ctx, ck, oracle, key, name, head_rows):
    """The witness paths of a fold (max_batch 2: three batches, or two for crop): every chain on the GPU (head rows 0), and the head
    batch's chains on the host, scattered into the wires by k_wit_scatter (head rows 6)."""
    from vimz_amd import hip
    run = we.find(key, name)
    status, zs = states(oracle, key, name)
    assert not any(status)
    hip.set_head_rows(head_rows)
    try:
        P = hip.Prover(ctx, circuit(key), ck, max_batch=2)
        try:
            P.reset(run.z0)
            P.fold(np.stack(run.rows))
            assert P.verify() == 0
            inst = P.instance()
            assert inst["steps"] == len(run.rows) and from_limbs(inst["z"]) == zs[-1]
        finally:
            P.close()
    finally:
        hip.set_head_rows(-1)


@pytest.mark.parametrize("head_rows", [0, 6])
def test_folds_of_unsatisfiable_rows_fail(ctx, ck, head_rows):
    """Contrast at f10 = 23 is refused with ERR_UNSAT.  A crop row with x = 160 has no status bit (the literal Decoder): its fold is
    either refused or leaves a running instance that does not verify.  By the code the second is what happens: vimz_prover_fold
    refuses a row only for its status word, which these rows leave at 0, and the relaxed R1CS check of verify() sees the violated
    Decoder rows (the test prints which of the two it met)."""
    from vimz_amd import hip
    hip.set_head_rows(head_rows)
    try:
        run = we.find("contrast-16", "extremes-f23")
        P = hip.Prover(ctx, circuit("contrast-16"), ck, max_batch=2)
        try:
            P.reset(run.z0)
            with pytest.raises(_lib.VimzError) as e:
                P.fold(np.stack(run.rows))
            assert e.value.code == _lib.ERR_UNSAT
        finally:
            P.close()
        run = we.find("crop-16", "x160")
        P = hip.Prover(ctx, circuit("crop-16"), ck, max_batch=2)
        try:
            P.reset(run.z0)
            try:
                P.fold(np.stack(run.rows))
                refused, bad = False, P.verify()
            except _lib.VimzError as err:
                refused, bad = err.code == _lib.ERR_UNSAT, 0
            print(f"crop x = 160, head rows {head_rows}: refused {refused}, verify() {bad}")
            assert refused or bad != 0
        finally:
            P.close()
    finally:
        hip.set_head_rows(-1)


def _refused(ctx, make):
    with pytest.raises(_lib.VimzError) as e:
        make()
    assert e.value.code == _lib.ERR_INVALID
    msg = ctx.lib.vimz_last_error(ctx.h).decode()
    assert "Poseidon" in msg and "widths 3 and 9" in msg, msg


def test_unsupported_row_widths_are_refused(ctx, ck, oracle):
    """The builder accepts hash at width 13 and crop (4, 2, 3); their window-fold hashers need a permutation of another width than
    3 or 9, which the chain kernel would replace by the wrong one.  The prover and the IVC (whose constructor takes the step circuit
    itself) refuse them, and the context goes on working."""
    from vimz_amd import hip
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-secondary")
    try:
        for key in we.REFUSED:
            c = circuit(key)
            _refused(ctx, lambda: hip.Prover(ctx, c, ck))
            _refused(ctx, lambda: hip.IVC(ctx, c, ck, ck2, max_batch=2))
    finally:
        ck2.free()
    run = we.find("hash-8", "random")
    status, zs = states(oracle, "hash-8", "random")
    P = hip.Prover(ctx, circuit("hash-8"), ck, max_batch=8)
    try:
        P.reset(run.z0)
        _, got, st = P.witness(np.stack(run.rows), want_wires=False)
        assert not st.any() and [from_limbs(z) for z in got] == zs
    finally:
        P.close()
