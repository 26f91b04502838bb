"""The batch producer's row groups (prover_internal.hpp: fold_issue): the witness commitments and S_1 sums of several rows of a batch go out as ONE
chain of launches.  Ten contrast-HD rows folded as a Nova IVC with groups of up to eight rows (vimz_set_rows_group(8); one batch of ten: groups of
1, 1, 2, 4, 2 rows; batches of at most three: the first ramps 1, 1, 1, the others are one group each) and with one chain per row
(vimz_set_rows_group(0)) must give the very same proof —
both running instances, the running vectors, the last fresh instance and witness, the exported proof bytes — and the verifier must accept it."""
import numpy as np
import pytest

from tests.test_circuits import step_inputs
from vimz_amd import _lib
from vimz_amd.circuit import Circuit

pytestmark = pytest.mark.gpu

ROWS = 10


@pytest.fixture(scope="module")
def setup():
    from vimz_amd import hip
    ctx = hip.Context(0)
    ck1 = ctx.bases_generate(_lib.CURVE_BN254_G1, 1 << 19).precompute(15)      # the shared-bucket tables the benchmark folds with
    ck2 = ctx.bases_generate(_lib.CURVE_GRUMPKIN, 1 << 13, b"ck-secondary")
    yield ctx, ck1, ck2
    ck1.free(); ck2.free()
    ctx.close()


def _proof(ctx, ck1, ck2, max_batch, rows_group):
    """everything the proof consists of after ten rows, as bytes, and the verifier's code"""
    from vimz_amd import hip
    z0, inputs = step_inputs("contrast")
    rows = np.stack(inputs)[:ROWS]
    assert len(rows) == ROWS
    c = Circuit.for_resolution("contrast", "HD")
    head = hip.set_head_rows(0)                  # every row's witness — and commitment — from the GPU's producer
    group = hip.set_rows_group(rows_group)
    try:
        ivc = hip.IVC(ctx, c, ck1, ck2, max_batch=max_batch)
        try:
            ivc.reset(z0)
            ivc.fold(rows)
            code = ivc.verify(ROWS, z0)
            parts = {"state": repr(ivc.state()).encode(), "proof": ivc.proof_export().tobytes()}
            for side in (0, 1):
                for name, what in (("instance", hip.IX_INSTANCE), ("running_z", hip.IX_RUNNING_Z), ("running_e", hip.IX_RUNNING_E)):
                    parts[f"{name}{side}"] = np.ascontiguousarray(ivc.export(side, what)).tobytes()
            for name, what in (("fresh_instance1", hip.IX_FRESH_INSTANCE), ("fresh_z1", hip.IX_FRESH_Z)):          # (the last fresh secondary instance and its witness)
                parts[name] = np.ascontiguousarray(ivc.export(1, what)).tobytes()
        finally:
            ivc.close()
    finally:
        hip.set_rows_group(group)
        hip.set_head_rows(head)
    return code, parts


@pytest.mark.parametrize("max_batch", [16, 3])
def test_the_proof_is_the_same_with_row_groups_and_without(setup, max_batch):
    ctx, ck1, ck2 = setup
    code_g, grouped = _proof(ctx, ck1, ck2, max_batch, 8)
    code_r, per_row = _proof(ctx, ck1, ck2, max_batch, 0)
    assert code_g == 0 and code_r == 0, (code_g, code_r)
    assert grouped.keys() == per_row.keys()
    for k in grouped:
        assert len(grouped[k]) > 0 and grouped[k] == per_row[k], f"{k} differs between grouped and per-row issue (max_batch {max_batch})"
