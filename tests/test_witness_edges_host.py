"""The edge cases of tests/_witness_edges.py, checked on the CPU by three independent judges: the oracle's executor over the
product-built witness program, the oracle's R1CS check of the executor's wires, and the semantic step oracle (oracle/steps.hpp, the
authority).  This validates the cases themselves — the GPU test (tests/test_gpu_witness_edges.py) compares the kernels with the
executor on exactly these rows — and re-derives the factor ceilings (contrast 2.2, brightness 1.6 on rows that hold 0 and 255)
from the semantic oracle on every run."""
import numpy as np
import pytest

from tests import _witness_edges as we
from tests._oracle import T_CROP, r1cs_check, witness_execute
from tests.test_circuits import ORC_T as _ORC_T
from vimz_amd.circuit import Circuit

ORC_T = dict(_ORC_T, crop=T_CROP)
KEYS = list(we.CIRCUITS)

_circuits = {}


def circuit(key):
    if key not in _circuits:
        args = we.CIRCUITS.get(key) or we.REFUSED[key]
        _circuits[key] = Circuit(*args)
    return _circuits[key]


def executed(oracle, key):
    """The executor over every run of a circuit: yields (run, [(status, wires, z_in, z_out) per row]).  Rows are chained through the
    executor's own output state, satisfied or not."""
    c = circuit(key)
    for run in we.cases()[key][1]:
        z, rows = [int(v) for v in run.z0], []
        for priv in run.rows:
            st, wires, z_out = witness_execute(oracle, c, z, priv)
            rows.append((st, wires, z, z_out))
            z = z_out
        yield run, rows


def poseidon_widths(c):
    jobs = c.export("JOBS", np.uint32).reshape(-1, 20)      # HashJob: t, wire_base, out_wire, chain, eight (kind, idx) inputs
    assert jobs.shape[0] == c.n_jobs
    return sorted(set(int(t) for t in jobs[:, 0]))


@pytest.mark.parametrize("key", KEYS)
def test_edge_cases_are_what_they_claim(oracle, key):
    args = we.CIRCUITS[key]
    c = circuit(key)
    kw = we.step_kwargs(args)
    n = 0
    for run, rows in executed(oracle, key):
        for i, (st, wires, z, z_out) in enumerate(rows):
            what, where = we.expect_of(run, i), f"{key} / {run.name} / row {i}"
            bad = r1cs_check(oracle, c, wires)
            ok, z_sem = oracle.step_eval(ORC_T[args[0]], z, run.rows[i], **kw)
            if what == "sat":
                assert st == 0 and bad == -1, f"{where}: executor status {st}, first violated R1CS row {bad}"
                assert ok and z_out == z_sem, f"{where}: the semantic oracle disagrees"
            else:
                assert what in ("unsat", "r1cs"), what
                assert st != 0 or bad != -1, f"{where}: expected to fail, but the executor's witness satisfies the R1CS"
                assert not ok, f"{where}: expected to fail, but the semantic oracle accepts it"
                if what == "r1cs":
                    assert st == 0 and bad != -1, f"{where}: executor status {st}, first violated R1CS row {bad}"
            n += 1
    assert n == sum(len(r.rows) for r in we.cases()[key][1]) > 0


def test_every_kind_of_case_is_present():
    """The builder's own census: an empty or thinned list cannot pass for the whole."""
    cs = we.cases()
    assert list(cs) == KEYS and len(KEYS) == 17
    for key, (args, runs) in cs.items():
        names = [r.name for r in runs]
        op, width = args[0], args[1]
        if op in we.PIXEL_OPS:
            assert names[:7] == list(we.IMAGES)
            tol = [we.expect_of(r, i) for r in runs for i in range(len(r.rows)) if r.name.startswith("tol")]
            assert sorted(tol) == ["sat"] * 8 + ["unsat"] * 8 and sum(r.name.count("tol-x") for r in runs) == 16
            assert len([r for r in runs if r.name.startswith("tol")]) == (16 if op in ("blur", "sharpness") else 2)
            assert any("bit240-first" in x for x in names) and any("bit240-last" in x for x in names) and any("bit239" in x for x in names)
        if op in we.FACTOR10:
            sat, first_unsat = we.FACTOR10[op]
            for img in ("extremes", "checker"):
                for f10 in sat:
                    assert we.find(key, f"{img}-f{f10}").expect == "sat"
                if width == 16:
                    assert we.find(key, f"{img}-f{first_unsat}").expect == ("unsat",) * 6
    assert we.find("contrast-16", "mid-batch").expect == ("sat", "sat", "unsat", "sat", "sat")
    assert [r.name for r in cs["crop-16"][1]].count("three-rows") == 1 and we.find("crop-16", "x160").expect == ("r1cs",)
    assert we.n_triples() == sum(len(r.rows) for _, runs in cs.values() for r in runs) > 1000


def test_poseidon_widths_of_the_shapes():
    """The GPU chain kernel has the permutations of width 3 and 9 only: every circuit of the table uses no other, and the two shapes
    the prover must refuse (tests/test_gpu_witness_edges.py) do."""
    for key in KEYS:
        assert poseidon_widths(circuit(key)) == [3, 9], key      # (the pair hash with the state is three wide)
    for key in we.REFUSED:
        assert set(poseidon_widths(circuit(key))) - {3, 9}, key
