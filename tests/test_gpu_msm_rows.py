"""msm_launch_rows: G vectors over one key committed by ONE chain of launches (the row in a grid dimension, a slice of every workspace array per
row) and the group's unit sums in two launches.  Every row of every group must come out bit-equal to vimz_msm on that row alone — rows that
differ as much as rows can (all zero, all one, one dense value repeated: the two-stage fold of very heavy buckets and its tickets, dense, p - small,
40 % ones), at n = 33 000 just above the fused small path's limit, the rows further apart than they are long, with the key's c = 15 tables and
without, for G in {1, 2, 3, 8}; the same call twice on one workspace (every ticket resets itself); the grouped S_1 sums against one ones_launch per
row; one row against the CPU oracle."""
import json
import os
import subprocess
import sys

import pytest

from tests import _msm_rows_gpu as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = tmp_path_factory.mktemp("msm_rows") / "points.json"
    r = subprocess.run([sys.executable, "-m", "tests._msm_rows_gpu", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "VIMZ_HIP_LIBRARY": "testing"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as fp:
        return json.load(fp)


@pytest.mark.parametrize("tables", [0, 1])
@pytest.mark.parametrize("G", sorted(R.GROUPS))
def test_every_row_of_a_group_equals_the_row_alone(probe, tables, G):
    got = probe["groups"][f"{tables}/{G}"]["out"]
    assert len(got) == R.CALLS * G
    for call in range(R.CALLS):          # the second call finds the workspace as the first left it
        for j, m in enumerate(R.GROUPS[G]):
            assert got[call * G + j] == probe["alone"][f"{tables}/{R.KINDS[m]}"], (f"call {call} row {j} ({R.KINDS[m]})")
    if 0 in R.GROUPS[G]:
        assert got[R.GROUPS[G].index(0)] == [0, 0]          # the all-zero row commits to the identity


@pytest.mark.parametrize("tables", [0, 1])
@pytest.mark.parametrize("G", sorted(R.GROUPS))
def test_grouped_unit_sums_equal_one_launch_per_row(probe, tables, G):
    g = probe["groups"][f"{tables}/{G}"]
    assert len(g["s1"]) == R.CALLS * G and len(g["s1_ref"]) == G
    for call in range(R.CALLS):
        assert g["s1"][call * G:(call + 1) * G] == g["s1_ref"], f"call {call}"
    for j, m in enumerate(R.GROUPS[G]):
        if R.KINDS[m] in ("zero", "repeat", "neg_small"):
            assert g["s1_ref"][j] == [0, 0]                 # no unit scalar among them
        if R.KINDS[m] == "ones40":
            assert g["s1_ref"][j] == probe["oracle_s1_ones40"] != [0, 0]


def test_a_row_equals_the_oracle(probe):
    assert probe["oracle"] != [0, 0]
    for tables in (0, 1):
        assert probe["alone"][f"{tables}/{R.KINDS[R.ORACLE_ROW]}"] == probe["oracle"]
        assert probe["groups"][f"{tables}/8"]["out"][R.GROUPS[8].index(R.ORACLE_ROW)] == probe["oracle"]
