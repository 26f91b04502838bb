#!/usr/bin/env python3
"""How many wires of a step circuit's fresh witness are "negative small" field elements — above (p - 1)/2 with p - w below 2^128 —, i.e. what
the MSM's signed scalar loader (VIMZ_TUNE=signed_scalars, msm.hpp) saves on the witness commitment MSM(W).  No GPU: the witness comes from the
oracle's executor over the circuit library's witness program, on the fixture rows.
usage: witness_negative_wires.py [transformation] [resolution] [rows]"""
import json
import sys

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from tests import _oracle  # noqa: E402
from tests.test_circuits import step_inputs  # noqa: E402
from vimz_amd.circuit import Circuit  # noqa: E402

P = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def main():
    t = sys.argv[1] if len(sys.argv) > 1 else "contrast"
    res = sys.argv[2] if len(sys.argv) > 2 else "HD"
    rows = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    orc = _oracle.load()
    c = Circuit.for_resolution(t, res)
    z, inputs = step_inputs(t)
    out = []
    for i in range(rows):
        st, wires, z_out = _oracle.witness_execute(orc, c, z, inputs[i])
        assert st == 0, st
        w = _oracle.from_limbs(wires)
        half = (P - 1) // 2
        out.append({"row": i, "wires": len(w), "zero": sum(1 for x in w if x == 0), "one": sum(1 for x in w if x == 1),
                    "above_half": sum(1 for x in w if x > half),
                    "negative_below_2_128": sum(1 for x in w if x > half and P - x < (1 << 128)),
                    "negative_below_2_64": sum(1 for x in w if x > half and P - x < (1 << 64)),
                    "positive_below_2_128": sum(1 for x in w if 1 < x < (1 << 128))})
        z = list(z_out)
    print(json.dumps({"circuit": f"{t}_step_{res}", "rows": out}))


if __name__ == "__main__":
    main()
