"""The chains of the full decider's check 5 without a GPU: the Python reference (tests/_cf_chains_ref.py) against the circuit's rows and an independent
scalar multiplication, and against the host function the prover and the circuit's witness generator share (cf_open_chains_host, through
vimz_test_decider_chains with where = 0).  Every comparison is exact equality of integers."""
import ctypes
import functools
import os

import pytest

from tests import _cf_chains_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _testing_lib():
    from vimz_amd import _lib
    if not os.path.exists(_lib.TESTING_SO_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_lib.TESTING_SO_PATH)


@functools.lru_cache(maxsize=None)
def hook(name):
    """the host function on a case: (wires, ends, H, bad)"""
    n, sc = R.cases()[name]
    rc, w, e, h, bad = R.run_hook(_testing_lib(), None, 0, R.multiples(n), sc)
    assert rc == 0
    return w, e, h, bad


@functools.lru_cache(maxsize=None)
def derived_H():
    return hook("1/zero")[2]


def test_the_derived_generator_is_a_point_of_grumpkin():
    H = derived_H()
    assert R.on_curve(H) and all(0 < c < R.P for c in H) and R.on_curve(R.G) and R.mul(R.G, R.Q) is None
    assert all(hook(name)[2] == H for name in ("1/one", "65/different"))      # (it does not depend on the key)


def test_table_entries_are_the_multiples_they_stand_for():
    T = R.shared_table()
    for k, j, d in ((0, 0, 0), (0, 0, 3), (1, 1, 2), (256, 126, 3), (100, 63, 1)):
        assert T[k][j][d] == R.mul(R.G, (d + 1) * 4 ** j * (k + 1) % R.Q), (k, j, d)


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_reference_windows_satisfy_the_rows_and_end_where_they_must(name):
    H, T = derived_H(), R.shared_table()
    n, sc = R.cases()[name]
    wires, ends, bad = R.chains(T, H, sc)
    assert not bad and len(wires) == len(ends) == n
    gens = R.multiples(n)
    seen = {}
    for k, s in enumerate(sc):
        assert R.rows_hold(H, T[k], s, wires[k]), (name, k)
        assert ends[k] == (wires[k][-1][2], wires[k][-1][3])
        if (k, s) not in seen:      # H + (s + Σ_j 4^j)·G_k by double-and-add
            seen[(k, s)] = R.add(H, R.mul(gens[k], (s + R.OFFSET) % R.Q))
        assert ends[k] == seen[(k, s)], (name, k)


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_host_function_equals_the_reference(name):
    w, e, h, bad = hook(name)
    want_w, want_e = R.expected(name, derived_H())
    assert bad == 0 and h == derived_H()
    assert e == want_e
    assert w == want_w


@pytest.mark.parametrize("name", R.DEGENERATE)
def test_host_function_flags_an_addition_of_points_with_the_same_x(name):
    H = derived_H()
    gens, sc = R.degenerate_case(name, H)
    assert R.chains(R.table(gens[:1]), H, sc[:1])[2]                       # the reference meets it in window 0 of chain 0
    rc, _, _, h, bad = R.run_hook(_testing_lib(), None, 0, gens, sc)
    assert rc == 0 and h == H and bad == 1
    honest = list(gens); honest[0] = R.G
    assert R.run_hook(_testing_lib(), None, 0, honest, sc)[4] == 0          # the same launch over G_0 = G: nothing to flag


def test_hook_refuses_what_is_outside_its_contract():
    from vimz_amd import _lib
    lib, g2 = _testing_lib(), R.multiples(2)
    assert R.run_hook(lib, None, 0, g2, [R.Q])[0] == _lib.ERR_INVALID              # a scalar not below q
    assert R.run_hook(lib, None, 0, g2[:1], [1, 2])[0] == _lib.ERR_INVALID         # more scalars than generators
    assert R.run_hook(lib, None, 0, [(R.P, 1)], [1])[0] == _lib.ERR_INVALID        # a coordinate not below the modulus
    assert R.run_hook(lib, None, 1, g2, [1])[0] == _lib.ERR_INVALID                # the device path without a context
