"""The kernels of the multilinear KZG opening on the GPU (vimz_amd/csrc/mlkzg.hip: k_mle_fold, k_poly_eval3 + k_eval3_sum, k_batch_levels, k_div_carry + k_div_scan +
k_div_chunk) through their hooks, every output word for word against tests/_mlkzg_ref.py.  The sizes come from the hook's own constants B (threads of a block) and c
(coefficients of a thread): the evaluation and the division run at n = 1, 2, c − 1, c, c + 1, B·c − 1, B·c, B·c + 1 and 2·B·c + 3 — on each side of the chunk, the
block and the cross-block boundary — with u = 0, 1, r − 1 and random ones; the fold and the batching at ℓ = 1, 2, 3 and the least ℓ with 2^ℓ > B·c, with x_k = 0, 1
and random ones.  The division is compared launch by launch: each chunk's carry-out, the carry into each chunk, then the quotient and the remainder.  The GPU half
is tests/_mlkzg_gpu.py, one child process."""
import pytest

from tests import _mlkzg_gpu as G
from tests import _mlkzg_ref as M
from tests._g16_kernels_gpu import hex_ints
from tests._pairing import R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return G.run_part(tmp_path_factory, "kernels")


def _sizes(probe):
    block, chunk = probe["shape"]
    assert block % 64 == 0 and chunk % 2 == 0 and chunk >= 2
    return G.sizes(block, chunk)


@pytest.mark.parametrize("which", range(9))
def test_evaluation_at_r_minus_r_and_r_squared(probe, which):
    n = _sizes(probe)[which]
    p = G.coeffs(n)
    for u in G.EVAL_U:
        assert hex_ints(probe["eval"][f"{n}/{u}"]) == M.eval3(p, u), (n, u)


def test_evaluation_of_several_levels_in_one_launch(probe):
    n0 = _sizes(probe)[-1]
    levels = [G.coeffs(ln, f"levels{k}") for k, ln in enumerate(G.level_lengths(n0, 3))]
    want = [M.eval3(p, G.U_RANDOM[1]) for p in levels]
    assert hex_ints(probe["eval_levels"]) == [want[k][u] for u in range(3) for k in range(3)]


@pytest.mark.parametrize("which", range(9))
def test_division_launch_by_launch(probe, which):
    n = _sizes(probe)[which]
    chunk = probe["shape"][1]
    b = G.coeffs(n)
    for k, us in enumerate(G.DIVIDE_U):
        got = probe["divide"][f"{n}/{k}"]
        want = [M.divide(b, u) for u in us]
        carries = [M.division_carries(b, u, chunk) for u in us]
        assert hex_ints(got["carry"]) == [c for out, _ in carries for c in out], (n, k)
        assert hex_ints(got["carry_in"]) == [c for _, cin in carries for c in cin], (n, k)
        assert hex_ints(got["quot"]) == [c for quot, _ in want for c in quot], (n, k)
        assert hex_ints(got["rem"]) == [rem for _, rem in want] == [M.horner(b, u) for u in us], (n, k)


@pytest.mark.parametrize("which", range(4))
def test_fold_and_batching(probe, which):
    logn = G.fold_logns(*probe["shape"])[which]
    N = 1 << logn
    assert which < 3 or N > probe["shape"][0] * probe["shape"][1] >= N // 2
    v = G.coeffs(N, "fold")
    for kind in G.X_KINDS:
        x = G.point(logn, kind)
        levels = M.fold_levels(v, x)
        assert hex_ints(probe["fold"][f"{logn}/{kind}"]) == [c for p in levels for c in p], (logn, kind)
        assert levels[logn] == [{"zero": v[0], "one": v[N - 1]}.get(kind, levels[logn][0])]
    levels = [G.coeffs(N >> k, f"batch{k}") for k in range(logn)]
    for name, q in (("random", G.U_RANDOM[0]), ("minus_one", R - 1), ("zero", 0)):
        assert hex_ints(probe["batch"][f"{logn}/{name}"]) == M.batch_levels(levels, q), (logn, name)


def test_the_hooks_refusals(probe):
    assert set(probe["refused"]) == {"eval_n_0", "eval_element_r", "divide_n_0", "fold_logn_0"}
    assert all(rc == probe["invalid"] for rc in probe["refused"].values()), probe["refused"]
