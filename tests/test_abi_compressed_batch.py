"""The batched compressed-proof verifier's C ABI: what include/vimz_hip.h and include/vimz_hip_testing.h declare for it is what the two libraries export — the two
entry points in both, the hooks and the given-multiplier twins in libvimz_hip_testing.so alone (no GPU needed)."""
import ctypes
import os

from tests.test_abi import declared_symbols

ENTRIES = {"vimz_ivc_verify_compressed_batch", "vimz_cf_verify_compressed_batch"}
HOOKS = {"vimz_test_spartan_batch_group", "vimz_test_spartan_batch_split", "vimz_test_spartan_mat_eval", "vimz_test_spartan_svec_accum", "vimz_test_spartan_instance_batch",
         "vimz_testing_ivc_verify_compressed_batch_scalars", "vimz_testing_cf_verify_compressed_batch_scalars"}


def _libs():
    from vimz_amd import _lib
    if not os.path.exists(_lib.PRODUCT_SO_PATH) or not os.path.exists(_lib.TESTING_SO_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_lib.PRODUCT_SO_PATH), ctypes.CDLL(_lib.TESTING_SO_PATH)


def test_the_headers_declare_the_batch_entries_and_hooks():
    product, testing = set(declared_symbols()), set(declared_symbols("vimz_hip_testing.h"))
    assert ENTRIES <= product
    assert HOOKS <= testing - product
    named = {s for s in product | testing if "compressed_batch" in s or s.startswith("vimz_test_spartan_batch") or s in ("vimz_test_spartan_mat_eval", "vimz_test_spartan_svec_accum",
                                                                                                                         "vimz_test_spartan_instance_batch")}
    assert named == ENTRIES | HOOKS          # nothing of the batch is declared beyond these


def test_the_libraries_export_exactly_what_is_declared():
    P, T = _libs()
    assert all(hasattr(P, s) for s in ENTRIES) and all(hasattr(T, s) for s in ENTRIES | HOOKS)
    assert not [s for s in HOOKS if hasattr(P, s)]


def test_an_empty_batch_needs_a_verifier_key():
    """n = 0 is accepted only with a key: a NULL one is an invalid argument, not a crash"""
    from vimz_amd import _lib
    P, _ = _libs()
    for name in ENTRIES:
        fn = getattr(P, name)
        fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        assert fn(None, 0, None, None, None, None, 0, None, None) == _lib.ERR_INVALID
