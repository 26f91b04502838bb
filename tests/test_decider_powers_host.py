"""The refusals of the set-up from a powers-of-tau string that need no device: hip.Decider(powers=) with a second source of the KZG verifying key or a seed,
folding.prepare_folding(powers=) for a backend without a tau, and the command line's usage."""
import pytest


class NoDevice:
    """stands where a prover or a context would: any use of it is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"touched the device side ({name}) before refusing")


def test_decider_refuses_powers_with_a_kzg_vk_or_a_seed():
    from vimz_amd import _lib, hip
    for extra in ({"kzg_vk": [[0] * 4] * 4}, {"seed": b"x"}):
        with pytest.raises(_lib.VimzError, match="powers= brings its own KZG verifying key") as e:
            hip.Decider(NoDevice(), powers={}, **extra)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.VimzError, match="delta= goes with powers="):
        hip.Decider(NoDevice(), delta=5)


def test_prepare_folding_takes_powers_for_the_sonobe_backend_only():
    from vimz_amd import _lib, folding
    with pytest.raises(_lib.VimzError, match="powers= is for the Sonobe backend") as e:
        folding.prepare_folding(NoDevice(), "hash", "HD", powers={})
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.VimzError, match="powers= is for the Sonobe backend"):      # before a context or a thread is made
        folding.prepare_folding_overlapped(0, 2, "hash", "HD", mode="ivc", powers={})


def test_command_line_states_both_forms(capsys):
    from vimz_amd import iden3
    assert iden3._main(["decider-key", "only.ptau"]) == 2 and iden3._main(["decider-key", "a.ptau", "hash", "HD", "out.key", "--full"]) == 2
    err = capsys.readouterr().err
    assert "decider-key FILE.ptau TRANSFORMATION RESOLUTION OUT.key [--light]" in err and "lagrange FILE.ptau LOGN OUT.npz" in err
