"""pf_create at the widths of the width-generic family: accepted (PF_OK with a device; without one, the "no HIP device" error
-2 rather than the argument error -1), and widths outside the supported set still rejected with the field named."""
import ctypes

import pytest
import torch

import pharmacoforge_amd as pfa

SUPPORTED = [(256, 16), (64, 32), (192, 32)]
REJECTED = [((100, 16), b"n_hidden_scalars"), ((128, 24), b"vector_size"), ((288, 16), b"n_hidden_scalars"),
            ((128, 8), b"vector_size")]


def config(S, V):
    # the struct of test_host_logic.test_bad_config_rejected, at the given widths
    return pfa._lib.PfConfig(pfa._lib.PF_ABI_VERSION, 6, 11, V, S, 2, 3, 2, 4, 0, 1.0, 0, 5, 3.5, 8, 8, 9, 15.0, 16)


def create(S, V):
    lib = pfa._lib.load()
    h = ctypes.c_void_p()
    rc = lib.pf_create(ctypes.byref(config(S, V)), ctypes.byref(h))
    msg = lib.pf_last_error(None)
    if rc == 0:
        lib.pf_destroy(h)
    return rc, msg


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-device answer; test_supported_widths_create covers a GPU")
@pytest.mark.parametrize("S,V", SUPPORTED)
def test_supported_widths_pass_validation_without_device(S, V):
    rc, msg = create(S, V)
    assert rc == -2, (rc, msg)
    assert b"no HIP device" in msg


@pytest.mark.gpu
@pytest.mark.parametrize("S,V", SUPPORTED)
def test_supported_widths_create(S, V):
    rc, msg = create(S, V)
    assert rc == 0, (rc, msg)


@pytest.mark.parametrize("wh,field", REJECTED)
def test_unsupported_widths_rejected(wh, field):
    rc, msg = create(*wh)
    assert rc == -1 and field in msg, (rc, msg)
