"""CPU-only checks of the select entry points (vlg_select_support, vlg_bit_select_batch, vlg_wt_select_batch, vlg_int_select_batch,
vlg_psi_batch, vlg_lf_batch, vlg_bwt_batch): they are bound, their argument checks answer before a device is asked for, and without a
GPU a create is refused loudly."""
import ctypes as C
import os

import numpy as np
import pytest

NAMES = ["vlg_bitvector_select_create", "vlg_rrr_bitvector_select_create", "vlg_index_select_create", "vlg_select_support_hbm_bytes",
         "vlg_select_support_destroy", "vlg_bit_select_batch", "vlg_wt_select_batch", "vlg_int_select_batch", "vlg_psi_batch", "vlg_lf_batch",
         "vlg_bwt_batch"]
CREATES = NAMES[:3]


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    if not os.path.exists(v.library_path()):
        v.build_library()
    return v


@pytest.fixture(scope="module")
def source():
    """a non-null pointer that stands for a bit-vector / an index: the checks under test answer before it is looked at"""
    buf = np.zeros(512, np.uint64)
    return buf, C.c_void_p(buf.ctypes.data)


def test_bindings_exist(V):
    L = V.lib()
    bound = {s[0] for s in V.capi.SYMBOLS}
    for n in NAMES:
        assert n in bound and hasattr(L, n), n
    for n in ("SelectSupport",):
        assert hasattr(V, n)
    for cls in (V.VlgIndex, V.BitVector, V.RrrBitVector):
        assert hasattr(cls, "select_support")
    for m in ("hbm_bytes", "bit_select", "bit_select_device", "select", "select_device", "psi", "psi_device"):
        assert hasattr(V.SelectSupport, m), m
    for m in ("lf", "lf_device", "bwt", "bwt_device"):
        assert hasattr(V.VlgIndex, m), m


def test_create_refuses_null_and_bad_sample_before_the_device(V, source):
    L = V.lib()
    _, src = source
    h = C.c_void_p()
    for n in CREATES:
        f = getattr(L, n)
        assert f(None, 0, None, C.byref(h)) == V.capi.E_INVALID, n
        assert f(src, 0, None, None) == V.capi.E_INVALID, n
        for sample in (1, 100):
            h.value = 1
            assert f(src, sample, None, C.byref(h)) == V.capi.E_INVALID, (n, sample)
            assert not h.value
            assert b"sample" in L.vlg_last_error()


def test_batches_refuse_null_arguments(V, source):
    L = V.lib()
    buf, p = source
    assert L.vlg_bit_select_batch(None, 1, p, p, 1, None) == V.capi.E_INVALID
    assert L.vlg_wt_select_batch(None, p, p, p, 1, None) == V.capi.E_INVALID
    assert L.vlg_int_select_batch(None, p, p, p, 1, None) == V.capi.E_INVALID
    assert L.vlg_psi_batch(None, p, p, 1, None) == V.capi.E_INVALID
    assert L.vlg_lf_batch(None, p, p, 1, None) == V.capi.E_INVALID
    assert L.vlg_bwt_batch(None, p, p, 1, None) == V.capi.E_INVALID
    assert L.vlg_select_support_hbm_bytes(None) == 0
    L.vlg_select_support_destroy(None)


def test_no_gpu_means_every_create_is_refused(V, source):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = V.lib()
    _, src = source
    for n in CREATES:
        for sample in (0, 64, 512):
            h = C.c_void_p(1)
            assert getattr(L, n)(src, sample, None, C.byref(h)) == V.capi.E_NO_DEVICE, (n, sample)
            assert not h.value
