"""Text access without a GPU: the C-ABI of vlg_text_access is bound as the header declares it, refuses null arguments, and the Python
wrapper checks its arguments before any device work."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    return v


def test_text_access_symbols_bound(V):
    bound = {s[0]: s for s in V.capi.SYMBOLS}
    for name in ("vlg_text_access_create", "vlg_text_access_destroy", "vlg_extract_batch", "vlg_isa_batch"):
        assert name in bound
        assert hasattr(C.CDLL(V.capi.library_path()), name)
    assert len(bound["vlg_extract_batch"][2]) == 8 and len(bound["vlg_isa_batch"][2]) == 5
    assert bound["vlg_text_access_create"][2][1] is C.c_uint32


def test_null_and_empty_arguments(V):
    L = V.lib()
    assert L.vlg_text_access_create(None, 64, None, None) == V.capi.E_INVALID
    assert L.vlg_extract_batch(None, None, None, None, 0, 0, None, None) == V.capi.E_INVALID
    assert L.vlg_isa_batch(None, None, None, 0, None) == V.capi.E_INVALID
    L.vlg_text_access_destroy(None)


def _fake(V, n, is_int):
    t = V.index.TextAccess.__new__(V.index.TextAccess)
    t._h, t.n, t.is_int, t.inv_dens = None, n, is_int, 64
    return t


def test_python_argument_checks(V):
    t = _fake(V, 100, False)
    with pytest.raises(ValueError):
        t.extract(5, 4)
    with pytest.raises(ValueError):
        t.extract(0, 100)
    with pytest.raises(ValueError):
        t.extract(-1, 3)
    with pytest.raises(ValueError):
        t.extract_batch([0, 1], [3])
    with pytest.raises(ValueError):
        t.extract_batch([0, 9], [3, 8])
    with pytest.raises(ValueError):
        t.extract_batch([0.5], [3])
    with pytest.raises(ValueError):
        t.isa([3, 100])
    with pytest.raises(ValueError):
        t.isa(-2)
    out, off = t.extract_batch([], [])
    assert out.dtype == np.uint8 and len(out) == 0 and off.tolist() == [0]
    assert _fake(V, 10, True).extract_batch([], [])[0].dtype == np.uint32
    with pytest.raises(ValueError):
        V.index.TextAccess(None, inv_dens=0)
