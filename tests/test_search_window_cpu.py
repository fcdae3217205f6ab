"""vlg_queries_set_windows / vlg_queries_get_windows without a device: a NULL batch is refused on the host, nothing asks for a GPU."""
import ctypes as C


def test_null_batch_is_refused_without_a_device():
    import vlg_matching_amd as V
    L = V.lib()
    b, e = (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 2)(5, 6)
    has = C.c_int(7)
    assert L.vlg_queries_set_windows(None, b, e) == V.capi.E_INVALID
    assert L.vlg_queries_set_windows(None, None, None) == V.capi.E_INVALID
    assert L.vlg_queries_get_windows(None, C.byref(has), b, e) == V.capi.E_INVALID
    assert L.vlg_queries_get_windows(None, None, None, None) == V.capi.E_INVALID
    assert has.value == 7 and list(b) == [0, 1] and list(e) == [5, 6]          # (nothing was written)
    assert b"null" in L.vlg_last_error()
