"""olap_store_set_values / olap_sharded_store_set_values check their arguments on the host before any device work: the
same errors with and without a GPU, and a refused batch writes nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_package

pkg = load_package()
capi = pkg.capi


def test_null_arguments_without_a_device():
    L = capi.lib()
    idx = (C.c_uint64 * 1)(0)
    val = (C.c_double * 1)(1.0)
    for fn in (L.olap_store_set_values, L.olap_sharded_store_set_values):
        assert fn(None, 1, idx, val, None) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "store is NULL"
        assert fn(None, 0, None, None, None) == capi.ERR_INVALID_ARGUMENT


def test_entries_are_decoded_on_the_host():
    from olap_in_memory_amd.hipstore import _entries

    n, idx, vals, nulls = _entries([3, 1, 3], [1.5, None, 2])
    assert n == 3 and list(idx[:3]) == [3, 1, 3] and list(vals[:3]) == [1.5, 0.0, 2.0] and list(nulls[:3]) == [0, 1, 0]
    n, idx, vals, nulls = _entries(np.array([4, 0]), np.array([1.0, 2.0]))
    assert n == 2 and nulls is None and list(vals[:2]) == [1.0, 2.0]
    with pytest.raises(ValueError, match="2 indexes, 1 values"):
        _entries([1, 2], [0.5])


@pytest.mark.gpu
def test_argument_errors_leave_the_store_unchanged():
    L = capi.lib()
    s = pkg.HipStore(10, "float32", 0.0).track_order()
    s.set_data_f64(np.arange(10.0))
    before = (s.get_data().tobytes(), s.get_status().tobytes(), list(s.keys()), s.order_tracked)

    def state():
        return (s.get_data().tobytes(), s.get_status().tobytes(), list(s.keys()), s.order_tracked)

    val = (C.c_double * 3)(1.0, 2.0, 3.0)
    assert L.olap_store_set_values(s._h, 3, None, val, None) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "indexes/values is NULL"
    assert L.olap_store_set_values(s._h, 3, (C.c_uint64 * 3)(0, 1, 2), None, None) == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(pkg.OlapError) as ei:
        s.set_values([4, 0, 10], [1.0, 2.0, 3.0])
    assert ei.value.code == capi.ERR_INDEX_RANGE
    assert "entry 2: cell index 10 out of bounds [0, 10[" in str(ei.value)
    assert state() == before
    # n == 0 is a no-op, NULL lists included: the lazy order stays lazy
    assert L.olap_store_set_values(s._h, 0, None, None, None) == capi.OK
    s.set_values([], [])
    assert state() == before and s.order_tracked == 1
