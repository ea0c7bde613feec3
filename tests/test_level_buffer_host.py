"""SourceFuncLW without a GPU: host containers hold two separate level arrays, and the pointer helper takes a pair of
views only when it is exactly the two views of one level buffer (tests/test_gpu_level_buffer.py covers the device side)."""
import numpy as np
import pytest


class Desc:
    def get_ngpt(self):
        return 5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_containers_hold_two_arrays(pkg, dtype):
    ng, nlay, ncol = 5, 4, 7
    src = pkg.SourceFuncLW()
    assert src.lev_source is None and src.lev_source_inc is None and src.level_views() == (None, None)
    assert src.alloc(ncol, nlay, Desc(), like=np.empty(0, dtype)) == ""
    assert src.lev_source is None and not src.levels_shared
    inc, dec = src.level_views()
    assert inc is src.lev_source_inc and dec is src.lev_source_dec
    assert inc.shape == dec.shape == (ng, nlay, ncol) and inc.dtype == dec.dtype == dtype
    assert inc.flags.c_contiguous and dec.flags.c_contiguous and not np.shares_memory(inc, dec)
    assert src.separate_levels() is src and src.lev_source_inc is inc      # nothing to copy out
    own = np.zeros((ng, nlay, ncol), dtype)
    src.lev_source_dec = own
    assert src.lev_source_dec is own and src.level_views() == (inc, own)


def test_pointer_helper_refuses_other_views(pkg):
    ng, nlay, ncol = 3, 4, 6
    lev = np.zeros((ng, nlay + 1, ncol))
    src = pkg.SourceFuncLW()
    src.lev_source_inc, src.lev_source_dec = lev[:, 1:], lev[:, :-1]      # host views: not taken (ECCKD_HOST copies arrays)
    with pytest.raises(TypeError):
        pkg._lev_ptrs(src, (ng, nlay, ncol))
    src.lev_source_inc, src.lev_source_dec = np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1])
    a, b = pkg._lev_ptrs(src, (ng, nlay, ncol))
    assert a.value == src.lev_source_inc.ctypes.data and b.value == src.lev_source_dec.ctypes.data
    with pytest.raises(ValueError):
        pkg._lev_ptrs(src, (ng, nlay + 1, ncol))
