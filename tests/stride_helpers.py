"""Shared by the tests that run a form once on a few distinct columns and once on those columns repeated cyclically past a
grid cap (tests/test_gpu_lw_split_stride.py, tests/test_gpu_grid_rounds.py): a column's fluxes do not depend on where the
column sits, so the large call must hold the small call's column i % nsmall bit for bit."""
import numpy as np

COLUMN_FIRST = ("emis", "alb_dir", "alb_dif")   # (ncol, nband): every other array has the columns on its last axis


def repeated(d, ncol, wanted, nsmall, column_first=COLUMN_FIRST):
    """The arrays of `d` that the form reads, their columns repeated cyclically to ncol columns (on the device); the index of
    each column's origin."""
    import torch
    device = next(v.device for v in d.values() if isinstance(v, torch.Tensor))
    idx = torch.arange(ncol, device=device) % nsmall
    out = {}
    for n, v in d.items():
        if v is None or np.isscalar(v) or isinstance(v, np.ndarray):   # (numpy: call constants such as band2gpt)
            out[n] = v
        elif wanted(n):
            out[n] = v.index_select(0 if n in column_first else v.ndim - 1, idx).contiguous()
    return out, idx


def new(d, nlay, sentinel=-1.0, planes=None, like="plev"):
    """An output array (nlay+1, ncol) -- with `planes`, (planes, nlay+1, ncol) -- with the columns, the precision and the
    device of d[like], filled with `sentinel`."""
    import torch
    ncol = d[like].shape[-1]
    shape = (nlay + 1, ncol) if planes is None else (planes, nlay + 1, ncol)
    return torch.full(shape, sentinel, dtype=d[like].dtype, device=d[like].device)


def count_differing(got, want, idx):
    """How many values of `got` differ in their bits from the columns idx of `want` (same precision, columns last)."""
    import torch
    assert got.dtype == want.dtype and got.dtype in (torch.float64, torch.float32)
    bits = torch.int64 if got.dtype == torch.float64 else torch.int32
    return int((got.view(bits) != want.index_select(want.ndim - 1, idx).view(bits)).sum())
