"""The shortwave on the daylit columns only, on the GPU: ecckd_daylit_columns, ecckd_gather_columns, ecckd_scatter_columns
and ecckd_sw_fluxes_daylit.

No tolerance anywhere.  The selection is compared with numpy.flatnonzero, gather and scatter with numpy fancy indexing, and
the fluxes of sw_fluxes_daylit bit for bit with (i) the existing call on columns gathered beforehand with numpy and
scattered back with zeros and (ii) the reference driver's recipe -- the existing call on ALL columns with mu0 = 1 in the
night columns, compared at the daylit columns (this rests on the standing promise that a column's fluxes do not depend on
the columns computed beside it: DESIGN.md section 7, tests/test_distributed_cpu.py).  Night columns are +0.0 at every level,
planes that were not requested keep their sentinel, and the caller's inputs come back bit-identical."""
import numpy as np
import pytest

import helpers
import mcica_helpers as mh
import test_gpu_allsky as swt
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
T, back = swt.T, swt.back
HOST = np.ascontiguousarray
NCOL = 300
GUARD = -77.0


@pytest.fixture(autouse=True)
def default_options(pkg):
    def reset():
        pkg.reset_solver_options()
        pkg.set_solver_option("sw_solver", 0)
        pkg.set_solver_option("sw_tail_split", 1)
        pkg.set_arithmetic(pkg.FAST)
    reset()
    yield
    reset()


@pytest.fixture(scope="module")
def sw(pkg, gpu):
    from conftest import SW_WIDE
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=0) == ""
    return k


# ------------------------------------------------------------------------------------------------
# selection
# ------------------------------------------------------------------------------------------------
def mu0_patterns(ncol, mu0_min):
    c = np.arange(ncol)
    rng = np.random.default_rng(ncol)
    night, day = mu0_min - 0.5, mu0_min + 0.25
    out = {"all night": np.full(ncol, night), "all day": np.full(ncol, day),
           "first only": np.where(c == 0, day, night), "last only": np.where(c == ncol - 1, day, night),
           "alternating": np.where(c % 2 == 0, day, night),
           "run over a block edge": np.where((c >= 200) & (c < 320), day, night),     # blocks of 256 columns: 200..319 straddles
           "random": rng.uniform(mu0_min - 1.0, mu0_min + 1.0, ncol)}
    nan = out["random"].copy()
    nan[::3] = np.nan
    out["NaN entries"] = nan
    equal = out["random"].copy()
    equal[::2] = mu0_min                                                               # exactly the threshold: night
    out["equal to mu0_min"] = equal
    return out


@pytest.mark.parametrize("ncol", [1, 63, 64, 65, 257, 1000, 70001])
def test_selection(pkg, gpu, ncol):
    """Wave edge (63, 64, 65), block edge (257), several blocks (1000) and more block counts than one trip of the scan takes
    (70 001 columns: 274 blocks of 256); fp64 and float32, host and device arrays; thresholds exact in float32."""
    t = T(gpu)
    for mu0_min in (0.0, 0.25):
        for name, mu0 in mu0_patterns(ncol, mu0_min).items():
            for dtype in (np.float64, np.float32):
                m = mu0.astype(dtype)
                want = np.flatnonzero(m.astype(np.float64) > mu0_min).astype(np.int32)
                for to in (t, HOST):
                    index, nday = pkg.daylit_columns(to(m), mu0_min)
                    what = (ncol, mu0_min, name, dtype.__name__, "device" if to is t else "host")
                    assert isinstance(nday, int) and nday == want.size, what
                    got = back(index)
                    assert got.dtype == np.int32 and got.shape == (nday,) and np.array_equal(got, want), what


# ------------------------------------------------------------------------------------------------
# gather / scatter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ninner,ncol,nouter", [(1, 300, 61), (5, 300, 1), (1, 65, 60 * 5)])
def test_gather_and_scatter(pkg, gpu, ninner, ncol, nouter):
    """Against numpy fancy indexing, bit for bit: 4- and 8-byte elements (fp64, float32, the 64-bit mask words, int32), lists
    of none, some and all columns, host and device arrays; the scatter leaves exactly `fill` in every unlisted column."""
    t = T(gpu)
    rng = np.random.default_rng(ninner * 1000 + ncol + nouter)
    lists = [np.zeros(0, np.int32), np.flatnonzero(rng.uniform(size=ncol) < 0.5).astype(np.int32), np.arange(ncol, dtype=np.int32),
             np.array([0], np.int32), np.array([ncol - 1], np.int32)]
    shape = (nouter, ncol, ninner)                                   # C order: the reverse of (ninner, ncol, nouter)
    for dtype in (np.float64, np.float32, np.uint64, np.int32):
        if dtype in (np.float64, np.float32):
            src = rng.standard_normal(shape).astype(dtype)
            src[0, 0, 0] = np.nan                                    # bits are moved, not values
        else:
            src = rng.integers(0, 2 ** 31 - 1, shape).astype(dtype)
            if dtype is np.uint64:
                src |= np.uint64(1) << np.uint64(63)
        dev = (lambda a: t(a.view(np.int64))) if dtype is np.uint64 else t           # (torch: the bits as int64)
        for idx in lists:
            for to in (dev, HOST):
                g = pkg.gather_columns(to(src), (t if to is dev else HOST)(idx), axis=1)
                got = back(g)
                got = got.view(dtype) if dtype is np.uint64 else got
                assert got.shape == (nouter, idx.size, ninner)
                assert np.array_equal(got.view(np.uint8), src[:, idx, :].view(np.uint8)), (dtype.__name__, idx.size)
                for fill in (0.0, -3.5):
                    packed = np.ascontiguousarray(src[:, idx, :])
                    dst = np.full(shape, 9, dtype=dtype)
                    d = to(dst)
                    pkg.scatter_columns(to(packed), (t if to is dev else HOST)(idx), d, axis=1, fill=fill)
                    got = back(d)
                    got = got.view(dtype) if dtype is np.uint64 else got
                    if dtype in (np.float64, np.float32):
                        fill_bits = np.array(fill, dtype=dtype)
                    else:                                            # integers receive the bits of the double / float fill
                        fill_bits = np.array(fill, dtype=np.float64 if dtype is np.uint64 else np.float32).view(dtype)
                    want = np.full(shape, fill_bits, dtype=dtype)
                    want[:, idx, :] = packed
                    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (dtype.__name__, idx.size, fill)


# ------------------------------------------------------------------------------------------------
# fluxes
# ------------------------------------------------------------------------------------------------
def daylit_case(k, c0, ncol, nlay, top_at_1=True):
    """sw_case with a true mu0 field: about half the columns at mu0 <= 0 (one exactly 0, one NaN)."""
    cols, cloud = swt.sw_case(k, c0, ncol, nlay, 23, top_at_1=top_at_1)
    mu0 = 2.0 * cols["mu0"] - 1.05
    mu0[1 % ncol] = 0.0
    mu0[2 % ncol] = np.nan
    cols["mu0"] = mu0
    cf = synthetic.cloud_fraction(c0, ncol, nlay)
    mask = mh.sample(cf if top_at_1 else HOST(cf[::-1]), k.get_ngpt(), mh.MAX_RAN, None, 5, c0)
    return cols, cloud, mask


def take_columns(cols, cloud, mask, idx):
    """The same case on the columns idx, gathered with numpy."""
    ncol = cols["mu0"].shape[0]
    def pick(v):
        if not isinstance(v, np.ndarray) or v.ndim == 0:
            return v
        if v.shape[-1] == ncol:
            return HOST(v[..., idx])
        return HOST(v[idx]) if v.shape[0] == ncol else v
    return ({n: pick(v) for n, v in cols.items()}, {n: pick(v) for n, v in cloud.items() if n in ("tau", "ssa", "g")},
            None if mask is None else pick(mask))


CONFIGS = {   # particles, delta_scale, mask, clear-sky outputs, flux_dir
    "clear sky": (False, False, False, False, True),
    "clear sky, no flux_dir": (False, False, False, False, False),
    "all-sky": (True, False, False, False, True),
    "all-sky, delta-scaled": (True, True, False, False, False),
    "McICA": (True, True, True, False, True),
    "both skies": (True, True, True, True, True),
}


def existing_call(pkg, k, cols, cloud, mask, to, config, top_at_1):
    """[up, dn(, dir)(, up_clear, dn_clear, dir_clear)] of the existing call that `config` names, as numpy arrays."""
    particles, delta, masked, clear, with_dir = CONFIGS[config]
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to, swt.SW_NAMES)
    args = (to(cols["plev"]), to(cols["tlay"]), gc, top_at_1, to(cols["mu0"]), to(cols["alb_dir"]), to(cols["alb_dif"]))
    new = lambda n: pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), GUARD)) for _ in range(n)))
    fl, fc = new(3 if with_dir else 2), new(3)
    scale = to(cols["scale"])
    dmask = None
    if masked:
        dmask = mask if to is HOST else to(mask.view(np.int64))
    if particles:
        part = swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), to)
    if not particles:
        assert k.sw_fluxes(*args, fl, toa_scale=scale) == ""
    elif clear:
        assert k.sw_fluxes_clear_allsky(*args, part, fl, fc, delta_scale=delta, toa_scale=scale, cloud_mask=dmask) == ""
    else:
        assert k.sw_fluxes_allsky(*args, part, fl, delta_scale=delta, toa_scale=scale, cloud_mask=dmask) == ""
    out = [fl.flux_up, fl.flux_dn] + ([fl.flux_dn_dir] if with_dir else [])
    if clear:
        out += [fc.flux_up, fc.flux_dn, fc.flux_dn_dir]
    return [back(a) for a in out]


def daylit_call(pkg, k, cols, cloud, mask, to, config, top_at_1, index=None):
    """The same outputs from sw_fluxes_daylit.  The outputs are every other plane of one pool filled with a sentinel: the
    planes between them, and those of outputs that were not requested, must keep it.  The inputs must come back as they went."""
    particles, delta, masked, clear, with_dir = CONFIGS[config]
    nlay, ncol = cols["tlay"].shape
    moved = []
    def rec(a):
        d = to(a)
        moved.append((np.ascontiguousarray(a).copy(), d))
        return d
    gc = helpers.product_gas_concs(pkg, cols, rec, swt.SW_NAMES)
    pool = to(np.full((13, nlay + 1, ncol), GUARD))
    planes = [pool[2 * i + 1] for i in range(6)]
    fl = pkg.FluxesBroadband(planes[0], planes[1], planes[2] if with_dir else None)
    fc = pkg.FluxesBroadband(planes[3], planes[4], planes[5]) if clear else None
    part = dmask = None
    if particles:
        part = pkg.OpticalProps2str()
        part.tau, part.ssa, part.g = rec(cloud["tau"]), rec(cloud["ssa"]), rec(cloud["g"])
    if masked:
        dmask = mask if to is HOST else to(mask.view(np.int64))
        moved.append((mask.copy(), dmask))
    args = (rec(cols["plev"]), rec(cols["tlay"]), gc, top_at_1, rec(cols["mu0"]), rec(cols["alb_dir"]), rec(cols["alb_dif"]))
    assert k.sw_fluxes_daylit(*args, fl, particles=part, fluxes_clear=fc, delta_scale=delta, toa_scale=rec(cols["scale"]),
                              cloud_mask=dmask, day_index=index) == ""
    used = [0, 1] + ([2] if with_dir else []) + ([3, 4, 5] if clear else [])
    whole = back(pool)
    for p in range(13):
        if p not in [2 * i + 1 for i in used]:
            assert np.all(whole[p] == GUARD), ("plane %d was written" % p, config)
    for before, after in moved:
        a = back(after)
        assert np.array_equal(before.view(np.uint8), (a.view(np.uint64) if before.dtype == np.uint64 else a).view(np.uint8)), config
    return [whole[2 * i + 1] for i in used]


def check_against_existing(pkg, k, cols, cloud, mask, to, config, top_at_1, got):
    day = np.flatnonzero(cols["mu0"] > 0)
    night = np.setdiff1d(np.arange(cols["mu0"].shape[0]), day)
    assert 0 < day.size < cols["mu0"].shape[0]
    what = (config, cols["tlay"].shape, top_at_1, "host" if to is HOST else "device")
    # (i) the existing call on the columns gathered beforehand with numpy, scattered back with zeros
    gcols, gcloud, gmask = take_columns(cols, cloud, mask, day)
    packed = existing_call(pkg, k, gcols, gcloud, gmask, to, config, top_at_1)
    assert len(got) == len(packed)
    for a, p in zip(got, packed):
        want = np.zeros_like(a)
        want[:, day] = p
        assert np.array_equal(a, want, equal_nan=not top_at_1), ("(i)",) + what
        assert np.all(a[:, night] == 0.0) and not np.any(np.signbit(a[:, night])), ("night columns",) + what
    if top_at_1:
        assert all(np.all(np.isfinite(a)) for a in got), what
    # (ii) the reference driver's recipe: all columns, mu0 = 1 in the night columns, compared at the daylit columns
    full = dict(cols)
    full["mu0"] = np.where(cols["mu0"] > 0, cols["mu0"], 1.0)
    everything = existing_call(pkg, k, full, cloud, mask, to, config, top_at_1)
    for a, e in zip(got, everything):
        assert np.array_equal(a[:, day], e[:, day], equal_nan=not top_at_1), ("(ii)",) + what


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("nlay", [60, 7, 61])
def test_fluxes(pkg, gpu, sw, nlay, config):
    """300 columns at 60 layers (the layer-systolic solver) and at 7 and 61 layers (the two-pass solver), both orientations,
    host and device arrays, with a list made beforehand and with the selection inside the call."""
    k, t = sw, T(gpu)
    if nlay == 7:   # (the layer-systolic solver serves up to 60 layers; "sw_solver" = 1 hands a shallow call to the two-pass one)
        pkg.set_solver_option("sw_solver", 1)
    for top_at_1 in (True, False):
        cols, cloud, mask = daylit_case(k, 5 * nlay, NCOL, nlay, top_at_1)
        for to in (t, HOST):
            index, nday = pkg.daylit_columns(to(cols["mu0"]))
            assert nday == int(np.sum(cols["mu0"] > 0))
            got = daylit_call(pkg, k, cols, cloud, mask, to, config, top_at_1, index)
            check_against_existing(pkg, k, cols, cloud, mask, to, config, top_at_1, got)
            again = daylit_call(pkg, k, cols, cloud, mask, to, config, top_at_1, None)     # the call selects
            for a, b in zip(got, again):
                assert np.array_equal(a, b, equal_nan=not top_at_1)


def test_fluxes_no_daylit_column_and_all(pkg, gpu, sw):
    """nday = 0 only zeroes the requested outputs; every column daylit equals the existing call."""
    k, t = sw, T(gpu)
    cols, cloud, mask = daylit_case(k, 11, 130, 60)
    for to in (t, HOST):
        dark = dict(cols)
        dark["mu0"] = np.where(np.isnan(cols["mu0"]), np.nan, -np.abs(cols["mu0"]))
        for config in ("clear sky, no flux_dir", "both skies"):
            for a in daylit_call(pkg, k, dark, cloud, mask, to, config, True):
                assert np.all(a == 0.0) and not np.any(np.signbit(a))
        lit = dict(cols)
        lit["mu0"] = np.where(cols["mu0"] > 0, cols["mu0"], 0.5)
        for config in ("clear sky", "both skies"):
            got = daylit_call(pkg, k, lit, cloud, mask, to, config, True)
            for a, b in zip(got, existing_call(pkg, k, lit, cloud, mask, to, config, True)):
                assert np.array_equal(a, b)


def test_fluxes_small_call_route(pkg, gpu, sw):
    """20 000 columns with about 8 000 daylit, 60 layers, clear sky: the inner call runs below 16 384 columns, the full call of
    (ii) above."""
    k, t = sw, T(gpu)
    ncol = 20000
    cols, cloud, mask = daylit_case(k, 77, ncol, 60)
    cols["mu0"] = np.where(np.random.default_rng(77).uniform(size=ncol) < 0.4, np.abs(cols["mu0"]) + 0.01, -0.2)
    nday = int(np.sum(cols["mu0"] > 0))
    assert 7000 < nday < 9000
    got = daylit_call(pkg, k, cols, cloud, mask, t, "clear sky", True)
    check_against_existing(pkg, k, cols, cloud, mask, t, "clear sky", True, got)


class StridedConcs:
    """A gas description whose h2o array has a column stride of 2 (every other column of a wider array) and whose other
    gases are scalars: what a host hands over through vmr_col_stride / vmr_lay_stride."""

    def __init__(self, pkg, names, wide, scalars):
        self.pkg, self.names, self.wide, self.scalars = pkg, list(names), wide, scalars

    def get_num_gases(self):
        return len(self.names)

    def entries(self, ncol, nlay, known=None):
        out = []
        for n in self.names:
            if known is not None and n not in known:
                out.append((n, None, 0, 0, 0.0))
            elif n == "h2o":
                out.append((n, self.wide, 2, 2 * ncol, 0.0))
            else:
                out.append((n, None, 0, 0, float(self.scalars.get(n, 0.0))))
        return out


def test_strided_gas_array_and_scalar_gases(pkg, gpu, sw):
    k, t = sw, T(gpu)
    nlay = 60
    cols, cloud, mask = daylit_case(k, 41, NCOL, nlay)
    scalars = {n: float(np.mean(cols[n])) for n in swt.SW_NAMES if n != "h2o" and n in cols}
    wide = np.full((nlay, 2 * NCOL), 0.5)                           # the odd columns would show: 0.5 is no trace gas
    wide[:, ::2] = cols["h2o"]
    dense = dict(cols)
    for n, v in scalars.items():
        dense[n] = v
    day = np.flatnonzero(cols["mu0"] > 0)
    for to in (t, HOST):
        w = to(wide)
        gc = StridedConcs(pkg, swt.SW_NAMES, w, scalars)
        fl = pkg.FluxesBroadband(*(to(np.full((nlay + 1, NCOL), GUARD)) for _ in range(2)))
        assert k.sw_fluxes_daylit(to(cols["plev"]), to(cols["tlay"]), gc, True, to(cols["mu0"]), to(cols["alb_dir"]),
                                  to(cols["alb_dif"]), fl, toa_scale=to(cols["scale"])) == ""
        assert np.array_equal(back(w), wide)
        gcols, _, _ = take_columns(dense, cloud, None, day)
        packed = existing_call(pkg, k, gcols, None, None, to, "clear sky, no flux_dir", True)
        for a, p in zip((back(fl.flux_up), back(fl.flux_dn)), packed):
            want = np.zeros_like(a)
            want[:, day] = p
            assert np.array_equal(a, want)


def test_graph_capture(pkg, gpu, sw):
    """After one warm-up call on the stream, sw_fluxes_daylit with a list made beforehand is captured and replayed once: the
    eager bits.  (The selection synchronises and stays outside the capture.)"""
    import torch
    k, t = sw, T(gpu)
    nlay = 60
    cols, cloud, mask = daylit_case(k, 3, NCOL, nlay)
    ref = daylit_call(pkg, k, cols, cloud, mask, t, "both skies", True)
    index, nday = pkg.daylit_columns(t(cols["mu0"]))
    gc = helpers.product_gas_concs(pkg, cols, t, swt.SW_NAMES)
    part = swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), t)
    args = (t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]), t(cols["alb_dif"]))
    kw = dict(particles=part, delta_scale=True, toa_scale=t(cols["scale"]), cloud_mask=t(mask.view(np.int64)), day_index=index)
    outs = [t(np.full((nlay + 1, NCOL), GUARD)) for _ in range(6)]
    fl, fc = pkg.FluxesBroadband(*outs[:3]), pkg.FluxesBroadband(*outs[3:])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert k.sw_fluxes_daylit(*args, fl, fluxes_clear=fc, **kw) == ""      # warm-up: the stream's block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.sw_fluxes_daylit(*args, fl, fluxes_clear=fc, **kw) == ""
    for a in outs:
        a.fill_(GUARD)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, ref):
        assert np.array_equal(a.cpu().numpy(), b)
    del graph
    pkg.release_scratch(0)
