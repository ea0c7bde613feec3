"""The single-precision fused calls on the GPU: lw_fluxes, lw_fluxes_allsky (plain and McICA), lw_fluxes_clear_allsky,
sw_fluxes_allsky (plain and McICA) and sw_fluxes_clear_allsky on float32 arrays.

Longwave: equalities, no tolerance.  The fused call runs the single-precision gas optics and the single-precision
register-resident solver of the composition gas_optics -> OpticalProps1scl.increment(particles, band2gpt[, cloud_mask]) ->
rte_lw, and rte_lw_allsky_f32_kernel spells the increment's operations one by one where it consumes tau, so every flux is
the composition's, bit for bit.  The composition's parts are each tied to the fp64 oracle (test_gpu_lw_f32.py,
test_gpu_allsky.py::test_increment_and_delta_scale, test_gpu_gas_f32.py).  One case per file is also held to
ah.oracle_lw_allsky on the float32-rounded inputs at 1/20 of the smallest cloud signal.

Shortwave: as in fp64 the fused call forms ssa in another order than the composition, so F (fused float32) and C (composed
float32: gas_optics -> delta_scale of a copy -> increment -> rte_sw) are both measured against R, the fp64 fused call on the
float32-rounded inputs (held to the oracle at 1e-8 W m-2 by test_gpu_allsky.py).  With e(X) the per-column maximum over
levels and fluxes of |X - R|, over the columns of the 130-column cases pooled per layer count: max e(F) <= 2 max e(C) and
the 99th percentile of e(F) <= 2 x that of e(C).

Measured on an MI355X, next to the bars (which come from the issue, not from these figures):
  longwave: every equality holds; 7.0e-4 (fsck) and 5.3e-4 W m-2 (rrtmgp) from the fp64 oracle, bars 1.87 and 1.60;
  shortwave, W m-2, max e(F) / max e(C) / p99 e(F) / p99 e(C): 60 layers 0.1263 / 0.1263 / 0.01915 / 0.01915; 37 layers
  0.1114 / 0.1114 / 0.02446 / 0.02446; 61 layers 0.1698 / 0.1698 / 0.09176 / 0.09176; 137 layers 0.07084 / 0.07084 / 0.04644 /
  0.04644 -- both ratios 1.00 at every layer count: F and C hold the same bits in all but 3 of 304 590 flux values;
  extreme particles: tau_p = 0 and 1e-12 0.04 - 0.20 W m-2 from the fp64 call, tau_p = 1e4 with ssa_p = 1 966 - 972 W m-2 (the
  k floor of the single-precision solvers; finite, not barred)."""
import json

import numpy as np
import pytest

import allsky_helpers as ah
import helpers
import mcica_helpers as mh
from helpers import SW_NAMES, r32
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
F4 = np.float32


@pytest.fixture(autouse=True)
def default_options(pkg):
    def reset():
        pkg.reset_solver_options()
        for n, v in (("lw_tail_split", 1), ("sw_tail_split", 1), ("sw_solver", 0)):
            pkg.set_solver_option(n, v)
        pkg.set_arithmetic(pkg.FAST)
    reset()
    yield
    reset()


@pytest.fixture(scope="module")
def models(pkg, gpu, oracle_mod):
    from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP), ("sw_wide", SW_WIDE)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = (k, oracle_mod.CkdModel(path))
    return out


def T(gpu, dtype=F4):
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)


def H(dtype=F4):
    return lambda a: np.ascontiguousarray(a, dtype=dtype)


def back(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def to_mask(mask, to):
    """A uint64 mask in the memory space of `to`'s arrays (device: the int64 tensor with the same bits)."""
    if mask is None:
        return None
    probe = to(np.zeros(1))
    if hasattr(probe, "cpu"):
        import torch
        return torch.from_numpy(np.ascontiguousarray(mask).view(np.int64)).to(probe.device)
    return np.ascontiguousarray(mask)


def particles(pkg, cloud, to, one_stream=False):
    op = pkg.OpticalProps1scl() if one_stream else pkg.OpticalProps2str()
    op.tau = to(cloud["tau"].copy())
    if not one_stream:
        op.ssa, op.g = to(cloud["ssa"].copy()), to(cloud["g"].copy())
    return op


def unchanged(part, cloud, one_stream=False):
    """The caller's band planes hold what they were given (float32-rounded), NaN included."""
    ok = np.array_equal(back(part.tau), cloud["tau"].astype(F4), equal_nan=True)
    if not one_stream:
        ok = ok and np.array_equal(back(part.ssa), cloud["ssa"].astype(F4), equal_nan=True)
        ok = ok and np.array_equal(back(part.g), cloud["g"].astype(F4), equal_nan=True)
    return ok


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ------------------------------------------------------------------------------------------------
# longwave
# ------------------------------------------------------------------------------------------------
def lw_case(k, ncol, nlay, c0=None):
    c0 = 7 * ncol + nlay if c0 is None else c0
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
    rng = np.random.default_rng(ncol + nlay)
    cols["inc_flux"] = rng.uniform(0.0, 2.0, (k.get_ngpt(), ncol))
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1)
    mask = mh.sample(synthetic.cloud_fraction(c0, ncol, nlay), k.get_ngpt(), mh.MAX_RAN, None, 99, c0)
    return cols, cloud, mask


def lw_fused(pkg, k, cols, cloud, to, one_stream=False, nmus=1, inc=False, top_at_1=True, mask=None, clear=False, dtype=F4):
    """lw_fluxes_allsky (cloud None: lw_fluxes; clear: lw_fluxes_clear_allsky, which returns all-sky + clear-sky fluxes)."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    new = lambda: pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    fl, fc = new(), new()
    args = (to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1, to(cols["emis"]))
    kw = dict(n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None)
    if cloud is None:
        assert k.lw_fluxes(*args, fl, **kw) == ""
    else:
        part = particles(pkg, cloud, to, one_stream)
        if clear:
            assert k.lw_fluxes_clear_allsky(*args, part, fl, fc, cloud_mask=to_mask(mask, to), **kw) == ""
        else:
            assert k.lw_fluxes_allsky(*args, part, fl, cloud_mask=to_mask(mask, to), **kw) == ""
        assert unchanged(part, cloud, one_stream) if dtype == F4 else True   # the caller's arrays are never written
    out = [back(fl.flux_up), back(fl.flux_dn)] + ([back(fc.flux_up), back(fc.flux_dn)] if clear else [])
    assert all(a.dtype == dtype for a in out)
    return out


def lw_composed(pkg, k, cols, cloud, to, one_stream=False, nmus=1, inc=False, top_at_1=True, mask=None):
    """gas_optics (float32) -> OpticalProps1scl.increment(particles, band2gpt[, cloud_mask]) -> rte_lw (float32)."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    like = to(np.zeros(1))
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=like)
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=like, separate_levels=True)
    assert k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), gc, op, src, tlev=to(cols["tlev"])) == ""
    if cloud is not None:
        assert op.increment(particles(pkg, cloud, to, one_stream), band2gpt=k.get_band2gpt(), cloud_mask=to_mask(mask, to)) == ""
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -2.0)), to(np.full((nlay + 1, ncol), -2.0)))
    assert pkg.rte_lw(op, top_at_1, src, to(cols["emis"]), fl, n_gauss_angles=nmus,
                      inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    out = [back(fl.flux_up), back(fl.flux_dn)]
    assert all(a.dtype == F4 for a in out)
    return out


def lw_variants(full):
    """(one_stream, nmus, inc, masked): the full cross, or a walk in which every factor flips at least once."""
    if full:
        return [(o, n, i, m) for o in (False, True) for n in (1, 3) for i in (False, True) for m in (False, True)]
    return [(False, 1, False, False), (True, 3, True, True), (False, 3, False, True), (True, 1, True, False)]


@pytest.mark.parametrize("ncol", [1, 33, 130])
@pytest.mark.parametrize("nlay", [60, 37, 137])
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_fused_equals_composed(pkg, gpu, models, which, nlay, ncol):
    """float32 device tensors: lw_fluxes_allsky equals gas_optics + increment + rte_lw bit for bit -- two- and one-stream
    particles, 1 and 3 angles, with and without inc_flux, with and without a mask (the full cross at rrtmgp / 60 / 130); at
    60 and 137 layers also bottom-up; and lw_fluxes equals gas_optics + rte_lw."""
    k = models[which][0]
    t = T(gpu)
    cols, cloud, mask = lw_case(k, ncol, nlay)
    full = (which, nlay, ncol) == ("rrtmgp", 60, 130)
    for top_at_1 in ((True, False) if nlay in (60, 137) else (True,)):
        for one_stream, nmus, inc, masked in lw_variants(full):
            m_ = mask if masked else None
            f = lw_fused(pkg, k, cols, cloud, t, one_stream, nmus, inc, top_at_1, m_)
            c = lw_composed(pkg, k, cols, cloud, t, one_stream, nmus, inc, top_at_1, m_)
            what = (which, nlay, ncol, top_at_1, one_stream, nmus, inc, masked)
            assert all(np.all(np.isfinite(a)) for a in f), what
            assert same(f, c), what
        for nmus, inc in ((1, False), (3, True)):
            assert same(lw_fused(pkg, k, cols, None, t, nmus=nmus, inc=inc, top_at_1=top_at_1),
                        lw_composed(pkg, k, cols, None, t, nmus=nmus, inc=inc, top_at_1=top_at_1)), (which, nlay, ncol, top_at_1, nmus, inc)


@pytest.mark.parametrize("which,nlay", [("rrtmgp", 60), ("fsck", 37), ("fsck", 60)])
def test_longwave_tail_split_and_lane_offsets(pkg, gpu, models, monkeypatch, which, nlay):
    """130 columns: "lw_tail_split" 0 and 1 give the same bits, and both equal the composition; at 60 layers the 64-bit
    lane-offset form of the kernel (ECCKD_LW_NO_OFF32) gives the bits of the 32-bit form."""
    k = models[which][0]
    t = T(gpu)
    cols, cloud, mask = lw_case(k, 130, nlay)
    ref = lw_composed(pkg, k, cols, cloud, t, False, 3, True, True, mask)
    for split in (0, 1):
        pkg.set_solver_option("lw_tail_split", split)
        assert same(lw_fused(pkg, k, cols, cloud, t, False, 3, True, True, mask), ref), split
        assert same(lw_fused(pkg, k, cols, cloud, t, True, 1, False, True, None),
                    lw_composed(pkg, k, cols, cloud, t, True, 1, False, True, None)), split
    if nlay == 60:
        monkeypatch.setenv("ECCKD_LW_NO_OFF32", "1")
        for top_at_1 in (True, False):
            for one_stream, nmus, inc, masked in lw_variants(False):
                m_ = mask if masked else None
                assert same(lw_fused(pkg, k, cols, cloud, t, one_stream, nmus, inc, top_at_1, m_),
                            lw_composed(pkg, k, cols, cloud, t, one_stream, nmus, inc, top_at_1, m_)), (top_at_1, one_stream, nmus, inc, masked)
        monkeypatch.delenv("ECCKD_LW_NO_OFF32")
        assert same(lw_fused(pkg, k, cols, cloud, t, False, 3, True, True, mask), ref)


@pytest.mark.parametrize("which,ncol,nlay", [("fsck", 130, 60), ("rrtmgp", 33, 37), ("rrtmgp", 130, 137)])
def test_longwave_zero_particles_clear_columns_both_skies(pkg, gpu, models, which, ncol, nlay):
    """tau_p = 0 gives lw_fluxes (float32) bit for bit; the clear columns of a cloudy call equal the clear-sky call's columns
    and the cloudy ones differ; lw_fluxes_clear_allsky gives both results, masked and unmasked."""
    k = models[which][0]
    t = T(gpu)
    cols, cloud, mask = lw_case(k, ncol, nlay, c0=23)
    zero = dict(cloud, tau=np.zeros_like(cloud["tau"]))
    for nmus, inc in ((1, False), (3, True)):
        clear = lw_fused(pkg, k, cols, None, t, nmus=nmus, inc=inc)
        for one_stream in (False, True):
            assert same(lw_fused(pkg, k, cols, zero, t, one_stream, nmus, inc), clear)
            f = lw_fused(pkg, k, cols, cloud, t, one_stream, nmus, inc)
            keep = ~cloud["cloudy"]
            assert keep.any() and cloud["cloudy"].any()
            assert all(np.array_equal(a[:, keep], b[:, keep]) for a, b in zip(f, clear))
            assert np.all(np.abs(f[0].astype(np.float64) - clear[0]).max(axis=0)[cloud["cloudy"]] > 0)
            for m_ in (None, mask):
                both = lw_fused(pkg, k, cols, cloud, t, one_stream, nmus, inc, mask=m_, clear=True)
                assert same(both[:2], lw_fused(pkg, k, cols, cloud, t, one_stream, nmus, inc, mask=m_)) and same(both[2:], clear)


@pytest.mark.parametrize("which,ncol,nlay", [("fsck", 33, 60), ("rrtmgp", 130, 37), ("fsck", 33, 137)])
def test_longwave_host_arrays_equal_device_arrays(pkg, gpu, models, which, ncol, nlay):
    k = models[which][0]
    cols, cloud, mask = lw_case(k, ncol, nlay, c0=11)
    for one_stream, nmus, inc, masked in lw_variants(False):
        m_ = mask if masked else None
        assert same(lw_fused(pkg, k, cols, cloud, T(gpu), one_stream, nmus, inc, mask=m_),
                    lw_fused(pkg, k, cols, cloud, H(), one_stream, nmus, inc, mask=m_)), (one_stream, nmus, inc, masked)
    assert same(lw_fused(pkg, k, cols, None, T(gpu), nmus=3, inc=True), lw_fused(pkg, k, cols, None, H(), nmus=3, inc=True))
    assert same(lw_fused(pkg, k, cols, cloud, T(gpu), mask=mask, clear=True), lw_fused(pkg, k, cols, cloud, H(), mask=mask, clear=True))


def _on_block(pkg, gpu, stream, size, body):
    """Runs body() on `stream` with a caller-owned scratch block of `size` bytes filled with 0xFF (stale data would show)."""
    import torch
    buf = torch.full((size,), 0xFF, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    pkg.set_stream_scratch(buf, stream=stream)
    try:
        with torch.cuda.stream(stream):
            out = body()
        torch.cuda.synchronize()
    finally:
        pkg.set_stream_scratch(None, stream=stream)
    del buf
    return out


def test_longwave_caller_owned_scratch_and_capture(pkg, gpu, models):
    """A caller-owned block of exactly ecckd_lw_fluxes_f32_scratch_bytes gives the eager bits, one byte less is refused with the
    outputs untouched; the call captured on that block and replayed once gives the eager bits."""
    import torch
    k = models["rrtmgp"][0]
    ncol, nlay = 130, 137
    t = T(gpu)
    cols, cloud, mask = lw_case(k, ncol, nlay, c0=3)
    ref = lw_fused(pkg, k, cols, cloud, t, False, 3, True, mask=mask)
    need = int(pkg.lib().ecckd_lw_fluxes_f32_scratch_bytes(k._need(), ncol, nlay))
    stream = torch.cuda.Stream()
    assert same(_on_block(pkg, gpu, stream, need, lambda: lw_fused(pkg, k, cols, cloud, t, False, 3, True, mask=mask)), ref)
    gc = helpers.product_gas_concs(pkg, cols, t)
    fl = pkg.FluxesBroadband(t(np.full((nlay + 1, ncol), -5.0)), t(np.full((nlay + 1, ncol), -5.0)))
    part, d_mask = particles(pkg, cloud, t), to_mask(mask, t)
    args = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(cols["emis"]), part, fl)
    kw = dict(n_gauss_angles=3, inc_flux=t(cols["inc_flux"]), cloud_mask=d_mask)
    msg = _on_block(pkg, gpu, stream, need - 1, lambda: k.lw_fluxes_allsky(*args, **kw))
    assert "too small" in msg and np.all(back(fl.flux_up) == -5.0) and np.all(back(fl.flux_dn) == -5.0), msg
    buf = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    pkg.set_stream_scratch(buf, stream=stream)
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            assert k.lw_fluxes_allsky(*args, **kw) == ""
        torch.cuda.synchronize()
        fl.flux_up.zero_(); fl.flux_dn.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same([back(fl.flux_up), back(fl.flux_dn)], ref)
        del graph
    finally:
        pkg.set_stream_scratch(None, stream=stream)
    del buf
    pkg.release_scratch(0)


@pytest.mark.parametrize("which,nlay", [("fsck", 60), ("rrtmgp", 137)])
def test_longwave_nan_stays_in_its_column(pkg, gpu, models, which, nlay):
    """A NaN in one column's tau_p makes that column NaN and leaves every other column's bits as they were."""
    k = models[which][0]
    t = T(gpu)
    ncol = 33
    cols, cloud, mask = lw_case(k, ncol, nlay, c0=5)
    ref = lw_fused(pkg, k, cols, cloud, t, nmus=3, inc=True)
    bad = dict(cloud, tau=cloud["tau"].copy())
    col = 17
    bad["tau"][:, nlay // 2, col] = np.nan
    out = lw_fused(pkg, k, cols, bad, t, nmus=3, inc=True)
    others = np.arange(ncol) != col
    assert all(np.array_equal(a[:, others], b[:, others]) for a, b in zip(out, ref))
    assert np.isnan(out[0][:, col]).any() and np.isnan(out[1][:, col]).any()


def test_longwave_against_the_oracle(pkg, gpu, oracle_mod, models):
    """So that two equal wrong answers cannot pass: the fused float32 call against ah.oracle_lw_allsky on the float32-rounded
    inputs, below 1/20 of the smallest all-sky-minus-clear-sky signal of a cloudy column (the condition of the fp64 tests).
    Columns 9 .. 138 (78 of them cloudy): the signal, computed on the CPU beforehand, is 37.4 W m-2 (fsck) and 32.1 W m-2
    (rrtmgp), so the bars are 1.87 and 1.60 W m-2 -- four orders above the 1e-4 W m-2 floor of helpers.lw_f32_bar, which the
    parts of the composition are held to; the equalities above carry those bars over, this one only guards against two
    equal wrong answers."""
    ncol, nlay, c0 = 130, 60, 9
    for which in ("fsck", "rrtmgp"):
        k, m = models[which]
        cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
        cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
        cols["emis"] = np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1)
        rc = {n: (r32(v) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for n, v in cols.items()}
        rcl = {n: (r32(v) if v.dtype == np.float64 else v) for n, v in cloud.items()}
        items = helpers.oracle_gas_items(rc)
        ref = ah.oracle_lw_allsky(oracle_mod, m, rc, items, rcl)
        clear = ah.oracle_lw_allsky(oracle_mod, m, rc, items, None)
        bar = ah.smallest_cloud_signal(ref, clear, cloud["cloudy"]) / 20
        out = lw_fused(pkg, k, cols, cloud, T(gpu))
        err = max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(out, ref))
        print("longwave f32 %s: %.3e W m-2 from the oracle (bar %.3e = smallest cloud signal / 20)" % (which, err, bar))
        assert bar >= 1e-4 and err < bar


# ------------------------------------------------------------------------------------------------
# shortwave
# ------------------------------------------------------------------------------------------------
def sw_case(k, ncol, nlay, c0=None):
    c0 = 7 * ncol + nlay if c0 is None else c0
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    rng = np.random.default_rng(ncol + nlay)
    nb = k.get_nband()
    cols["alb_dir"], cols["alb_dif"] = rng.uniform(0.02, 0.6, (ncol, nb)), rng.uniform(0.02, 0.6, (ncol, nb))
    cols["scale"] = rng.uniform(0.97, 1.03, ncol)
    cloud = synthetic.clouds(c0, ncol, nlay, nb)
    mask = mh.sample(synthetic.cloud_fraction(c0, ncol, nlay), k.get_ngpt(), mh.MAX_RAN, None, 5, c0)
    # what a float32 host holds: every array rounded once, so that the fp64 reference sees the same numbers
    cols = {n: (r32(v) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for n, v in cols.items()}
    cloud = {n: (r32(v) if v.dtype == np.float64 else v) for n, v in cloud.items()}
    return cols, cloud, mask


def sw_fused(pkg, k, cols, cloud, to, delta=True, top_at_1=True, scale=False, with_dir=True, mask=None, clear=False):
    """sw_fluxes_allsky (cloud None: sw_fluxes; clear: sw_fluxes_clear_allsky, all-sky fluxes then clear-sky fluxes) in the
    precision of `to`."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to, SW_NAMES)
    new = lambda: pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), -1.0)) for _ in range(3 if with_dir else 2)))
    fl, fc = new(), new()
    args = (to(cols["plev"]), to(cols["tlay"]), gc, top_at_1, to(cols["mu0"]), to(cols["alb_dir"]), to(cols["alb_dif"]))
    sc = to(cols["scale"]) if scale else None
    if cloud is None:
        assert k.sw_fluxes(*args, fl, toa_scale=sc) == ""
    else:
        part = particles(pkg, cloud, to)
        if clear:
            assert k.sw_fluxes_clear_allsky(*args, part, fl, fc, delta_scale=delta, toa_scale=sc, cloud_mask=to_mask(mask, to)) == ""
        else:
            assert k.sw_fluxes_allsky(*args, part, fl, delta_scale=delta, toa_scale=sc, cloud_mask=to_mask(mask, to)) == ""
        for a, n in ((part.tau, "tau"), (part.ssa, "ssa"), (part.g, "g")):   # the caller's arrays are never written
            assert np.array_equal(back(a), cloud[n].astype(back(a).dtype), equal_nan=True)
    both = [fl, fc] if clear else [fl]
    return [back(a) for f in both for a in ([f.flux_up, f.flux_dn] + ([f.flux_dn_dir] if with_dir else []))]


def sw_composed(pkg, k, cols, cloud, to, delta=True, top_at_1=True, scale=False, mask=None):
    """gas_optics -> delta_scale of a copy -> increment(particles, band2gpt[, cloud_mask]) -> rte_sw, float32."""
    nlay, ncol = cols["tlay"].shape
    ng = k.get_ngpt()
    gc = helpers.product_gas_concs(pkg, cols, to, SW_NAMES)
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=to(np.zeros(1)))
    toa = to(np.zeros((ng, ncol)))
    assert k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), gc, op, toa) == ""
    part = particles(pkg, cloud, to)
    if delta:
        assert part.delta_scale() == ""
    assert op.increment(part, band2gpt=k.get_band2gpt(), cloud_mask=to_mask(mask, to)) == ""
    if scale:
        toa = toa * to(cols["scale"])[None, :]
    fl = pkg.FluxesBroadband(*(to(np.zeros((nlay + 1, ncol))) for _ in range(3)))
    assert pkg.rte_sw(op, top_at_1, to(cols["mu0"]), toa, to(cols["alb_dir"]), to(cols["alb_dif"]), fl) == ""
    return [back(fl.flux_up), back(fl.flux_dn), back(fl.flux_dn_dir)]


def column_error(x, ref):
    """e(X): per column, the largest |X - R| over levels and over the three fluxes."""
    return np.max([np.abs(a.astype(np.float64) - b).max(axis=0) for a, b in zip(x, ref)], axis=0)


# (delta_scale, toa_scale, mask, "sw_tail_split", "sw_solver", top_at_1) at 130 columns, pooled per layer count
SW_POOL = {60: [(1, 0, 0, 1, 0, True), (0, 1, 1, 1, 0, True), (1, 1, 1, 0, 0, True), (1, 0, 0, 1, 1, True), (0, 1, 1, 1, 0, False)],
           37: [(1, 0, 0, 1, 0, True), (0, 1, 1, 0, 0, True)],
           61: [(1, 1, 0, 1, 0, True), (0, 0, 1, 0, 0, True)],
           137: [(1, 0, 1, 1, 0, True), (0, 1, 0, 0, 0, True)]}


@pytest.mark.parametrize("nlay", [60, 37, 61, 137])
def test_shortwave_fused_is_as_close_as_the_composition(pkg, gpu, models, nlay):
    """F = the fused float32 call, C = the float32 composition, R = the fp64 fused call on the same (float32-rounded) inputs;
    e(X) = per-column max over levels and fluxes of |X - R|.  Over the columns of the 130-column cases of the layer count
    (delta_scale 0 and 1, with and without toa_scale and a mask, "sw_tail_split" 0 and 1, at 60 layers "sw_solver" = 1 and
    once top_at_1 = False -- the solver's orientation alone, both sides on the same arrays): max e(F) <= 2 max e(C) and the
    99th percentile of e(F) <= 2 x that of e(C).  The factor 2: two float evaluations of one quantity in another operation
    order have errors of the same size that are not the same numbers, and a maximum over a few hundred columns moves by
    that much.  max e(C) is printed next to the clear-sky single-precision bars (0.5 W m-2 worst column, 0.05 at the 99th
    percentile: test_single_precision_sw_path) for information.
    Measured on an MI355X (W m-2; max e(F), max e(C), p99 e(F), p99 e(C)): 60 layers 0.1263, 0.1263, 0.01915, 0.01915;
    37 layers 0.1114, 0.1114, 0.02446, 0.02446; 61 layers 0.1698, 0.1698, 0.09176, 0.09176; 137 layers 0.07084, 0.07084,
    0.04644, 0.04644 (profiles/allsky_f32.json, "sw_accuracy")."""
    k = models["sw_wide"][0]
    t32, t64 = T(gpu), T(gpu, np.float64)
    cols, cloud, mask = sw_case(k, 130, nlay)
    ef, ec = [], []
    for delta, scale, masked, split, solver, top_at_1 in SW_POOL[nlay]:
        pkg.set_solver_option("sw_tail_split", split)
        pkg.set_solver_option("sw_solver", solver)
        m_ = mask if masked else None
        f = sw_fused(pkg, k, cols, cloud, t32, bool(delta), top_at_1, bool(scale), mask=m_)
        c = sw_composed(pkg, k, cols, cloud, t32, bool(delta), top_at_1, bool(scale), mask=m_)
        r = sw_fused(pkg, k, cols, cloud, t64, bool(delta), top_at_1, bool(scale), mask=m_)
        assert all(a.dtype == F4 for a in f) and all(a.dtype == np.float64 for a in r)
        assert all(np.all(np.isfinite(a)) for a in f + c + r), (nlay, delta, scale, masked, split, solver, top_at_1)
        ef.append(column_error(f, r)); ec.append(column_error(c, r))
        ndiff = sum(int(np.count_nonzero(a != b)) for a, b in zip(f, c))
        print("SWF32 nlay %3d delta %d scale %d mask %d split %d solver %d top %d: max e(F) %.3e  max e(C) %.3e, F != C in %d of %d values"
              % (nlay, delta, scale, masked, split, solver, top_at_1, ef[-1].max(), ec[-1].max(), ndiff, 3 * f[0].size))
        two = sw_fused(pkg, k, cols, cloud, t32, bool(delta), top_at_1, bool(scale), with_dir=False, mask=m_)
        assert same(two, f[:2])   # without flux_dir: the same flux_up / flux_dn
    ef, ec = np.concatenate(ef), np.concatenate(ec)
    fig = dict(nlay=nlay, columns=int(ef.size), max_eF=float(ef.max()), max_eC=float(ec.max()),
               p99_eF=float(np.percentile(ef, 99)), p99_eC=float(np.percentile(ec, 99)))
    print("SWF32 pooled " + json.dumps(fig))
    print("SWF32 nlay %d: max e(C) %.3e W m-2 (clear-sky single-precision bars: 0.5 worst column, 0.05 at the 99th percentile)"
          % (nlay, fig["max_eC"]))
    assert fig["max_eF"] <= 2 * fig["max_eC"] and fig["p99_eF"] <= 2 * fig["p99_eC"], fig


@pytest.mark.parametrize("ncol,nlay,solver", [(1, 60, 0), (65, 37, 0), (65, 61, 0), (1, 137, 0), (65, 60, 1)])
def test_shortwave_equalities(pkg, gpu, models, ncol, nlay, solver):
    """No tolerance: host arrays equal device arrays; the clear-sky output of sw_fluxes_clear_allsky equals sw_fluxes
    (float32) and its all-sky output sw_fluxes_allsky (float32), masked and unmasked; a mask of all ones equals the
    unmasked call; without flux_dir the same flux_up / flux_dn."""
    k = models["sw_wide"][0]
    pkg.set_solver_option("sw_solver", solver)
    t = T(gpu)
    cols, cloud, mask = sw_case(k, ncol, nlay)
    ones = np.full_like(mask, 2 ** k.get_ngpt() - 1)
    for delta, scale in ((True, False), (False, True)):
        f = sw_fused(pkg, k, cols, cloud, t, delta, scale=scale)
        assert all(np.all(np.isfinite(a)) for a in f)
        assert same(sw_fused(pkg, k, cols, cloud, H(), delta, scale=scale), f)
        assert same(sw_fused(pkg, k, cols, cloud, t, delta, scale=scale, mask=ones), f)
        assert same(sw_fused(pkg, k, cols, cloud, t, delta, scale=scale, with_dir=False), f[:2])
        fm = sw_fused(pkg, k, cols, cloud, t, delta, scale=scale, mask=mask)
        assert same(sw_fused(pkg, k, cols, cloud, H(), delta, scale=scale, mask=mask), fm)
        clear = sw_fused(pkg, k, cols, None, t, scale=scale)
        for m_, want in ((None, f), (mask, fm)):
            both = sw_fused(pkg, k, cols, cloud, t, delta, scale=scale, mask=m_, clear=True)
            assert same(both[:3], want) and same(both[3:], clear), (delta, scale, m_ is not None)


@pytest.mark.parametrize("nlay,delta", [(60, True), (137, False)])
def test_shortwave_caller_owned_scratch_and_capture(pkg, gpu, models, nlay, delta):
    """A caller-owned block of exactly ecckd_sw_fluxes_allsky_f32_scratch_bytes gives the eager bits and one byte less is
    refused with the outputs untouched; the call captured on that block and replayed once gives the eager bits."""
    import torch
    k = models["sw_wide"][0]
    ncol = 130
    t = T(gpu)
    cols, cloud, mask = sw_case(k, ncol, nlay, c0=3)
    ref = sw_fused(pkg, k, cols, cloud, t, delta, scale=True, mask=mask)
    need = int(pkg.lib().ecckd_sw_fluxes_allsky_f32_scratch_bytes(k._need(), ncol, nlay, int(delta)))
    stream = torch.cuda.Stream()
    assert same(_on_block(pkg, gpu, stream, need, lambda: sw_fused(pkg, k, cols, cloud, t, delta, scale=True, mask=mask)), ref)
    gc = helpers.product_gas_concs(pkg, cols, t, SW_NAMES)
    fl = pkg.FluxesBroadband(*(t(np.full((nlay + 1, ncol), -5.0)) for _ in range(3)))
    args = (t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]), t(cols["alb_dif"]), particles(pkg, cloud, t), fl)
    kw = dict(delta_scale=delta, toa_scale=t(cols["scale"]), cloud_mask=to_mask(mask, t))
    msg = _on_block(pkg, gpu, stream, need - 1, lambda: k.sw_fluxes_allsky(*args, **kw))
    assert "too small" in msg and all(np.all(back(a) == -5.0) for a in (fl.flux_up, fl.flux_dn, fl.flux_dn_dir)), msg
    buf = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    pkg.set_stream_scratch(buf, stream=stream)
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            assert k.sw_fluxes_allsky(*args, **kw) == ""
        torch.cuda.synchronize()
        for a in (fl.flux_up, fl.flux_dn, fl.flux_dn_dir):
            a.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same([back(fl.flux_up), back(fl.flux_dn), back(fl.flux_dn_dir)], ref)
        del graph
    finally:
        pkg.set_stream_scratch(None, stream=stream)
    del buf
    pkg.release_scratch(0)


@pytest.mark.parametrize("nlay", [60, 61])
def test_shortwave_nan_stays_in_its_column_and_extreme_particles(pkg, gpu, models, nlay):
    """A NaN in one column's planes stays in that column (the other columns keep their bits).  Extreme particles -- tau_p of
    0, 1e-12 and 1e4 with ssa_p = 1 and g_p = 0 -- give finite fluxes; their distance to the fp64 call is printed and not
    barred: a conservative thick float layer sits on the k floor by design."""
    k = models["sw_wide"][0]
    t, t64 = T(gpu), T(gpu, np.float64)
    ncol = 65
    cols, cloud, mask = sw_case(k, ncol, nlay, c0=5)
    ref = sw_fused(pkg, k, cols, cloud, t, True, scale=True)
    bad = {n: v.copy() for n, v in cloud.items()}
    col = 40
    bad["tau"][:, nlay // 2, col] = np.nan
    bad["g"][:, nlay // 3, col] = np.nan
    out = sw_fused(pkg, k, cols, bad, t, True, scale=True)
    others = np.arange(ncol) != col
    assert all(np.array_equal(a[:, others], b[:, others]) for a, b in zip(out, ref))
    assert np.isnan(out[0][:, col]).any() and np.isnan(out[1][:, col]).any()
    for tau_p in (0.0, 1e-12, 1e4):
        ext = dict(tau=r32(np.full_like(cloud["tau"], tau_p)), ssa=np.ones_like(cloud["ssa"]), g=np.zeros_like(cloud["g"]))
        for delta in (False, True):
            f = sw_fused(pkg, k, cols, ext, t, delta)
            assert all(np.all(np.isfinite(a)) for a in f), (tau_p, delta)
            r = sw_fused(pkg, k, cols, ext, t64, delta)
            print("SWF32 extreme nlay %d tau_p %g delta %d: %.3e W m-2 from the fp64 call" % (nlay, tau_p, delta, column_error(f, r).max()))
