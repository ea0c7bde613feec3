"""Host arrays give the device arrays' results, bit for bit, at every entry point of the C ABI that takes a `memspace`.

A table of calls, each run once on device tensors (ECCKD_DEVICE) and once on numpy arrays (ECCKD_HOST, staged by the
library); every output is compared bit for bit.  The calls on a model that carry such a test in their own files
(ecckd_gas_optics_lw / _f32, ecckd_lw_fluxes_jac, ecckd_lw_fluxes_allsky, the two *_clear_allsky calls) are not
repeated here.  ecckd_planck_sources, ecckd_gas_optics_lw_tau and ecckd_rte_lw_fused take ECCKD_DEVICE only and
ecckd_sum_broadband sums host arrays on the host: none of them stages anything, so none has a row.

Shapes: ncol 1 and 33 (33 doubles is one element past a 256-byte room of the staging arena: a miscounted room
overlaps its neighbour), longwave nlay 60 / 37 / 97 (fused 60-layer kernels, general route, scratch ring beyond 96
layers), shortwave nlay 60 / 61 (layer-systolic and two-pass solver).  Gas descriptions mix a scalar, per-column,
per-layer and full arrays.  Two more cases: the arenas growing and being reused (ncol 33, 130, 33 in one process) and
ECCKD_MIXED chains through the raw ABI (host inputs, device optical properties, host fluxes).
"""
import ctypes as C

import numpy as np
import pytest

import helpers
import mcica_helpers as mh
from conftest import LW_FSCK, SW_WIDE
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
NCOLS = (1, 33)
LW_NLAYS = (60, 37, 97)
SW_NLAYS = (60, 61)
NG = 7                                                      # g-points of the stand-alone solver rows ...
B2G = np.array([[1, 3], [4, 7]], dtype=np.int32)            # ... in two bands
MIXED = 2                                                   # ECCKD_MIXED


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.set_arithmetic(pkg.FAST)


@pytest.fixture(scope="module")
def models(pkg, gpu):
    out = {}
    for name, path in (("lw", LW_FSCK), ("sw", SW_WIDE)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = k
    return out


class Space:
    """Where the arrays of one run live: `to` moves a numpy array there (always a fresh copy), `back` reads one."""

    def __init__(self, gpu=None):
        self.gpu = gpu
        self.code = 1 if gpu is not None else 0

    def to(self, a, dtype=None):
        if a is None:
            return None
        a = np.array(a, dtype=a.dtype if dtype is None else dtype, order="C", copy=True)
        if self.gpu is None:
            return a
        import torch
        return torch.from_numpy(a).to(self.gpu)

    def mask(self, m):
        if m is None:
            return None
        return m.copy() if self.gpu is None else self.to(m.view(np.int64))

    def back(self, a):
        if self.gpu is None:
            return a
        import torch
        torch.cuda.synchronize()
        return a.cpu().numpy()

    def ptr(self, a):
        if a is None:
            return None
        return C.c_void_p(a.ctypes.data if self.gpu is None else a.data_ptr())

    def stream(self):
        if self.gpu is None:
            return None
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def both(gpu, run):
    """run(space) -> list of numpy outputs, on device tensors and on host arrays: the two lists must hold the same bits."""
    d, h = run(Space(gpu)), run(Space())
    assert len(d) == len(h) and len(d) > 0
    for i, (a, b) in enumerate(zip(d, h)):
        assert a.dtype == b.dtype and a.shape == b.shape, i
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "output %d differs between host and device arrays" % i
    return d


def filled(sp, shape, dtype=np.float64, value=-7.0):
    return sp.to(np.full(shape, value, dtype=dtype))


# ------------------------------------------------------------------------------------------------
# stand-alone solvers on random optical properties
# ------------------------------------------------------------------------------------------------
def solver_case(ncol, nlay, seed):
    rng = np.random.default_rng(1000 * seed + 10 * ncol + nlay)
    s3 = (NG, nlay, ncol)
    c = dict(tau=rng.uniform(0, 2, s3) * rng.choice([1e-9, 1e-3, 1.0], size=s3), ssa=rng.uniform(0, 1, s3),
             g=rng.uniform(-0.3, 0.8, s3), lay=rng.uniform(1, 9, s3), sfc=rng.uniform(1, 9, (NG, ncol)),
             sfc_jac=rng.uniform(0.01, 0.1, (NG, ncol)), emis=rng.uniform(0.7, 1.0, (ncol, 2)),
             emis_g=rng.uniform(0.7, 1.0, (NG, ncol)), inc_flux=rng.uniform(0, 2, (NG, ncol)),
             mu0=rng.uniform(0.1, 1.0, ncol), toa=rng.uniform(1, 50, (NG, ncol)), adir=rng.uniform(0.05, 0.4, (ncol, 2)),
             adif=rng.uniform(0.05, 0.4, (ncol, 2)), adir_g=rng.uniform(0.05, 0.4, (NG, ncol)),
             adif_g=rng.uniform(0.05, 0.4, (NG, ncol)))
    lev = rng.uniform(1, 9, (NG, nlay + 1, ncol))
    c["inc"], c["dec"] = np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1])
    return c


def lw_objects(pkg, sp, c, dtype, two_stream=False):
    op = pkg.OpticalProps2str() if two_stream else pkg.OpticalProps1scl()
    op.tau, op.band2gpt = sp.to(c["tau"], dtype), B2G
    if two_stream:
        op.ssa, op.g = sp.to(c["ssa"], dtype), sp.to(c["g"], dtype)
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec = (sp.to(c[n], dtype) for n in ("lay", "inc", "dec"))
    src.sfc_source, src.sfc_source_jac = sp.to(c["sfc"], dtype), sp.to(c["sfc_jac"], dtype)
    return op, src


def run_rte_lw(pkg, c, dtype, inc, top_at_1, nmus, shared=False, byband=False, jac=False, two_stream=False):
    def run(sp):
        nlay, ncol = c["tau"].shape[1:]
        op, src = lw_objects(pkg, sp, c, dtype, two_stream)
        lev = (nlay + 1, ncol)
        if byband:
            fl = pkg.FluxesByband(filled(sp, (2,) + lev, dtype), filled(sp, (2,) + lev, dtype), flux_up=filled(sp, lev, dtype),
                                  flux_dn=filled(sp, lev, dtype))
        else:
            fl = pkg.FluxesBroadband(filled(sp, lev, dtype), filled(sp, lev, dtype))
        fj = filled(sp, lev) if jac else None
        assert pkg.rte_lw(op, top_at_1, src, sp.to(c["emis"], dtype), fl, n_gauss_angles=nmus, shared_levels=shared,
                          inc_flux=sp.to(c["inc_flux"], dtype) if inc else None, use_2stream=two_stream, flux_up_jac=fj) == ""
        out = [fl.flux_up, fl.flux_dn] + ([fl.bnd_flux_up, fl.bnd_flux_dn] if byband else []) + ([fj] if jac else [])
        return [sp.back(a) for a in out]
    return run


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlay", LW_NLAYS)
def test_rte_lw(pkg, gpu, ncol, nlay):
    """ecckd_rte_lw, _f32, _inc_flux, _inc_flux_f32, _shared_levels, _byband, _byband_f32, ecckd_rte_lw_jac and
    ecckd_rte_lw_2stream."""
    c = solver_case(ncol, nlay, 1)
    for dtype in (np.float64, np.float32):
        for inc in (False, True):
            out = both(gpu, run_rte_lw(pkg, c, dtype, inc, top_at_1=not inc, nmus=3 if inc else 1))
            assert np.all(np.isfinite(out[0])) and np.all(out[0] > 0)
        both(gpu, run_rte_lw(pkg, c, dtype, False, True, 2, byband=True))
    both(gpu, run_rte_lw(pkg, c, np.float64, False, True, 2, shared=True))
    both(gpu, run_rte_lw(pkg, c, np.float64, True, False, 2, jac=True))
    both(gpu, run_rte_lw(pkg, c, np.float64, True, True, 1, two_stream=True))
    both(gpu, run_rte_lw(pkg, c, np.float64, False, False, 1, two_stream=True))


def run_rte_sw(pkg, c, dtype, with_dir, top_at_1, byband=False):
    def run(sp):
        nlay, ncol = c["tau"].shape[1:]
        op = pkg.OpticalProps2str()
        op.tau, op.ssa, op.g, op.band2gpt = sp.to(c["tau"], dtype), sp.to(c["ssa"], dtype), sp.to(c["g"], dtype), B2G
        lev = (nlay + 1, ncol)
        n = 3 if with_dir else 2
        if byband:
            fl = pkg.FluxesByband(*([filled(sp, (2,) + lev, dtype) for _ in range(n)] + [None] * (3 - n)),
                                  *[filled(sp, lev, dtype) for _ in range(n)])
        else:
            fl = pkg.FluxesBroadband(*[filled(sp, lev, dtype) for _ in range(n)])
        assert pkg.rte_sw(op, top_at_1, sp.to(c["mu0"], dtype), sp.to(c["toa"], dtype), sp.to(c["adir"], dtype),
                          sp.to(c["adif"], dtype), fl) == ""
        out = [fl.flux_up, fl.flux_dn] + ([fl.flux_dn_dir] if with_dir else [])
        if byband:
            out += [fl.bnd_flux_up, fl.bnd_flux_dn] + ([fl.bnd_flux_dn_dir] if with_dir else [])
        return [sp.back(a) for a in out]
    return run


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlay", SW_NLAYS)
def test_rte_sw(pkg, gpu, ncol, nlay):
    """ecckd_rte_sw, _f32, _byband, _byband_f32; with and without flux_dir."""
    c = solver_case(ncol, nlay, 2)
    for dtype in (np.float64, np.float32):
        for with_dir in (True, False):
            out = both(gpu, run_rte_sw(pkg, c, dtype, with_dir, top_at_1=with_dir))
            assert np.all(np.isfinite(out[0]))
            both(gpu, run_rte_sw(pkg, c, dtype, with_dir, True, byband=True))


def run_gpt(pkg, which, c, top_at_1, optional):
    """The three spectral-output solvers through the raw ABI; `optional`: with inc_flux / inc_flux_dif (and flux_dir)."""
    def run(sp):
        L = pkg.lib()
        nlay, ncol = c["tau"].shape[1:]
        a = {n: sp.to(v) for n, v in c.items()}
        P = sp.ptr
        nf = (NG, nlay + 1, ncol)
        up, dn, dr = filled(sp, nf), filled(sp, nf), filled(sp, nf)
        head = (0, ncol, nlay, NG, int(top_at_1))
        incf = P(a["inc_flux"]) if optional else None
        if which == "lw_noscat":
            ds = (C.c_double * 2)(1.18350343, 2.81649655)
            wt = (C.c_double * 2)(0.3180413817, 0.1819586183)
            rc = L.ecckd_lw_solver_noscat_gpt(*head, 2, ds, wt, P(a["tau"]), P(a["lay"]), P(a["inc"]), P(a["dec"]), P(a["emis_g"]),
                                              P(a["sfc"]), incf, P(up), P(dn), sp.code, sp.stream())
            out = [up, dn]
        elif which == "lw_2stream":
            rc = L.ecckd_lw_solver_2stream_gpt(*head, P(a["tau"]), P(a["ssa"]), P(a["g"]), P(a["lay"]), P(a["inc"]), P(a["dec"]),
                                               P(a["emis_g"]), P(a["sfc"]), incf, P(up), P(dn), sp.code, sp.stream())
            out = [up, dn]
        else:
            rc = L.ecckd_sw_solver_2stream_gpt(*head, P(a["tau"]), P(a["ssa"]), P(a["g"]), P(a["mu0"]), P(a["toa"]), incf,
                                               P(a["adir_g"]), P(a["adif_g"]), P(up), P(dn), P(dr) if optional else None,
                                               sp.code, sp.stream())
            out = [up, dn] + ([dr] if optional else [])
        assert rc == 0, pkg.last_error()
        return [sp.back(x) for x in out]
    return run


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlay", (60, 37))
def test_spectral_output_solvers(pkg, gpu, ncol, nlay):
    """ecckd_lw_solver_noscat_gpt, ecckd_lw_solver_2stream_gpt, ecckd_sw_solver_2stream_gpt."""
    c = solver_case(ncol, nlay, 3)
    for which in ("lw_noscat", "lw_2stream", "sw_2stream"):
        for optional in (False, True):
            out = both(gpu, run_gpt(pkg, which, c, top_at_1=optional, optional=optional))
            assert np.all(np.isfinite(out[0]))


# ------------------------------------------------------------------------------------------------
# element-wise operations and cloud sampling
# ------------------------------------------------------------------------------------------------
def particle_case(ncol, nlay, seed):
    rng = np.random.default_rng(100 * seed + ncol + nlay)
    s3, sb = (NG, nlay, ncol), (2, nlay, ncol)
    return dict(gas=(rng.uniform(0, 2, s3) * rng.choice([0.0, 1e-6, 1.0], size=s3), rng.uniform(0, 1, s3), rng.uniform(0, 0.9, s3)),
                same=(rng.uniform(0, 3, s3), rng.uniform(0.5, 1, s3), rng.uniform(0.6, 0.9, s3)),
                band=(rng.uniform(0, 3, sb), rng.uniform(0.5, 1, sb), rng.uniform(0.6, 0.9, sb)),
                mask=rng.integers(0, 2 ** NG, (nlay, ncol), dtype=np.uint64))


def make_op(pkg, sp, arrays, dtype):
    op = pkg.OpticalProps2str() if len(arrays) == 3 else pkg.OpticalProps1scl()
    op.tau = sp.to(arrays[0], dtype)
    if len(arrays) == 3:
        op.ssa, op.g = sp.to(arrays[1], dtype), sp.to(arrays[2], dtype)
    return op


def op_values(sp, op):
    return [sp.back(op.tau)] + ([sp.back(op.ssa), sp.back(op.g)] if hasattr(op, "ssa") else [])


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlay", (60, 37))
def test_delta_scale_and_increment(pkg, gpu, ncol, nlay):
    """ecckd_delta_scale / _f32 with and without `forward`; ecckd_increment / _f32 for every pair of one- and two-stream
    operands, on g-points and by band; ecckd_increment_masked / _f32.  op2 must come through untouched."""
    p = particle_case(ncol, nlay, 4)
    fwd = 0.9 * p["same"][2] ** 2
    for dtype in (np.float64, np.float32):
        for f in (None, fwd):
            def run(sp):
                op = make_op(pkg, sp, p["same"], dtype)
                assert op.delta_scale(forward=sp.to(f, dtype)) == ""
                return op_values(sp, op)
            both(gpu, run)
        for n1 in (1, 3):
            for op2, bands in ((p["same"][:1], None), (p["same"], None), (p["band"][:1], B2G), (p["band"], B2G)):
                for mask in (None, p["mask"]):
                    def run(sp):
                        a, b = make_op(pkg, sp, p["gas"][:n1], dtype), make_op(pkg, sp, op2, dtype)
                        assert a.increment(b, band2gpt=bands, cloud_mask=sp.mask(mask)) == ""
                        for got, want in zip(op_values(sp, b), op2):
                            assert np.array_equal(got, want.astype(dtype))
                        return op_values(sp, a)
                    both(gpu, run)


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlay", (60, 1))
def test_cloud_mask_sample(pkg, gpu, ncol, nlay):
    """ecckd_cloud_mask_sample with both overlap rules (a single layer has no overlap parameter)."""
    cf = synthetic.cloud_fraction(21, ncol, 60)[-nlay:]
    cf[0, 0] = 0.5                                       # at least one cloudy cell whatever the columns drew
    alpha = np.random.default_rng(ncol + nlay).uniform(0, 1, (max(nlay - 1, 0), ncol))
    for overlap, al in (("max_ran", None), ("exp_ran", alpha)):
        def run(sp):
            m = pkg.sample_cloud_mask(sp.to(cf), 32, overlap, sp.to(al), seed=5, col0=21)
            return [sp.back(m).view(np.uint64)]
        out = both(gpu, run)
        assert np.any(out[0] != 0)


# ------------------------------------------------------------------------------------------------
# calls on a model: gas optics, Planck Jacobian term, fused fluxes
# ------------------------------------------------------------------------------------------------
def model_case(k, c0, ncol, nlay, shortwave=False):
    """Columns with a scalar gas (o2), per-column gases (co2, ch4, ...), a per-layer profile (n2o) and full fields (h2o, o3)."""
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay, shortwave=shortwave)
    cols["n2o"] = np.linspace(2e-7, 5e-7, nlay)
    rng = np.random.default_rng(c0 + ncol + nlay)
    nb = k.get_nband()
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], nb, 1)
    cols["inc_flux"] = rng.uniform(0.0, 2.0, (k.get_ngpt(), ncol))
    cols["alb_dir"], cols["alb_dif"] = rng.uniform(0.02, 0.6, (ncol, nb)), rng.uniform(0.02, 0.6, (ncol, nb))
    cols["scale"] = rng.uniform(0.97, 1.03, ncol)
    return cols


def gas_concs(pkg, sp, cols, dtype=np.float64, names=None):
    return helpers.product_gas_concs(pkg, cols, lambda a: sp.to(a, dtype), names)


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlay", SW_NLAYS)
def test_gas_optics_sw(pkg, gpu, models, ncol, nlay):
    """ecckd_gas_optics_sw / _f32 (tau, ssa, g, toa_src)."""
    k = models["sw"]
    cols = model_case(k, 31, ncol, nlay, shortwave=True)
    for dtype in (np.float64, np.float32):
        def run(sp):
            like = sp.to(np.zeros(1), dtype)
            op = pkg.OpticalProps2str()
            op.alloc_2str(ncol, nlay, k, like=like)
            toa = filled(sp, (k.get_ngpt(), ncol), dtype)
            assert k.gas_optics(None, sp.to(cols["plev"], dtype), sp.to(cols["tlay"], dtype),
                                gas_concs(pkg, sp, cols, dtype, helpers.SW_NAMES), op, toa) == ""
            return [sp.back(a) for a in (op.tau, op.ssa, op.g, toa)]
        out = both(gpu, run)
        assert np.all(out[0] >= 0) and np.all(out[3] > 0)


@pytest.mark.parametrize("ncol", NCOLS)
def test_planck_sfc_source_jac(pkg, gpu, models, ncol):
    k = models["lw"]
    tsfc = model_case(k, 41, ncol, 60)["tsfc"]

    def run(sp):
        src = pkg.SourceFuncLW()
        src.sfc_source_jac = filled(sp, (k.get_ngpt(), ncol))
        assert k.planck_sfc_source_jac(sp.to(tsfc), src) == ""
        return [sp.back(src.sfc_source_jac)]
    assert np.all(both(gpu, run)[0] > 0)


def run_lw_fluxes(pkg, k, cols, nmus=1, inc=False, top_at_1=True, cloud=None, mask=None):
    """ecckd_lw_fluxes, or with `cloud` ecckd_lw_fluxes_allsky_2stream."""
    def run(sp):
        nlay, ncol = cols["tlay"].shape
        fl = pkg.FluxesBroadband(filled(sp, (nlay + 1, ncol)), filled(sp, (nlay + 1, ncol)))
        args = (sp.to(cols["plev"]), sp.to(cols["tlay"]), sp.to(cols["tsfc"]), sp.to(cols["tlev"]), gas_concs(pkg, sp, cols),
                top_at_1, sp.to(cols["emis"]))
        incf = sp.to(cols["inc_flux"]) if inc else None
        if cloud is None:
            assert k.lw_fluxes(*args, fl, n_gauss_angles=nmus, inc_flux=incf) == ""
        else:
            part = make_op(pkg, sp, (cloud["tau"], cloud["ssa"], cloud["g"]), np.float64)
            assert k.lw_fluxes_allsky(*args, part, fl, inc_flux=incf, cloud_mask=sp.mask(mask), use_2stream=True) == ""
            for got, want in zip(op_values(sp, part), (cloud["tau"], cloud["ssa"], cloud["g"])):
                assert np.array_equal(got, want)
        return [sp.back(fl.flux_up), sp.back(fl.flux_dn)]
    return run


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlay", LW_NLAYS)
def test_lw_fluxes_and_allsky_2stream(pkg, gpu, models, ncol, nlay):
    """ecckd_lw_fluxes and ecckd_lw_fluxes_allsky_2stream (with and without a mask)."""
    k = models["lw"]
    cols = model_case(k, 51, ncol, nlay)
    cloud = synthetic.clouds(51, ncol, nlay, k.get_nband())
    mask = mh.sample(synthetic.cloud_fraction(51, ncol, nlay), k.get_ngpt(), mh.MAX_RAN, None, 8, 51)
    for nmus, inc in ((1, False), (3, True)):
        out = both(gpu, run_lw_fluxes(pkg, k, cols, nmus, inc, top_at_1=not inc))
        assert np.all(np.isfinite(out[0])) and np.all(out[0] > 0)
    for m, inc in ((mask, True), (None, False)):
        out = both(gpu, run_lw_fluxes(pkg, k, cols, inc=inc, cloud=cloud, mask=m))
        assert np.all(np.isfinite(out[0])) and np.all(out[0] > 0)


def run_sw_fluxes(pkg, k, cols, dtype, with_dir=True, scale=False):
    def run(sp):
        nlay, ncol = cols["tlay"].shape
        t = lambda a: sp.to(a, dtype)
        fl = pkg.FluxesBroadband(*[filled(sp, (nlay + 1, ncol), dtype) for _ in range(3 if with_dir else 2)])
        assert k.sw_fluxes(t(cols["plev"]), t(cols["tlay"]), gas_concs(pkg, sp, cols, dtype, helpers.SW_NAMES), True, t(cols["mu0"]),
                           t(cols["alb_dir"]), t(cols["alb_dif"]), fl, toa_scale=t(cols["scale"]) if scale else None) == ""
        return [sp.back(a) for a in (fl.flux_up, fl.flux_dn) + ((fl.flux_dn_dir,) if with_dir else ())]
    return run


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlay", SW_NLAYS)
def test_sw_fluxes(pkg, gpu, models, ncol, nlay):
    """ecckd_sw_fluxes and ecckd_sw_fluxes_f32; ecckd_sw_fluxes_allsky (delta-scaled and not) and _allsky_mcica."""
    k = models["sw"]
    cols = model_case(k, 61, ncol, nlay, shortwave=True)
    for dtype in (np.float64, np.float32):
        for with_dir, scale in ((True, False), (False, True)):
            out = both(gpu, run_sw_fluxes(pkg, k, cols, dtype, with_dir, scale))
            assert np.all(np.isfinite(out[0]))
    cloud = synthetic.clouds(61, ncol, nlay, k.get_nband())
    mask = mh.sample(synthetic.cloud_fraction(61, ncol, nlay), k.get_ngpt(), mh.MAX_RAN, None, 8, 61)
    for delta, m in ((True, None), (False, mask), (True, mask)):
        def run(sp):
            part = make_op(pkg, sp, (cloud["tau"], cloud["ssa"], cloud["g"]), np.float64)
            fl = pkg.FluxesBroadband(*[filled(sp, (nlay + 1, ncol)) for _ in range(3)])
            assert k.sw_fluxes_allsky(sp.to(cols["plev"]), sp.to(cols["tlay"]), gas_concs(pkg, sp, cols, names=helpers.SW_NAMES), True,
                                      sp.to(cols["mu0"]), sp.to(cols["alb_dir"]), sp.to(cols["alb_dif"]), part, fl, delta_scale=delta,
                                      cloud_mask=sp.mask(m)) == ""
            for got, want in zip(op_values(sp, part), (cloud["tau"], cloud["ssa"], cloud["g"])):
                assert np.array_equal(got, want)
            return [sp.back(a) for a in (fl.flux_up, fl.flux_dn, fl.flux_dn_dir)]
        both(gpu, run)


# ------------------------------------------------------------------------------------------------
# the arenas grow and are reused
# ------------------------------------------------------------------------------------------------
def test_arena_growth_and_reuse(pkg, gpu, models):
    """The host route at 33, then 130, then 33 columns again in one process: a solver call (the solver arena of the
    device) and a fused call (the arena of the model); each result equals its device result."""
    k = models["lw"]
    first = {}
    for step, ncol in enumerate((33, 130, 33)):
        c = solver_case(ncol, 60, 7)
        cols = model_case(k, 71, ncol, 60)
        for name, run in (("rte_lw", run_rte_lw(pkg, c, np.float64, True, True, 2)), ("lw_fluxes", run_lw_fluxes(pkg, k, cols, 1, True)),
                          ("rte_sw", run_rte_sw(pkg, c, np.float64, True, True))):
            out = both(gpu, run)
            if step == 0:
                first[name] = out
            elif step == 2:
                for a, b in zip(first[name], out):
                    assert np.array_equal(a, b), name


# ------------------------------------------------------------------------------------------------
# ECCKD_MIXED through the raw ABI
# ------------------------------------------------------------------------------------------------
def raw_gas_args(pkg, k, sp, cols, names=None):
    gc = gas_concs(pkg, sp, cols, names=names)
    nlay, ncol = cols["tlay"].shape
    return k._gas_args(gc, ncol, nlay, sp.code)


def test_mixed_chains_equal_the_device_chains(pkg, gpu, models):
    """gas optics ECCKD_MIXED (host inputs, device optical properties) -> solver ECCKD_MIXED (device optical properties,
    host boundary conditions and fluxes) equals the all-device chain, longwave and shortwave, at 33 x 60."""
    import torch
    L = pkg.lib()
    ncol, nlay = 33, 60
    dev, host = Space(gpu), Space()
    i32 = lambda a: C.c_void_p(a.ctypes.data)

    # ---- longwave ----
    k = models["lw"]
    ng, nb = k.get_ngpt(), k.get_nband()
    b2g = np.ascontiguousarray(k.get_band2gpt(), dtype=np.int32)
    cols = model_case(k, 81, ncol, nlay)

    def lw_chain(inp, out, space_go, space_rte):
        """inp / out: where the inputs and the fluxes live; the optical properties and sources are device tensors."""
        a = {n: inp.to(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev", "emis", "inc_flux")}
        n, names, ptrs, cs, ls, sc, keep = raw_gas_args(pkg, k, inp, cols)
        big = [filled(dev, (ng, nlay, ncol)) for _ in range(4)] + [filled(dev, (ng, ncol))]
        st = dev.stream()
        assert L.ecckd_gas_optics_lw(k._need(), ncol, nlay, inp.ptr(a["plev"]), inp.ptr(a["tlay"]), inp.ptr(a["tsfc"]),
                                     inp.ptr(a["tlev"]), n, names, ptrs, cs, ls, sc, *[dev.ptr(x) for x in big], space_go, st) == 0, \
            pkg.last_error()
        up, dn = filled(out, (nlay + 1, ncol)), filled(out, (nlay + 1, ncol))
        assert L.ecckd_rte_lw_inc_flux(0, ncol, nlay, ng, 1, 2, *[dev.ptr(x) for x in big], nb, i32(b2g), inp.ptr(a["emis"]),
                                       inp.ptr(a["inc_flux"]), out.ptr(up), out.ptr(dn), space_rte, st) == 0, pkg.last_error()
        torch.cuda.synchronize()
        return [out.back(up), out.back(dn)] + [dev.back(x) for x in big]

    d, m = lw_chain(dev, dev, 1, 1), lw_chain(host, host, MIXED, MIXED)
    for x, y in zip(d, m):
        assert np.array_equal(x, y)
    assert np.all(d[0] > 0)

    # ---- shortwave ----
    k = models["sw"]
    ng, nb = k.get_ngpt(), k.get_nband()
    b2g = np.ascontiguousarray(k.get_band2gpt(), dtype=np.int32)
    cols = model_case(k, 82, ncol, nlay, shortwave=True)

    def sw_chain(inp, out, space_go, space_rte):
        a = {n: inp.to(cols[n]) for n in ("plev", "tlay", "mu0", "alb_dir", "alb_dif")}
        n, names, ptrs, cs, ls, sc, keep = raw_gas_args(pkg, k, inp, cols, helpers.SW_NAMES)
        big = [filled(dev, (ng, nlay, ncol)) for _ in range(3)]
        toa = filled(inp, (ng, ncol))                        # (MIXED: toa_src goes back to the host)
        st = dev.stream()
        assert L.ecckd_gas_optics_sw(k._need(), ncol, nlay, inp.ptr(a["plev"]), inp.ptr(a["tlay"]), n, names, ptrs, cs, ls, sc,
                                     *[dev.ptr(x) for x in big], inp.ptr(toa), space_go, st) == 0, pkg.last_error()
        fl = [filled(out, (nlay + 1, ncol)) for _ in range(3)]
        assert L.ecckd_rte_sw(0, ncol, nlay, ng, 1, *[dev.ptr(x) for x in big], inp.ptr(a["mu0"]), inp.ptr(toa), nb, i32(b2g),
                              inp.ptr(a["alb_dir"]), inp.ptr(a["alb_dif"]), *[out.ptr(x) for x in fl], space_rte, st) == 0, \
            pkg.last_error()
        torch.cuda.synchronize()
        return [out.back(x) for x in fl] + [inp.back(toa)] + [dev.back(x) for x in big]

    d, m = sw_chain(dev, dev, 1, 1), sw_chain(host, host, MIXED, MIXED)
    for x, y in zip(d, m):
        assert np.array_equal(x, y)
    assert np.all(np.isfinite(d[0]))
