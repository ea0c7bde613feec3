"""Every launcher family of the layer-split longwave solver (kernels_rte_lw_split.hip) past its grid cap: the blocks walk
several tiles by grid stride, clear their LDS accumulators between tiles, and the last tile is ragged.  (The group without
a tile, which computes on clamped columns and stores nothing, is met in the small call of the two-group families: 96 columns
are 3 tiles in 2 blocks.)

A column's fluxes do not depend on where the column sits, so there is no yardstick and no tolerance: the form is called
once on 96 distinct columns and once on those columns repeated cyclically to ncol columns, and every output array of the
large call must equal the small call's column i % 96 bit for bit.  The large inputs are built on the device by indexing the
small ones.

ncol per family (tiles of 32 columns): two groups per block, cap 1 024 blocks -- 65 573 (2 050 tiles: a full round of 2 048, then
block 0 takes a full tile and the ragged one); one group per block, cap 1 024 -- 32 805; the rescaled array form, cap 2 048 -- 65 573; the
array form at 10 layers per wave, cap 3 072 -- 98 341."""
import numpy as np
import pytest

import helpers
import stride_helpers
import test_gpu_lw_allsky as lwt
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
NSMALL, NLAY, C0 = 96, 60, 11
OPTIONS = ("lw_solver", "lw_split_seg", "lw_both_skies", "lw_jac_inline")


@pytest.fixture(autouse=True)
def options(pkg):
    saved = [pkg.get_solver_option(n) for n in OPTIONS]
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    for n, v in zip(OPTIONS, saved):
        pkg.set_solver_option(n, v)


@pytest.fixture(scope="module")
def small(pkg, gpu):
    """The model, and the 96 columns on the device: atmosphere, two-stream cloud on the bands, sampled mask, and the arrays of
    the composed route (gas optical depth, Planck sources, the cell's (tau, ssa, g) after the increment)."""
    import torch
    from conftest import LW_FSCK
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=0) == ""
    assert k.get_ngpt() == 32
    t = lwt.T(gpu)
    cols, cloud = lwt.case(k, C0, NSMALL, NLAY)
    assert cloud["cloudy"].any() and not cloud["cloudy"].all()
    mask = pkg.sample_cloud_mask(np.ascontiguousarray(synthetic.cloud_fraction(C0, NSMALL, NLAY)), k.get_ngpt(), seed=C0)
    assert np.any(mask != 0) and np.any(mask != np.uint64(2 ** 32 - 1))
    d = {n: (v if np.isscalar(v) else t(v)) for n, v in cols.items()}
    d.update({"part_" + n: t(cloud[n]) for n in ("tau", "ssa", "g")})
    d["mask"] = t(mask.view(np.int64))
    # the array forms' inputs
    gc = helpers.product_gas_concs(pkg, d)
    op = pkg.OpticalProps1scl(); op.alloc_1scl(NSMALL, NLAY, k, like=d["plev"])
    src = pkg.SourceFuncLW(); src.alloc(NSMALL, NLAY, k, like=d["plev"])
    assert k.gas_optics(None, d["plev"], d["tlay"], d["tsfc"], gc, op, src, tlev=d["tlev"]) == ""
    two = pkg.OpticalProps2str(); two.alloc_2str(NSMALL, NLAY, k, like=d["plev"])
    two.tau.copy_(op.tau); two.ssa.zero_(); two.g.zero_()
    assert two.increment(particles(pkg, d), band2gpt=k.get_band2gpt()) == ""
    torch.cuda.synchronize()
    assert float(two.ssa.max()) > 0.0
    d.update(gas_tau=op.tau, lay=src.lay_source, inc=src.lev_source_inc, dec=src.lev_source_dec, sfc=src.sfc_source,
             cell_tau=two.tau, cell_ssa=two.ssa, cell_g=two.g)
    return k, d


def particles(pkg, d):
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = d["part_tau"], d["part_ssa"], d["part_g"]
    return op


def repeated(d, ncol, wanted):
    return stride_helpers.repeated(d, ncol, wanted, NSMALL)


def new(d, sentinel=-1.0):
    return stride_helpers.new(d, NLAY, sentinel)


def head(pkg, d):
    return (d["plev"], d["tlay"], d["tsfc"], d["tlev"], helpers.product_gas_concs(pkg, d), True, d["emis"])


# each form: (pkg, k, d) -> list of output tensors
def clear_form(pkg, k, d):
    fl = pkg.FluxesBroadband(new(d), new(d))
    assert k.lw_fluxes(*head(pkg, d), fl, n_gauss_angles=2, inc_flux=d["inc_flux"]) == ""
    return [fl.flux_up, fl.flux_dn]


def mcica_form(pkg, k, d):
    fl = pkg.FluxesBroadband(new(d), new(d))
    assert k.lw_fluxes_allsky(*head(pkg, d), particles(pkg, d), fl, n_gauss_angles=2, inc_flux=d["inc_flux"], cloud_mask=d["mask"]) == ""
    return [fl.flux_up, fl.flux_dn]


def both_form(pkg, k, d):
    pkg.set_solver_option("lw_both_skies", 1)
    fl, fc = pkg.FluxesBroadband(new(d), new(d)), pkg.FluxesBroadband(new(d), new(d))
    assert k.lw_fluxes_clear_allsky(*head(pkg, d), particles(pkg, d), fl, fc, n_gauss_angles=2, inc_flux=d["inc_flux"],
                                    cloud_mask=d["mask"]) == ""
    return [fl.flux_up, fl.flux_dn, fc.flux_up, fc.flux_dn]


def jac_form(pkg, k, d):
    pkg.set_solver_option("lw_jac_inline", 1)
    fl, jac = pkg.FluxesBroadband(new(d), new(d)), new(d)
    assert k.lw_fluxes_allsky(*head(pkg, d), particles(pkg, d), fl, n_gauss_angles=2, inc_flux=d["inc_flux"], cloud_mask=d["mask"],
                              flux_up_jac=jac) == ""
    return [fl.flux_up, fl.flux_dn, jac]


def rescaled_form(pkg, k, d):
    fl = pkg.FluxesBroadband(new(d), new(d))
    assert k.lw_fluxes_allsky(*head(pkg, d), particles(pkg, d), fl, n_gauss_angles=2, inc_flux=d["inc_flux"], cloud_mask=d["mask"],
                              rescaled=True) == ""
    return [fl.flux_up, fl.flux_dn]


def rescaled_jac_form(pkg, k, d):
    pkg.set_solver_option("lw_jac_inline", 1)
    fl, jac = pkg.FluxesBroadband(new(d), new(d)), new(d)
    assert k.lw_fluxes_rescaled(*head(pkg, d), particles(pkg, d), fl, flux_up_jac=jac, n_gauss_angles=2, inc_flux=d["inc_flux"],
                                cloud_mask=d["mask"]) == ""
    return [fl.flux_up, fl.flux_dn, jac]


def sources_of(pkg, d):
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = d["lay"], d["inc"], d["dec"], d["sfc"]
    return src


def rescaled_arrays_form(pkg, k, d):
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = d["cell_tau"], d["cell_ssa"], d["cell_g"]
    op.band2gpt = np.asarray(k.get_band2gpt())
    fl = pkg.FluxesBroadband(new(d), new(d))
    assert pkg.rte_lw(op, True, sources_of(pkg, d), d["emis"], fl, n_gauss_angles=2, inc_flux=d["inc_flux"], rescaled=True) == ""
    return [fl.flux_up, fl.flux_dn]


def arrays_form(shared):
    def form(pkg, k, d):
        pkg.set_solver_option("lw_solver", 1)
        pkg.set_solver_option("lw_split_seg", 10)
        op = pkg.OpticalProps1scl()
        op.tau = d["gas_tau"]
        op.band2gpt = np.asarray(k.get_band2gpt())
        fl = pkg.FluxesBroadband(new(d), new(d))
        # (the shared-levels form takes no inc_flux)
        assert pkg.rte_lw(op, True, sources_of(pkg, d), d["emis"], fl, n_gauss_angles=2, inc_flux=None if shared else d["inc_flux"],
                          shared_levels=shared) == ""
        return [fl.flux_up, fl.flux_dn]
    return form


ARRAYS = ("gas_tau", "lay", "inc", "dec", "sfc", "cell_tau", "cell_ssa", "cell_g")   # (ng, nlay, ncol): the array forms' alone
FUSED = lambda n: n not in ARRAYS
SOLVER = ("plev", "emis", "inc_flux", "lay", "inc", "dec", "sfc")
RESCALED = lambda n: n in SOLVER + ("cell_tau", "cell_ssa", "cell_g")
SPLIT = lambda n: n in SOLVER + ("gas_tau",)
CASES = [
    ("lw_fluxes", clear_form, 65573, FUSED),
    ("lw_fluxes_allsky_mcica", mcica_form, 65573, FUSED),
    ("lw_fluxes_clear_allsky", both_form, 32805, FUSED),
    ("lw_fluxes_jac", jac_form, 32805, FUSED),
    ("lw_fluxes_allsky_rescaled", rescaled_form, 32805, FUSED),
    ("lw_fluxes_rescaled_jac", rescaled_jac_form, 32805, FUSED),
    ("rte_lw_rescaled", rescaled_arrays_form, 65573, RESCALED),
    ("rte_lw_split", arrays_form(False), 98341, SPLIT),
    ("rte_lw_split_shared_levels", arrays_form(True), 98341, SPLIT),
]


@pytest.mark.parametrize("name,form,ncol,wanted", CASES, ids=[c[0] for c in CASES])
def test_columns_past_the_grid_cap_equal_the_small_call(pkg, gpu, small, name, form, ncol, wanted):
    import torch
    k, d = small
    want = form(pkg, k, d)
    big, idx = repeated(d, ncol, wanted)
    got = form(pkg, k, big)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0.0, (name, i)
        differ = int((g.view(torch.int64) != w.index_select(1, idx).view(torch.int64)).sum())
        print("%s, %d columns, output %d: %d of %d values differ from the 96-column call" % (name, ncol, i, differ, g.numel()))
        assert differ == 0, (name, i)
    del big, got
    pkg.release_scratch(0)
