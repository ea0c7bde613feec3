"""The Fortran form of the sampled optical-depth scaling: ty_cloud_scaling and the type-bound sample_cloud_scaling /
lw_flux_scaled / sw_flux_scaled of ty_gas_optics_ecckd (iso_c_binding over the C calls) and the program
ecckd_scaling_driver.  Built with amdflang by __graft_entry__.build(), run here as a child process; compared with the
Python calls on the same block (host arrays, the gases handed over as the driver hands them)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cloud_scaling_ref as ref
from conftest import LW_RRTMGP, SW_WIDE
from rte_ecckd_amd import synthetic
from test_fortran_shim import write_input
from test_gpu_lw_allsky import block_gas_concs, write_particles


def test_fortran_forms_are_in_the_sources(pkg):
    text = open(os.path.join(pkg.FORTRAN_DIR, "gas_optics_ecckd.F90")).read()
    for sym in ("ecckd_cloud_scaling_create", "ecckd_cloud_scaling_destroy", "ecckd_cloud_scaling_lognormal",
                "ecckd_cloud_scaling_sample", "ecckd_lw_flux_scaled", "ecckd_sw_flux_scaled"):
        assert 'name="%s"' % sym in text, sym
    for proc in ("sample_cloud_scaling", "lw_flux_scaled", "sw_flux_scaled"):
        assert "procedure, public :: " + proc in text, proc
    assert "type, public :: ty_cloud_scaling" in text
    assert ("ecckd_scaling_driver", "ecckd_scaling_driver.F90", []) in pkg._FORTRAN_PROGRAMS
    # ecckd_driver takes no further positional arguments for this
    assert "scaling" not in open(os.path.join(pkg.FORTRAN_DIR, "ecckd_driver.F90")).read()
    drv = pkg.build_fortran()
    if drv is None:
        pytest.skip("no amdflang in this image")
    assert os.path.exists(pkg.SCALING_DRIVER)
    out = subprocess.run([pkg.SCALING_DRIVER], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_scaling_driver" in out.stderr


def write_scaling(path, overlap, seed, nfsd, nq, fsd0, dfsd, cf, fsd, alpha):
    with open(path, "wb") as f:
        f.write(struct.pack("<iqiidd", overlap, seed, nfsd, nq, fsd0, dfsd))
        f.write(np.ascontiguousarray(cf, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(fsd, dtype="<f8").tobytes())
        if overlap == 1:
            f.write(np.ascontiguousarray(alpha, dtype="<f8").tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("mode,overlap,with_ssa_g", [("lw", 0, True), ("sw", 1, True), ("lw", 1, False)])
def test_fortran_scaling_driver(pkg, gpu, tmp_path, mode, overlap, with_ssa_g):
    """The driver's scaling equals the restatement and the Python sampler, and its fluxes the Python lw_flux_scaled /
    sw_flux_scaled on the same block, bit for bit (both sides run the same C calls on host arrays)."""
    if not os.path.exists(pkg.SCALING_DRIVER) and pkg.build_fortran() is None:
        pytest.skip("no Fortran driver binary and no amdflang")
    shortwave = mode == "sw"
    path = SW_WIDE if shortwave else LW_RRTMGP
    k = pkg.GasOpticsEcckd()
    assert k.load(path, device=0) == ""
    nb, ng = k.get_nband(), k.get_ngpt()
    ncol, nlay = 150, 60
    cols = synthetic.columns(40, ncol, k.get_press_min(), nlay=nlay, shortwave=shortwave)
    cloud = synthetic.clouds(40, ncol, nlay, nb)
    assert cloud["cloudy"].any()
    cf = synthetic.cloud_fraction(40, ncol, nlay)
    rng = np.random.default_rng(1)
    alpha, fsd = rng.uniform(0, 1, (nlay - 1, ncol)), rng.uniform(0, 2.5, (nlay, ncol))
    seed, table = 2 ** 40 + 17, (5, 16, 0.0, 0.5)
    names = synthetic.GAS_ORDER
    write_input(tmp_path / "in.bin", cols, names, shortwave)
    write_particles(tmp_path / "part.bin", cloud, with_ssa_g, True)
    write_scaling(tmp_path / "scal.bin", overlap, seed, table[0], table[1], table[2], table[3], cf, fsd, alpha)
    r = subprocess.run([pkg.SCALING_DRIVER, mode, path, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "part.bin"),
                        str(tmp_path / "scal.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    nflux = ncol * (nlay + 1)
    assert len(raw) == 2 * nflux * 8 + ncol * nlay * ng * 4
    fu, fd = (np.frombuffer(raw, dtype="<f8", count=nflux, offset=i * nflux * 8).reshape(nlay + 1, ncol) for i in range(2))
    scaling = np.frombuffer(raw, dtype="<f4", offset=2 * nflux * 8).reshape(ng, nlay, ncol)

    tab = pkg.CloudScaling.lognormal(table[0], table[2], table[3], table[1])
    ov = "exp_ran" if overlap else "max_ran"
    want = pkg.sample_cloud_scaling(cf, ng, tab, fsd, ov, alpha if overlap else None, seed=seed, col0=0)
    assert np.array_equal(scaling, want)
    assert np.array_equal(want, ref.sample(cf, ng, tab.get_values(), table[2], table[3], fsd, overlap, alpha if overlap else None,
                                           seed, 0)[0])
    assert (want > 0).any() and len(np.unique(want)) > 100

    gc = block_gas_concs(pkg, cols, names, 0, ncol)
    part = pkg.OpticalProps2str() if with_ssa_g else pkg.OpticalProps1scl()
    part.tau = cloud["tau"].copy()
    if with_ssa_g:
        part.ssa, part.g = cloud["ssa"].copy(), cloud["g"].copy()
    fl = pkg.FluxesBroadband(np.empty((nlay + 1, ncol)), np.empty((nlay + 1, ncol)))
    if shortwave:
        alb = np.repeat(cols["albedo"][:, None], nb, 1)
        assert k.sw_flux_scaled(cols["plev"], cols["tlay"], gc, True, cols["mu0"], alb, alb.copy(), part, fl, want, delta_scale=True) == ""
    else:
        emis = np.repeat(cols["sfc_emis"][:, None], nb, 1)
        assert k.lw_flux_scaled(cols["plev"], cols["tlay"], cols["tsfc"], cols["tlev"], gc, True, emis, part, fl, want) == ""
    assert np.array_equal(fu, fl.flux_up) and np.array_equal(fd, fl.flux_dn)
    # the scaling changed something: the homogeneous cloud differs
    ones = np.ones_like(want)
    fl1 = pkg.FluxesBroadband(np.empty((nlay + 1, ncol)), np.empty((nlay + 1, ncol)))
    if shortwave:
        assert k.sw_flux_scaled(cols["plev"], cols["tlay"], gc, True, cols["mu0"], alb, alb.copy(), part, fl1, ones, delta_scale=True) == ""
    else:
        assert k.lw_flux_scaled(cols["plev"], cols["tlay"], cols["tsfc"], cols["tlev"], gc, True, emis, part, fl1, ones) == ""
    assert not np.array_equal(fl1.flux_up, fu)
