"""The Fortran form of the fused per-band fluxes: the type-bound lw_flux_bands / sw_flux_bands of ty_gas_optics_ecckd
(iso_c_binding over ecckd_lw_flux_bands / ecckd_sw_flux_bands) and the program ecckd_bands_driver, which writes the band
planes of one block.  Built with amdflang by __graft_entry__.build(), run here as a child process; compared with the Python
call on the same block (host arrays, the gases handed over as the driver hands them)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import LW_RRTMGP, SW_WIDE
from rte_ecckd_amd import synthetic
from test_fortran_shim import write_input
from test_gpu_lw_allsky import block_gas_concs, write_particles


def test_fortran_forms_are_in_the_sources(pkg):
    text = open(os.path.join(pkg.FORTRAN_DIR, "gas_optics_ecckd.F90")).read()
    for sym in ("ecckd_lw_flux_bands", "ecckd_sw_flux_bands"):
        assert 'name="%s"' % sym in text, sym
    assert "procedure, public :: lw_flux_bands" in text and "procedure, public :: sw_flux_bands" in text
    assert ("ecckd_bands_driver", "ecckd_bands_driver.F90", []) in pkg._FORTRAN_PROGRAMS
    drv = pkg.build_fortran()
    if drv is None:
        pytest.skip("no amdflang in this image")
    assert os.path.exists(pkg.BANDS_DRIVER)
    out = subprocess.run([pkg.BANDS_DRIVER], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_bands_driver" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode,kind", [("lw", "clear"), ("lw", "2str"), ("lw", "1scl"), ("sw", "clear"), ("sw", "2str")])
def test_fortran_bands_driver(pkg, gpu, tmp_path, mode, kind):
    """The driver's band planes and broadband members against the Python call on the same block: bit for bit in the
    longwave and in the clear-sky shortwave; the shortwave all sky at 1e-9 * max(1, max|flux_dn|), the bar of
    tests/test_gpu_flux_bands.py for that route (here both sides run the same call, so the distance is expected to be 0)."""
    if not os.path.exists(pkg.BANDS_DRIVER) and pkg.build_fortran() is None:
        pytest.skip("no Fortran driver binary and no amdflang")
    sw = mode == "sw"
    path = SW_WIDE if sw else LW_RRTMGP
    k = pkg.GasOpticsEcckd()
    assert k.load(path, device=0) == ""
    ncol, nlay, nb = 70, 60, k.get_nband()
    cols = synthetic.columns(40, ncol, k.get_press_min(), nlay=nlay, shortwave=sw)
    cloud = synthetic.clouds(40, ncol, nlay, nb)
    assert cloud["cloudy"].any()
    names = synthetic.GAS_ORDER
    write_input(tmp_path / "in.bin", cols, names, sw)
    cmd = [pkg.BANDS_DRIVER, mode, path, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")]
    if kind != "clear":
        write_particles(tmp_path / "part.bin", cloud, kind == "2str", True)
        cmd.append(str(tmp_path / "part.bin"))
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a = np.fromfile(tmp_path / "out.bin", dtype="<f8")
    nlev, nout = (nlay + 1) * ncol, 3 if sw else 2
    assert a.size == nout * nlev * (nb + 1)
    planes = [a[i * nb * nlev:(i + 1) * nb * nlev].reshape(nb, nlay + 1, ncol) for i in range(nout)]
    broad = [a[nout * nb * nlev + i * nlev:nout * nb * nlev + (i + 1) * nlev].reshape(nlay + 1, ncol) for i in range(nout)]

    gc = block_gas_concs(pkg, cols, names, 0, ncol)
    c = np.ascontiguousarray
    part = None
    if kind != "clear":
        part = pkg.OpticalProps2str() if kind == "2str" else pkg.OpticalProps1scl()
        part.tau = c(cloud["tau"])
        if kind == "2str":
            part.ssa, part.g = c(cloud["ssa"]), c(cloud["g"])
    nan3, nan2 = (lambda: np.full((nb, nlay + 1, ncol), np.nan)), (lambda: np.full((nlay + 1, ncol), np.nan))
    fl = pkg.FluxesByband(nan3(), nan3(), nan3() if sw else None, nan2(), nan2(), nan2() if sw else None)
    if not sw:
        emis = np.repeat(c(cols["sfc_emis"])[:, None], nb, 1)
        assert k.lw_fluxes_byband(c(cols["plev"]), c(cols["tlay"]), c(cols["tsfc"]), c(cols["tlev"]), gc, True, emis, fl,
                                  particles=part) == ""
        want_planes, want_broad = [fl.bnd_flux_up, fl.bnd_flux_dn], [fl.flux_up, fl.flux_dn]
    else:
        alb = np.repeat(c(cols["albedo"])[:, None], nb, 1)
        assert k.sw_fluxes_byband(c(cols["plev"]), c(cols["tlay"]), gc, True, c(cols["mu0"]), alb, alb.copy(), fl, particles=part,
                                  delta_scale=True) == ""
        want_planes, want_broad = [fl.bnd_flux_up, fl.bnd_flux_dn, fl.bnd_flux_dn_dir], [fl.flux_up, fl.flux_dn, fl.flux_dn_dir]
    exact = not (sw and kind != "clear")
    bar = 0.0 if exact else 1e-9 * max(1.0, float(np.max(np.abs(want_broad[1]))))
    for got, want in zip(planes + broad, want_planes + want_broad):
        assert np.isfinite(want).all() and (want != 0).any()
        if exact:
            assert np.array_equal(got, want)
        else:
            d = float(np.max(np.abs(got - want)))
            print("fortran %s %s: %.2e from the Python call (bar %.1e)" % (mode, kind, d, bar))
            assert d <= bar
