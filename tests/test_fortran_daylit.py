"""The shortwave RFMIP driver with -l: the block loop goes through the type-bound sw_fluxes_daylit (the library selects the
daylit columns, gathers the inputs and scatters the fluxes) instead of computing the night columns with mu0 = 1 and zeroing
them on the host.  Built on the fixtures of tests/test_rfmip_driver.py, whose site list ends in night columns."""
import os
import subprocess

import numpy as np
import pytest

import test_rfmip_driver as drv
from conftest import SW_WIDE

UP, DN = "rsu_Efx_RTE-ecckd_rad-irf_r1i1p1f1_gn.nc", "rsd_Efx_RTE-ecckd_rad-irf_r1i1p1f1_gn.nc"


def test_driver_sources(pkg):
    """CPU: the module binds the four C symbols, the type has the procedure, the driver takes -l and says so."""
    text = open(os.path.join(pkg.FORTRAN_DIR, "gas_optics_ecckd.F90")).read()
    for sym in ("ecckd_daylit_columns", "ecckd_sw_fluxes_daylit", "ecckd_gather_columns", "ecckd_scatter_columns"):
        assert 'name="%s"' % sym in text, sym
    assert "procedure, public :: sw_fluxes_daylit" in text
    assert "ecckd%sw_fluxes_daylit(" in open(os.path.join(pkg.FORTRAN_DIR, "ecckd_rfmip.F90")).read()
    if pkg.build_fortran() is None:
        pytest.skip("no amdflang in this image")
    r = subprocess.run([pkg.RFMIP_SW, "a.nc", "b.nc", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "-l - Shortwave: compute the daylit columns only" in r.stderr


@pytest.mark.gpu
def test_rfmip_sw_daylit_equals_the_default_route(pkg, gpu, oracle_mod, tmp_path):
    """With and without -l the flux variables of the two output files must be identical byte for byte, and the night sites
    zero.  The largest difference is printed before anything is asserted.

    -l takes the tsi route of sw_fluxes_daylit: the daylit columns go through the unfused calls the default route uses, with the
    incoming beam renormalised by the same expression, (solar(g)*tsi)/sum(solar) on the host (ecckd_rfmip_sw.F90:126-133).
    (The fused calls form solar(g)*toa_scale instead; with toa_scale = tsi/sum(solar) that beam differs from the host's in the
    last bit at 93 of the fixture's 100 sites, and the fluxes by up to 6.8e-13 W m-2 -- measured -- so a driver that must
    reproduce the default route's bytes cannot take them.)"""
    if not os.path.exists(pkg.RFMIP_SW) and pkg.build_fortran() is None:
        pytest.skip("no Fortran toolchain / binaries")
    m = oracle_mod.CkdModel(SW_WIDE)
    pmin = float(np.exp(m.log_pressure[0]))
    _, _, _, sza = drv.make_rfmip_files(str(tmp_path), pmin)
    use = np.tile(sza, drv.NEXP) < 90.0 - 2.0 * np.spacing(90.0)
    got = {}
    for flags in ((), ("-l",)):
        r = subprocess.run([pkg.RFMIP_SW, "rfmip.nc", SW_WIDE, "-b", "150"] + list(flags), cwd=str(tmp_path), capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr
        got[flags] = (drv.read_flux(str(tmp_path / UP), "rsu"), drv.read_flux(str(tmp_path / DN), "rsd"))
    for name, a, b in zip(("rsu", "rsd"), got[()], got[("-l",)]):
        diff = np.abs(a - b)
        print("%s: max |default - daylit| = %.3e W m-2 (max relative %.3e), %d of %d values differ"
              % (name, diff.max(), (diff / np.maximum(np.abs(a), 1e-300)).max(), int((a != b).sum()), a.size))
    for a, b in zip(got[()], got[("-l",)]):
        assert np.all(b[:, ~use] == 0) and (~use).sum() > 0 and np.any(b[:, use] > 0)
        assert a.tobytes() == b.tobytes()
