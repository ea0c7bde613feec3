"""The Fortran form of the aerosol optics: module `mo_aerosol_optics` (type ty_aerosol_optics, an iso_c_binding shim over the
C ABI) and the program ecckd_aerosol_driver, which goes from species, sizes, masses, humidity and tables to band planes and
on to all-sky longwave fluxes.  Built with amdflang by __graft_entry__.build(), run here as a child process."""
import os
import struct
import subprocess

import numpy as np
import pytest

import aerosol_optics_ref as ref
import helpers
from conftest import LW_RRTMGP
from rte_ecckd_amd import synthetic
from test_fortran_shim import FLUX_ATOL, write_input

TABLE_NAMES = ("merra_aero_bin_lims", "aero_rh", "aero_dust_tbl", "aero_salt_tbl", "aero_sulf_tbl", "aero_bcar_tbl",
               "aero_bcar_rh_tbl", "aero_ocar_tbl", "aero_ocar_rh_tbl")


def write_aerosols(path, lut, aer):
    kind, size, mass, rh = aer
    nband, nbin = lut["aero_dust_tbl"].shape[:2]
    with open(path, "wb") as f:
        f.write(struct.pack("<iiii", nband, nbin, lut["aero_rh"].shape[0], kind.shape[0]))
        for n in TABLE_NAMES:
            f.write(np.ascontiguousarray(lut[n], dtype="<f8").tobytes())   # (C order of the reversed shape = Fortran order)
        f.write(np.ascontiguousarray(kind, dtype="<i4").tobytes())
        for a in (size, mass, rh):
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())


def test_fortran_aerosol_sources_compile(pkg):
    """CPU: the module and the program build with amdflang against the C ABI library (skipped without it)."""
    if pkg.build_fortran() is None:
        pytest.skip("no amdflang in this image")
    assert os.path.exists(pkg.AEROSOL_DRIVER)
    assert os.path.exists(os.path.join(pkg.FORTRAN_BUILD, "mo_aerosol_optics.o"))
    out = subprocess.run([pkg.AEROSOL_DRIVER], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_aerosol_driver" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("device_resident,nspec", [(0, 5), (1, 5), (0, 1)])
def test_fortran_aerosol_driver(pkg, gpu, tmp_path, device_resident, nspec):
    """The program's planes equal the numpy restatement's bit for bit (host containers and the device twin; several
    species, and RTE-RRTMGP's two-dimensional call); its fluxes equal those of the Python chain (AerosolOptics ->
    lw_fluxes_allsky) within FLUX_ATOL of tests/test_fortran_shim.py."""
    import torch
    if not os.path.exists(pkg.AEROSOL_DRIVER) and pkg.build_fortran() is None:
        pytest.skip("no Fortran driver binary and no amdflang")
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_RRTMGP, device=0) == ""
    ncol, nlay, nband = 70, 60, k.get_nband()
    cols = synthetic.columns(5, ncol, k.get_press_min(), nlay=nlay)
    lut = synthetic.aerosol_lut(nband, 5, 36)
    aer = synthetic.aerosols(5, ncol, nlay, max(nspec, 2))
    aer = (aer[0][-nspec:], aer[1][-nspec:], aer[2][-nspec:], aer[3])   # (nspec = 1: the sea-salt plane)
    write_input(tmp_path / "in.bin", cols, synthetic.GAS_ORDER, False)
    write_aerosols(tmp_path / "aerosols.bin", lut, aer)
    r = subprocess.run([pkg.AEROSOL_DRIVER, LW_RRTMGP, str(tmp_path / "in.bin"), str(tmp_path / "aerosols.bin"),
                        str(tmp_path / "out.bin"), str(device_resident)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a = np.fromfile(tmp_path / "out.bin", dtype="<f8")
    n3, n2 = nband * nlay * ncol, (nlay + 1) * ncol
    assert a.size == 3 * n3 + 2 * n2
    planes = [a[i * n3:(i + 1) * n3].reshape(nband, nlay, ncol) for i in range(3)]
    fu, fd = (a[3 * n3 + i * n2:3 * n3 + (i + 1) * n2].reshape(nlay + 1, ncol) for i in range(2))
    exp = ref.aerosol_optics(lut, *aer, True)
    for got, want in zip(planes, exp):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (exp[0] > 0).any()

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    ao = pkg.AerosolOptics()
    assert ao.load(None, *[lut[n] for n in TABLE_NAMES]) == ""
    part = pkg.OpticalProps2str()
    assert part.alloc_2str_bands(ncol, nlay, k, like=t(np.zeros(1))) == ""
    assert ao.aerosol_optics(*[t(x) for x in aer], part) == ""
    fl = pkg.FluxesBroadband(t(np.zeros((nlay + 1, ncol))), t(np.zeros((nlay + 1, ncol))))
    emis = t(np.repeat(cols["sfc_emis"][:, None], nband, 1))
    assert k.lw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]),
                              helpers.product_gas_concs(pkg, cols, t), True, emis, part, fl) == ""
    assert np.max(np.abs(fu - fl.flux_up.cpu().numpy())) < FLUX_ATOL and np.max(np.abs(fd - fl.flux_dn.cpu().numpy())) < FLUX_ATOL
