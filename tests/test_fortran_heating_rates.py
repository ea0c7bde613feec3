"""The Fortran form of the heating rates: module `mo_heating_rates` (compute_heating_rate, an iso_c_binding shim over the C
ABI) and the program ecckd_heating_driver, which goes from the atmosphere through ecckd%lw_fluxes to fluxes and on to
heating rates, into a host array or the device container.  Built with amdflang by __graft_entry__.build(), run here as a
child process."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import heating_rate_ref as ref
from conftest import LW_RRTMGP
from rte_ecckd_amd import synthetic
from test_fortran_shim import FLUX_ATOL, write_input


@pytest.mark.gpu
@pytest.mark.parametrize("device_resident", [0, 1])
def test_fortran_heating_driver(pkg, gpu, tmp_path, device_resident):
    """The program's heating_rate equals the numpy restatement applied to the flux_up / flux_dn the program itself wrote,
    bit for bit (host array and device container); its fluxes equal those of the Python lw_fluxes within FLUX_ATOL of
    tests/test_fortran_shim.py."""
    import torch
    if not os.path.exists(pkg.HEATING_DRIVER) and pkg.build_fortran() is None:
        pytest.skip("no Fortran driver binary and no amdflang")
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_RRTMGP, device=0) == ""
    ncol, nlay, nband = 70, 60, k.get_nband()
    cols = synthetic.columns(5, ncol, k.get_press_min(), nlay=nlay)
    write_input(tmp_path / "in.bin", cols, synthetic.GAS_ORDER, False)
    r = subprocess.run([pkg.HEATING_DRIVER, LW_RRTMGP, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(device_resident)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a = np.fromfile(tmp_path / "out.bin", dtype="<f8")
    nlev, nl = (nlay + 1) * ncol, nlay * ncol
    assert a.size == 2 * nlev + nl
    fu, fd = (a[i * nlev:(i + 1) * nlev].reshape(nlay + 1, ncol) for i in range(2))
    hr = a[2 * nlev:].reshape(nlay, ncol)
    want = ref.heating_rate(fu, fd, cols["plev"])
    assert np.array_equal(ref.bits(hr), ref.bits(want))
    assert np.isfinite(hr).all() and (hr != 0).any()

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    fl = pkg.FluxesBroadband(t(np.zeros((nlay + 1, ncol))), t(np.zeros((nlay + 1, ncol))))
    emis = t(np.repeat(cols["sfc_emis"][:, None], nband, 1))
    assert k.lw_fluxes(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]),
                       helpers.product_gas_concs(pkg, cols, t), True, emis, fl) == ""
    assert np.max(np.abs(fu - fl.flux_up.cpu().numpy())) < FLUX_ATOL and np.max(np.abs(fd - fl.flux_dn.cpu().numpy())) < FLUX_ATOL
