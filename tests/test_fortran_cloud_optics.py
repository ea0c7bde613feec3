"""The Fortran form of the cloud optics: module `mo_cloud_optics` (type ty_cloud_optics, an iso_c_binding shim over the C
ABI) and the program ecckd_cloud_driver, which goes from water paths and tables to band planes and on to all-sky longwave
fluxes.  Built with amdflang by __graft_entry__.build(), run here as a child process."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cloud_optics_ref as ref
import helpers
from conftest import LW_RRTMGP
from rte_ecckd_amd import synthetic
from test_fortran_shim import FLUX_ATOL, write_input


def write_clouds(path, lut, icergh, water):
    nband, nsl = lut["lut_extliq"].shape
    nrgh, _, nsi = lut["lut_extice"].shape
    with open(path, "wb") as f:
        f.write(struct.pack("<iiiii", nband, nsl, nsi, nrgh, icergh))
        f.write(struct.pack("<dddd", lut["radliq_lwr"], lut["radliq_upr"], lut["radice_lwr"], lut["radice_upr"]))
        for n in ("lut_extliq", "lut_ssaliq", "lut_asyliq", "lut_extice", "lut_ssaice", "lut_asyice"):
            f.write(np.ascontiguousarray(lut[n], dtype="<f8").tobytes())   # (C order of the reversed shape = Fortran order)
        for a in water:
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())


def test_fortran_cloud_sources_compile(pkg):
    """CPU: the module and the program build with amdflang against the C ABI library (skipped without it)."""
    if pkg.build_fortran() is None:
        pytest.skip("no amdflang in this image")
    assert os.path.exists(pkg.CLOUD_DRIVER)
    assert os.path.exists(os.path.join(pkg.FORTRAN_BUILD, "mo_cloud_optics.o"))
    out = subprocess.run([pkg.CLOUD_DRIVER], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_cloud_driver" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("device_resident", [0, 1])
def test_fortran_cloud_driver(pkg, gpu, tmp_path, device_resident):
    """The program's planes equal the numpy restatement's bit for bit (host containers and the device twin); its fluxes
    equal those of the Python chain (CloudOptics -> lw_fluxes_allsky) within FLUX_ATOL of tests/test_fortran_shim.py."""
    import torch
    if not os.path.exists(pkg.CLOUD_DRIVER) and pkg.build_fortran() is None:
        pytest.skip("no Fortran driver binary and no amdflang")
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_RRTMGP, device=0) == ""
    ncol, nlay, nband, icergh = 70, 60, k.get_nband(), 2
    cols = synthetic.columns(5, ncol, k.get_press_min(), nlay=nlay)
    names = synthetic.GAS_ORDER
    lut = synthetic.cloud_lut(nband, 20, 18, 3)
    water = synthetic.cloud_water(5, ncol, nlay)
    write_input(tmp_path / "in.bin", cols, names, False)
    write_clouds(tmp_path / "clouds.bin", lut, icergh, water)
    r = subprocess.run([pkg.CLOUD_DRIVER, LW_RRTMGP, str(tmp_path / "in.bin"), str(tmp_path / "clouds.bin"),
                        str(tmp_path / "out.bin"), str(device_resident)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a = np.fromfile(tmp_path / "out.bin", dtype="<f8")
    n3, n2 = nband * nlay * ncol, (nlay + 1) * ncol
    assert a.size == 3 * n3 + 2 * n2
    planes = [a[i * n3:(i + 1) * n3].reshape(nband, nlay, ncol) for i in range(3)]
    fu, fd = (a[3 * n3 + i * n2:3 * n3 + (i + 1) * n2].reshape(nlay + 1, ncol) for i in range(2))
    exp = ref.cloud_optics(*water, lut, icergh=icergh)
    for got, want in zip(planes, exp):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (exp[0] > 0).any()

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    co = pkg.CloudOptics()
    assert co.load_lut(None, lut["radliq_lwr"], lut["radliq_upr"], 1.0, lut["radice_lwr"], lut["radice_upr"], 1.0,
                       *[lut["lut_" + q + p] for p in ("liq", "ice") for q in ("ext", "ssa", "asy")]) == ""
    assert co.set_ice_roughness(icergh) == ""
    part = pkg.OpticalProps2str()
    assert part.alloc_2str_bands(ncol, nlay, k, like=t(np.zeros(1))) == ""
    assert co.cloud_optics(*[t(w) for w in water], part) == ""
    fl = pkg.FluxesBroadband(t(np.zeros((nlay + 1, ncol))), t(np.zeros((nlay + 1, ncol))))
    emis = t(np.repeat(cols["sfc_emis"][:, None], nband, 1))
    assert k.lw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]),
                              helpers.product_gas_concs(pkg, cols, t), True, emis, part, fl) == ""
    assert np.max(np.abs(fu - fl.flux_up.cpu().numpy())) < FLUX_ATOL and np.max(np.abs(fd - fl.flux_dn.cpu().numpy())) < FLUX_ATOL
