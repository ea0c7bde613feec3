"""CPU tests of the fused all-sky longwave call and the Fortran forms of the all-sky calls: the C ABI symbol and its
Python binding, the refusals of ecckd_lw_fluxes_allsky in their documented order on a host-only model (nothing computes
without a GPU), the code objects of the all-sky form of the Planck-recomputing layer-split solver, and the Fortran
sources (type-bound lw_fluxes_allsky / sw_fluxes_allsky, the driver's particle-file argument)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import LW_FSCK, SW_WIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound(pkg):
    assert "ecckd_lw_fluxes_allsky" in entry.exported_symbols()
    assert hasattr(pkg.lib(), "ecckd_lw_fluxes_allsky")
    assert pkg.lib().ecckd_lw_fluxes_allsky.argtypes is not None and len(pkg.lib().ecckd_lw_fluxes_allsky.argtypes) == 24
    assert callable(pkg.GasOpticsEcckd.lw_fluxes_allsky) and callable(pkg.OpticalProps1scl.alloc_1scl_bands)


def test_refusals_in_order_launch_nothing(pkg):
    """Every refusal of include/ecckd_hip.h, in its order, on a host-only model: each returns its message and leaves the
    fluxes and the particle arrays alone; with valid arguments the call fails loudly instead of computing on the CPU."""
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    nlay, ncol, nb = 60, 4, k.get_nband()
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    fl = pkg.FluxesBroadband(np.full((nlay + 1, ncol), -7.0), np.full((nlay + 1, ncol), -7.0))
    plev, tlay, tsfc, tlev = (np.full((nlay + 1, ncol), 1e4), np.full((nlay, ncol), 250.), np.full(ncol, 250.),
                              np.full((nlay + 1, ncol), 250.))
    emis = np.full((ncol, nb), 0.98)
    two = pkg.OpticalProps2str()
    assert two.alloc_2str_bands(ncol, nlay, k) == "" and two.tau.shape == (nb, nlay, ncol)
    one = pkg.OpticalProps1scl()
    assert one.alloc_1scl_bands(ncol, nlay, k) == "" and one.tau.shape == (nb, nlay, ncol) and not hasattr(one, "ssa")
    for a in (two.tau, two.ssa, two.g, one.tau):
        a[:] = 0.5

    def untouched():
        return (np.all(fl.flux_up == -7.0) and np.all(fl.flux_dn == -7.0) and
                all(np.all(a == 0.5) for a in (two.tau, two.ssa, two.g, one.tau)))

    call = lambda part, model=k, tlev_=tlev: model.lw_fluxes_allsky(plev, tlay, tsfc, tlev_, gc, True, emis, part, fl)
    # 1. wrong band count -- it wins over everything that follows: no tlev, reference-order mode
    wrong = pkg.OpticalProps2str()
    wrong.tau, wrong.ssa, wrong.g = (np.full((nb + 1, nlay, ncol), 0.5) for _ in range(3))
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        msg = call(wrong, tlev_=None)
        assert "nband_p = %d" % (nb + 1) in msg and "the model has %d bands" % nb in msg and untouched()
        # 2. missing tau_p (still in reference-order mode: the null check comes first)
        none = pkg.OpticalProps1scl()
        none.tau = None
        L, P = pkg.lib(), lambda a: a.ctypes.data
        names, n = b"h2o".ljust(pkg.NAME_LEN, b" "), 1
        import ctypes as C
        ptrs, cs, ls, sc = (C.c_void_p * 1)(), (C.c_longlong * 1)(0), (C.c_longlong * 1)(0), (C.c_double * 1)(1e-3)
        rc = L.ecckd_lw_fluxes_allsky(k._need(), ncol, nlay, P(plev), P(tlay), P(tsfc), None, n, names, ptrs, cs, ls, sc, 1, 1,
                                      P(emis), None, nb, None, P(two.ssa), P(fl.flux_up), P(fl.flux_dn), pkg.HOST, None)
        assert rc != 0 and "tau_p is required" in pkg.last_error() and untouched()
        # 3. reference-order mode (wins over the missing tlev)
        assert "fast arithmetic mode" in call(two, tlev_=None) and untouched()
        assert "fast arithmetic mode" in call(one) and untouched()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    # 4. a model without a Planck table (wins over the missing tlev)
    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    sw_part = pkg.OpticalProps1scl()
    assert sw_part.alloc_1scl_bands(ncol, nlay, ksw) == ""
    sw_part.tau[:] = 0.5
    msg = ksw.lw_fluxes_allsky(plev, tlay, tsfc, None, gc, True, np.full((ncol, ksw.get_nband()), 0.98), sw_part, fl)
    assert "no Planck table" in msg and untouched()
    # 5. missing tlev
    assert call(two, tlev_=None) == "tlev is required for ecckd" and untouched()
    # 6. host-only model: no GPU, no compute
    for part in (two, one):
        assert "no CPU fallback" in call(part) and untouched()


def test_allsky_longwave_code_objects(pkg):
    """The all-sky form of the Planck-recomputing solver is in the library under its own name -- one- and two-stream
    particles x the two source series -- and every instantiation keeps what the Planck form it extends has: no spilled
    register and two waves per SIMD.  The Planck form itself keeps its name, its argument list and zero spills."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.LIB_PATH)
    sky = {n: k for n, k in ks.items() if "rte_lw_split_allsky_kernel<" in n}
    assert len(sky) == 4, list(sky)
    for n, k in sky.items():
        assert "rte_lw_split_allsky_kernel<15, 4, 32, " in n and n.split(">")[0].endswith(", 2"), n
        assert k["spill_vgpr"] == 0 and k["scratch_bytes"] == 0 and kernel_resources.waves_per_simd(k) == 2, (n, k)
        assert k["max_flat_wg"] == 512, (n, k)
    planck = {n: k for n, k in ks.items() if "rte_lw_split_kernel<15, 4, 32, false, " in n and "true, 2>" in n}
    assert len(planck) == 2, list(planck)
    for n, k in planck.items():
        assert k["spill_vgpr"] == 0 and kernel_resources.waves_per_simd(k) == 2, (n, k)


def test_fortran_all_sky_forms(pkg):
    """The module declares the two type-bound procedures over the C symbols, the sources still compile, and the driver's
    usage names the particle file (skipped without amdflang)."""
    text = open(os.path.join(pkg.FORTRAN_DIR, "gas_optics_ecckd.F90")).read()
    for name in ("lw_fluxes_allsky", "sw_fluxes_allsky"):
        assert "procedure, public :: " + name in text and 'name="ecckd_' + name + '"' in text, name
    drv = pkg.build_fortran()
    if drv is None:
        pytest.skip("no amdflang in this image")
    out = subprocess.run([drv], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_driver" in out.stderr and "[particles.bin]" in out.stderr
    # a particle file without fused = 1 is refused with the usage text, before any file is opened
    out = subprocess.run([drv, "lw", "none.nc", "none.bin", "none.out", "0", "1", "0", "1", "0", "0", "particles.bin"],
                         capture_output=True, text=True)
    assert out.returncode != 0 and "needs fused = 1" in out.stderr and "usage: ecckd_driver" in out.stderr
