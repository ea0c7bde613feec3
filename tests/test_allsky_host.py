"""CPU tests of the all-sky additions: the new C ABI symbols and their refusals (nothing computes without a GPU), the
numpy restatement of delta scaling and the increments (tests/allsky_helpers.py) against itself in extended precision,
the all-sky oracle composition, and the code objects of the new kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import allsky_helpers as ah
import helpers
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
from rte_ecckd_amd import synthetic

NEW = ("ecckd_delta_scale", "ecckd_delta_scale_f32", "ecckd_increment", "ecckd_increment_f32", "ecckd_sw_fluxes_allsky")


def test_new_symbols_are_declared_and_exported(pkg):
    syms = entry.exported_symbols()
    for s in NEW:
        assert s in syms and hasattr(pkg.lib(), s), s


def _props(pkg, cls, shape, dtype=np.float64, fill=0.5):
    op = cls()
    op.tau = np.full(shape, fill, dtype=dtype)
    if cls is pkg.OpticalProps2str:
        op.ssa = np.full(shape, fill, dtype=dtype)
        op.g = np.full(shape, fill, dtype=dtype)
    return op


def test_refusals_launch_nothing(pkg):
    """Every refusal returns non-zero with a message and leaves the arrays alone; with valid arguments and no GPU the
    calls fail loudly instead of computing on the CPU."""
    import torch
    L = pkg.lib()
    ng, nlay, ncol = 6, 3, 4
    one = _props(pkg, pkg.OpticalProps1scl, (ng, nlay, ncol))
    two = _props(pkg, pkg.OpticalProps2str, (ng, nlay, ncol))
    bands = _props(pkg, pkg.OpticalProps2str, (2, nlay, ncol))
    for b2g, text in (([[1, 3], [5, 6]], "does not tile"), ([[1, 3], [3, 6]], "does not tile"), ([[1, 3], [4, 5]], "does not tile"),
                      ([[4, 6], [1, 3]], "does not tile"), ([[1, 3], [4, 7]], "does not tile")):
        msg = two.increment(bands, band2gpt=np.array(b2g))
        assert text in msg, (b2g, msg)
        assert np.all(two.tau == 0.5) and np.all(two.g == 0.5)
    # ssa without g, through the C ABI (the Python containers always carry both)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = L.ecckd_increment(0, ncol, nlay, ng, p(two.tau), p(two.ssa), None, 0, None, p(one.tau), None, None, pkg.HOST, None)
    assert rc != 0 and "ssa without g" in pkg.last_error()
    rc = L.ecckd_increment(0, ncol, nlay, ng, p(one.tau), None, None, 0, None, p(two.tau), p(two.ssa), None, pkg.HOST, None)
    assert rc != 0 and "ssa without g" in pkg.last_error()
    rc = L.ecckd_increment(0, ncol, nlay, ng, p(one.tau), None, None, 2, None, p(bands.tau), None, None, pkg.HOST, None)
    assert rc != 0 and "band2gpt is required" in pkg.last_error()
    rc = L.ecckd_delta_scale(0, ncol, nlay, ng, p(two.tau), None, p(two.g), None, pkg.HOST, None)
    assert rc != 0 and "null argument" in pkg.last_error()
    # forward outside [0, 1] on host arrays (NaN included), fp64 and f32
    for dt in (np.float64, np.float32):
        t2 = _props(pkg, pkg.OpticalProps2str, (ng, nlay, ncol), dt)
        for bad in (1.5, -0.1, np.nan):
            f = np.full((ng, nlay, ncol), 0.3, dtype=dt)
            f[2, 1, 3] = bad
            assert "outside [0, 1]" in t2.delta_scale(forward=f)
            assert np.all(t2.tau == 0.5)
    # the fused call: band count, reference-order mode, null triple -- on a host-only model, before any device is asked for
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=-1) == ""
    nlay, ncol, nb = 60, 4, k.get_nband()
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    fl = pkg.FluxesBroadband(np.zeros((nlay + 1, ncol)), np.zeros((nlay + 1, ncol)))
    args = (np.full((nlay + 1, ncol), 1e4), np.full((nlay, ncol), 250.), gc, True, np.full(ncol, 0.5), np.full((ncol, nb), 0.1),
            np.full((ncol, nb), 0.1))
    wrong = _props(pkg, pkg.OpticalProps2str, (nb + 1, nlay, ncol))
    msg = k.sw_fluxes_allsky(*args, wrong, fl)
    assert "nband_p = %d" % (nb + 1) in msg and "%d bands" % nb in msg
    part = pkg.OpticalProps2str()
    assert part.alloc_2str_bands(ncol, nlay, k) == "" and part.tau.shape == (nb, nlay, ncol)
    for a in (part.tau, part.ssa, part.g):
        a[:] = 0.5
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        assert "fast arithmetic mode" in k.sw_fluxes_allsky(*args, part, fl)
    finally:
        pkg.set_arithmetic(pkg.FAST)
    assert "no CPU fallback" in k.sw_fluxes_allsky(*args, part, fl)      # host-only model: no GPU, no compute
    assert np.all(fl.flux_up == 0) and np.all(part.tau == 0.5)
    if not torch.cuda.is_available():
        assert "no HIP device" in two.increment(one) and np.all(two.tau == 0.5)
        assert "no HIP device" in one.increment(bands, band2gpt=np.array([[1, 2], [3, 6]])) and np.all(one.tau == 0.5)
        assert "no HIP device" in two.delta_scale() and np.all(two.tau == 0.5)


@pytest.mark.parametrize("nband,nlay", [(5, 60), (16, 137), (1, 1)])
def test_restatement_float64_against_longdouble(nband, nlay):
    """The float64 restatement stays under HALF of each derived bar from its own evaluation in np.longdouble (64-bit
    mantissa on x86) on synthetic.clouds, and the bookkeeping identities hold."""
    assert np.finfo(np.longdouble).eps < 2e-19
    ncol = 700
    c = synthetic.clouds(11, ncol, nlay, nband)
    part = (c["tau"], c["ssa"], c["g"])
    L = lambda t: tuple(a.astype(np.longdouble) for a in t)
    worst = max(ah.worst_ulp(a, b) for a, b in zip(ah.delta_scale(*part), ah.delta_scale(*L(part))))
    fwd = 0.9 * c["g"] * c["g"]
    worst = max([worst] + [ah.worst_ulp(a, b) for a, b in zip(ah.delta_scale(*part, forward=fwd),
                                                               ah.delta_scale(*L(part), forward=fwd.astype(np.longdouble)))])
    print("delta scaling: float64 against longdouble %.2f u (bar %.1f u)" % (worst, ah.DELTA_SCALE_BAR_ULP))
    assert worst <= ah.DELTA_SCALE_BAR_ULP / 2
    # increments, by band, onto gas-like properties on g-points
    rng = np.random.default_rng(nband)
    ng = 3 * nband + 2
    edges = np.sort(rng.choice(np.arange(1, ng), nband - 1, replace=False)) if nband > 1 else np.array([], dtype=int)
    b2g = np.stack([np.concatenate([[1], edges + 1]), np.concatenate([edges, [ng]])], axis=1)
    gas = (rng.uniform(0, 2, (ng, nlay, ncol)) * rng.choice([0.0, 1e-6, 1.0], size=(ng, nlay, ncol)),
           rng.uniform(0, 1, (ng, nlay, ncol)), rng.uniform(0, 0.9, (ng, nlay, ncol)))
    worst = 0.0
    for op1 in (gas[:1], gas):
        for op2 in (part[:1], part):
            got, want = ah.increment(op1, op2, b2g), ah.increment(L(op1), L(op2), b2g)
            worst = max([worst] + [ah.worst_ulp(a, b) for a, b in zip(got, want)])
    print("increments: float64 against longdouble %.2f u (bar %d u)" % (worst, ah.INCREMENT_BAR_ULP))
    assert worst <= ah.INCREMENT_BAR_ULP / 2
    # energy bookkeeping: the absorption optical depth survives delta scaling; a zero increment is the identity;
    # two increments commute to rounding
    ds = ah.delta_scale(*part)
    # (1 - ssa' divides the 7 roundings of ssa' by 1 - ssa'; tau' carries 4, the inputs' side 2, the products 1 each)
    amp = 1.0 / float((1 - ds[1]).min())
    assert np.allclose(ds[0] * (1 - ds[1]), part[0] * (1 - part[1]), rtol=(8 + 7 * amp) * ah.unit_roundoff(np.float64), atol=0)
    zero = (np.zeros_like(part[0]), part[1], part[2])
    live = gas[0] > 0       # (where the gas optical depth is 0 as well, ssa and g fall to 0 under the eps floor)
    for a, b in zip(ah.increment(gas, zero, b2g), gas):
        assert ah.worst_ulp(a[live], b[live]) <= ah.INCREMENT_BAR_ULP
    other = (0.3 * part[0], 0.5 + 0.5 * part[1], 0.9 * part[2])
    ab = ah.increment(ah.increment(gas, part, b2g), other, b2g)
    ba = ah.increment(ah.increment(gas, other, b2g), part, b2g)
    for a, b in zip(ab, ba):
        assert ah.worst_ulp(a, b) <= 4 * ah.INCREMENT_BAR_ULP      # (two increments on either side)


def test_allsky_oracle_sees_the_clouds(oracle_mod):
    """The all-sky oracle fluxes (oracle.gas_optics_ext + numpy increment + oracle.rte_sw; oracle.gas_optics_int + numpy
    increment + oracle.rte_lw) differ from the clear-sky ones by W m-2 in every cloudy column and by nothing in clear ones:
    what makes the bars of the GPU tests (1e-8 W m-2) meaningful."""
    ncol, nlay = 160, 60
    m = oracle_mod.CkdModel(SW_WIDE)
    cols = synthetic.columns(5, ncol, float(np.exp(m.log_pressure[0])), nlay=nlay, shortwave=True)
    rng = np.random.default_rng(1)
    nb = m.band2gpt.shape[0]
    cols["alb_dir"], cols["alb_dif"] = rng.uniform(0.02, 0.6, (ncol, nb)), rng.uniform(0.02, 0.6, (ncol, nb))
    cloud = synthetic.clouds(5, ncol, nlay, nb)
    items = helpers.oracle_gas_items(cols, helpers.SW_NAMES)
    clear = ah.oracle_sw_allsky(oracle_mod, m, cols, items, None)
    cloudy = cloud["cloudy"]
    assert 0.3 < cloudy.mean() < 0.8
    for delta in (True, False):
        allsky = ah.oracle_sw_allsky(oracle_mod, m, cols, items, cloud, delta=delta)
        assert ah.smallest_cloud_signal(allsky, clear, cloudy) > 1.0
        for a, b in zip(allsky, clear):
            assert np.array_equal(a[:, ~cloudy], b[:, ~cloudy])
    for path in (LW_FSCK, LW_RRTMGP):
        ml = oracle_mod.CkdModel(path)
        lc = synthetic.columns(5, ncol, float(np.exp(ml.log_pressure[0])), nlay=nlay)
        lcloud = synthetic.clouds(5, ncol, nlay, ml.band2gpt.shape[0])
        litems = helpers.oracle_gas_items(lc)
        lclear = ah.oracle_lw_allsky(oracle_mod, ml, lc, litems, None)
        lall = ah.oracle_lw_allsky(oracle_mod, ml, lc, litems, lcloud)
        assert ah.smallest_cloud_signal(lall, lclear, lcloud["cloudy"]) > 0.01
        for a, b in zip(lall, lclear):
            assert np.array_equal(a[:, ~lcloud["cloudy"]], b[:, ~lcloud["cloudy"]])


def test_allsky_code_objects(pkg):
    """The new kernels are in the library; the two-pass all-sky solver keeps everything in registers at three waves per
    SIMD, as the clear-sky fused form it extends; the layer-systolic all-sky form keeps three waves per SIMD."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.LIB_PATH)
    inc = [n for n in ks if "increment_kernel<" in n]
    assert len(inc) == 16, inc                                   # 4 combinations x g-point / band x fp64 / f32
    assert len([n for n in ks if "delta_scale_kernel<" in n]) == 4
    for n in inc + [n for n in ks if "delta_scale_kernel<" in n]:
        assert ks[n]["spill_vgpr"] == 0 and ks[n]["lds_bytes"] == 0, n
    sky = {n: k for n, k in ks.items() if "rte_sw_allsky_kernel<" in n}
    assert len(sky) == 2, list(sky)
    for n, k in sky.items():
        assert k["spill_vgpr"] == 0 and kernel_resources.waves_per_simd(k) == 3, (n, k)
    sys_sky = {n: k for n, k in ks.items() if "rte_sw_sys_allsky_kernel<" in n}
    assert len(sys_sky) == 4, list(sys_sky)                     # CLAMP x FULL
    for n, k in sys_sky.items():
        assert kernel_resources.waves_per_simd(k) == 3, (n, k)
