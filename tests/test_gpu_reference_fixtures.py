"""GPU tests: the product's gas optics against the reference module's own outputs, committed under
tests/golden/ref_*.npz by make_golden_ref.py (branch columns of every model file: p/T/vmr clamps,
Planck extrapolation, relative-linear gases around their reference, zero-thickness and
bottom-first layers).  Nothing here reads the reference tree.  Both memory spaces (torch arrays on
the device, numpy arrays on the host).  Bars as in test_gpu_parity.py:

  Planck sources, toa_src, g     bit-identical to the reference
  tau, ssa                       relative 1e-12 (device log() against libm) x cond
  zero (clamped) tau cells, NaN ssa cells (0/0 of zero-thickness layers): the same positions

cond = (|tau_gas| + |tau_ray|) / |tau| is 1 wherever the shortwave tau sums terms of one sign, which is
every top-first layer.  In bottom-first layers the Rayleigh depth is negative while a relative-linear
gas below its reference turns positive, so tau cancels and a last-bit difference of a term becomes a
relative difference of up to cond ulps in tau and in ssa = tau_ray/tau.  Measured on this fixture:
relative difference / cond <= 8e-15 everywhere, 5.5e-15 on the cond = 1 cells.

fp32: the single-precision entry points on the same inputs, held to the bars of
test_gpu_gas_f32.py against the oracle on the float32-rounded inputs (the oracle equals the
reference bit for bit: test_oracle.py::test_reference_fixtures_match_oracle), scaled by the
condition number of the operation where it exceeds 1: cond above for the shortwave, and for Planck
sources extrapolated far above the table (the t_above_grid column, up to 412 K) kappa =
(|w0| B0 + |w1| B1) / |w0 B0 + w1 B1| with w0 = 1 - w1 down to -61 (src/gas_optics_ecckd.f90:278-282).
Measured: relative difference / kappa <= 1.3e-7, about two float32 ulps.
"""
import numpy as np
import pytest

import helpers
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE

pytestmark = pytest.mark.gpu
TAU_RTOL = 1e-12
FILES = {"lw_fsck": LW_FSCK, "lw_rrtmgp": LW_RRTMGP, "sw_wide": SW_WIDE}
LW_SETS = [s for s in helpers.REF_FIXTURE_SETS if not s[0].startswith("sw")]
SPACES = ["device", "host"]


@pytest.fixture(autouse=True)
def default_options(pkg):
    """Default switches around every test, the implementation choices these tests set included (reset_solver_options
    leaves those alone)."""
    keep = {n: pkg.get_solver_option(n) for n in ("gas_slab_f32", "gas_merge_scalars")}
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    for n, v in keep.items():
        pkg.set_solver_option(n, v)
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)


_models = {}


def product_model(pkg, key):
    if key not in _models:
        k = pkg.GasOpticsEcckd()
        assert k.load(FILES[key], device=0) == ""
        _models[key] = k
    return _models[key]


def close(got, ref, what, cond=None):
    """tau / ssa: NaN and zero cells at the reference's positions, the rest within TAU_RTOL x cond."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN cells differ" % what
    ok = ~np.isnan(ref)
    assert np.array_equal(got[ok] == 0, ref[ok] == 0), "%s: zero cells differ" % what
    c = np.ones_like(ref) if cond is None else cond
    rel = np.abs(got[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-300)
    assert np.max(rel / c[ok]) < TAU_RTOL, what


def sw_cond(tau, ssa):
    """(|tau_gas| + |tau_ray|) / |tau| from the reference's tau and ssa (tau_ray = ssa tau); 1 at NaN ssa."""
    with np.errstate(all="ignore"):
        ray = ssa * tau
        c = (np.abs(tau - ray) + np.abs(ray)) / np.abs(tau)
    return np.where(np.isfinite(c), np.maximum(c, 1.0), 1.0)


def check_lw_against_fixture(got, ref):
    err, tau, lay, inc, dec, sfc = got
    assert err == ""
    close(tau, ref[0], "tau")
    for name, a, b in zip(("lay_source", "lev_source_inc", "lev_source_dec", "sfc_source"), (lay, inc, dec, sfc),
                          ref[1:]):
        assert np.array_equal(a.view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), name


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("slab", [0, 1, 2])
@pytest.mark.parametrize("key,nlay", LW_SETS)
def test_lw_fp64_matches_reference(pkg, gpu, key, nlay, slab, space):
    """Longwave fp64 with the tables staged as fp64 (gas_slab_f32 = 0), as their float32 image (1) and as the
    probe picks (2).  The 137-layer set gives its well-mixed gases as scalars: the merged-table path."""
    k = product_model(pkg, key)
    cols, ref, _ = helpers.load_ref_fixture(key, nlay)
    pkg.set_solver_option("gas_slab_f32", slab)
    got = helpers.run_lw_gas_optics(pkg, k, cols, gpu if space == "device" else None, helpers.REF_FIXTURE_GASES)
    check_lw_against_fixture(got, ref)


@pytest.mark.parametrize("merge", [1, 0])
def test_lw_scalar_gases_merged_and_not(pkg, gpu, merge):
    """The scalar well-mixed gases of the 137-layer set (ch4 below its reference: clamped per gas, also in the
    bottom-first column) through the merged table and gas by gas: both the reference's tau."""
    k = product_model(pkg, "lw_fsck")
    cols, ref, _ = helpers.load_ref_fixture("lw_fsck", 137)
    assert all(isinstance(cols[n], float) for n in helpers.WELL_MIXED)
    plan = k.plan(cols["plev"].shape[1], 137, helpers.REF_FIXTURE_GASES, scalar_gases=list(helpers.WELL_MIXED))
    assert plan["merged"] == 6
    pkg.set_solver_option("gas_merge_scalars", merge)
    got = helpers.run_lw_gas_optics(pkg, k, cols, gpu, helpers.REF_FIXTURE_GASES)
    check_lw_against_fixture(got, ref)


def run_sw(pkg, k, cols, gpu, space, dtype=np.float64):
    import torch
    ncol, nlay = cols["plev"].shape[1], cols["tlay"].shape[0]
    if space == "device":
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)
        back = lambda a: a.cpu().numpy()
    else:
        to = lambda a: np.ascontiguousarray(a, dtype=dtype)
        back = lambda a: a
    gc = helpers.product_gas_concs(pkg, cols, to, helpers.REF_FIXTURE_GASES)
    op = pkg.OpticalProps2str()
    op.alloc_2str(ncol, nlay, k, like=to(np.zeros(1)))
    toa = to(np.full((k.get_ngpt(), ncol), np.nan))
    err = k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), gc, op, toa)
    if space == "device":
        torch.cuda.synchronize()
    return err, back(op.tau), back(op.ssa), back(op.g), back(toa)


@pytest.mark.parametrize("space", SPACES)
def test_sw_fp64_matches_reference(pkg, gpu, space):
    """Shortwave fp64 on the edge columns: tau and ssa to 1e-12 (NaN ssa of the zero-thickness layers in place),
    g and toa_src bit-identical."""
    k = product_model(pkg, "sw_wide")
    cols, ref, _ = helpers.load_ref_fixture("sw_wide", 60)
    assert np.isnan(ref[1]).any()
    err, tau, ssa, g, toa = run_sw(pkg, k, cols, gpu, space)
    assert err == ""
    cond = sw_cond(ref[0], ref[1])
    assert np.all(cond[..., :-4] < 1 + 1e-12) and cond.max() > 1e3     # cancellation only in the bottom-first columns
    close(tau, ref[0], "tau", cond)
    close(ssa, ref[1], "ssa", cond)
    assert np.array_equal(g.view(np.uint64), ref[2].view(np.uint64))
    assert np.array_equal(toa.view(np.uint64), ref[3].view(np.uint64))


# ------------------------------------------------------------------------------------------------
# single precision
# ------------------------------------------------------------------------------------------------
def planck_kappa(m, T):
    """Condition number of the Planck interpolation at temperatures T (ng, ...): 1 inside the table."""
    idx = 1.0 + (T - m.temperature_planck[0]) / (m.temperature_planck[1] - m.temperature_planck[0])
    it0 = np.clip(idx.astype(int), 1, m.ntp - 1)
    w1 = idx - it0
    b0, b1 = np.moveaxis(m.planck_function[it0 - 1], -1, 0), np.moveaxis(m.planck_function[it0], -1, 0)
    k = (np.abs(1.0 - w1) * b0 + np.abs(w1) * b1) / np.abs((1.0 - w1) * b0 + w1 * b1)
    return np.where(idx >= 1.0, k, 1.0)


@pytest.mark.parametrize("key,nlay", LW_SETS)
def test_lw_fp32_on_reference_inputs(pkg, gpu, oracle_mod, key, nlay):
    """Every column but t_above_grid through test_gpu_gas_f32.check_lw_f32; that one with the same bars on tau and
    the Planck bars times kappa."""
    from test_gpu_gas_f32 import BARS, check_lw_f32
    k = product_model(pkg, key)
    m = oracle_mod.CkdModel(FILES[key])
    cols, _, names = helpers.load_ref_fixture(key, nlay)
    hot = [names.index("t_above_grid")] if "t_above_grid" in names else []
    rest = [c for c in range(len(names)) if c not in hot]
    pick = lambda idx: {n: (np.ascontiguousarray(v[..., idx]) if isinstance(v, np.ndarray) else v) for n, v in cols.items()}
    check_lw_f32(pkg, k, m, oracle_mod, pick(rest), gpu, names=helpers.REF_FIXTURE_GASES,
                 name="reference fixture %s %d" % (key, nlay))
    if not hot:
        return
    c32 = {n: (helpers.r32(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for n, v in pick(hot).items()}
    err, *got = helpers.run_lw_gas_optics(pkg, k, c32, gpu, helpers.REF_FIXTURE_GASES, dtype=np.float32)
    assert err == ""
    ref = oracle_mod.gas_optics_int(m, c32["plev"], c32["tlay"], c32["tsfc"],
                                    helpers.oracle_gas_items(c32, helpers.REF_FIXTURE_GASES), c32["tlev"])
    assert ref[-1] == ""
    temps = (None, c32["tlay"], c32["tlev"][1:], c32["tlev"][:-1], c32["tsfc"])
    kappa = [np.ones_like(ref[0])] + [planck_kappa(m, T) for T in temps[1:]]
    assert kappa[1].max() > 50
    big = ref[0] > 1e-6 * ref[0].max()
    for what, g, o, b, kp in zip(("tau", "lay", "inc", "dec", "sfc"), got, ref[:5], BARS, kappa):
        rel = np.abs(np.asarray(g, np.float64) - o) / np.maximum(np.abs(o), 1e-300)
        if what == "tau":
            rel = np.where(big, rel, 0.0)
        assert np.max(rel / kp) < b, what


def test_sw_fp32_on_reference_inputs(pkg, gpu, oracle_mod):
    """The bars of test_gpu_gas_f32.py::test_f32_sw_gas_optics_edges (tau 5e-5 relative where tau > 1e-6 max, clamped
    cells <= 1e-6 max, ssa 5e-5), and NaN ssa exactly where the reference has it."""
    k = product_model(pkg, "sw_wide")
    m = oracle_mod.CkdModel(SW_WIDE)
    cols, ref, _ = helpers.load_ref_fixture("sw_wide", 60)
    c32 = {n: (helpers.r32(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for n, v in cols.items()}
    err, tau, ssa, g, toa = run_sw(pkg, k, c32, gpu, "device", np.float32)
    assert err == ""
    otau, ossa, og, otoa, oerr = oracle_mod.gas_optics_ext(m, c32["plev"], c32["tlay"],
                                                           helpers.oracle_gas_items(c32, helpers.REF_FIXTURE_GASES))
    assert oerr == ""
    assert np.array_equal(np.isnan(ossa), np.isnan(ref[1]))
    gt = tau.astype(np.float64)
    big = otau > 1e-6 * otau.max()
    assert np.max(np.abs(gt - otau)[big] / otau[big]) < 5e-5
    assert np.all(gt[otau == 0] <= 1e-6 * otau.max())
    cond = sw_cond(otau, ossa)
    neg = otau < 0                                   # bottom-first layers: tau = Rayleigh (< 0) + gases
    assert np.max(np.abs(gt - otau)[neg] / (-otau[neg] * cond[neg])) < 5e-5
    assert np.array_equal(np.isnan(ssa), np.isnan(ossa))
    ok = ~np.isnan(ossa)
    one = ok & (cond < 1 + 1e-9)
    assert np.max(np.abs(ssa.astype(np.float64) - ossa)[one]) < 5e-5
    many = ok & ~one
    assert np.max(np.abs(ssa.astype(np.float64) - ossa)[many] / (np.abs(ossa[many]) * cond[many])) < 5e-5
    assert np.all(g == 0) and np.array_equal(toa, m.solar_irradiance.astype(np.float32)[:, None].repeat(toa.shape[1], 1))
