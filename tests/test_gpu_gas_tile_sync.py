"""Solver option "gas_tile_sync": the waves of a block of gas_fused_kernel meet at an execution barrier before every tile.
The rendezvous moves time only: with the option at 0 and at 1 every output holds the same bits, and at 1 the outputs sit
against the CPU oracle at the bars of tests/test_gpu_parity.py (tau and ssa 1e-12 relative, Planck sources bit-identical;
single precision: tau 2e-5 relative where it is not tiny, sources 2e-6; shortwave single precision as
tests/test_gpu_gas_f32.py: 5e-5).  The shapes are the smallest at which some waves of a block take one path of the tile
loop while others take another -- where a misplaced barrier would hang the block or lose a wave: a tile in which seven of
eight waves own no column, blocks that end in such a tile, several slab positions per segment with waves that own no lane
in a pass, the stray-wave path of a NaN pressure, the out-of-window path of the Planck table, and the 768-thread
instantiations (shortwave, tau only)."""
import numpy as np
import pytest

import helpers
from helpers import SW_NAMES, r32
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
TAU_RTOL = 1e-12


@pytest.fixture(autouse=True)
def options_back(pkg):
    saved = {n: pkg.get_solver_option(n) for n in ("gas_tile_sync", "gas_slab_f32")}
    pkg.set_arithmetic(pkg.FAST)
    yield
    for n, v in saved.items():
        pkg.set_solver_option(n, v)


@pytest.fixture(scope="module")
def lw(pkg, gpu, oracle_mod):
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=0) == ""
    return k, oracle_mod.CkdModel(LW_FSCK)


@pytest.fixture(scope="module")
def sw(pkg, gpu, oracle_mod):
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=0) == ""
    return k, oracle_mod.CkdModel(SW_WIDE)


def same_bits(a, b):
    """Bit for bit, NaN payloads included."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def both_settings(pkg, run):
    """run() with the option at 0, at 1 and at -1 (each mode's shipped default): the same bits in every output; returns the
    outputs of setting 1."""
    out = []
    for v in (0, 1, -1):
        pkg.set_solver_option("gas_tile_sync", v)
        assert pkg.get_solver_option("gas_tile_sync") == v
        out.append(run())
    for other in out[1:]:
        assert len(other) == len(out[0])
        for a, b in zip(out[0], other):
            assert same_bits(a, b)
    return out[1]


def lw_outputs(pkg, k, cols, gpu, dtype=np.float64):
    def run():
        err, *arrays = helpers.run_lw_gas_optics(pkg, k, cols, gpu, dtype=dtype)
        assert err == ""
        return arrays
    return both_settings(pkg, run)


def check_lw(pkg, k, m, oracle_mod, cols, gpu, nan_cols=()):
    """fp64 longwave: both settings, then setting 1 against the oracle as tests/test_gpu_parity.py check_lw does."""
    tau, lay, inc, dec, sfc = lw_outputs(pkg, k, cols, gpu)
    otau, olay, oinc, odec, osfc, oerr = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"],
                                                                   helpers.oracle_gas_items(cols), cols["tlev"])
    assert oerr == ""
    good = np.ones(tau.shape[-1], bool)
    good[list(nan_cols)] = False
    for a, b in ((tau, otau), (lay, olay), (inc, oinc), (dec, odec), (sfc, osfc)):
        assert np.array_equal(np.isnan(a), np.isnan(b))          # NaN exactly where the oracle has it
        assert np.all(np.isfinite(a[..., good]))
    for a, b in ((lay, olay), (inc, oinc), (dec, odec), (sfc, osfc)):
        assert np.array_equal(a[..., good], b[..., good])
    assert helpers.max_rel(tau[..., good], otau[..., good]) < TAU_RTOL
    assert np.array_equal(tau[..., good] == 0, otau[..., good] == 0)


def shuffled_orography(press_min, ncol, seed=1):
    """Surface pressures of 50-103 kPa shuffled over the columns (tools/bench_gas_optics_spread.py, "mountains")."""
    c = synthetic.columns(0, ncol, press_min)
    c = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in c.items()}
    nlay = c["tlay"].shape[0]
    eta = (np.arange(nlay + 1, dtype=np.float64) / nlay) ** 2
    ptop = c["plev"][0, 0]
    ps = 50000 + 53000 * np.random.default_rng(seed).random(ncol)
    c["plev"] = np.ascontiguousarray(ptop + (ps[None, :] - ptop) * eta[:, None])
    return c


def test_option_is_listed_and_checked(pkg, gpu):
    assert "gas_tile_sync" in pkg.solver_options()
    with pytest.raises(ValueError):
        pkg.set_solver_option("gas_tile_sync", 2)


@pytest.mark.parametrize("ncol", [513, 4609])
def test_ragged_tile(pkg, gpu, oracle_mod, lw, ncol):
    """513: one full tile, then one in which seven of eight waves have no column; 4609: a block that walks several
    tiles and ends in such a tile."""
    k, m = lw
    check_lw(pkg, k, m, oracle_mod, synthetic.columns(7, ncol, k.get_press_min()), gpu)


@pytest.mark.parametrize("ncol", [1, 63, 65])
def test_columns_in_the_last_tile_only(pkg, gpu, oracle_mod, lw, ncol):
    k, m = lw
    check_lw(pkg, k, m, oracle_mod, synthetic.columns(7, ncol, k.get_press_min()), gpu)


@pytest.mark.parametrize("slab_f32", [0, 1])
def test_orography(pkg, gpu, oracle_mod, lw, slab_f32):
    """Several slab positions per segment, waves that own no lane in a pass, waves split between positions; with the
    fp64 slab and with the float32 image of the tables."""
    k, m = lw
    pkg.set_solver_option("gas_slab_f32", slab_f32)
    check_lw(pkg, k, m, oracle_mod, shuffled_orography(k.get_press_min(), 4609), gpu)


def test_nan_pressure(pkg, gpu, oracle_mod, lw):
    """A NaN pressure sends its wave down the stray-wave path; the column is NaN exactly where the oracle's is."""
    k, m = lw
    cols = synthetic.columns(11, 4609, k.get_press_min())
    cols = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in cols.items()}
    cols["plev"][:, 2100] = np.nan
    check_lw(pkg, k, m, oracle_mod, cols, gpu, nan_cols=[2100])


def test_planck_window(pkg, gpu, oracle_mod, monkeypatch):
    """The 36-g table with a small forced Planck window: most waves take the tables-from-global-memory path."""
    monkeypatch.setenv("ECCKD_PLANCK_WINDOW", "16")
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_RRTMGP, device=0) == ""
    check_lw(pkg, k, oracle_mod.CkdModel(LW_RRTMGP), oracle_mod, synthetic.columns(11, 4609, k.get_press_min()), gpu)


@pytest.mark.parametrize("ncol", [513, 4609])
def test_lw_single_precision(pkg, gpu, oracle_mod, lw, ncol):
    """The bars are those of test_gpu_parity.py::test_single_precision_lw_path, and so are the columns: its 700
    (generator columns 3 .. 702), repeated to fill the call (700 is no multiple of 64: every wave still holds another
    set).  This test is about the rendezvous at ragged and multi-tile shapes, not about how far float32 arithmetic moves
    tau on columns nobody has looked at: on generator columns 3 .. 4611 the largest of the 8.3e6 relative differences
    is 2.2e-5, with either setting of the option (the same bits) -- the float32 pressure index, which
    tests/test_gpu_gas_f32.py accounts for cell by cell (working_precision_spread) and the plain bar does not."""
    k, m = lw
    cols = synthetic.columns(3, 700, k.get_press_min())
    idx = np.arange(ncol) % 700
    cols = {n: (np.ascontiguousarray(v[..., idx]) if isinstance(v, np.ndarray) else v) for n, v in cols.items()}
    c32 = {n: (r32(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for n, v in cols.items()}
    tau, lay, inc, dec, sfc = lw_outputs(pkg, k, c32, gpu, dtype=np.float32)
    assert tau.dtype == np.float32
    otau, olay, oinc, odec, osfc, _ = oracle_mod.gas_optics_int(m, c32["plev"], c32["tlay"], c32["tsfc"],
                                                               helpers.oracle_gas_items(c32), c32["tlev"])
    big = otau > 1e-6 * otau.max()
    assert np.max(np.abs(tau.astype(np.float64) - otau)[big] / otau[big]) < 2e-5
    for a, b in ((lay, olay), (inc, oinc), (dec, odec), (sfc, osfc)):
        assert helpers.max_rel(a, b) < 2e-6


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("ncol", [513, 4609])
def test_shortwave(pkg, gpu, oracle_mod, sw, ncol, dtype):
    import torch
    k, m = sw
    cols = synthetic.columns(9, ncol, k.get_press_min(), shortwave=True)
    if dtype == np.float32:
        cols = {n: (r32(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for n, v in cols.items()}
    nlay = cols["tlay"].shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)
    gc = helpers.product_gas_concs(pkg, cols, t, SW_NAMES)
    plev, tlay = t(cols["plev"]), t(cols["tlay"])

    def run():
        op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=plev)
        toa = torch.empty((k.get_ngpt(), ncol), dtype=plev.dtype, device=gpu)
        assert k.gas_optics(None, plev, tlay, gc, op, toa) == ""
        torch.cuda.synchronize()
        return [op.tau.cpu().numpy(), op.ssa.cpu().numpy(), op.g.cpu().numpy()]

    tau, ssa, g = both_settings(pkg, run)
    otau, ossa, og, _, oerr = oracle_mod.gas_optics_ext(m, cols["plev"], cols["tlay"], helpers.oracle_gas_items(cols, SW_NAMES))
    assert oerr == ""
    assert np.all(g == 0)
    if dtype == np.float64:
        assert helpers.max_rel(tau, otau) < TAU_RTOL and helpers.max_rel(ssa, ossa) < TAU_RTOL
    else:
        big = otau > 1e-6 * otau.max()
        assert np.max(np.abs(tau.astype(np.float64) - otau)[big] / otau[big]) < 5e-5
        assert np.max(np.abs(ssa - ossa)) < 5e-5


@pytest.mark.parametrize("ncol", [513, 4609])
def test_tau_only(pkg, gpu, oracle_mod, lw, ncol):
    """ecckd_gas_optics_lw_tau: the tau-only mode of the kernel (768 threads per block)."""
    import torch
    k, m = lw
    cols = synthetic.columns(7, ncol, k.get_press_min())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    gc = helpers.product_gas_concs(pkg, cols, to=t)
    plev, tlay = t(cols["plev"]), t(cols["tlay"])

    def run():
        op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, tlay.shape[0], k, like=plev)
        assert k.gas_optics_tau(plev, tlay, gc, op) == ""
        torch.cuda.synchronize()
        return [op.tau.cpu().numpy()]

    tau, = both_settings(pkg, run)
    otau = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], helpers.oracle_gas_items(cols), cols["tlev"])[0]
    assert helpers.max_rel(tau, otau) < TAU_RTOL
    assert np.array_equal(tau == 0, otau == 0)
