"""Solver option "gas_wave_roles": fp64 longwave gas optics by gas_roles_kernel, in which the eight tau waves of a
512-column tile and four source waves share a block of 768 threads ("Wave roles").  The split moves
time only.  The bar is bit equality, so there is no tolerance to choose: with the option at 1 (and at -1, each shape's
shipped default) tau, lay_source, lev_source_inc, lev_source_dec and sfc_source hold the bits they hold with the option at 0
on the same inputs, NaN payloads included; the outputs of setting 1 then pass the oracle check of
tests/test_gpu_gas_tile_sync.py's check_lw (tau 1e-12 relative, Planck sources bit-identical, NaN where the oracle has it).

The shapes are the smallest at which a path of the new kernel can go wrong: a partial wave, a source wave with one empty
set, one column in its second set, a ragged second tile, several tiles and segments; one and two layers (no next layer; the
edge kernel's planes); both store forms of the level sources and none; several slab positions with split and masked waves;
source waves on the global-memory path of a small Planck window; a NaN pressure column; the per-tile barrier on and off;
the three settings of the table image; the merged-slot shape; one captured-graph replay."""
import numpy as np
import pytest

import helpers
from conftest import LW_FSCK, LW_RRTMGP
from rte_ecckd_amd import synthetic
from test_gpu_gas_tile_sync import same_bits, shuffled_orography, TAU_RTOL

pytestmark = pytest.mark.gpu
OPTION = "gas_wave_roles"
NAMES = ("tau", "lay_source", "lev_source_inc", "lev_source_dec", "sfc_source")
SCALARS = ("co2", "ch4", "n2o", "o2", "cfc11", "cfc12")
SENTINEL = -7.0   # what the level arrays hold before a call


@pytest.fixture(autouse=True)
def options_back(pkg):
    saved = {n: pkg.get_solver_option(n) for n in (OPTION, "gas_tile_sync", "gas_slab_f32")}
    pkg.set_arithmetic(pkg.FAST)
    yield
    for n, v in saved.items():
        pkg.set_solver_option(n, v)


@pytest.fixture(scope="module")
def lw(pkg, gpu, oracle_mod):
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=0) == ""
    return k, oracle_mod.CkdModel(LW_FSCK)


_columns = {}


def columns(k, ncol, nlay=60):
    """synthetic.columns(7, ...) of the size, made once (read-only)."""
    key = (ncol, nlay)
    if key not in _columns:
        _columns[key] = synthetic.columns(7, ncol, k.get_press_min(), nlay=nlay)
    return _columns[key]


def gas_call(pkg, k, cols, gpu, separate=False, tlev=True, overrides=None, graph=False):
    """One gas_optics call on device tensors; the five outputs as numpy arrays.  separate: two contiguous level arrays
    instead of the level buffer.  graph: the call is captured and the outputs are those of one replay."""
    import torch
    ncol, nlay = cols["plev"].shape[1], cols["tlay"].shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)
    gc = helpers.product_gas_concs(pkg, cols, t, overrides=overrides)
    plev, tlay, tsfc = t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"])
    tl = t(cols["tlev"]) if tlev else None
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=plev)
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=plev, separate_levels=separate)
    assert (src.lev_source is None) == separate
    for a in src.level_views():
        a.fill_(SENTINEL)

    def step():   # (without tlev the call does its work and then answers as the reference does)
        assert k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tl) == ("" if tlev else "tlev is required for ecckd")

    def outputs():
        torch.cuda.synchronize()
        inc, dec = src.level_views()
        return [a.contiguous().cpu().numpy() for a in (op.tau, src.lay_source, inc, dec, src.sfc_source)]

    if not graph:
        step()
        return outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()          # warm-up on the stream that will be captured: its scratch exists now
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    inc, dec = src.level_views()
    for a in (op.tau, src.lay_source, inc, dec, src.sfc_source):
        a.zero_()
    g.replay()
    out = outputs()
    del g
    return out


def roles_keep_the_bits(pkg, run):
    """run() with the option at 0, at 1 and at -1: the same bits in all five outputs; returns the outputs of setting 1."""
    out = {}
    for v in (0, 1, -1):
        pkg.set_solver_option(OPTION, v)
        assert pkg.get_solver_option(OPTION) == v
        out[v] = run()
    for v in (1, -1):
        for name, a, b in zip(NAMES, out[0], out[v]):
            assert same_bits(a, b), (name, v)
    return out[1]


_oracle = {}


def against_oracle(oracle_mod, m, cols, out, key, tlev=True, overrides=None, nan_cols=()):
    """The oracle's outputs (computed once per key), as tests/test_gpu_gas_tile_sync.py check_lw."""
    if key not in _oracle:
        _oracle[key] = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"],
                                                 helpers.oracle_gas_items(cols, overrides=overrides), cols["tlev"] if tlev else None)
    otau, olay, oinc, odec, osfc, oerr = _oracle[key]
    assert oerr == ""
    tau, lay, inc, dec, sfc = out
    good = np.ones(tau.shape[-1], bool)
    good[list(nan_cols)] = False
    for a, b in ((tau, otau), (lay, olay), (inc, oinc), (dec, odec), (sfc, osfc)):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.all(np.isfinite(a[..., good]))
    for a, b in ((lay, olay), (inc, oinc), (dec, odec), (sfc, osfc)):
        assert np.array_equal(a[..., good], b[..., good])
    assert helpers.max_rel(tau[..., good], otau[..., good]) < TAU_RTOL
    assert np.array_equal(tau[..., good] == 0, otau[..., good] == 0)


def test_option_is_listed_and_checked(pkg, gpu, lw):
    assert OPTION in pkg.solver_options()
    assert pkg.get_solver_option(OPTION) == -1
    for bad in (2, -2, 0.5):
        with pytest.raises(ValueError):
            pkg.set_solver_option(OPTION, bad)
    # the wave-roles form keeps the slab rows and the whole Planck table of the fused form (four more waves' words of
    # reduction scratch: 128 bytes of LDS)
    k, _ = lw
    plans = {}
    for v in (0, 1):
        pkg.set_solver_option(OPTION, v)
        plans[v] = k.plan(4609, 60, synthetic.GAS_ORDER)
    assert plans[1]["lds_bytes"] == plans[0]["lds_bytes"] + 128
    assert all(plans[1][n] == plans[0][n] for n in plans[0] if n != "lds_bytes")
    assert plans[1]["slab_rows"] == 3 and plans[1]["planck_rows"] == 231


@pytest.mark.parametrize("ncol", [1, 63, 65, 128, 129, 513, 4609])
def test_column_counts(pkg, gpu, oracle_mod, lw, ncol):
    k, m = lw
    cols = columns(k, ncol)
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu))
    against_oracle(oracle_mod, m, cols, out, ("fsck", ncol, 60))


@pytest.mark.parametrize("nlay", [1, 2])
def test_layer_counts(pkg, gpu, oracle_mod, lw, nlay):
    k, m = lw
    cols = columns(k, 129, nlay)
    for separate in (False, True):
        out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu, separate=separate))
        against_oracle(oracle_mod, m, cols, out, ("fsck", 129, nlay))


@pytest.mark.parametrize("ncol", [129, 4609])
def test_separate_level_arrays(pkg, gpu, oracle_mod, lw, ncol):
    """Two contiguous level arrays: the second store of a level, to lev_source_dec of the next layer."""
    k, m = lw
    cols = columns(k, ncol)
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu, separate=True))
    against_oracle(oracle_mod, m, cols, out, ("fsck", ncol, 60))


@pytest.mark.parametrize("separate", [False, True])
def test_no_tlev(pkg, gpu, oracle_mod, lw, separate):
    """No level stores: tau, lay_source and sfc_source are those of the call with tlev, the level arrays stay as they were."""
    k, m = lw
    cols = columns(k, 513)
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu, separate=separate, tlev=False))
    assert np.all(out[2] == SENTINEL) and np.all(out[3] == SENTINEL)
    pkg.set_solver_option(OPTION, 0)
    ref = gas_call(pkg, k, cols, gpu, separate=separate)
    for i in (0, 1, 4):
        assert same_bits(out[i], ref[i]), NAMES[i]
    against_oracle(oracle_mod, m, cols, ref, ("fsck", 513, 60))


@pytest.mark.parametrize("ncol", [513, 4609])
def test_pressure_spread(pkg, gpu, oracle_mod, lw, ncol):
    """Several slab positions per segment (the source waves store in the first one only), split and masked tau waves."""
    k, m = lw
    pkg.set_solver_option("gas_slab_f32", 0)
    cols = shuffled_orography(k.get_press_min(), ncol)
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu))
    against_oracle(oracle_mod, m, cols, out, ("fsck-orography", ncol, 60))


def test_planck_window(pkg, gpu, oracle_mod, monkeypatch):
    """The 36-g table with a small forced Planck window: source waves on the global-memory path."""
    monkeypatch.setenv("ECCKD_PLANCK_WINDOW", "16")
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_RRTMGP, device=0) == ""
    cols = synthetic.columns(11, 4609, k.get_press_min())
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu))
    against_oracle(oracle_mod, oracle_mod.CkdModel(LW_RRTMGP), cols, out, ("rrtmgp", 4609, 60))


def test_36g_table(pkg, gpu, oracle_mod):
    """The 36-g table as it is planned (chunks of 4 g-points, its own Planck window)."""
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_RRTMGP, device=0) == ""
    cols = synthetic.columns(11, 4609, k.get_press_min())
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu))
    against_oracle(oracle_mod, oracle_mod.CkdModel(LW_RRTMGP), cols, out, ("rrtmgp", 4609, 60))


def test_nan_pressure(pkg, gpu, oracle_mod, lw):
    """The column comes out NaN as the oracle's, and the call returns."""
    k, m = lw
    cols = synthetic.columns(11, 4609, k.get_press_min())
    cols = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in cols.items()}
    cols["plev"][:, 2100] = np.nan
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu))
    against_oracle(oracle_mod, m, cols, out, ("fsck-nan", 4609, 60), nan_cols=[2100])


@pytest.mark.parametrize("tile_sync", [0, 1])
def test_tile_barrier(pkg, gpu, oracle_mod, lw, tile_sync):
    k, m = lw
    pkg.set_solver_option("gas_tile_sync", tile_sync)
    cols = columns(k, 4609)
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu))
    against_oracle(oracle_mod, m, cols, out, ("fsck", 4609, 60))


@pytest.mark.parametrize("slab_f32", [0, 1, 2])
def test_table_image(pkg, gpu, oracle_mod, lw, slab_f32):
    """0: the wave-roles kernel; 1: the float32-image form keeps its own kernel; 2: the probe picks one of the two."""
    k, m = lw
    pkg.set_solver_option("gas_slab_f32", slab_f32)
    for name, cols in (("fsck", columns(k, 4609)), ("fsck-orography", shuffled_orography(k.get_press_min(), 4609))):
        out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu))
        against_oracle(oracle_mod, m, cols, out, (name, 4609, 60))


def test_well_mixed_gases_as_scalars(pkg, gpu, oracle_mod, lw):
    """The merged-slot shape (two bilinear slots)."""
    k, m = lw
    cols = columns(k, 4609)
    overrides = {n: float(np.mean(cols[n])) for n in SCALARS}
    pkg.set_solver_option(OPTION, 1)
    assert k.plan(4609, 60, synthetic.GAS_ORDER, scalar_gases=SCALARS)["slots"] == 2
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu, overrides=overrides))
    against_oracle(oracle_mod, m, cols, out, ("fsck-scalars", 4609, 60), overrides=overrides)


def test_graph_replay(pkg, gpu, oracle_mod, lw):
    k, m = lw
    cols = columns(k, 4609)
    out = roles_keep_the_bits(pkg, lambda: gas_call(pkg, k, cols, gpu, graph=True))
    against_oracle(oracle_mod, m, cols, out, ("fsck", 4609, 60))
