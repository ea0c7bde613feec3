"""Longwave gas optics as two kernels: gas_fused_kernel writes what belongs to a layer (tau, lay_source, lev_source_inc and
the lev_source_dec of the next layer), planck_edge_kernel the two sources that belong to none -- sfc_source and, with tlev,
lev_source_dec of storage layer 0 -- and solver option "gas_input_ahead" loads a tile's per-column inputs one tile ahead.

In fp64 the Planck sources are bit-identical to the CPU oracle's (array_equal) and tau sits at the bar of
tests/test_gpu_parity.py (1e-12 relative).  array_equal against the oracle is an fp64 statement only: the oracle computes in
fp64, so single precision is held to the bars of tests/test_gpu_gas_tile_sync.py (tau 2e-5 relative where it is not tiny,
sources 2e-6), and what is bit-exact there is checked inside the precision -- the same bits with the option at 0, at 1 and
at -1 (every precision), and the edge kernel's planes equal to the main kernel's where the temperatures are equal
(test_both_kernels_interpolate_alike).

Shapes, the smallest at which the split or the tile-ahead loads can go wrong: 1 column (a lone lane), 63 / 64 / 65 (ragged
waves), 512 (exactly one tile: the tile ahead lies wholly beyond the call), 513 (a tile plus one column), 1541 (a ragged
fourth tile), 8705 (17 tiles plus one column: several blocks share a layer, and a block's last tile is followed by
another block's); 1 layer (first and last at once: no lev_source_dec but the edge kernel's), 2 (has_next flips), 3, 60."""
import ctypes as C

import numpy as np
import pytest

import helpers
from helpers import r32
from conftest import LW_FSCK, LW_RRTMGP
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
TAU_RTOL = 1e-12
NCOLS = (1, 63, 64, 65, 512, 513, 1541, 8705)
NLAYS = (1, 2, 3, 60)
OPTIONS = ("gas_input_ahead", "gas_slab_f32", "gas_tile_sync")
FILL = -7.0


@pytest.fixture(autouse=True)
def options_back(pkg):
    saved = {n: pkg.get_solver_option(n) for n in OPTIONS}
    pkg.set_arithmetic(pkg.FAST)
    yield
    for n, v in saved.items():
        pkg.set_solver_option(n, v)


@pytest.fixture(scope="module")
def models(pkg, gpu, oracle_mod):
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = (k, oracle_mod.CkdModel(path))
    return out


_columns = {}


def columns(k, c0, ncol, nlay=60):
    """synthetic.columns, computed once per shape and never written to (copy before editing)."""
    key = (c0, ncol, nlay, k.get_press_min())
    if key not in _columns:
        _columns[key] = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    return _columns[key]


def copied(cols):
    return {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in cols.items()}


def same_bits(a, b):
    """Bit for bit, NaN payloads included."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_gas_optics(pkg, k, cols, device, dtype=np.float64, overrides=None, tlev=True):
    """k.gas_optics on device tensors (or, device None, on host arrays) whose outputs start out as FILL: (tau, lay, inc, dec,
    sfc) as numpy arrays."""
    import torch
    nlay, ncol = cols["tlay"].shape
    ng = k.get_ngpt()
    if device is None:
        to = lambda a: np.ascontiguousarray(a, dtype=dtype)
        back = lambda a: a
    else:
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
        back = lambda a: a.cpu().numpy()
    gc = helpers.product_gas_concs(pkg, cols, to, overrides=overrides)
    op = pkg.OpticalProps1scl()
    op.alloc_1scl(ncol, nlay, k, like=to(np.zeros(1)))
    src = pkg.SourceFuncLW()
    src.alloc(ncol, nlay, k, like=to(np.zeros(1)))
    op.tau = to(np.full((ng, nlay, ncol), FILL))
    src.lay_source, src.lev_source_inc, src.lev_source_dec = (to(np.full((ng, nlay, ncol), FILL)) for _ in range(3))
    src.sfc_source = to(np.full((ng, ncol), FILL))
    err = k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), gc, op, src,
                       tlev=to(cols["tlev"]) if tlev else None)
    # (without tlev the call does its work and then answers as the reference does: src/gas_optics_ecckd.f90:414-417)
    assert err == ("" if tlev else "tlev is required for ecckd")
    torch.cuda.synchronize()
    return [back(a) for a in (op.tau, src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source)]


def every_setting(pkg, run):
    """run() with "gas_input_ahead" at 0, at 1 and at -1 (each mode's shipped default): the same bits in all five arrays;
    returns the outputs of setting 1."""
    out = []
    for v in (0, 1, -1):
        pkg.set_solver_option("gas_input_ahead", v)
        assert pkg.get_solver_option("gas_input_ahead") == v
        out.append(run())
    for other in (out[0], out[2]):
        assert len(other) == len(out[1]) == 5
        for a, b in zip(out[1], other):
            assert same_bits(a, b)
    return out[1]


def check(pkg, k, m, oracle_mod, cols, device, nan_cols=(), overrides=None, tlev=True):
    """fp64: every setting of the option, then setting 1 against the oracle."""
    tau, lay, inc, dec, sfc = every_setting(pkg, lambda: run_gas_optics(pkg, k, cols, device, overrides=overrides, tlev=tlev))
    otau, olay, oinc, odec, osfc, oerr = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"],
                                                                   helpers.oracle_gas_items(cols, overrides=overrides),
                                                                   cols["tlev"] if tlev else None)
    assert oerr == ("" if tlev else "tlev is required for ecckd")
    good = np.ones(tau.shape[-1], bool)
    good[list(nan_cols)] = False
    pairs = [(tau, otau), (lay, olay), (sfc, osfc)]
    if tlev:
        pairs += [(inc, oinc), (dec, odec)]
    else:   # no level temperatures: neither kernel touches the level sources
        assert np.all(inc == FILL) and np.all(dec == FILL)
    for a, b in pairs:
        assert np.array_equal(np.isnan(a), np.isnan(b))          # NaN exactly where the oracle has it
        assert np.all(np.isfinite(a[..., good]))
    for a, b in pairs[1:]:
        assert np.array_equal(a[..., good], b[..., good])
    assert helpers.max_rel(tau[..., good], otau[..., good]) < TAU_RTOL
    assert np.array_equal(tau[..., good] == 0, otau[..., good] == 0)
    return tau, lay, inc, dec, sfc


def shuffled_orography(k, ncol, nlay=60, seed=1):
    """Surface pressures of 50-103 kPa shuffled over the columns, as test_lw_gas_optics_orography spreads them: several
    slab positions per segment, waves split between positions, waves on the tables-from-global-memory path."""
    c = copied(columns(k, 0, ncol, nlay))
    eta = (np.arange(nlay + 1, dtype=np.float64) / nlay) ** 2
    ptop = c["plev"][0, 0]
    ps = 50000 + 53000 * np.random.default_rng(seed).random(ncol)
    c["plev"] = np.ascontiguousarray(ptop + (ps[None, :] - ptop) * eta[:, None])
    return c


def test_option_is_listed_and_checked(pkg, gpu):
    assert "gas_input_ahead" in pkg.solver_options()
    assert pkg.get_solver_option("gas_input_ahead") == -1
    for bad in (2, -2, 0.5):
        with pytest.raises(ValueError):
            pkg.set_solver_option("gas_input_ahead", bad)


@pytest.mark.parametrize("nlay", NLAYS)
@pytest.mark.parametrize("ncol", NCOLS)
def test_shapes(pkg, gpu, oracle_mod, models, ncol, nlay):
    k, m = models["fsck"]
    check(pkg, k, m, oracle_mod, columns(k, 7, ncol, nlay), gpu)


@pytest.mark.parametrize("nlay", [1, 2, 60])
@pytest.mark.parametrize("ncol", [65, 513, 1541])
def test_table_with_planck_window(pkg, gpu, oracle_mod, models, ncol, nlay):
    """The 36-g table: a window of the Planck table in LDS; the edge kernel reads the table's rows from memory."""
    k, m = models["rrtmgp"]
    check(pkg, k, m, oracle_mod, columns(k, 11, ncol, nlay), gpu)


@pytest.mark.parametrize("table", ["fsck", "rrtmgp"])
@pytest.mark.parametrize("nlay", [2, 60])
def test_forced_planck_window(pkg, gpu, oracle_mod, monkeypatch, table, nlay):
    """A window of 16 rows: most waves take the tables-from-global-memory path, which lost its first-layer branch too."""
    monkeypatch.setenv("ECCKD_PLANCK_WINDOW", "16")
    k = pkg.GasOpticsEcckd()
    path = LW_FSCK if table == "fsck" else LW_RRTMGP
    assert k.load(path, device=0) == ""
    check(pkg, k, oracle_mod.CkdModel(path), oracle_mod, columns(k, 11, 1541, nlay), gpu)


@pytest.mark.parametrize("nlay", [1, 2, 60])
@pytest.mark.parametrize("ncol", [65, 513, 1541])
def test_single_precision(pkg, gpu, oracle_mod, models, ncol, nlay):
    """The columns and bars of tests/test_gpu_gas_tile_sync.py::test_lw_single_precision (generator columns 3 .. 702,
    repeated to fill the call), at every setting of the option."""
    k, m = models["fsck"]
    cols = columns(k, 3, 700, nlay)
    idx = np.arange(ncol) % 700
    cols = {n: (np.ascontiguousarray(v[..., idx]) if isinstance(v, np.ndarray) else v) for n, v in cols.items()}
    c32 = {n: (r32(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for n, v in cols.items()}
    tau, lay, inc, dec, sfc = every_setting(pkg, lambda: run_gas_optics(pkg, k, c32, gpu, dtype=np.float32))
    assert tau.dtype == np.float32 and sfc.dtype == np.float32
    otau, olay, oinc, odec, osfc, _ = oracle_mod.gas_optics_int(m, c32["plev"], c32["tlay"], c32["tsfc"],
                                                               helpers.oracle_gas_items(c32), c32["tlev"])
    big = otau > 1e-6 * otau.max()
    assert np.max(np.abs(tau.astype(np.float64) - otau)[big] / otau[big]) < 2e-5
    for a, b in ((lay, olay), (inc, oinc), (dec, odec), (sfc, osfc)):
        assert helpers.max_rel(a, b) < 2e-6


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nlay", [1, 60])
def test_both_kernels_interpolate_alike(pkg, gpu, models, dtype, nlay):
    """Where the top level, the level below it and the surface have the same temperature, the edge kernel's two planes hold
    the bits of the main kernel's lev_source_inc of layer 0: one interpolation, in either precision."""
    k, _ = models["fsck"]
    cols = copied(columns(k, 5, 1541, nlay))
    cols["tlev"][0] = cols["tlev"][1]
    cols["tsfc"] = cols["tlev"][1].copy()
    if dtype == np.float32:
        cols = {n: (r32(v) if isinstance(v, np.ndarray) else float(np.float32(v))) for n, v in cols.items()}
    tau, lay, inc, dec, sfc = every_setting(pkg, lambda: run_gas_optics(pkg, k, cols, gpu, dtype=dtype))
    assert same_bits(dec[:, 0], inc[:, 0]) and same_bits(sfc, inc[:, 0])
    if nlay > 1:
        assert same_bits(dec[:, 1:], inc[:, :-1])


@pytest.mark.parametrize("nlay", [1, 60])
@pytest.mark.parametrize("ncol", [65, 513])
def test_without_level_temperatures(pkg, gpu, oracle_mod, models, ncol, nlay):
    k, m = models["fsck"]
    check(pkg, k, m, oracle_mod, columns(k, 7, ncol, nlay), gpu, tlev=False)


@pytest.mark.parametrize("form", ["columns", "scalars", "full"])
def test_well_mixed_gas_forms(pkg, gpu, oracle_mod, models, form):
    """The well-mixed gases as per-column arrays (the generator's), as scalars (they share the merged slot: another
    instantiation) and as full (nlay, ncol) arrays."""
    k, m = models["fsck"]
    cols = columns(k, 7, 1541)
    ov = None
    if form == "scalars":
        ov = dict(helpers.WELL_MIXED)
    elif form == "full":
        ov = {n: np.ascontiguousarray(np.repeat(cols[n][None, :], 60, 0) * np.linspace(1.0, 1.1, 60)[:, None])
              for n in ("co2", "ch4", "n2o", "cfc11", "cfc12")}
    check(pkg, k, m, oracle_mod, cols, gpu, overrides=ov)


@pytest.mark.parametrize("slab_f32", [0, 1, 2])
@pytest.mark.parametrize("ncol", [1541, 8705])
def test_orography(pkg, gpu, oracle_mod, models, ncol, slab_f32):
    """Slab-position passes and the slow path, over the fp64 slab, the float32 image and the probe's choice of the two
    (both forms are launched then; the edge kernel once)."""
    k, m = models["fsck"]
    pkg.set_solver_option("gas_slab_f32", slab_f32)
    check(pkg, k, m, oracle_mod, shuffled_orography(k, ncol), gpu)


@pytest.mark.parametrize("slab_f32", [0, 1, 2])
def test_slab_forms_on_plain_columns(pkg, gpu, oracle_mod, models, slab_f32):
    k, m = models["fsck"]
    pkg.set_solver_option("gas_slab_f32", slab_f32)
    check(pkg, k, m, oracle_mod, columns(k, 7, 1541, 3), gpu)


def test_nan_pressure(pkg, gpu, oracle_mod, models):
    """A NaN pressure sends its wave down the stray-wave path; the column's tau is NaN where the oracle's is, and the edge
    kernel, which reads no pressure, gives the column its surface and top-level sources."""
    k, m = models["fsck"]
    cols = copied(columns(k, 11, 1541))
    cols["plev"][:, 1100] = np.nan
    check(pkg, k, m, oracle_mod, cols, gpu, nan_cols=[1100])


@pytest.mark.parametrize("ncol", [65, 1541])
def test_host_arrays(pkg, gpu, oracle_mod, models, ncol):
    k, m = models["fsck"]
    check(pkg, k, m, oracle_mod, columns(k, 7, ncol, 3), None)


def test_mixed_memory_space(pkg, gpu, oracle_mod, models):
    """ECCKD_MIXED through the C ABI: host inputs, device-resident spectral arrays."""
    import torch
    k, m = models["fsck"]
    L = pkg.lib()
    ncol, nlay, ng = 1541, 3, k.get_ngpt()
    cols = columns(k, 7, ncol, nlay)
    host = {n: np.ascontiguousarray(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev")}
    gc = helpers.product_gas_concs(pkg, cols, np.ascontiguousarray)
    n, names, ptrs, cs, ls, sc, keep = k._gas_args(gc, ncol, nlay, pkg.HOST)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    dp = lambda a: C.c_void_p(a.data_ptr())

    def run():
        big = [torch.full((ng, nlay, ncol), FILL, dtype=torch.float64, device=gpu) for _ in range(4)]
        big.append(torch.full((ng, ncol), FILL, dtype=torch.float64, device=gpu))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.ecckd_gas_optics_lw(k._need(), ncol, nlay, hp(host["plev"]), hp(host["tlay"]), hp(host["tsfc"]), hp(host["tlev"]),
                                     n, names, ptrs, cs, ls, sc, *[dp(x) for x in big], pkg.MIXED, st) == 0, pkg.last_error()
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in big]

    tau, lay, inc, dec, sfc = every_setting(pkg, run)
    otau, olay, oinc, odec, osfc, oerr = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"],
                                                                   helpers.oracle_gas_items(cols), cols["tlev"])
    assert oerr == ""
    for a, b in ((lay, olay), (inc, oinc), (dec, odec), (sfc, osfc)):
        assert np.array_equal(a, b)
    assert helpers.max_rel(tau, otau) < TAU_RTOL


@pytest.mark.parametrize("ahead", [0, 1])
def test_graph_capture_and_replay(pkg, gpu, oracle_mod, models, ahead):
    """gas_optics captured on a side stream after one warm-up call there: both kernels are in the graph."""
    import torch
    k, m = models["fsck"]
    pkg.set_solver_option("gas_input_ahead", ahead)
    ncol, nlay, ng = 1541, 60, k.get_ngpt()
    cols = columns(k, 7, ncol, nlay)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    gc = helpers.product_gas_concs(pkg, cols, to)
    plev, tlay, tsfc, tlev = (to(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev"))
    op = pkg.OpticalProps1scl()
    op.alloc_1scl(ncol, nlay, k, like=plev)
    src = pkg.SourceFuncLW()
    src.alloc(ncol, nlay, k, like=plev)
    outs = lambda: (op.tau, src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source)

    def step():
        assert k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tlev) == ""

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    ref = [a.clone() for a in outs()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for a in outs():
        a.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs(), ref):
        assert torch.equal(a, b)
    odec, osfc = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], helpers.oracle_gas_items(cols), cols["tlev"])[3:5]
    assert np.array_equal(src.lev_source_dec.cpu().numpy(), odec) and np.array_equal(src.sfc_source.cpu().numpy(), osfc)
    del graph
