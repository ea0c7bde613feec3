"""CPU tests of the two-stream longwave solver (include/ecckd_hip.h, "Two-stream longwave"): the yardstick of the GPU
tests -- the numpy restatement (tests/lw_2stream_ref.py) against the multi-digit truth in tests/golden/lw_2stream_truth.npz
and in its two closed-form limits -- the refusals of the three new calls and of the two Python keywords in their documented
order (nothing computes on the CPU: host-only models, no device is asked for before the refusal), and the scratch formula."""
import ctypes as C
import inspect
import json
import math
import os
import re

import numpy as np

import __graft_entry__ as entry
import helpers
import lw_2stream_ref as ref
import truth_fixture
from conftest import LW_FSCK, SW_WIDE
from helpers import FLUX_ATOL

SETS = ("cloudy_n1", "cloudy_n2", "cloudy_n8", "cloudy_n61", "thin_n8", "near_conservative_n8", "cutoff_n8")
NLAY, NCOL = 5, 4


def load_fixture():
    z = np.load(os.path.join(helpers.GOLDEN, "lw_2stream_truth.npz"))
    arrays = {k: z[k] for k in z.files}
    meta = json.loads(str(arrays.pop("meta")))
    assert meta["band2gpt"] == truth_fixture.BAND2GPT.tolist()
    return arrays, meta["sets"]


def fixture_set(arrays, name):
    pre = name + "."
    return {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}


def run_restate(a, top_at_1=True):
    return ref.restate(a["tau"], a["ssa"], a["g"], a["inc"], a["dec"], truth_fixture.per_gpt(a["sfc_emis"]), a["sfc_source"],
                       a["inc_flux"], top_at_1)


def test_restatement_lies_within_the_recorded_distances():
    """Every set, both orientations, per g-point and broadband; the sets against the truth within the distance the
    generator recorded, the cutoff set bit for bit (its expected fluxes ARE the restatement's).  The bars: 4 x the distance,
    every cloudy bar at most FLUX_ATOL."""
    arrays, meta = load_fixture()
    assert sorted(meta) == sorted(SETS)
    for name in SETS:
        a, rec = fixture_set(arrays, name), meta[name]
        assert a["tau"].shape == (3, rec["nlay"], 9) and a["up"].shape == (rec["nlay"] + 1, 9)
        up, dn = run_restate(a)
        fu, fd = run_restate(ref.flip_orientation(a), False)
        if rec["against"] == "restate":
            assert rec["bar"] == FLUX_ATOL and np.any((a["tau"] > 0) & (a["tau"] <= ref.TAU_MIN))
            assert np.array_equal(up, a["gpt_up"]) and np.array_equal(dn, a["gpt_dn"])
            assert np.array_equal(ref.broadband(up), a["up"]) and np.array_equal(ref.broadband(dn), a["dn"])
            continue
        dist = max(np.max(np.abs(up - a["gpt_up"])), np.max(np.abs(dn - a["gpt_dn"])),
                   np.max(np.abs(ref.broadband(up) - a["up"])), np.max(np.abs(ref.broadband(dn) - a["dn"])),
                   np.max(np.abs(ref.broadband(fu)[::-1] - a["up"])), np.max(np.abs(ref.broadband(fd)[::-1] - a["dn"])))
        print("%s: restatement %.2e W m-2 from the truth (recorded %.2e, bar %.2e)" % (name, dist, rec["restate_distance"], rec["bar"]))
        assert dist <= rec["restate_distance"] and rec["bar"] == 4.0 * rec["restate_distance"]
        if name.startswith("cloudy"):
            assert rec["bar"] <= FLUX_ATOL
            assert np.any(a["tau"] == 0) or rec["nlay"] == 1
            assert np.all(a["ssa"][:, :, 2] == 0) and np.any(a["inc_flux"] > 0) and np.any(a["inc_flux"] == 0)
            if rec["nlay"] > 1:   # the geometric mean is exercised in the odd columns only
                assert np.any(a["inc"][:, :-1, 1::2] != a["dec"][:, 1:, 1::2]) and np.array_equal(a["inc"][:, :-1, 0::2], a["dec"][:, 1:, 0::2])
        if name.startswith("near"):
            assert 0.3 < np.mean(a["ssa"] == 1.0) < 0.5 and np.max(a["ssa"][a["ssa"] < 1]) > 0.99999
        if name.startswith("thin"):
            assert a["tau"].min() < 3e-6


def test_truth_of_one_small_case_again():
    """The stored truth is what lw_2stream_ref.truth gives today (one g-point of the two-layer set, both orientations)."""
    arrays, _ = load_fixture()
    a = fixture_set(arrays, "cloudy_n2")
    one = {k: (v[:1] if v.ndim >= 2 and v.shape[0] == 3 else v) for k, v in a.items()}
    emis = truth_fixture.per_gpt(a["sfc_emis"])[:1]
    up, dn = ref.truth(one["tau"], one["ssa"], one["g"], one["inc"], one["dec"], emis, one["sfc_source"], one["inc_flux"])
    assert np.array_equal(ref.to_f64(up)[0], a["gpt_up"][0]) and np.array_equal(ref.to_f64(dn)[0], a["gpt_dn"][0])
    f = ref.flip_orientation(one)
    fu, fd = ref.truth(f["tau"], f["ssa"], f["g"], f["inc"], f["dec"], emis, one["sfc_source"], one["inc_flux"], top_at_1=False)
    assert np.array_equal(ref.to_f64(fu)[0, ::-1], a["gpt_up"][0]) and np.array_equal(ref.to_f64(fd)[0, ::-1], a["gpt_dn"][0])


def test_restatement_limits():
    rng = np.random.default_rng(5)
    shape = (3, 7, 6)
    tau, ssa, g = 10.0 ** rng.uniform(-2, 1.3, shape), rng.uniform(0, 0.999, shape), rng.uniform(-0.2, 0.9, shape)
    # an isothermal column over a black surface at the same temperature, lit by pi B from above: pi B everywhere
    B = np.array([3.0, 4.0, 5.5])[:, None, None] * np.ones(shape)
    one = np.ones((3, 6))
    up, dn = ref.restate(tau, ssa, g, B, B, one, B[:, 0], math.pi * B[:, 0])
    want = math.pi * B[:, :1] * np.ones((3, 8, 6))
    assert np.max(np.abs(up / want - 1)) <= 1e-12 and np.max(np.abs(dn / want - 1)) <= 1e-12
    # tau = 0 everywhere passes the boundary values through: Rdif = 0 exactly, Tdif = (1 / (2 k)) * 2 * k * 1 is 1 to an ulp
    # or two, and a level sees it squared once per layer below: 7 layers, some 2e-15 relative -- 1e-13 here
    emis, bsfc, inc = rng.uniform(0.8, 1, (3, 6)), rng.uniform(2, 6, (3, 6)), rng.uniform(0, 20, (3, 6))
    lev = rng.uniform(2, 6, shape)
    for top in (True, False):
        up, dn = ref.restate(np.zeros(shape), ssa, g, lev, lev * 1.01, emis, bsfc, inc, top)
        want_up = (inc * (1 - emis) + math.pi * emis * bsfc)[:, None] * np.ones(up.shape)
        assert np.allclose(dn, inc[:, None] * np.ones(dn.shape), rtol=1e-13, atol=0) and np.allclose(up, want_up, rtol=1e-13, atol=0)


def test_symbols_bindings_and_scratch_formula(pkg):
    L = pkg.lib()
    for s in ("ecckd_rte_lw_2stream", "ecckd_lw_solver_2stream_gpt", "ecckd_rte_lw_2stream_scratch_bytes", "ecckd_lw_fluxes_allsky_2stream"):
        assert s in entry.exported_symbols() and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert len(L.ecckd_rte_lw_2stream.argtypes) == 20 and len(L.ecckd_lw_solver_2stream_gpt.argtypes) == 18
    assert len(L.ecckd_lw_fluxes_allsky_2stream.argtypes) == 25
    # RTE's bind(C) name: exported by the second library, declared in a header of its own that rte_kernels_hip.h includes
    assert hasattr(C.CDLL(pkg.RTE_KERNELS_LIB), "lw_solver_2stream")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "rte_kernels_lw_2stream_hip.h")).read(), flags=re.S)
    assert re.findall(r"\bvoid\s+([A-Za-z0-9_]+)\s*\(", text) == ["lw_solver_2stream"]   # (as entry.rte_kernel_symbols() parses)
    K = C.CDLL(pkg.RTE_KERNELS_LIB)
    for sym in entry.rte_kernel_symbols() + ["lw_solver_2stream"]:   # everything the two headers declare is exported
        assert hasattr(K, sym), sym
    assert '#include "rte_kernels_lw_2stream_hip.h"' in open(os.path.join(inc, "rte_kernels_hip.h")).read()
    assert "kernels_rte_lw_2str.hip" in pkg._SOURCES
    for f in (pkg.rte_lw, pkg.GasOpticsEcckd.lw_fluxes_allsky):
        p = inspect.signature(f).parameters
        assert p["use_2stream"].default is False and list(p)[-2:] == ["use_2stream", "flux_up_jac"]
    # 8 * 2*(nlay+1)*64 * min(ceil(ncol/16), 4096): one ring of two level arrays per wave, whatever ngpt is
    for ncol, nlay, ng in ((1, 1, 3), (16, 60, 32), (17, 61, 5), (37, 137, 27), (65536, 60, 32), (65537, 60, 32), (10**6, 137, 64)):
        want = 8 * 2 * (nlay + 1) * 64 * min(-(-ncol // 16), 4096)
        assert pkg.rte_lw_2stream_scratch_bytes(ncol, nlay, ng) == want, (ncol, nlay, ng)
    assert pkg.rte_lw_2stream_scratch_bytes(0, 60, 32) == 0


def _solver_inputs(pkg, k, dtype=np.float64):
    op = pkg.OpticalProps2str()
    op.alloc_2str(NCOL, NLAY, k, like=np.empty(0, dtype))
    src = pkg.SourceFuncLW()
    src.alloc(NCOL, NLAY, k, like=np.empty(0, dtype))
    for a in (op.tau, op.ssa, op.g, src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source):
        a[:] = 0.5
    return op, src


def test_solver_refusals_before_any_device(pkg):
    """ecckd_rte_lw_2stream and ecckd_lw_solver_2stream_gpt: bad sizes, a null required pointer, a bad band table, a bad
    memspace and ECCKD_MIXED are answered before a device is asked for (this machine may have none); lay_source and inc_flux
    may be NULL.  The keyword of rte_lw refuses what the solver does not serve, each with its message."""
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ng, nb = k.get_ngpt(), k.get_nband()
    op, src = _solver_inputs(pkg, k)
    emis = np.full((NCOL, nb), 0.98)
    up, dn = outs = [np.full((NLAY + 1, NCOL), -7.0) for _ in range(2)]
    untouched = lambda: all(np.all(a == -7.0) for a in outs)
    L = pkg.lib()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    b2g = np.ascontiguousarray(op.band2gpt, dtype=np.int32)
    args = dict(tau=op.tau, ssa=op.ssa, g=op.g, lay=src.lay_source, inc=src.lev_source_inc, dec=src.lev_source_dec,
                sfc=src.sfc_source, emis=emis, incf=None, up=up, dn=dn)

    def raw(ncol=NCOL, nlay=NLAY, ngpt=ng, nband=nb, b2=b2g, memspace=pkg.HOST, dev=0, **kw):
        a = dict(args, **kw)
        return L.ecckd_rte_lw_2stream(dev, ncol, nlay, ngpt, 1, P(a["tau"]), P(a["ssa"]), P(a["g"]), P(a["lay"]), P(a["inc"]),
                                      P(a["dec"]), P(a["sfc"]), nband, P(b2), P(a["emis"]), P(a["incf"]), P(a["up"]), P(a["dn"]),
                                      memspace, None)
    # every later refusal is armed too (memspace 7): the earlier one is the one named
    assert raw(ncol=-1, tau=None, memspace=7) == 1 and "bad ncol/nlay" in pkg.last_error()
    assert raw(nlay=0, tau=None, memspace=7) == 1 and "bad ncol/nlay" in pkg.last_error()
    for name in ("tau", "ssa", "g", "inc", "dec", "sfc", "emis", "up", "dn"):
        assert raw(ngpt=300, memspace=7, **{name: None}) == 1 and "ecckd_rte_lw_2stream: null argument" in pkg.last_error(), name
    assert raw(ngpt=300, memspace=7) == 1 and "ngpt must be in 1..256" in pkg.last_error()
    assert raw(b2=None, memspace=7) == 1 and "bad band description" in pkg.last_error()
    bad = b2g.copy(); bad[0, 0] = 2
    assert raw(b2=bad, memspace=7) == 1 and "band2gpt" in pkg.last_error()
    assert raw(nlay=700, memspace=7) == 1 and "too many layers" in pkg.last_error()
    assert raw(memspace=2) == 1 and "ECCKD_MIXED is not implemented" in pkg.last_error()
    assert raw(memspace=7) == 1 and pkg.last_error() == "ecckd: bad memspace"
    # valid arguments (lay_source and inc_flux NULL): the device is asked for, and there is none or not this one
    assert raw(lay=None, dev=99) == 1 and ("bad device ordinal" in pkg.last_error() or "no HIP device" in pkg.last_error())
    assert untouched()

    e2, s2 = np.full((ng, NCOL), 0.98), np.full((ng, NCOL), 0.5)
    gu, gd = gouts = [np.full((ng, NLAY + 1, NCOL), -7.0) for _ in range(2)]

    def gpt(ncol=NCOL, ngpt=ng, memspace=pkg.HOST, dev=0, **kw):
        a = dict(dict(args, emis=e2, sfc=s2, up=gu, dn=gd), **kw)
        return L.ecckd_lw_solver_2stream_gpt(dev, ncol, NLAY, ngpt, 1, P(a["tau"]), P(a["ssa"]), P(a["g"]), P(a["lay"]), P(a["inc"]),
                                             P(a["dec"]), P(a["emis"]), P(a["sfc"]), P(a["incf"]), P(a["up"]), P(a["dn"]), memspace, None)
    assert gpt(ncol=-1, ngpt=0, tau=None, memspace=7) == 1 and "bad ncol/nlay" in pkg.last_error()
    assert gpt(ngpt=0, tau=None, memspace=7) == 1 and "ecckd_lw_solver_2stream_gpt: bad ngpt" in pkg.last_error()
    for name in ("tau", "ssa", "g", "inc", "dec", "sfc", "emis", "up", "dn"):
        assert gpt(memspace=7, **{name: None}) == 1 and "ecckd_lw_solver_2stream_gpt: null argument" in pkg.last_error(), name
    assert gpt(memspace=2) == 1 and pkg.last_error() == "ecckd: bad memspace"
    assert gpt(lay=None, dev=99) == 1 and ("bad device ordinal" in pkg.last_error() or "no HIP device" in pkg.last_error())
    assert all(np.all(a == -7.0) for a in gouts)

    # the keyword of rte_lw
    fl = pkg.FluxesBroadband(up, dn)
    call = lambda o=op, f=fl, **kw: pkg.rte_lw(o, True, src, emis, f, use_2stream=True, **kw)
    one = pkg.OpticalProps1scl(); one.alloc_1scl(NCOL, NLAY, k)
    assert "two-stream optical properties required" in call(one)
    op32, _ = _solver_inputs(pkg, k, np.float32)
    assert "float64" in call(op32)
    assert "shared_levels" in call(shared_levels=True)
    bnd = [np.zeros((nb, NLAY + 1, NCOL)) for _ in range(2)]
    assert "per-band fluxes" in call(f=pkg.FluxesByband(bnd[0], bnd[1]))
    assert "flux_up_jac" in call(flux_up_jac=np.zeros((NLAY + 1, NCOL)))
    assert "no quadrature" in call(n_gauss_angles=2)
    assert "inc_flux" in call(inc_flux=np.zeros((ng + 1, NCOL))) and "shape" in call(inc_flux=np.zeros((ng + 1, NCOL)))
    m = call(inc_flux=np.zeros((ng, NCOL)), device=99)    # accepted by the mirror: the library asks for the device
    assert "bad device ordinal" in m or "no HIP device" in m
    assert untouched()
    # without the keyword nothing changes: the no-scattering call still answers for itself
    m = pkg.rte_lw(op, True, src, emis, fl, device=99)
    assert "bad device ordinal" in m or "no HIP device" in m


def _wide_model(pkg, ng=65):
    """A host-only model of `ng` g-points with a Planck table (the builder route of tests/test_mcica_host.py)."""
    lp = np.log([10., 100., 1000.])
    T = 200. + np.arange(6).reshape(2, 3)
    k = pkg.GasOpticsEcckd()
    err = k.init_from_tables(lp, T, [dict(name="x", code=1, coefficient=np.ones((2, 3, ng)))],
                             planck=(np.array([100., 200.]), np.ones((2, ng))), device=-1)
    assert err == "", err
    return k


def test_fused_refusals_in_order(pkg):
    """ecckd_lw_fluxes_allsky_2stream on host-only models: cloud_mask with more than 64 g-points; nband_p; tau_p, ssa_p or g_p
    NULL; reference-order arithmetic; no Planck table; tlev NULL; the host-only model -- with every later refusal armed."""
    L = pkg.lib()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    nb = k.get_nband()
    plev, tlay, tsfc, tlev = (np.full((NLAY + 1, NCOL), 1e4), np.full((NLAY, NCOL), 250.), np.full(NCOL, 250.), np.full((NLAY + 1, NCOL), 250.))
    emis = np.full((NCOL, nb), 0.98)
    up, dn = outs = [np.full((NLAY + 1, NCOL), -7.0) for _ in range(2)]
    untouched = lambda: all(np.all(a == -7.0) for a in outs)
    part = [np.full((nb, NLAY, NCOL), 0.5) for _ in range(3)]
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    names = b"h2o".ljust(32, b" ")
    vmr = (C.c_void_p * 1)(None)
    z, sc = (C.c_longlong * 1)(0), (C.c_double * 1)(1e-3)

    def raw(model=k, nband_p=nb, tp=part[0], sp=part[1], gp=part[2], m_=None, tlev_=tlev, memspace=pkg.HOST):
        return L.ecckd_lw_fluxes_allsky_2stream(None if model is None else model._need(), NCOL, NLAY, P(plev), P(tlay), P(tsfc),
                                                P(tlev_), 1, names, vmr, z, z, sc, 1, P(emis), None, nband_p, P(tp), P(sp), P(gp),
                                                P(m_), P(up), P(dn), memspace, None)
    assert raw(model=None) == 1 and "null model" in pkg.last_error()
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        # a 65-g-point model with a Planck table, every later refusal armed (wrong nband_p, NULL tau_p, reference-order mode,
        # NULL tlev): the g-point count is named first; without a mask the same call is answered by the band count
        wide = _wide_model(pkg)
        assert wide.get_ngpt() == 65 and wide.get_nband() != nb + 7
        assert raw(model=wide, nband_p=nb + 7, tp=None, m_=mask, tlev_=None) == 1
        assert "ecckd_lw_fluxes_allsky_2stream" in pkg.last_error() and "at most 64 g-points, not 65" in pkg.last_error()
        assert raw(model=wide, nband_p=nb + 7, tp=None, tlev_=None) == 1 and "nband_p = %d" % (nb + 7) in pkg.last_error()
        assert raw(nband_p=nb + 1, tp=None, tlev_=None) == 1 and "nband_p = %d" % (nb + 1) in pkg.last_error()
        for kw in (dict(tp=None), dict(sp=None), dict(gp=None)):
            assert raw(tlev_=None, **kw) == 1 and "tau_p, ssa_p and g_p are required" in pkg.last_error(), kw
        assert raw(tlev_=None) == 1 and "fast arithmetic mode" in pkg.last_error()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    nbs = ksw.get_nband()
    psw = np.full((nbs, NLAY, NCOL), 0.5)
    assert raw(model=ksw, nband_p=nbs, tp=psw, sp=psw, gp=psw, tlev_=None) == 1 and "no Planck table" in pkg.last_error()
    assert raw(tlev_=None, memspace=7) == 1 and pkg.last_error() == "tlev is required for ecckd"
    for m_ in (None, mask):
        assert raw(m_=m_, memspace=7) == 1 and "no CPU fallback" in pkg.last_error()
    assert untouched() and all(np.all(a == 0.5) for a in part) and np.all(mask == 5)

    # the keyword of lw_fluxes_allsky
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    fl = pkg.FluxesBroadband(up, dn)
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(NCOL, NLAY, k) == ""
    call = lambda p=good, **kw: k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, p, fl, use_2stream=True, **kw)
    one = pkg.OpticalProps1scl(); one.alloc_1scl_bands(NCOL, NLAY, k)
    assert "two-stream optical properties on the model's bands" in call(one)
    nog = pkg.OpticalProps2str(); nog.tau, nog.ssa, nog.g = good.tau, good.ssa, None
    assert "with g" in call(nog)
    assert "flux_up_jac" in call(flux_up_jac=np.zeros((NLAY + 1, NCOL)))
    assert "no quadrature" in call(n_gauss_angles=3)
    short = pkg.OpticalProps2str(); short.tau, short.ssa, short.g = good.tau, good.ssa, good.g[:, 1:]
    assert "particles.g" in call(short)
    assert "uint64" in call(cloud_mask=np.zeros((NLAY, NCOL), dtype=np.int64))
    assert "no CPU fallback" in call() and "no CPU fallback" in call(cloud_mask=mask)
    # without the keyword: the existing call, which ignores g
    assert "no CPU fallback" in k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, nog, fl)
    assert untouched()
