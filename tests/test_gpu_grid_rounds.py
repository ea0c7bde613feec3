"""Every flux-solver family but the layer-split longwave one (tests/test_gpu_lw_split_stride.py) past one round of its grid:
a block or wave takes a second tile by grid stride, clears its LDS accumulators, reuses its scratch ring and recomputes every
per-tile index (mask word, band plane, scaling factor), and the last tile is ragged -- while the small call of the same entry
point takes the other route (tail units of one g-point or g-point group per block).

A column's fluxes do not depend on where the column sits, so there is no yardstick and no tolerance: each form is called
once on NSMALL = 97 distinct columns (coprime to the tile widths 16, 32 and 64: every lane position of every tile sees every
column) and once on those columns repeated cyclically to ncol columns, and every output array of the large call must hold
the small call's column i % 97 bit for bit (compared as int64 / int32).  The large inputs are built on the device by
indexing the small ones; the McICA mask and the scaling factors are inputs like any other (the samplers depend on the
global column).  Outputs are prefilled with -1.

ncol per family, from the launchers' constants (cus = the device's compute units, read at run time; 256 on an MI355X):

  systolic shortwave -- kernels_rte_sw_sys.hip, rte_sw_sys_plan (l. 612) and launch_rte_sw_sys (l. 629): tiles of 64 columns,
    min(units, cus) blocks.  ncol = 2*cus*64 + 64 + 37 (32 869): 2*cus + 2 tiles, full = 2*cus, so every block walks two whole
    tiles in the `unit` loop (l. 204) and the two tail tiles (one of 37 columns) go out as 2*ng one-g-point units, of which the
    first blocks take a third unit.  97 columns: 2 tiles, full = 0: tail units only.
  two-pass shortwave -- kernels_rte_sw.hip, kSwWaves = 4096 (l. 44/60), ECCKD_SW_CW = 16 (l. 54), launch_rte_sw (l. 453):
    ncol = 4096*16 + 16 + 5 (65 557): 4 098 tiles on 4 096 blocks, blocks 0 and 1 take a second tile, the last of 5 columns;
    rte_sw_tail_plan (l. 408) returns 0 (`full > 0`, l. 421): whole-tile blocks only.  97 columns: 7 tiles, full = 0, the
    gain test passes and the partial sums are small: every tile is split into g-point groups.
  two-stream longwave -- kernels_rte_lw_2str.hip, kL2Waves = 4096 (l. 36), kL2CW = 16 (l. 38), l2_blocks (l. 225), tile loop
    l. 70, ring `sc` per block (l. 65): ncol = 4096*16 + 16 + 5 (65 557), blocks 0 and 1 take a second tile on the same ring.
    97 columns: 7 blocks of one tile (this family has no tail split).
  float32 longwave, register forms -- kernels_rte_lw.hip, launch_ser (l. 147: one block per unit, no cap), rte_lw_tail_plan
    (l. 208), ECCKD_LW_CW_F32 = 32 (l. 56), slots = 4*cus SIMDs (capi.cpp simd_slots, l. 167): ncol = 4*cus*32 + 32 + 5
    (32 805): 4*cus + 2 tiles, full = 4*cus whole-tile waves (the route no small call takes: below 4*cus tiles full = 0) and two
    tail tiles as one-iteration units.  97 columns: 4 tiles, all tail units.  The fp64 general route (ECCKD_LW_CW = 32, l. 53)
    has the same plan and takes the same count.
  float32 longwave, overflow form (more than kMaxRegisterLayers = 96 layers, l. 143) -- kOverWaves = 2048 (l. 142), kOverCW =
    16 (l. 144), launch_ser l. 157, unit loop rte_lw_body.inc l. 52, ring per block l. 69: ncol = 2048*16 + 16 + 5 (32 789):
    2 050 tiles on 2 048 blocks, blocks 0 and 1 take a second tile on the same ring.  97 columns: 7 blocks of one tile.
  stand-alone Jacobian kernels -- kernels_rte_lw_jac.hip, launch_jac_kernel (l. 219): kJacCW = 32 (l. 37), cap 256*64 =
    16 384 blocks (l. 227): ncol = 16384*32 + 32 + 5 (524 325): blocks 0 and 1 take a second tile.  97 columns: 4 blocks.
    The instantiations that read band planes and mask words (l. 114-122) run only behind the 60-layer fused calls with
    "lw_jac_inline" 0: those six cases are the large ones of this module, 8.05 GB of optical depth each (see CASES, 5.).

The sum_planes kernel behind the per-band calls (kernels_rte_sw.hip l. 516: 4 096 blocks of 256) is taken past its cap by
the by-band cases: 61 levels x 32 869 columns = 2 005 009 values > 1 048 576.

Measured on an MI355X: 0 of N values differ in every output of every case (the cases print their counts).

Sensitivity, shown once on scratch builds.  (a) The statement that clears the accumulators made to run for a block's first
tile only -- `acc[i] = 0.` at the top of the unit loop of rte_sw_body (kernels_rte_sw.hip l. 141), of the tile loop of
rte_lw_2str_body (l. 74) and of the unit loop of rte_lw_body.inc (l. 64), the three `acc_* = 0.` of rte_sw_sys_kernel
(l. 221-223) -- and the `acc[i] = 0.` behind the Jacobian kernels' store (kernels_rte_lw_jac.hip l. 165) taken out: every
case of the systolic, two-pass, two-stream, overflow and Jacobian families failed (two-pass clear sky: 1 302 of 4 064 534
values per output, the 21 columns of the two second tiles; rte_lw_jac: 111 of 1 572 975 in flux_up_jac); the 9 register-form
longwave cases passed, whose waves never take a second tile -- they guard the tile and tail-unit arithmetic of the
whole-tile route instead (the six 60-layer Jacobian cases were run under (b) and (c) only).  (b) In the Jacobian kernel, `a.part_tau[q2 + qb]` (l. 114) and `a.part_mask[q2]` (l. 116) read at
the column of the block's FIRST tile: the six 60-layer cases failed (1 512 of 31 983 825 values of flux_up_jac) and the
array and 2-layer cases passed, as they must: they run the instantiation without particles.  (c) The mask word alone (l. 116):
exactly the three masked 60-layer cases failed (972 values)."""
import numpy as np
import pytest

import helpers
import stride_helpers
import test_gpu_allsky as swt
import test_gpu_lw_allsky as lwt
import test_gpu_lw_rescaled as rsc
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
NSMALL, C0 = 97, 11
OPTIONS = ("sw_solver", "sw_tail_split", "lw_tail_split", "lw_solver", "lw_both_skies", "lw_jac_inline")


def ncol_of(family):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"sw_sys": 2 * cus * 64 + 64 + 37, "sw_2pass": 4096 * 16 + 16 + 5, "lw_2str": 4096 * 16 + 16 + 5,
            "lw_reg": 4 * cus * 32 + 32 + 5, "lw_over": 2048 * 16 + 16 + 5, "lw_jac": 16384 * 32 + 32 + 5}[family]


@pytest.fixture(autouse=True)
def options(pkg):
    saved = [pkg.get_solver_option(n) for n in OPTIONS]
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    for n, v in zip(OPTIONS, saved):
        pkg.set_solver_option(n, v)


# ------------------------------------------------------------------------------------------------
# the 97 columns on the device, per kind of input
# ------------------------------------------------------------------------------------------------
def on_device(gpu, cols, cloud, mask, extra=()):
    t = lwt.T(gpu)
    d = {n: (v if np.isscalar(v) else t(v)) for n, v in cols.items()}
    d.update({"part_" + n: t(cloud[n]) for n in ("tau", "ssa", "g")})
    d["mask"] = t(mask.view(np.int64))
    d.update({n: t(v) for n, v in extra})
    assert float(d["part_ssa"].max()) > 0.0
    return d


def sampled_mask(pkg, nlay, ng):
    """The McICA mask of the 97 columns, sampled once: an input of both calls."""
    mask = pkg.sample_cloud_mask(np.ascontiguousarray(synthetic.cloud_fraction(C0, NSMALL, nlay)), ng, seed=C0)
    assert np.any(mask != 0) and np.any(mask != np.uint64(2 ** ng - 1))   # clear and cloudy bits
    return mask


def single(d):
    """The float32 image of a float64 input set (the mask keeps its words)."""
    import torch
    return {n: (v.to(torch.float32) if hasattr(v, "dtype") and v.dtype == torch.float64 else v) for n, v in d.items()}


class Inputs:
    """The models and the small input sets, each made once per module."""

    def __init__(self, pkg, gpu):
        from conftest import LW_FSCK, SW_WIDE
        self.pkg, self.gpu, self.sets = pkg, gpu, {}
        self.sw, self.lw = pkg.GasOpticsEcckd(), pkg.GasOpticsEcckd()
        assert self.sw.load(SW_WIDE, device=0) == "" and self.lw.load(LW_FSCK, device=0) == ""
        assert self.sw.get_ngpt() == 27 and self.lw.get_ngpt() == 32

    def get(self, kind, *key):
        full = (kind,) + key
        if full not in self.sets:
            self.sets[full] = getattr(self, kind)(*key)
        return self.sets[full]

    def sw_fused(self, nlay, f32):
        """(model, atmosphere + albedos + beam scaling + two-stream cloud on the bands + mask + optical-depth scaling).  The
        bottom-up cases run on the same arrays: the gas optics takes plev(l+1) - plev(l) as the layer mass whatever top_at_1
        says, so reversed profiles would give NaN fluxes; only the solver walks the other way, through an atmosphere that
        stands on its head -- finite fluxes, and every index of the bottom-up walk is used."""
        if f32:
            return self.sw, single(self.get("sw_fused", nlay, False)[1])
        k = self.sw
        cols, cloud = swt.sw_case(k, C0, NSMALL, nlay, NSMALL + nlay)
        assert cloud["cloudy"].any() and not cloud["cloudy"].all()
        rng = np.random.default_rng(nlay)
        shape = (k.get_ngpt(), nlay, NSMALL)
        scaling = np.where(rng.uniform(size=shape) < 0.3, 0.0, rng.uniform(0.0, 2.5, shape)).astype(np.float32)
        return k, on_device(self.gpu, cols, cloud, sampled_mask(self.pkg, nlay, k.get_ngpt()), (("scaling", scaling),))

    def lw_fused(self, nlay, f32):
        if f32:
            return self.lw, single(self.get("lw_fused", nlay, False)[1])
        k = self.lw
        cols, cloud = lwt.case(k, C0, NSMALL, nlay)
        assert cloud["cloudy"].any() and not cloud["cloudy"].all()
        return k, on_device(self.gpu, cols, cloud, sampled_mask(self.pkg, nlay, k.get_ngpt()))

    def sw_arrays(self, ng, nlay, f32):
        if f32:
            return None, single(self.get("sw_arrays", ng, nlay, False)[1])
        rng = np.random.default_rng(ng + nlay)
        shape, t = (ng, nlay, NSMALL), lwt.T(self.gpu)
        a = dict(tau=rng.uniform(0.001, 2.0, shape), ssa=rng.uniform(0.0, 0.999, shape),
                 g=rng.uniform(0.0, 0.8, shape) * (rng.uniform(size=(1, 1, NSMALL)) < 0.5), mu0=rng.uniform(0.05, 1.0, NSMALL),
                 toa=rng.uniform(10, 100, (ng, NSMALL)), alb_dir=rng.uniform(0.05, 0.4, (NSMALL, 2)),
                 alb_dif=rng.uniform(0.05, 0.4, (NSMALL, 2)))
        d = {n: t(v) for n, v in a.items()}
        d["band2gpt"] = np.array([[1, ng // 2], [ng // 2 + 1, ng]], dtype=np.int32)
        assert float(d["ssa"].max()) > 0.0
        return None, d

    def lw_arrays(self, ng, nlay):
        a = rsc.random_case(NSMALL, nlay, ng, 2, ng + nlay)
        a["sfc_jac"] = np.random.default_rng(ng).uniform(0.01, 0.2, (ng, NSMALL))
        a["emis"] = a.pop("sfc_emis")
        t = lwt.T(self.gpu)
        d = {n: t(v) for n, v in a.items()}
        d["band2gpt"] = np.array([[1, ng // 2], [ng // 2 + 1, ng]], dtype=np.int32)
        assert float(d["ssa"].max()) > 0.0
        return None, d


@pytest.fixture(scope="module")
def inputs(pkg, gpu):
    return Inputs(pkg, gpu)


def particles(pkg, d, one_stream=False):
    if one_stream:
        op = pkg.OpticalProps1scl()
        op.tau = d["part_tau"]
        return op
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = d["part_tau"], d["part_ssa"], d["part_g"]
    return op


def new(d, planes=None, like="plev"):
    nlay = (d["tlay"] if "tlay" in d else d["tau"]).shape[-2]
    return stride_helpers.new(d, nlay, planes=planes, like=like)


# ------------------------------------------------------------------------------------------------
# the forms: (pkg, k, d) -> list of output tensors.  None of them looks at the column count.
# ------------------------------------------------------------------------------------------------
def sw_head(pkg, d, top_at_1):
    return (d["plev"], d["tlay"], helpers.product_gas_concs(pkg, d, names=helpers.SW_NAMES), top_at_1, d["mu0"], d["alb_dir"],
            d["alb_dif"])


def sw3(pkg, d):
    return pkg.FluxesBroadband(new(d), new(d), new(d))


def out3(fl):
    return [fl.flux_up, fl.flux_dn, fl.flux_dn_dir]


def sw_clear(top_at_1=True):
    def form(pkg, k, d):
        fl = sw3(pkg, d)
        assert k.sw_fluxes(*sw_head(pkg, d, top_at_1), fl, toa_scale=d["scale"]) == ""
        return out3(fl)
    return form


def sw_allsky(delta, masked=False, top_at_1=True):
    def form(pkg, k, d):
        fl = sw3(pkg, d)
        assert k.sw_fluxes_allsky(*sw_head(pkg, d, top_at_1), particles(pkg, d), fl, delta_scale=delta, toa_scale=d["scale"],
                                  cloud_mask=d["mask"] if masked else None) == ""
        return out3(fl)
    return form


def sw_both(top_at_1=True):
    def form(pkg, k, d):
        fl, fc = sw3(pkg, d), sw3(pkg, d)
        assert k.sw_fluxes_clear_allsky(*sw_head(pkg, d, top_at_1), particles(pkg, d), fl, fc, toa_scale=d["scale"],
                                        cloud_mask=d["mask"]) == ""
        return out3(fl) + out3(fc)
    return form


def sw_byband(top_at_1=True):
    def form(pkg, k, d):
        nb = k.get_nband()
        fl = pkg.FluxesByband(new(d, nb), new(d, nb), new(d, nb), new(d), new(d), new(d))
        assert k.sw_fluxes_byband(*sw_head(pkg, d, top_at_1), fl, particles=particles(pkg, d), toa_scale=d["scale"],
                                  cloud_mask=d["mask"]) == ""
        return out3(fl) + [fl.bnd_flux_up, fl.bnd_flux_dn, fl.bnd_flux_dn_dir]
    return form


def sw_scaled(top_at_1=True):
    def form(pkg, k, d):
        fl = sw3(pkg, d)
        assert k.sw_flux_scaled(*sw_head(pkg, d, top_at_1), particles(pkg, d), fl, d["scaling"], toa_scale=d["scale"]) == ""
        return out3(fl)
    return form


def sw_arrays(arith=0, top_at_1=True):
    def form(pkg, k, d):
        pkg.set_arithmetic(arith)
        op = pkg.OpticalProps2str()
        op.tau, op.ssa, op.g, op.band2gpt = d["tau"], d["ssa"], d["g"], d["band2gpt"]
        fl = pkg.FluxesBroadband(*(new(d, like="tau") for _ in range(3)))
        assert pkg.rte_sw(op, top_at_1, d["mu0"], d["toa"], d["alb_dir"], d["alb_dif"], fl) == ""
        return out3(fl)
    return form


def lw_head(pkg, d, top_at_1=True):
    return (d["plev"], d["tlay"], d["tsfc"], d["tlev"], helpers.product_gas_concs(pkg, d), top_at_1, d["emis"])


def lw2(pkg, d):
    return pkg.FluxesBroadband(new(d), new(d))


def out2(fl):
    return [fl.flux_up, fl.flux_dn]


def lw_clear(nmus=2):
    def form(pkg, k, d):
        fl = lw2(pkg, d)
        assert k.lw_fluxes(*lw_head(pkg, d), fl, n_gauss_angles=nmus, inc_flux=d["inc_flux"]) == ""
        return out2(fl)
    return form


def lw_allsky(masked=False, nmus=2, **kw):
    def form(pkg, k, d):
        fl = lw2(pkg, d)
        assert k.lw_fluxes_allsky(*lw_head(pkg, d), particles(pkg, d), fl, n_gauss_angles=nmus, inc_flux=d["inc_flux"],
                                  cloud_mask=d["mask"] if masked else None, **kw) == ""
        return out2(fl)
    return form


def lw_both(pkg, k, d):
    fl, fc = lw2(pkg, d), lw2(pkg, d)
    assert k.lw_fluxes_clear_allsky(*lw_head(pkg, d), particles(pkg, d), fl, fc, n_gauss_angles=2, inc_flux=d["inc_flux"],
                                    cloud_mask=d["mask"]) == ""
    return out2(fl) + out2(fc)


def lw_jac_fused(masked, one_stream=False):
    def form(pkg, k, d):
        pkg.set_solver_option("lw_jac_inline", 0)
        fl, jac = lw2(pkg, d), new(d)
        assert k.lw_fluxes_allsky(*lw_head(pkg, d), particles(pkg, d, one_stream), fl, n_gauss_angles=2, inc_flux=d["inc_flux"],
                                  cloud_mask=d["mask"] if masked else None, flux_up_jac=jac) == ""
        return out2(fl) + [jac]
    return form


def lw_rescaled_jac_fused(masked):
    def form(pkg, k, d):
        pkg.set_solver_option("lw_jac_inline", 0)
        fl, jac = lw2(pkg, d), new(d)
        assert k.lw_fluxes_rescaled(*lw_head(pkg, d), particles(pkg, d), fl, flux_up_jac=jac, n_gauss_angles=2, inc_flux=d["inc_flux"],
                                    cloud_mask=d["mask"] if masked else None) == ""
        return out2(fl) + [jac]
    return form


def lw_sources(pkg, d):
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = d["lay"], d["inc"], d["dec"], d["sfc_source"]
    src.sfc_source_jac = d["sfc_jac"]
    return src


def lw_cells(pkg, d, two=True):
    op = pkg.OpticalProps2str() if two else pkg.OpticalProps1scl()
    op.tau, op.band2gpt = d["tau"], d["band2gpt"]
    if two:
        op.ssa, op.g = d["ssa"], d["g"]
    return op


def lw_2str_arrays(top_at_1):
    def form(pkg, k, d):
        fl = pkg.FluxesBroadband(new(d, like="tau"), new(d, like="tau"))
        assert pkg.rte_lw(lw_cells(pkg, d), top_at_1, lw_sources(pkg, d), d["emis"], fl, inc_flux=d["inc_flux"], use_2stream=True) == ""
        return out2(fl)
    return form


def lw_jac_arrays(pkg, k, d):
    fl, jac = pkg.FluxesBroadband(new(d, like="tau"), new(d, like="tau")), new(d, like="tau")
    assert pkg.rte_lw(lw_cells(pkg, d, False), True, lw_sources(pkg, d), d["emis"], fl, n_gauss_angles=2, inc_flux=d["inc_flux"],
                      flux_up_jac=jac) == ""
    return out2(fl) + [jac]


def lw_rescaled_jac_arrays(pkg, k, d):
    fl, jac = pkg.FluxesBroadband(new(d, like="tau"), new(d, like="tau")), new(d, like="tau")
    assert pkg.rte_lw_rescaled_jac(lw_cells(pkg, d), True, lw_sources(pkg, d), d["emis"], fl, jac, n_gauss_angles=2,
                                   inc_flux=d["inc_flux"]) == ""
    return out2(fl) + [jac]


# ------------------------------------------------------------------------------------------------
# the cases: (id, family, input set, form, the clear-sky form its first output must differ from, options)
# ------------------------------------------------------------------------------------------------
SW_FUSED_READS = lambda n: n not in ("scaling", "tlev", "tsfc", "albedo", "sfc_emis")
SW_SCALED_READS = lambda n: n not in ("tlev", "tsfc", "albedo", "sfc_emis")
LW_FUSED_READS = lambda n: n != "sfc_emis"
ALL = lambda n: True


def sw_list(family, nlay, opts, tag, with_scaled):
    """The fused shortwave forms and the array form of one solver at one layer count."""
    fp64, fp32 = ("sw_fused", nlay, False), ("sw_fused", nlay, True)
    cases = [
        ("sw_fluxes", fp64, sw_clear(), None),
        ("sw_fluxes_allsky_delta", fp64, sw_allsky(True), sw_clear()),
        ("sw_fluxes_allsky_nodelta", fp64, sw_allsky(False), sw_clear()),
        ("sw_fluxes_allsky_mcica_bottom_up", fp64, sw_allsky(True, True, False), sw_clear(False)),
        ("sw_fluxes_clear_allsky", fp64, sw_both(), sw_clear()),
        ("sw_fluxes_allsky_f32", fp32, sw_allsky(True), sw_clear()),
        ("sw_fluxes_allsky_mcica_f32", fp32, sw_allsky(True, True), sw_clear()),
        ("sw_fluxes_clear_allsky_f32_bottom_up", fp32, sw_both(False), sw_clear(False)),
        ("sw_fluxes_byband_mcica", fp64, sw_byband(), sw_clear()),
    ]
    if with_scaled:
        cases.append(("sw_flux_scaled", fp64, sw_scaled(), sw_clear()))
    return [(tag + name, family, key, form, clear, opts, SW_SCALED_READS if name == "sw_flux_scaled" else SW_FUSED_READS)
            for name, key, form, clear in cases]


TWO_PASS = {"sw_solver": 1}
CASES = (
    # 1. layer-systolic shortwave (60 layers and fewer, "sw_solver" 0)
    sw_list("sw_sys", 60, {}, "sys_", False) + [
        ("sys_rte_sw", "sw_sys", ("sw_arrays", 5, 12, False), sw_arrays(), None, {}, ALL),
        ("sys_rte_sw_f32_bottom_up", "sw_sys", ("sw_arrays", 6, 10, True), sw_arrays(0, False), None, {}, ALL)]
    # 2. two-pass shortwave: 61 layers, and 60 layers with "sw_solver" 1
    + sw_list("sw_2pass", 61, {}, "two_pass_61_", True) + sw_list("sw_2pass", 60, TWO_PASS, "two_pass_60_", True) + [
        ("two_pass_rte_sw", "sw_2pass", ("sw_arrays", 5, 12, False), sw_arrays(0), None, TWO_PASS, ALL),
        ("two_pass_rte_sw_reference_order", "sw_2pass", ("sw_arrays", 5, 12, False), sw_arrays(1, False), None, TWO_PASS, ALL),
        ("two_pass_rte_sw_f32", "sw_2pass", ("sw_arrays", 6, 10, True), sw_arrays(0), None, TWO_PASS, ALL),
        ("two_pass_rte_sw_f32_reference_order", "sw_2pass", ("sw_arrays", 6, 10, True), sw_arrays(1), None, TWO_PASS, ALL)]
    # 3. two-stream longwave
    + [("rte_lw_2stream_5g_8lay", "lw_2str", ("lw_arrays", 5, 8), lw_2str_arrays(True), None, {}, ALL),
       ("rte_lw_2stream_3g_61lay_bottom_up", "lw_2str", ("lw_arrays", 3, 61), lw_2str_arrays(False), None, {}, ALL),
       ("lw_fluxes_allsky_2stream", "lw_2str", ("lw_fused", 20, False), lw_allsky(False, 1, use_2stream=True), lw_clear(1), {},
        LW_FUSED_READS),
       ("lw_fluxes_allsky_2stream_mcica", "lw_2str", ("lw_fused", 20, False), lw_allsky(True, 1, use_2stream=True), lw_clear(1), {},
        LW_FUSED_READS)]
    # 4. float32 longwave with particles (register forms at 60 and 37 layers, overflow form at 137), and the fp64 general route
    + [("%s_%dlay" % (name, nlay), "lw_over" if nlay > 96 else "lw_reg", ("lw_fused", nlay, True), form, clear, {}, LW_FUSED_READS)
       for nlay in (60, 37, 137)
       for name, form, clear in (("lw_fluxes_f32", lw_clear(), None), ("lw_fluxes_allsky_f32", lw_allsky(), lw_clear()),
                                 ("lw_fluxes_allsky_mcica_f32", lw_allsky(True), lw_clear()),
                                 ("lw_fluxes_clear_allsky_f32", lw_both, lw_clear()))]
    + [("lw_fluxes_allsky_fp64_%dlay" % nlay, "lw_over" if nlay > 96 else "lw_reg", ("lw_fused", nlay, False), lw_allsky(), lw_clear(),
        {}, LW_FUSED_READS) for nlay in (37, 137)]
    # 5. stand-alone Jacobian kernels (kernels_rte_lw_jac.hip l. 200-216).  The array forms run the instantiations without
    #    particles on a given surface term (PLANCK false, SKY 0); a fused call away from 60 layers (2 layers here) increments tau
    #    in place first and runs SKY 0 with the Planck table, masked or not (capi.cpp lw_jac_dev l. 2203), so one unmasked case
    #    each is all that route has to show.  The instantiations that read the band planes and the mask word per tile --
    #    rte_lw_jac_kernel<., 1|2, false|true>, rte_lw_rescaled_jac_kernel<., 2, false|true> -- run only behind a 60-layer fused
    #    call with "lw_jac_inline" 0 (the forms set it): those cases hold 524 325 x 60 x 32 optical depths, 8.05 GB of scratch.
    + [("rte_lw_jac", "lw_jac", ("lw_arrays", 3, 2), lw_jac_arrays, None, {}, ALL),
       ("rte_lw_rescaled_jac", "lw_jac", ("lw_arrays", 3, 2), lw_rescaled_jac_arrays, None, {}, ALL),
       ("lw_fluxes_jac_2lay_incremented_tau", "lw_jac", ("lw_fused", 2, False), lw_jac_fused(False), lw_clear(), {}, LW_FUSED_READS),
       ("lw_fluxes_rescaled_jac_2lay_incremented_cells", "lw_jac", ("lw_fused", 2, False), lw_rescaled_jac_fused(False), lw_clear(), {},
        LW_FUSED_READS)]
    + [(name, "lw_jac", ("lw_fused", 60, False), form, lw_clear(), {}, LW_FUSED_READS) for name, form in (
        ("lw_fluxes_jac_60lay_two_stream_particles", lw_jac_fused(False)),
        ("lw_fluxes_jac_60lay_two_stream_particles_mcica", lw_jac_fused(True)),
        ("lw_fluxes_jac_60lay_one_stream_particles", lw_jac_fused(False, True)),
        ("lw_fluxes_jac_60lay_one_stream_particles_mcica", lw_jac_fused(True, True)),
        ("lw_fluxes_rescaled_jac_60lay", lw_rescaled_jac_fused(False)),
        ("lw_fluxes_rescaled_jac_60lay_mcica", lw_rescaled_jac_fused(True)))]
)


@pytest.mark.parametrize("name,family,key,form,clear,opts,wanted", CASES, ids=[c[0] for c in CASES])
def test_columns_past_one_round_equal_the_small_call(pkg, gpu, inputs, name, family, key, form, clear, opts, wanted):
    import torch

    def run(f, d):
        pkg.reset_solver_options()
        pkg.set_arithmetic(pkg.FAST)
        for n, v in opts.items():
            pkg.set_solver_option(n, v)
        return f(pkg, k, d)

    ncol = ncol_of(family)
    k, d = inputs.get(*key)
    want = run(form, d)
    torch.cuda.synchronize()
    for i, w in enumerate(want):   # the small call is meaningful
        assert bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0.0, (name, i)
        assert not bool((w == -1.0).any()), (name, i)   # every element was written (no flux is exactly the sentinel)
        assert w.shape[-1] == NSMALL
    if clear is not None:          # ... and its clouds show
        assert not torch.equal(want[0], run(clear, d)[0]), name
    big, idx = stride_helpers.repeated(d, ncol, wanted, NSMALL)
    got = run(form, big)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    counts = []
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape[-1] == ncol and g.shape[:-1] == w.shape[:-1]
        counts.append(stride_helpers.count_differing(g, w, idx))
        print("%s, %d columns, output %d: %d of %d values differ from the %d-column call" % (name, ncol, i, counts[-1], g.numel(), NSMALL))
    del big, got
    pkg.release_scratch(0)
    assert counts == [0] * len(want), (name, counts)
