#!/usr/bin/env python3
"""Single-precision fused all-sky fluxes against their float32 composition and against the fp64 fused call (DESIGN section
5.5c), synthetic.clouds, device tensors, plain and with a McICA mask:
  shortwave  1e5 x 60 x 27 g and 1e5 x 137 x 27 g:
    fused32    sw_fluxes_allsky on float32 tensors (ecckd_sw_fluxes_allsky[_mcica]_f32), delta_scale on
    composed32 gas_optics + delta_scale of a copy + increment(band2gpt[, cloud_mask]) + rte_sw on float32 tensors
    fused64    sw_fluxes_allsky on float64 tensors
  longwave   1e5 and 1e6 x 60 x 32 g, 1e5 x 137 x 36 g:
    fused32    lw_fluxes_allsky on float32 tensors (ecckd_lw_fluxes_allsky[_mcica]_f32)
    composed32 gas_optics + increment(band2gpt[, cloud_mask]) + rte_lw on float32 tensors
    fused64    lw_fluxes_allsky on float64 tensors
HIP-event timing, all in this process: five runs per shape; a run warms every variant up twice and times it `--repeats`
times, the variants interleaved round-robin, and yields the median; reported: the median and the min-max of the five runs,
and the ratios composed32 / fused32 and fused64 / fused32 of the medians with the range the runs span.
Usage: python tools/bench_allsky_f32.py [--shapes sw60,sw137,lw60,lw60m,lw137] [--repeats N] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
FILES = {"sw": "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc", "fsck": "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc",
         "rrtmgp": "ecckd-1.2_lw_ckd-definition_climate_rrtmgp-tol0.061.nc"}
SHAPES = {"sw60": ("sw", 100000, 60), "sw137": ("sw", 100000, 137), "lw60": ("fsck", 100000, 60), "lw60m": ("fsck", 1000000, 60),
          "lw137": ("rrtmgp", 100000, 137)}
SW_NAMES = ["co2", "ch4", "n2o", "o2", "h2o", "o3"]
RUNS = 5


def check(msg):
    if msg:
        raise SystemExit(msg)


def one_run(variants, repeats):
    """{name: median ms} of one run: two warm-up calls each, then `repeats` timed calls, interleaved round-robin."""
    import torch
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in variants}
    for _ in range(repeats):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1))
    return {n: float(np.median(v)) for n, v in ms.items()}


def summary(runs):
    """runs: [{name: ms}] -> per variant the median and min-max of the runs, and the two ratios with their ranges."""
    out = {n: {"median_ms": float(np.median([r[n] for r in runs])), "min_ms": min(r[n] for r in runs), "max_ms": max(r[n] for r in runs),
               "runs": len(runs)} for n in runs[0]}
    for kind in ("", "_mask"):
        f = "fused32" + kind
        for other in ("composed32", "fused64"):
            o = other + kind
            per_run = [r[o] / r[f] for r in runs]
            out["%s_over_%s" % (o, f)] = {"of_medians": out[o]["median_ms"] / out[f]["median_ms"], "min": min(per_run), "max": max(per_run),
                                          "ranges_apart": out[o]["min_ms"] > out[f]["max_ms"] or out[o]["max_ms"] < out[f]["min_ms"]}
    return out


def variants_for(pkg, synthetic, which, ncol, nlay, dev):
    """{name: callable} for one shape: fused32 / composed32 / fused64, plain and masked."""
    import torch
    k = pkg.GasOpticsEcckd()
    check(k.load(os.path.join(DATA, FILES[which]), device=0))
    sw = which == "sw"
    ng, nb = k.get_ngpt(), k.get_nband()
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay, shortwave=sw)
    cloud = synthetic.clouds(0, ncol, nlay, nb)
    rng = np.random.default_rng(nlay)
    alb = rng.uniform(0.02, 0.6, (2, ncol, nb))
    emis = np.repeat(cols["sfc_emis"][:, None], nb, 1) if not sw else None
    mask = pkg.sample_cloud_mask(torch.from_numpy(synthetic.cloud_fraction(0, ncol, nlay)).to(dev), ng, seed=1, col0=0)
    b2g = k.get_band2gpt()

    def in_precision(dt, tag):
        """the variants on arrays of one precision (a scope of their own: the closures keep these tensors)"""
        out = {}
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        names = SW_NAMES if sw else list(synthetic.GAS_ORDER)
        gc = pkg.GasConcs(names)
        for n in names:
            v = cols.get(n, 0.0)
            if np.isscalar(v):
                gc.set_vmr(n, float(v))
            elif v.ndim == 1:
                gc.set_vmr_column(n, t(v))
            else:
                gc.set_vmr(n, t(v))
        plev, tlay = t(cols["plev"]), t(cols["tlay"])
        part = pkg.OpticalProps2str()
        part.tau, part.ssa, part.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
        new = lambda n: pkg.FluxesBroadband(*(torch.empty((nlay + 1, ncol), dtype=plev.dtype, device=dev) for _ in range(n)))
        if sw:
            mu0, ad, af = t(cols["mu0"]), t(alb[0]), t(alb[1])
            fl = new(3)
            fused = lambda m=None: check(k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, ad, af, part, fl, delta_scale=True, cloud_mask=m))
        else:
            tsfc, tlev, em = t(cols["tsfc"]), t(cols["tlev"]), t(emis)
            fl = new(2)
            fused = lambda m=None: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, em, part, fl, cloud_mask=m))
        out["fused" + tag] = fused
        out["fused" + tag + "_mask"] = lambda: fused(mask)
        if dt is not np.float32:
            return out
        if sw:
            op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=plev)
            work = pkg.OpticalProps2str(); work.alloc_2str_bands(ncol, nlay, k, like=plev)
            toa = torch.empty((ng, ncol), dtype=plev.dtype, device=dev)

            def composed(m=None):
                check(k.gas_optics(None, plev, tlay, gc, op, toa))
                work.tau.copy_(part.tau); work.ssa.copy_(part.ssa); work.g.copy_(part.g)   # (the fused call scales a copy too)
                check(work.delta_scale())
                check(op.increment(work, band2gpt=b2g, cloud_mask=m))
                check(pkg.rte_sw(op, True, mu0, toa, ad, af, fl))
        else:
            op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=plev)
            src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=plev, separate_levels=True)

            def composed(m=None):
                check(k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tlev))
                check(op.increment(part, band2gpt=b2g, cloud_mask=m))
                check(pkg.rte_lw(op, True, src, em, fl))
        out["composed32"] = composed
        out["composed32_mask"] = lambda: composed(mask)
        return out

    out = dict(in_precision(np.float32, "32"), **in_precision(np.float64, "64"))
    return out, dict(file=FILES[which], ncol=ncol, nlay=nlay, ngpt=ng, nband=nb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "build": pkg.lib().ecckd_build_info().decode(), "repeats": args.repeats, "runs": RUNS,
           "timing": "HIP events; five runs in one process, each the median of `repeats` interleaved calls after two warm-up calls",
           "shapes": {}}
    for name in args.shapes.split(","):
        which, ncol, nlay = SHAPES[name]
        variants, shape = variants_for(pkg, synthetic, which, ncol, nlay, dev)
        runs = [one_run(variants, args.repeats) for _ in range(RUNS)]
        res["shapes"][name] = dict(shape, results=summary(runs))
        del variants
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        pkg.release_scratch(0)
        print(name, json.dumps(res["shapes"][name]["results"]), flush=True)
    line = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    else:
        print(line)


if __name__ == "__main__":
    main()
