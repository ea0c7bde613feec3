#!/usr/bin/env python3
"""Cloud-optics timings (ecckd_cloud_optics, fp64, device arrays) at 60 layers, synthetic.cloud_water and
synthetic.cloud_lut (20 liquid and 18 ice sizes, 3 roughness values: the LDS route), for the band count of each shipped
file (1: the 32-g longwave file, 16: the 36-g longwave file, 5: the shortwave file), at 1e5 and 1e6 columns:
  two_stream   tau, ssa, g planes          32 + 24*nband bytes per cell
  one_scalar   absorption optical depth    32 +  8*nband bytes per cell
  all_clear    two_stream on water paths that are all zero: the kernel's stores alone, no table is read
  copy         a torch copy_ of as many bytes (read + written) as two_stream / one_scalar move: the copy ceiling, measured
               the way tools/hbm_ceiling.py measures its own (torch elementwise copy, HIP events), in this process, interleaved
and, for the two longwave files, the cost of the chain from water paths:
  allsky                  lw_fluxes_allsky on planes that are already there
  cloud_optics_allsky     cloud_optics into the planes, then lw_fluxes_allsky
HIP-event timing: 3 warm-up calls, then `--repeats` timed calls per variant, the variants interleaved round-robin; median
and min-max spread.
Usage: python tools/bench_cloud_optics.py [--sizes 100000,1000000] [--repeats 20] [--out profiles/cloud_optics.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LW_FILES = {1: os.path.join(ROOT, "data", "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc"),
            16: os.path.join(ROOT, "data", "ecckd-1.2_lw_ckd-definition_climate_rrtmgp-tol0.061.nc")}
NBANDS = (1, 16, 5)
NLAY = 60


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def interleaved(variants, repeats):
    """{name: [ms]}: every variant warmed up three times, then timed `repeats` times round-robin with HIP events."""
    import torch
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in variants}
    for _ in range(repeats):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[n].append(e0.elapsed_time(e1))
    return out


def check(msg):
    if msg:
        raise SystemExit(msg)


def load_tables(pkg, synthetic, nband):
    lut = synthetic.cloud_lut(nband, 20, 18, 3)
    co = pkg.CloudOptics()
    check(co.load_lut(None, lut["radliq_lwr"], lut["radliq_upr"], 1.0, lut["radice_lwr"], lut["radice_upr"], 1.0,
                      *[lut["lut_" + q + p] for p in ("liq", "ice") for q in ("ext", "ssa", "asy")]))
    return co


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = sorted(int(s) for s in args.sizes.split(",") if s)

    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    water_all = synthetic.cloud_water(0, sizes[-1], NLAY)   # (a column range regenerates the same columns: slices serve)
    cases, chain = [], []
    for ncol in sizes:
        water_np = [np.ascontiguousarray(a[:, :ncol]) for a in water_all]
        water = [t(a) for a in water_np]
        zero = [torch.zeros_like(water[0]), torch.zeros_like(water[1]), water[2], water[3]]
        ncell = ncol * NLAY
        cloudy = float(((water_np[0] > 0) | (water_np[1] > 0)).mean())
        for nband in NBANDS:
            co = load_tables(pkg, synthetic, nband)
            two, one = pkg.OpticalProps2str(), pkg.OpticalProps1scl()
            two.tau, two.ssa, two.g = (torch.empty((nband, NLAY, ncol), dtype=torch.float64, device=dev) for _ in range(3))
            one.tau = torch.empty((nband, NLAY, ncol), dtype=torch.float64, device=dev)
            nbytes = {"two_stream": ncell * (32 + 24 * nband), "one_scalar": ncell * (32 + 8 * nband)}
            bufs = {n: (torch.empty(b // 16, dtype=torch.float64, device=dev), torch.empty(b // 16, dtype=torch.float64, device=dev))
                    for n, b in nbytes.items()}
            variants = {"two_stream": lambda: check(co.cloud_optics(*water, two)),
                        "one_scalar": lambda: check(co.cloud_optics(*water, one)),
                        "all_clear": lambda: check(co.cloud_optics(*zero, two)),
                        "copy_two_stream_bytes": lambda: bufs["two_stream"][1].copy_(bufs["two_stream"][0]),
                        "copy_one_scalar_bytes": lambda: bufs["one_scalar"][1].copy_(bufs["one_scalar"][0])}
            res = {n: stats(v) for n, v in interleaved(variants, args.repeats).items()}
            entry = {"ncol": ncol, "nlay": NLAY, "nband": nband, "cloudy_cell_fraction": cloudy, "bytes": nbytes, "results": res}
            for form in ("two_stream", "one_scalar"):
                entry[form + "_TB_per_s"] = nbytes[form] / (res[form]["median_ms"] * 1e-3) / 1e12
                entry["copy_" + form + "_TB_per_s"] = nbytes[form] / (res["copy_%s_bytes" % form]["median_ms"] * 1e-3) / 1e12
                entry[form + "_fraction_of_copy_ceiling"] = res["copy_%s_bytes" % form]["median_ms"] / res[form]["median_ms"]
            entry["all_clear_fraction_of_copy_ceiling"] = res["copy_two_stream_bytes"]["median_ms"] / res["all_clear"]["median_ms"]
            cases.append(entry)
            print(json.dumps(entry), flush=True)
            del bufs, variants
            if nband in LW_FILES:   # the chain: cloud_optics + lw_fluxes_allsky over lw_fluxes_allsky alone
                k = pkg.GasOpticsEcckd()
                check(k.load(LW_FILES[nband], device=0))
                cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=NLAY)
                gc = pkg.GasConcs(synthetic.GAS_ORDER)
                for n in synthetic.GAS_ORDER:
                    v = cols[n]
                    if np.isscalar(v):
                        gc.set_vmr(n, float(v))
                    elif v.ndim == 1:
                        gc.set_vmr_column(n, t(v))
                    else:
                        gc.set_vmr(n, t(v))
                plev, tlay, tlev, tsfc = t(cols["plev"]), t(cols["tlay"]), t(cols["tlev"]), t(cols["tsfc"])
                emis = t(np.repeat(cols["sfc_emis"][:, None], nband, 1))
                fl = pkg.FluxesBroadband(*(torch.empty((NLAY + 1, ncol), dtype=torch.float64, device=dev) for _ in range(2)))
                check(co.cloud_optics(*water, two))
                allsky = lambda: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, two, fl))

                def both():
                    check(co.cloud_optics(*water, two))
                    allsky()

                res = {n: stats(v) for n, v in interleaved({"allsky": allsky, "cloud_optics_allsky": both}, args.repeats).items()}
                entry = {"ncol": ncol, "nlay": NLAY, "nband": nband, "ngpt": k.get_ngpt(), "results": res,
                         "chain_over_allsky_alone": res["cloud_optics_allsky"]["median_ms"] / res["allsky"]["median_ms"]}
                chain.append(entry)
                print(json.dumps(entry), flush=True)
                del k, allsky, both
                pkg.release_scratch(0)
            del co, two, one
            torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "build": pkg.lib().ecckd_build_info().decode(), "dtype": "f64",
           "repeats": args.repeats, "timing": "HIP events, 3 warm-up calls, variants interleaved",
           "tables": "synthetic.cloud_lut(nband, 20, 18, 3): LDS route", "cloud_optics": cases, "chain": chain}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
