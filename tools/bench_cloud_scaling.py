#!/usr/bin/env python3
"""Timings of the sampled optical-depth scaling (in-cloud water variability), fp64, synthetic.clouds /
synthetic.cloud_fraction, per shape (sw | lw_fsck | lw_rrtmgp, ncol, 60 layers), interleaved in one
process:
  (a) the sampler: ecckd_cloud_scaling_sample for both overlaps with the 5 x 16 lognormal table (staged in LDS) and, for
      maximum-random overlap, with a 65 x 128 table (read through L2), with and without the mask output; against
      ecckd_cloud_mask_sample on the same inputs and a torch fill_ of the same bytes (ms, and GB/s of scaling written);
  (b) ecckd_increment_scaled by band against ecckd_increment_masked and ecckd_increment;
  (c) each fused scaled call against the fused McICA call, the unmasked fused call and its composed route (longwave:
      gas_optics_tau + increment_scaled + rte_lw_fused; shortwave: gas_optics + delta_scale of a copy + increment_scaled +
      rte_sw).  --fused-up-to bounds the column count of (b) and (c).
HIP-event timing: 3 warm-up calls, then --repeats timed calls per variant, the variants interleaved round-robin; median
and min-max.  Usage: python tools/bench_cloud_scaling.py [--shapes sw:100000,lw_fsck:100000,...] [--out f.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_allsky import interleaved, stats  # noqa: E402
from bench_mcica import DATA, FILES, SW_NAMES  # noqa: E402


def child(kind, ncol, nlay, repeats, fused):
    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def check(msg):
        if msg:
            raise SystemExit(msg)

    sw = kind == "sw"
    k = pkg.GasOpticsEcckd()
    check(k.load(os.path.join(DATA, FILES[kind]), device=0))
    ng, nb = k.get_ngpt(), k.get_nband()
    cf = t(synthetic.cloud_fraction(0, ncol, nlay))
    alpha = torch.full((nlay - 1, ncol), 0.7, dtype=torch.float64, device=dev)
    fsd = torch.full((nlay, ncol), 0.75, dtype=torch.float64, device=dev)
    small = pkg.CloudScaling.lognormal(5, 0.0, 0.5, 16)
    large = pkg.CloudScaling.lognormal(65, 0.0, 0.03125, 128)
    sample = lambda table, ov="max_ran", **kw: pkg.sample_cloud_scaling(cf, ng, table, fsd, ov, alpha if ov == "exp_ran" else None,
                                                                        seed=1, **kw)
    filled = torch.empty((ng, nlay, ncol), dtype=torch.float32, device=dev)
    variants = {"scaling_max_ran": lambda: sample(small), "scaling_exp_ran": lambda: sample(small, "exp_ran"),
                "scaling_max_ran_with_mask": lambda: sample(small, return_mask=True),
                "scaling_max_ran_table_in_l2": lambda: sample(large),
                "mask_max_ran": lambda: pkg.sample_cloud_mask(cf, ng, seed=1),
                "mask_exp_ran": lambda: pkg.sample_cloud_mask(cf, ng, "exp_ran", alpha, seed=1),
                "torch_fill_same_bytes": lambda: filled.fill_(1.0)}
    if fused:
        cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay, shortwave=sw)
        cloud = synthetic.clouds(0, ncol, nlay, nb)
        names = SW_NAMES if sw else synthetic.GAS_ORDER
        gc = pkg.GasConcs(names)
        for n in names:
            v = cols[n]
            if np.isscalar(v):
                gc.set_vmr(n, float(v))
            elif v.ndim == 1:
                gc.set_vmr_column(n, t(v))
            else:
                gc.set_vmr(n, t(v))
        plev, tlay = t(cols["plev"]), t(cols["tlay"])
        part = pkg.OpticalProps2str()
        part.tau, part.ssa, part.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
        fl = pkg.FluxesBroadband(*(torch.empty((nlay + 1, ncol), dtype=torch.float64, device=dev) for _ in range(3 if sw else 2)))
        scaling, mask = sample(small, return_mask=True)
        b2g = k.get_band2gpt()
        if sw:
            rng = np.random.default_rng(nlay)
            mu0, ad, af = t(cols["mu0"]), t(rng.uniform(0.02, 0.6, (ncol, nb))), t(rng.uniform(0.02, 0.6, (ncol, nb)))
            allsky = lambda **kw: check(k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, ad, af, part, fl, delta_scale=True, **kw))
            scaled = lambda: check(k.sw_flux_scaled(plev, tlay, gc, True, mu0, ad, af, part, fl, scaling, delta_scale=True))
            op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=plev)
            work = pkg.OpticalProps2str(); work.alloc_2str_bands(ncol, nlay, k, like=plev)
            toa = torch.empty((ng, ncol), dtype=torch.float64, device=dev)

            def composed():
                check(k.gas_optics(None, plev, tlay, gc, op, toa))
                work.tau.copy_(part.tau); work.ssa.copy_(part.ssa); work.g.copy_(part.g)
                check(work.delta_scale())
                check(op.increment_scaled(work, scaling, band2gpt=b2g))
                check(pkg.rte_sw(op, True, mu0, toa, ad, af, fl))
            check(k.gas_optics(None, plev, tlay, gc, op, toa))
        else:
            tsfc, tlev = t(cols["tsfc"]), t(cols["tlev"])
            emis = t(np.repeat(cols["sfc_emis"][:, None], nb, 1))
            allsky = lambda **kw: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, part, fl, **kw))
            scaled = lambda: check(k.lw_flux_scaled(plev, tlay, tsfc, tlev, gc, True, emis, part, fl, scaling))
            op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=plev)

            def composed():
                check(k.gas_optics_tau(plev, tlay, gc, op))
                check(op.increment_scaled(part, scaling, band2gpt=b2g))
                check(k.rte_lw_fused(op, True, tlay, tlev, tsfc, emis, fl))
            check(k.gas_optics_tau(plev, tlay, gc, op))
        variants.update({"allsky_fused": allsky, "allsky_fused_masked": lambda: allsky(cloud_mask=mask), "allsky_fused_scaled": scaled,
                         "composed_route_scaled": composed,
                         "increment_by_band": lambda: check(op.increment(part, band2gpt=b2g)),
                         "increment_by_band_masked": lambda: check(op.increment(part, band2gpt=b2g, cloud_mask=mask)),
                         "increment_by_band_scaled": lambda: check(op.increment_scaled(part, scaling, band2gpt=b2g))})
    res = {n: stats(v) for n, v in interleaved(variants, repeats).items()}
    nbytes = 4.0 * ncol * nlay * ng
    for n in res:
        if n.startswith("scaling_") or n == "torch_fill_same_bytes":
            res[n]["scaling_GBps"] = nbytes / (res[n]["median_ms"] * 1e-3) / 1e9
    print(json.dumps({"kind": kind, "ncol": ncol, "nlay": nlay, "ngpt": ng, "nband": nb, "scaling_bytes": nbytes,
                      "tau_bytes": 2 * nbytes, "device": torch.cuda.get_device_name(0),
                      "build": pkg.lib().ecckd_build_info().decode(), "results": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sw:100000,lw_fsck:100000,sw:1000000,lw_fsck:1000000")
    ap.add_argument("--nlay", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--fused-up-to", type=int, default=100000, help="largest column count at which (b) and (c) are timed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(child mode) kind:ncol")
    ap.add_argument("--fused", action="store_true", help="(child mode) time (b) and (c) as well")
    args = ap.parse_args()
    if args.child:
        kind, ncol = args.child.split(":")
        child(kind, int(ncol), args.nlay, args.repeats, args.fused)
        return
    out = {"timing": "HIP events, 3 warm-up calls, variants interleaved round-robin in one process per shape", "repeats": args.repeats,
           "shapes": []}
    for shape in args.shapes.split(","):
        fused = int(shape.split(":")[1]) <= args.fused_up_to
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--nlay", str(args.nlay), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd + (["--fused"] if fused else []), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:   # (a failed child ends the job: nothing more is started on the GPU)
            raise SystemExit("child failed (%s): %s" % (shape, r.stderr[-2000:]))
        entry = json.loads(r.stdout.strip().splitlines()[-1])
        res = entry["results"]
        ratio = lambda a, b: res[a]["median_ms"] / res[b]["median_ms"]
        entry["scaling_over_mask_sampler"] = {ov: ratio("scaling_" + ov, "mask_" + ov) for ov in ("max_ran", "exp_ran")}
        entry["scaling_over_fill"] = ratio("scaling_max_ran", "torch_fill_same_bytes")
        if fused:
            entry["scaled_over_masked_increment"] = ratio("increment_by_band_scaled", "increment_by_band_masked")
            entry["scaled_over_masked_fused"] = ratio("allsky_fused_scaled", "allsky_fused_masked")
            # (a fused call slower than its composed route shows here as a figure above 1)
            entry["scaled_fused_over_composed_route"] = ratio("allsky_fused_scaled", "composed_route_scaled")
        out["shapes"].append(entry)
        print(json.dumps({n: v for n, v in entry.items() if n != "results"}), flush=True)
        for n, v in res.items():
            print("  %-30s %9.3f ms  [%.3f, %.3f]" % (n, v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
