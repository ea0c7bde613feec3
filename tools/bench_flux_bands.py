#!/usr/bin/env python3
"""Fused per-band fluxes (ecckd_lw_flux_bands / ecckd_sw_flux_bands), fp64, device tensors,
synthetic.columns / synthetic.clouds, a random cloud mask.  Per shape kind:ncol:nlay (kind = sw | lw_fsck | lw_rrtmgp) and
per variant (clear, allsky, masked), in one process, interleaved round-robin:
  (a) the new call: lw_fluxes_byband / sw_fluxes_byband with band planes and broadband members;
  (b) the composed by-band route a host has to take without it: gas_optics -> [delta_scale of a copy ->] [increment by band
      (masked)] -> rte_lw / rte_sw with a FluxesByband, the host owning every (ngpt, nlay, ncol) array;
  (c) the broadband fused call of the same variant (lw_fluxes / lw_fluxes_allsky / sw_fluxes / sw_fluxes_allsky).
a/b is what the call buys, a/c the price of band output.  Columns beyond the first 100000 repeat the first 100000 on the
device (the host never holds the large shape).
HIP-event timing: 3 warm-up calls, then --repeats timed calls per variant; median and min-max.
Usage: python tools/bench_flux_bands.py [--shapes lw_rrtmgp:100000:60,...] [--repeats 10] [--parent COMMIT] [--out f.json]"""
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

DEFAULT_SHAPES = "lw_rrtmgp:100000:60,lw_rrtmgp:1000000:60,lw_rrtmgp:100000:137,sw:100000:60,sw:100000:137"
HOST_COLUMNS = 100000


def child(kind, ncol, nlay, repeats):
    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    base = min(ncol, HOST_COLUMNS)
    reps = -(-ncol // base)

    def t(a):   # to the device, the column axis (the last) repeated up to ncol
        a = np.ascontiguousarray(a)
        x = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
        return x if reps == 1 else x.repeat(*([1] * (x.dim() - 1)), reps)[..., :ncol].contiguous()

    def check(msg):
        if msg:
            raise SystemExit(msg)

    sw = kind == "sw"
    k = pkg.GasOpticsEcckd()
    check(k.load(os.path.join(DATA, FILES[kind]), device=0))
    ng, nb, b2g = k.get_ngpt(), k.get_nband(), k.get_band2gpt()
    cols = synthetic.columns(0, base, k.get_press_min(), nlay=nlay, shortwave=sw)
    cloud = synthetic.clouds(0, base, nlay, nb)
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
    two = pkg.OpticalProps2str()
    two.tau, two.ssa, two.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
    mask = t(np.random.default_rng(1).integers(0, 2**63, (nlay, base), dtype=np.uint64))
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    nout = 3 if sw else 2
    bands = pkg.FluxesByband(*([zeros(nb, nlay + 1, ncol) for _ in range(nout)] + ([] if sw else [None])),
                             *[zeros(nlay + 1, ncol) for _ in range(nout)])
    broad = pkg.FluxesBroadband(*[zeros(nlay + 1, ncol) for _ in range(nout)])
    like = zeros(1)
    variants = {}
    if sw:
        rng = np.random.default_rng(nlay)
        mu0 = t(cols["mu0"])
        # (the albedos are (ncol, nband): made band-major so that t() repeats their column axis)
        ad, af = (t(rng.uniform(0.02, 0.6, (nb, base))).t().contiguous() for _ in range(2))
        op = pkg.OpticalProps2str()
        op.alloc_2str(ncol, nlay, k, like=like)
        toa = zeros(ng, ncol)
        scaled = pkg.OpticalProps2str()
        scaled.tau, scaled.ssa, scaled.g = (torch.empty_like(two.tau) for _ in range(3))

        def composed(part, m):
            check(k.gas_optics(None, plev, tlay, gc, op, toa))
            if part is not None:
                for dst, src in ((scaled.tau, part.tau), (scaled.ssa, part.ssa), (scaled.g, part.g)):
                    dst.copy_(src)
                check(scaled.delta_scale())
                check(op.increment(scaled, band2gpt=b2g, cloud_mask=m))
            check(pkg.rte_sw(op, True, mu0, toa, ad, af, bands))

        new = lambda part, m: check(k.sw_fluxes_byband(plev, tlay, gc, True, mu0, ad, af, bands, particles=part, cloud_mask=m))
        fused = lambda part, m: check(k.sw_fluxes(plev, tlay, gc, True, mu0, ad, af, broad) if part is None else
                                      k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, ad, af, part, broad, cloud_mask=m))
    else:
        tsfc, tlev = t(cols["tsfc"]), t(cols["tlev"])
        emis = t(np.repeat(cols["sfc_emis"][None, :], nb, 0)).t().contiguous()
        op = pkg.OpticalProps1scl()
        op.alloc_1scl(ncol, nlay, k, like=like)
        src = pkg.SourceFuncLW()
        src.alloc(ncol, nlay, k, like=like)

        def composed(part, m):
            check(k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tlev))
            if part is not None:
                check(op.increment(part, band2gpt=b2g, cloud_mask=m))
            check(pkg.rte_lw(op, True, src, emis, bands))

        new = lambda part, m: check(k.lw_fluxes_byband(plev, tlay, tsfc, tlev, gc, True, emis, bands, particles=part, cloud_mask=m))
        fused = lambda part, m: check(k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, broad) if part is None else
                                      k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, part, broad, cloud_mask=m))
    for name, part, m in (("clear", None, None), ("allsky", two, None), ("masked", two, mask)):
        variants[name + ":a_bands_call"] = lambda part=part, m=m: new(part, m)
        variants[name + ":b_composed_byband"] = lambda part=part, m=m: composed(part, m)
        variants[name + ":c_broadband_fused"] = lambda part=part, m=m: fused(part, m)
    res = {n: stats(v) for n, v in interleaved(variants, repeats).items()}
    print(json.dumps({"kind": kind, "ncol": ncol, "nlay": nlay, "ngpt": ng, "nband": nb, "device": torch.cuda.get_device_name(0),
                      "build": pkg.lib().ecckd_build_info().decode(), "results": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--parent", default=None, help="the parent commit, recorded in the output")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(child mode) kind:ncol:nlay")
    args = ap.parse_args()
    if args.child:
        kind, ncol, nlay = args.child.split(":")
        child(kind, int(ncol), int(nlay), args.repeats)
        return
    out = {"timing": "HIP events, 3 warm-up calls, variants interleaved round-robin in one process per shape; device tensors",
           "repeats": args.repeats, "parent_commit": args.parent, "shapes": []}
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:   # (a failed child ends the job: nothing more is started on the GPU)
            raise SystemExit("child failed (%s): %s" % (shape, r.stderr[-2000:]))
        entry = json.loads(r.stdout.strip().splitlines()[-1])
        entry["shape"] = shape
        res, ratios = entry["results"], {}
        for v in ("clear", "allsky", "masked"):
            a, b, c = (res["%s:%s" % (v, n)] for n in ("a_bands_call", "b_composed_byband", "c_broadband_fused"))
            ratios[v] = {"b_over_a": b["median_ms"] / a["median_ms"], "a_wholly_below_b": a["max_ms"] < b["min_ms"],
                         "a_over_c": a["median_ms"] / c["median_ms"]}
        entry["ratios"] = ratios
        out["shapes"].append(entry)
        print(json.dumps({"shape": shape, "ratios": ratios, "median_ms": {n: s["median_ms"] for n, s in res.items()}}), flush=True)
        if args.out:   # (written shape by shape: a later child that fails leaves the earlier figures)
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
