#!/usr/bin/env python3
"""Heating-rate timings (ecckd_heating_rate / _f32, device arrays): 60 and 137 layers at 1e5 and 1e6 columns, 1 / 4 / 16
outer planes, fp64 and float32, with and without cp per cell.  Per case:
  heating_rate   the call, on random fluxes of 0-500 W m-2 and monotone pressures
  copy           a torch copy_ of as many bytes (read + written) as the call moves by its definition,
                   sizeof(real) * ncol * ((2*nouter + 1)*(nlay+1) + (nouter + [cp])*nlay):
                 the copy ceiling, measured the way tools/hbm_ceiling.py measures its own (torch elementwise copy, HIP
                 events), in this process, interleaved with the call
and what the call adds in front of nothing: lw_fluxes on the 32-g longwave file at 60 layers alone and followed by
heating_rate of its fluxes.
HIP-event timing: 3 warm-up calls, then `--repeats` timed calls per variant, the variants interleaved round-robin; median
and min-max spread.
Usage: python tools/bench_heating_rate.py [--sizes 100000,1000000] [--layers 60,137] [--outer 1,4,16] [--repeats 20]
                                          [--out profiles/heating_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LW_FILE = os.path.join(ROOT, "data", "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc")


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


def algorithmic_bytes(ncol, nlay, nouter, with_cp, size):
    return size * ncol * ((2 * nouter + 1) * (nlay + 1) + (nouter + int(with_cp)) * nlay)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--layers", default="60,137")
    ap.add_argument("--outer", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]
    sizes, layers, outers = sorted(ints(args.sizes)), ints(args.layers), ints(args.outer)

    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    cases = []
    for ncol in sizes:
        for nlay in layers:
            for nouter in outers:
                for dtype, size in ((torch.float64, 8), (torch.float32, 4)):
                    rand = lambda *shape: torch.rand(shape, dtype=dtype, device=dev, generator=gen)
                    fu, fd = rand(nouter, nlay + 1, ncol) * 500.0, rand(nouter, nlay + 1, ncol) * 500.0
                    thick = torch.exp(rand(nlay, ncol) * float(np.log(5000.0)))   # 1 Pa .. 5 kPa
                    plev = torch.cat([torch.full((1, ncol), 10.0, dtype=dtype, device=dev), 10.0 + torch.cumsum(thick, 0)]).contiguous()
                    cp = 1004.0 + 46.0 * rand(nlay, ncol)
                    hr = torch.empty((nouter, nlay, ncol), dtype=dtype, device=dev)
                    del thick
                    for with_cp in (False, True):
                        nbytes = algorithmic_bytes(ncol, nlay, nouter, with_cp, size)
                        half = nbytes // (2 * size)
                        src, dst = torch.empty(half, dtype=dtype, device=dev), torch.empty(half, dtype=dtype, device=dev)
                        variants = {"heating_rate": lambda: check(pkg.heating_rate(fu, fd, plev, heating_rate=hr,
                                                                                   cp=cp if with_cp else None)[0]),
                                    "copy": lambda: dst.copy_(src)}
                        res = {n: stats(v) for n, v in interleaved(variants, args.repeats).items()}
                        entry = {"ncol": ncol, "nlay": nlay, "nouter": nouter, "dtype": "f64" if size == 8 else "f32",
                                 "cp": with_cp, "bytes": nbytes, "results": res,
                                 "TB_per_s": nbytes / (res["heating_rate"]["median_ms"] * 1e-3) / 1e12,
                                 "copy_TB_per_s": nbytes / (res["copy"]["median_ms"] * 1e-3) / 1e12,
                                 "fraction_of_copy_ceiling": res["copy"]["median_ms"] / res["heating_rate"]["median_ms"]}
                        cases.append(entry)
                        print(json.dumps(entry), flush=True)
                        del src, dst, variants
                    del fu, fd, plev, cp, hr
                    torch.cuda.empty_cache()

    # beside the flux call whose output it consumes: lw_fluxes, 32 g-points, 60 layers, fp64
    chain = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    k = pkg.GasOpticsEcckd()
    check(k.load(LW_FILE, device=0))
    for ncol in sizes:
        nlay = 60
        cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay)
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
        emis = t(np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1))
        fl = pkg.FluxesBroadband(*(torch.empty((nlay + 1, ncol), dtype=torch.float64, device=dev) for _ in range(2)))
        hr = torch.empty((nlay, ncol), dtype=torch.float64, device=dev)
        fluxes = lambda: check(k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl))
        heating = lambda: check(fl.heating_rate(plev, heating_rate=hr)[0])

        def both():
            fluxes()
            heating()

        res = {n: stats(v) for n, v in interleaved({"lw_fluxes": fluxes, "heating_rate": heating,
                                                    "lw_fluxes_heating_rate": both}, args.repeats).items()}
        entry = {"ncol": ncol, "nlay": nlay, "ngpt": k.get_ngpt(), "results": res,
                 "heating_rate_over_lw_fluxes": res["heating_rate"]["median_ms"] / res["lw_fluxes"]["median_ms"],
                 "chain_over_lw_fluxes_alone": res["lw_fluxes_heating_rate"]["median_ms"] / res["lw_fluxes"]["median_ms"]}
        chain.append(entry)
        print(json.dumps(entry), flush=True)
        del fluxes, heating, both, fl, hr
        pkg.release_scratch(0)
        torch.cuda.empty_cache()

    out = {"device": torch.cuda.get_device_name(0), "build": pkg.lib().ecckd_build_info().decode(), "repeats": args.repeats,
           "timing": "HIP events, 3 warm-up calls, variants interleaved",
           "bytes": "sizeof(real) * ncol * ((2*nouter + 1)*(nlay+1) + (nouter + [cp])*nlay)",
           "heating_rate": cases, "chain": chain}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
