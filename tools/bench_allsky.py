#!/usr/bin/env python3
"""All-sky shortwave timings at 1e5 columns x 60 layers x 27 g-points, fp64, synthetic.clouds:
  (a) clear-sky ecckd_sw_fluxes -- on this build and, with --parent-lib, on another build of the library (the parent
      commit's), each in fresh child processes that alternate, so the two are compared on the same box;
  (b) the unfused all-sky composition gas_optics_sw + delta_scale (of a copy) + increment + rte_sw;
  (c) the fused sw_fluxes_allsky with delta_scale 0 and 1;
  (d) ecckd_increment alone (2str += 2str by band) with its bytes/s against a measured copy ceiling.
HIP-event timing: 3 warm-up calls, then `--repeats` (default 30) timed calls per variant, the variants interleaved
round-robin; median and min-max spread.  Usage: python tools/bench_allsky.py [--ncol N] [--parent-lib lib.so] [--out file.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SW_FILE = os.path.join(ROOT, "data", "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc")
NAMES = ["co2", "ch4", "n2o", "o2", "h2o", "o3"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--nlay", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--clear-only", action="store_true", help="(child mode) time ecckd_sw_fluxes alone, print one JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    clear_children = None
    if args.parent_lib and not args.clear_only:   # fresh processes, alternating, before this one opens the GPU
        clear_children = {"parent": [], "branch": []}
        for _ in range(2):
            for name, lib in (("parent", args.parent_lib), ("branch", None)):
                env = dict(os.environ)
                if lib:
                    env["ECCKD_LIB"] = os.path.abspath(lib)
                else:
                    env.pop("ECCKD_LIB", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--clear-only", "--ncol", str(args.ncol), "--nlay", str(args.nlay),
                                    "--repeats", str(args.repeats)], env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("child failed: " + r.stderr[-2000:])
                clear_children[name].append(json.loads(r.stdout.strip().splitlines()[-1]))

    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def check(msg):
        if msg:
            raise SystemExit(msg)

    k = pkg.GasOpticsEcckd()
    check(k.load(SW_FILE, device=0))
    ncol, nlay, ng, nb = args.ncol, args.nlay, k.get_ngpt(), k.get_nband()
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    cloud = synthetic.clouds(0, ncol, nlay, nb)
    rng = np.random.default_rng(nlay)
    ad, af = t(rng.uniform(0.02, 0.6, (ncol, nb))), t(rng.uniform(0.02, 0.6, (ncol, nb)))
    gc = pkg.GasConcs(NAMES)
    for n in NAMES:
        v = cols[n]
        if np.isscalar(v):
            gc.set_vmr(n, float(v))
        elif v.ndim == 1:
            gc.set_vmr_column(n, t(v))
        else:
            gc.set_vmr(n, t(v))
    plev, tlay, mu0 = t(cols["plev"]), t(cols["tlay"]), t(cols["mu0"])
    fl = pkg.FluxesBroadband(*(torch.empty((nlay + 1, ncol), dtype=torch.float64, device=dev) for _ in range(3)))
    clear = lambda: check(k.sw_fluxes(plev, tlay, gc, True, mu0, ad, af, fl))
    if args.clear_only:
        print(json.dumps(stats(interleaved({"clear": clear}, args.repeats)["clear"])))
        return

    b2g = k.get_band2gpt()
    part = pkg.OpticalProps2str(); part.alloc_2str_bands(ncol, nlay, k, like=plev)
    part.tau.copy_(t(cloud["tau"])); part.ssa.copy_(t(cloud["ssa"])); part.g.copy_(t(cloud["g"]))
    work = pkg.OpticalProps2str(); work.alloc_2str_bands(ncol, nlay, k, like=plev)
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=plev)
    toa = torch.empty((ng, ncol), dtype=torch.float64, device=dev)

    def unfused(delta):
        check(k.gas_optics(None, plev, tlay, gc, op, toa))
        src = part
        if delta:   # the host's copy of the band optics (the fused call scales a copy too)
            work.tau.copy_(part.tau); work.ssa.copy_(part.ssa); work.g.copy_(part.g)
            check(work.delta_scale())
            src = work
        check(op.increment(src, band2gpt=b2g))
        check(pkg.rte_sw(op, True, mu0, toa, ad, af, fl))

    check(k.gas_optics(None, plev, tlay, gc, op, toa))
    variants = {
        "a_clear_sw_fluxes": clear,
        "b_unfused_delta0": lambda: unfused(False),
        "b_unfused_delta1": lambda: unfused(True),
        "c_fused_delta0": lambda: check(k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, ad, af, part, fl, delta_scale=False)),
        "c_fused_delta1": lambda: check(k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, ad, af, part, fl, delta_scale=True)),
        "d_increment_2str_by_2str_bands": lambda: check(op.increment(part, band2gpt=b2g)),
    }
    ms = interleaved(variants, args.repeats)
    res = {n: stats(v) for n, v in ms.items()}
    cells = ncol * nlay * ng
    # bytes the increment has to move: op1 read and written (48 B per cell) + three band planes read
    inc_bytes = 48.0 * cells + 24.0 * ncol * nlay * nb
    x, y = torch.empty(3 * cells, dtype=torch.float64, device=dev), torch.empty(3 * cells, dtype=torch.float64, device=dev)
    copy = stats(interleaved({"copy": lambda: y.copy_(x)}, args.repeats)["copy"])
    out = {
        "device": torch.cuda.get_device_name(0), "build": pkg.lib().ecckd_build_info().decode(), "ncol": ncol, "nlay": nlay, "ngpt": ng,
        "nband": nb, "dtype": "f64", "repeats": args.repeats, "timing": "HIP events, 3 warm-up calls, variants interleaved", "results": res,
        "clear_sw_fluxes_fresh_processes": clear_children,
        "increment": {"bytes": inc_bytes, "GBps": inc_bytes / (res["d_increment_2str_by_2str_bands"]["median_ms"] * 1e-3) / 1e9,
                      "copy_ceiling_GBps": 2 * 24.0 * cells / (copy["median_ms"] * 1e-3) / 1e9, "copy_same_bytes": copy},
        "fused_over_unfused": {"delta0": res["b_unfused_delta0"]["median_ms"] / res["c_fused_delta0"]["median_ms"],
                               "delta1": res["b_unfused_delta1"]["median_ms"] / res["c_fused_delta1"]["median_ms"]},
        "cost_of_clouds_fused_over_clear": res["c_fused_delta1"]["median_ms"] / res["a_clear_sw_fluxes"]["median_ms"],
    }
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
