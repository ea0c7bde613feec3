#!/usr/bin/env python3
"""The shortwave on the daylit columns only: timings at 1e5 columns x 60 layers x 27 g-points, fp64, synthetic.clouds
(DESIGN section 5.5c).  For the daylit shares 0, 25, 50, 75 and 100 % (a mu0 field from synthetic.uniform: column c is
daylit where u(c) < share) and the four calls -- clear sky, all-sky, McICA, both skies:
  (a) the existing full call on ALL columns (what a host without compaction pays, the share does not enter) -- on this
      build and, with --parent-lib, on another build of the library (the parent commit's), each in fresh child processes
      that alternate, so the two are compared on the same box;
  (b) the existing call on columns the host gathered beforehand with torch indexing, the gather of every input and the
      scatter of every output into zeroed arrays included in the time;
  (c) sw_fluxes_daylit with a list made beforehand; the selection (daylit_columns, which synchronises) is timed apart.
HIP-event timing: 2 warm-up calls, then `--repeats` (default 7) timed calls per variant, the variants of a share
interleaved round-robin; minimum, median and maximum.
Usage: python tools/bench_sw_daylit.py [--ncol N] [--parent-lib lib.so] [--out file.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SW_FILE = os.path.join(ROOT, "data", "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc")
NAMES = ["co2", "ch4", "n2o", "o2", "h2o", "o3"]
SHARES = (0.0, 0.25, 0.5, 0.75, 1.0)
CALLS = ("clear", "allsky", "mcica", "both")
F_DAY = 90   # field id of the daylit draw (synthetic.uniform): none of synthetic's own


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def interleaved(variants, repeats, warmup=2):
    import torch
    for fn in variants.values():
        for _ in range(warmup):
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="fresh child processes per library for (a)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--full-only", action="store_true", help="(child mode) time the four existing full calls, print one JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    full_children = None
    if args.parent_lib and not args.full_only:   # fresh processes, alternating, before this one opens the GPU
        full_children = {"parent": [], "branch": []}
        for _ in range(args.rounds):
            for name, lib in (("parent", args.parent_lib), ("branch", None)):
                env = dict(os.environ)
                if lib:
                    env["ECCKD_LIB"] = os.path.abspath(lib)
                else:
                    env.pop("ECCKD_LIB", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--full-only", "--ncol", str(args.ncol), "--nlay",
                                    str(args.nlay), "--repeats", str(args.repeats)], env=env, capture_output=True, text=True, timeout=400)
                if r.returncode != 0:
                    raise SystemExit("child failed: " + r.stderr[-2000:])
                full_children[name].append(json.loads(r.stdout.strip().splitlines()[-1]))

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
    draw = np.asarray(synthetic.uniform(np.arange(ncol), F_DAY, 0)).reshape(-1)[:ncol]
    inputs = {"plev": t(cols["plev"]), "tlay": t(cols["tlay"]), "ad": t(rng.uniform(0.02, 0.6, (ncol, nb))),
              "af": t(rng.uniform(0.02, 0.6, (ncol, nb))), "tau": t(cloud["tau"]), "ssa": t(cloud["ssa"]), "g": t(cloud["g"])}
    cf = synthetic.cloud_fraction(0, ncol, nlay)
    inputs["mask"] = pkg.sample_cloud_mask(t(cf), ng, "max_ran", seed=5)
    gases = {n: (cols[n] if np.isscalar(cols[n]) else t(cols[n])) for n in NAMES}

    def concs(index=None):
        gc = pkg.GasConcs(NAMES)
        for n, v in gases.items():
            if np.isscalar(v):
                gc.set_vmr(n, float(v))
            elif v.ndim == 1:
                gc.set_vmr_column(n, v if index is None else v[index])
            else:
                gc.set_vmr(n, v if index is None else v[:, index].contiguous())
        return gc

    def existing(call, a, gc, mu0, fl, fc):
        """The existing call `call` on the arrays `a` (all of one column count)."""
        args_ = (a["plev"], a["tlay"], gc, True, mu0, a["ad"], a["af"])
        if call == "clear":
            check(k.sw_fluxes(*args_, fl))
            return
        part = pkg.OpticalProps2str()
        part.tau, part.ssa, part.g = a["tau"], a["ssa"], a["g"]
        if call == "allsky":
            check(k.sw_fluxes_allsky(*args_, part, fl, delta_scale=True))
        elif call == "mcica":
            check(k.sw_fluxes_allsky(*args_, part, fl, delta_scale=True, cloud_mask=a["mask"]))
        else:
            check(k.sw_fluxes_clear_allsky(*args_, part, fl, fc, delta_scale=True, cloud_mask=a["mask"]))

    new = lambda n: pkg.FluxesBroadband(*(torch.empty((nlay + 1, n), dtype=torch.float64, device=dev) for _ in range(3)))
    fl, fc = new(ncol), new(ncol)
    gc_full = concs()
    mu0_full = t(cols["mu0"])                                      # every column lit: the driver's mu0 = 1 recipe costs the same
    if args.full_only:
        ms = interleaved({c: (lambda c=c: existing(c, inputs, gc_full, mu0_full, fl, fc)) for c in CALLS}, args.repeats)
        print(json.dumps({c: stats(v) for c, v in ms.items()}))
        return

    def host_gathered(call, index, mu0):
        """(b): torch indexing of every input the call reads, the existing call, the outputs scattered into zeroed arrays."""
        a = {n: (v[index].contiguous() if n in ("ad", "af") else v[..., index].contiguous()) for n, v in inputs.items()
             if n in ("plev", "tlay", "ad", "af") or (call != "clear" and (n != "mask" or call in ("mcica", "both")))}
        n = int(index.shape[0])
        gfl, gfc = new(n), new(n)
        if n:
            existing(call, a, concs(index), mu0[index].contiguous(), gfl, gfc)
        for dst, src in ((fl, gfl), (fc, gfc)) if call == "both" else ((fl, gfl),):
            for name in ("flux_up", "flux_dn", "flux_dn_dir"):
                d = getattr(dst, name)
                d.zero_()
                d[:, index] = getattr(src, name)

    def daylit(call, index, mu0):
        part = None
        if call != "clear":
            part = pkg.OpticalProps2str()
            part.tau, part.ssa, part.g = inputs["tau"], inputs["ssa"], inputs["g"]
        check(k.sw_fluxes_daylit(inputs["plev"], inputs["tlay"], gc_full, True, mu0, inputs["ad"], inputs["af"], fl, particles=part,
                                 fluxes_clear=fc if call == "both" else None, delta_scale=True,
                                 cloud_mask=inputs["mask"] if call in ("mcica", "both") else None, day_index=index))

    results = {}
    for share in SHARES:
        mu0 = t(np.where(draw < share, cols["mu0"], -cols["mu0"]))
        index, nday = pkg.daylit_columns(mu0)
        long_index = index.long()
        variants = {"select": lambda: pkg.daylit_columns(mu0)}
        for c in CALLS:
            variants["b_host_gathered_" + c] = lambda c=c: host_gathered(c, long_index, mu0)
            variants["c_daylit_" + c] = lambda c=c: daylit(c, index, mu0)
        if share == SHARES[-1]:
            for c in CALLS:
                variants["a_full_" + c] = lambda c=c: existing(c, inputs, gc_full, mu0_full, fl, fc)
        ms = interleaved(variants, args.repeats)
        results["%d%%" % round(100 * share)] = dict({n: stats(v) for n, v in ms.items()}, nday=nday)
        print("share %3d%%: nday %d" % (round(100 * share), nday), {n: round(stats(v)["median_ms"], 3) for n, v in ms.items()},
              file=sys.stderr, flush=True)
    out = {"device": torch.cuda.get_device_name(0), "build": pkg.lib().ecckd_build_info().decode(), "ncol": ncol, "nlay": nlay,
           "ngpt": ng, "nband": nb, "dtype": "f64", "repeats": args.repeats,
           "timing": "HIP events, 2 warm-up calls, the variants of a share interleaved", "shares": results,
           "a_full_calls_fresh_processes": full_children}
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
