#!/usr/bin/env python3
"""The single-precision two-stream longwave calls next to their fp64 namesakes, fast arithmetic mode.
Per shape kind:ncol:nlay (kind = lw_fsck | lw_rrtmgp), in ONE process per shape, the variants of a group interleaved:
  solver   ecckd_rte_lw_2stream_f32 beside ecckd_rte_lw_2stream on the same random optical properties (generated on the device
           in float64, rounded to float32 for the float call); achieved bytes/s for the 56 B (float) and 112 B (fp64) per cell;
  fused    ecckd_lw_fluxes_allsky_2stream_f32, unmasked and with a sampled cloud mask, beside its float32 composed route
           (gas_optics, zeroed ssa and g, increment by band, rte_lw_2stream) and beside the fp64 fused call, unmasked and masked,
           on synthetic.columns / synthetic.clouds.
With --other-lib, the float solver and the float fused call are also timed on another build of the library (a variant of the
float kernels, or the parent's build for calls that exist there) in fresh child processes that alternate with this build's.
HIP-event timing: 3 warm-up calls, then --repeats timed calls per variant, round-robin; median and min-max.
An --out file that exists is extended by the shapes of the run.
Usage: python tools/bench_lw_2stream_f32.py [--shapes lw_fsck:100000:60,...] [--other-lib lib.so] [--out f.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_allsky import interleaved, stats  # noqa: E402
from bench_mcica import DATA, FILES  # noqa: E402

DEFAULT_SHAPES = "lw_fsck:100000:60,lw_fsck:1000000:60,lw_rrtmgp:100000:137"
BYTES_PER_CELL = {"f32": 56, "f64": 112}   # two passes over tau, ssa, g and the two level-source planes, the ring to and fro


def child(kind, ncol, nlay, repeats, f32_only):
    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")

    def check(msg):
        if msg:
            raise SystemExit(msg)

    k = pkg.GasOpticsEcckd()
    check(k.load(os.path.join(DATA, FILES[kind]), device=0))
    ng, nb = k.get_ngpt(), k.get_nband()
    res = {}
    precisions = (("f32", torch.float32),) if f32_only else (("f32", torch.float32), ("f64", torch.float64))

    # ---- the solvers alone, on arrays of the same size and values (no lay_source: the solver never reads it) ----
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    shape = (ng, nlay, ncol)
    rand = lambda: torch.rand(shape, generator=gen, device=dev, dtype=torch.float32)   # (float32 values: both calls see the same)
    base = {"tau": 10.0 ** (rand() * 3.0 - 2.0), "ssa": rand() * 0.999, "g": rand() * 0.9, "dec": 3.0 + rand()}
    solvers = {}
    keep = []
    for name, dt in precisions:
        op = pkg.OpticalProps2str()
        op.tau, op.ssa, op.g = (base[n].to(dt) for n in ("tau", "ssa", "g"))
        op.band2gpt = np.asarray(k.get_band2gpt())
        src = pkg.SourceFuncLW()
        src.lay_source = None
        src.lev_source_dec = base["dec"].to(dt)
        src.lev_source_inc = src.lev_source_dec * 1.01
        src.sfc_source = torch.full((ng, ncol), 4.0, dtype=dt, device=dev)
        emis = torch.full((ncol, nb), 0.98, dtype=dt, device=dev)
        fl = pkg.FluxesBroadband(torch.empty((nlay + 1, ncol), dtype=dt, device=dev), torch.empty((nlay + 1, ncol), dtype=dt, device=dev))
        keep.append((op, src, emis, fl))
        solvers["solver:rte_lw_2stream_" + name] = (lambda o=op, s=src, e=emis, f=fl: check(pkg.rte_lw_2stream(o, True, s, e, f)))
    del base
    res.update({n: stats(v) for n, v in interleaved(solvers, repeats).items()})
    cells = float(ncol) * nlay * ng
    for name, _ in precisions:
        r = res["solver:rte_lw_2stream_" + name]
        r["achieved_TB_per_s"] = BYTES_PER_CELL[name] * cells / (r["median_ms"] * 1e-3) / 1e12
    del solvers, keep
    torch.cuda.empty_cache()

    # ---- the fused calls and the float composed route, on synthetic columns with clouds ----
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(0, ncol, nlay, nb)
    mask64 = pkg.sample_cloud_mask(np.ascontiguousarray(synthetic.cloud_fraction(0, ncol, nlay)), ng, seed=1)
    mask = torch.from_numpy(mask64.view(np.int64)).to(dev)
    variants = {}
    for name, dt in precisions:
        t = lambda a, dt=dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
        gc = pkg.GasConcs(synthetic.GAS_ORDER)
        for n in synthetic.GAS_ORDER:
            v = cols[n]
            if np.isscalar(v):
                gc.set_vmr(n, float(v))
            elif v.ndim == 1:
                gc.set_vmr_column(n, t(v))
            else:
                gc.set_vmr(n, t(v))
        head = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(np.repeat(cols["sfc_emis"][:, None], nb, 1)))
        two = pkg.OpticalProps2str()
        two.tau, two.ssa, two.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
        fl = pkg.FluxesBroadband(torch.empty((nlay + 1, ncol), dtype=dt, device=dev), torch.empty((nlay + 1, ncol), dtype=dt, device=dev))
        variants["fused:lw_fluxes_allsky_2stream_" + name] = (lambda h=head, p=two, f=fl: check(k.lw_fluxes_allsky_2stream(*h, p, f)))
        variants["fused:lw_fluxes_allsky_2stream_mcica_" + name] = (
            lambda h=head, p=two, f=fl: check(k.lw_fluxes_allsky_2stream(*h, p, f, cloud_mask=mask)))
        if name == "f32":
            like = head[0]
            one = pkg.OpticalProps1scl()
            one.alloc_1scl(ncol, nlay, k, like=like)
            op = pkg.OpticalProps2str()
            op.tau, op.band2gpt = one.tau, one.band2gpt          # (gas optics writes into the two-stream container's tau)
            op.ssa, op.g = torch.empty_like(one.tau), torch.empty_like(one.tau)
            src = pkg.SourceFuncLW()
            src.alloc(ncol, nlay, k, like=like, separate_levels=True)
            b2g = k.get_band2gpt()

            def composed(h=head, one=one, op=op, src=src, p=two, f=fl):
                check(k.gas_optics(None, h[0], h[1], h[2], h[4], one, src, tlev=h[3]))
                op.ssa.zero_()
                op.g.zero_()
                check(op.increment(p, band2gpt=b2g))
                check(pkg.rte_lw_2stream(op, True, src, h[6], f))
            variants["fused:composed_route_f32"] = composed
    res.update({n: stats(v) for n, v in interleaved(variants, repeats).items()})
    print(json.dumps({"kind": kind, "ncol": ncol, "nlay": nlay, "ngpt": ng, "nband": nb, "device": torch.cuda.get_device_name(0),
                      "build": pkg.lib().ecckd_build_info().decode(), "results": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2, help="fresh processes per build and shape with --other-lib, alternating")
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the output: the commit the tree was built from")
    ap.add_argument("--hbm-tb-per-s", type=float, default=None, help="copy ceiling from tools/hbm_ceiling.py, recorded beside the achieved rates")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lw_2stream_f32.json"))
    ap.add_argument("--child", default=None, help="(child mode) kind:ncol:nlay")
    ap.add_argument("--f32-only", action="store_true", help="(child mode) time the float calls alone")
    args = ap.parse_args()
    if args.child:
        kind, ncol, nlay = args.child.split(":")
        child(kind, int(ncol), int(nlay), args.repeats, args.f32_only)
        return

    def run(shape, lib, f32_only):
        env = dict(os.environ)
        env.pop("ECCKD_LIB", None)
        if lib:
            env["ECCKD_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--repeats", str(args.repeats)]
        print("bench_lw_2stream_f32: %s, %s" % (shape, "another build, float calls" if lib else "this build"), file=sys.stderr, flush=True)
        r = subprocess.run(cmd + (["--f32-only"] if f32_only else []), env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:   # (a failed child ends the job: nothing more is started on the GPU)
            raise SystemExit("child failed (%s): %s" % (shape, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"timing": "HIP events, 3 warm-up calls, variants interleaved in one process per shape", "repeats": args.repeats,
           "bytes_per_cell": BYTES_PER_CELL, "hbm_copy_ceiling_TB_per_s": args.hbm_tb_per_s, "commit": args.commit, "shapes": []}
    if args.out and os.path.exists(args.out):   # (an --out file that exists is extended: one file can hold several jobs)
        out["shapes"] = [e for e in json.load(open(args.out)).get("shapes", []) if e["shape"] not in args.shapes.split(",")]
    for shape in args.shapes.split(","):
        entry = {"shape": shape}
        if args.other_lib:
            runs = {"other": [], "this": []}
            for _ in range(args.rounds):
                for name, lib in (("other", args.other_lib), ("this", None)):
                    runs[name].append(run(shape, lib, True)["results"])
            entry["float_calls_on_two_builds"] = {
                call: {b: {"min_ms": min(c[call]["min_ms"] for c in runs[b]), "max_ms": max(c[call]["max_ms"] for c in runs[b]),
                           "median_ms": sorted(c[call]["median_ms"] for c in runs[b])[len(runs[b]) // 2]} for b in runs}
                for call in runs["this"][0]}
        new = run(shape, None, False)
        entry.update({n: new[n] for n in ("kind", "ncol", "nlay", "ngpt", "nband", "device", "build")})
        r = new["results"]
        entry["results"] = r
        s32, s64 = r["solver:rte_lw_2stream_f32"], r["solver:rte_lw_2stream_f64"]
        f32, f64 = r["fused:lw_fluxes_allsky_2stream_f32"], r["fused:lw_fluxes_allsky_2stream_f64"]
        m32, m64 = r["fused:lw_fluxes_allsky_2stream_mcica_f32"], r["fused:lw_fluxes_allsky_2stream_mcica_f64"]
        comp = r["fused:composed_route_f32"]
        entry["ratios"] = {"solver_f32_over_f64": s32["median_ms"] / s64["median_ms"],
                           "solver_f32_wholly_below_f64": s32["max_ms"] < s64["min_ms"],
                           "fused_f32_over_composed_f32": f32["median_ms"] / comp["median_ms"],
                           "fused_f32_wholly_below_composed_f32": f32["max_ms"] < comp["min_ms"],
                           "fused_f32_over_fused_f64": f32["median_ms"] / f64["median_ms"],
                           "masked_over_unmasked_f32": m32["median_ms"] / f32["median_ms"],
                           "masked_over_unmasked_f64": m64["median_ms"] / f64["median_ms"]}
        if args.hbm_tb_per_s:
            entry["ratios"]["solver_f32_fraction_of_hbm_copy_ceiling"] = s32["achieved_TB_per_s"] / args.hbm_tb_per_s
            entry["ratios"]["solver_f64_fraction_of_hbm_copy_ceiling"] = s64["achieved_TB_per_s"] / args.hbm_tb_per_s
        out["shapes"].append(entry)
        print(json.dumps({n: v for n, v in entry.items() if n != "results"}), flush=True)
        if args.out:   # (rewritten after every shape: a job cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
