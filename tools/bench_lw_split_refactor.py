#!/usr/bin/env python3
"""Bits and time of every public call that the layer-split longwave solver (kernels_rte_lw_split.hip) serves, this build
against the parent's: the check that goes with a refactor of that file.

Both libraries run in alternating fresh child processes (ECCKD_LIB selects the library; the runner is that of
tools/bench_gas_tile_sync.py: every child under its own time limit, the chain stops at the first failure).  A child runs
every call once on 1 003 distinct synthetic columns x 60 layers and reports a SHA-256 of each output array, then repeats the
columns cyclically to 100 000 on the device and times each call with HIP events (median of --steps calls after a warm-up).
Only the library call lies between the events: gas concentrations, particle and flux objects are built before.
Verdicts: `bits_equal` -- every output of every child of one build has the digest of the other's; `overlaps_parent` -- the
min-max range of a call's times over the rounds overlaps the parent's; `wholly_above_parent` (the one that fails the build) and
`wholly_below_parent` -- it does not, and on which side.  The parent's commit goes into the record: that of --parent-ref, or
--parent-commit for a library built elsewhere; without it nothing runs.

Usage: python tools/bench_lw_split_refactor.py (--parent-lib lib.so --parent-commit SHA | --parent-ref HEAD~1) [--rounds 3]
       [--calls a,b] [--out profiles/lw_split_refactor.json]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_gas_tile_sync import build_parent, run, stats  # noqa: E402

NSMALL, NBIG, NLAY, C0 = 1003, 100000, 60, 11


def gas_concs(pkg, d):
    import numpy as np
    from rte_ecckd_amd import synthetic
    gc = pkg.GasConcs(synthetic.GAS_ORDER)
    for n in synthetic.GAS_ORDER:
        v = d.get(n, 0.0)
        e = gc.set_vmr(n, float(v)) if np.isscalar(v) else (gc.set_vmr_column(n, v) if v.ndim == 1 else gc.set_vmr(n, v))
        if e:
            raise SystemExit(e)
    return gc


def calls(pkg, k):
    """name -> function(d) -> (run, outputs): everything a call needs beside the library call itself (gas concentrations, particle
    and flux objects) is built here, outside the timed region; run() is the call alone and fills the list of output tensors.
    d is the dict of device arrays of child()."""
    import numpy as np
    import torch

    def new(d):
        return torch.full((NLAY + 1, d["plev"].shape[-1]), -1.0, dtype=torch.float64, device=d["plev"].device)

    def head(d):
        return (d["plev"], d["tlay"], d["tsfc"], d["tlev"], gas_concs(pkg, d), True, d["emis"])

    def particles(d, one):
        op = pkg.OpticalProps1scl() if one else pkg.OpticalProps2str()
        op.tau = d["part_tau"]
        if not one:
            op.ssa, op.g = d["part_ssa"], d["part_g"]
        return op

    def fluxes(d, n=1):
        return [pkg.FluxesBroadband(new(d), new(d)) for _ in range(n)]

    def ok(e):
        if e:
            raise SystemExit(e)

    def clear(d):
        fl, = fluxes(d)
        h = head(d)
        return (lambda: ok(k.lw_fluxes(*h, fl, n_gauss_angles=2, inc_flux=d["inc_flux"]))), [fl.flux_up, fl.flux_dn]

    def allsky(one, masked, jac=False, rescaled=False):
        def f(d):
            fl, = fluxes(d)
            j = new(d) if jac else None
            kw = dict(rescaled=True) if rescaled else {}
            h, op = head(d), particles(d, one)
            return (lambda: ok(k.lw_fluxes_allsky(*h, op, fl, n_gauss_angles=2, inc_flux=d["inc_flux"],
                                                  cloud_mask=d["mask"] if masked else None, flux_up_jac=j, **kw))), \
                [fl.flux_up, fl.flux_dn] + ([j] if jac else [])
        return f

    def clear_jac(d):
        fl, = fluxes(d)
        j = new(d)
        h = head(d)
        return (lambda: ok(k.lw_fluxes(*h, fl, n_gauss_angles=2, inc_flux=d["inc_flux"], flux_up_jac=j))), [fl.flux_up, fl.flux_dn, j]

    def both(one, masked):
        def f(d):
            fl, fc = fluxes(d, 2)
            h, op = head(d), particles(d, one)
            return (lambda: ok(k.lw_fluxes_clear_allsky(*h, op, fl, fc, n_gauss_angles=2, inc_flux=d["inc_flux"],
                                                        cloud_mask=d["mask"] if masked else None))), \
                [fl.flux_up, fl.flux_dn, fc.flux_up, fc.flux_dn]
        return f

    def rescaled_jac(masked):
        def f(d):
            fl, = fluxes(d)
            j = new(d)
            h, op = head(d), particles(d, False)
            return (lambda: ok(k.lw_fluxes_rescaled(*h, op, fl, flux_up_jac=j, n_gauss_angles=2, inc_flux=d["inc_flux"],
                                                    cloud_mask=d["mask"] if masked else None))), [fl.flux_up, fl.flux_dn, j]
        return f

    def sources(d):
        src = pkg.SourceFuncLW()
        src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = d["lay"], d["inc"], d["dec"], d["sfc"]
        return src

    def rescaled_arrays(d):
        op = pkg.OpticalProps2str()
        op.tau, op.ssa, op.g = d["cell_tau"], d["cell_ssa"], d["cell_g"]
        op.band2gpt = np.asarray(k.get_band2gpt())
        fl, = fluxes(d)
        src = sources(d)
        return (lambda: ok(pkg.rte_lw(op, True, src, d["emis"], fl, n_gauss_angles=2, inc_flux=d["inc_flux"], rescaled=True))), \
            [fl.flux_up, fl.flux_dn]

    def arrays(shared):
        def f(d):
            op = pkg.OpticalProps1scl()
            op.tau = d["gas_tau"]
            op.band2gpt = np.asarray(k.get_band2gpt())
            fl, = fluxes(d)
            src = sources(d)
            return (lambda: ok(pkg.rte_lw(op, True, src, d["emis"], fl, n_gauss_angles=2, inc_flux=None if shared else d["inc_flux"],
                                          shared_levels=shared))), [fl.flux_up, fl.flux_dn]
        return f

    out = {"lw_fluxes": clear, "lw_fluxes_jac": clear_jac}
    for one in (False, True):
        for masked in (True, False):
            tag = ("_1scl" if one else "_2str") + ("_mask" if masked else "")
            out["lw_fluxes_allsky" + tag] = allsky(one, masked)
            out["lw_fluxes_clear_allsky" + tag] = both(one, masked)
            out["lw_fluxes_allsky_jac" + tag] = allsky(one, masked, jac=True)
    for masked in (True, False):
        tag = "_mask" if masked else ""
        out["lw_fluxes_allsky_rescaled" + tag] = allsky(False, masked, rescaled=True)
        out["lw_fluxes_rescaled_jac" + tag] = rescaled_jac(masked)
    out["rte_lw_rescaled"] = rescaled_arrays
    out["rte_lw_split"] = arrays(False)
    out["rte_lw_split_shared_levels"] = arrays(True)
    return out


def child(steps, warmup, only=None):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    k = pkg.GasOpticsEcckd()
    msg = k.load(bench.LW_FILE, device=0)
    if msg:
        raise SystemExit(msg)
    for name, v in (("lw_solver", 1), ("lw_split_seg", 10), ("lw_both_skies", 1), ("lw_jac_inline", 1)):
        pkg.set_solver_option(name, v)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cols = synthetic.columns(C0, NSMALL, k.get_press_min(), nlay=NLAY)
    cloud = synthetic.clouds(C0, NSMALL, NLAY, k.get_nband())
    rng = np.random.default_rng(C0)
    cols["inc_flux"] = rng.uniform(0.0, 2.0, (k.get_ngpt(), NSMALL))
    cols["emis"] = np.repeat(cols.pop("sfc_emis")[:, None], k.get_nband(), 1)
    mask = pkg.sample_cloud_mask(np.ascontiguousarray(synthetic.cloud_fraction(C0, NSMALL, NLAY)), k.get_ngpt(), seed=C0)
    d = {n: (v if np.isscalar(v) else t(v)) for n, v in cols.items()}
    d.update({"part_" + n: t(cloud[n]) for n in ("tau", "ssa", "g")})
    d["mask"] = t(mask.view(np.int64))
    fs = {n: f for n, f in calls(pkg, k).items() if not only or n in only}

    def with_arrays(d):
        """... plus the inputs of the array forms: gas optical depth, Planck sources, the cell's (tau, ssa, g)."""
        ncol = d["plev"].shape[-1]
        gc = gas_concs(pkg, d)
        op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, NLAY, k, like=d["plev"])
        src = pkg.SourceFuncLW(); src.alloc(ncol, NLAY, k, like=d["plev"])
        e = k.gas_optics(None, d["plev"], d["tlay"], d["tsfc"], gc, op, src, tlev=d["tlev"])
        assert e == "", e
        two = pkg.OpticalProps2str(); two.alloc_2str(ncol, NLAY, k, like=d["plev"])
        two.tau.copy_(op.tau); two.ssa.zero_(); two.g.zero_()
        part = pkg.OpticalProps2str()
        part.tau, part.ssa, part.g = d["part_tau"], d["part_ssa"], d["part_g"]
        e = two.increment(part, band2gpt=k.get_band2gpt())
        assert e == "", e
        return dict(d, gas_tau=op.tau, lay=src.lay_source, inc=src.lev_source_inc, dec=src.lev_source_dec, sfc=src.sfc_source,
                    cell_tau=two.tau, cell_ssa=two.ssa, cell_g=two.g)

    small = with_arrays(d)
    digests = {}
    for name, f in fs.items():
        call, outs = f(small)
        call()
        torch.cuda.synchronize()
        digests[name] = [hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() for o in outs]
    idx = torch.arange(NBIG, device=dev) % NSMALL
    big = with_arrays({n: (v if np.isscalar(v) else v.index_select(0 if n == "emis" else v.ndim - 1, idx).contiguous()) for n, v in d.items()})
    del small
    times = {}
    for name, f in fs.items():
        call, _ = f(big)
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        times[name] = statistics.median(ms)
    print(json.dumps({"digests": digests, "ms": times}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-ref", default=None)
    ap.add_argument("--parent-commit", default=None, help="the commit --parent-lib was built from (with --parent-ref: that ref's)")
    ap.add_argument("--calls", default=None, help="comma-separated subset of the calls")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.steps, a.warmup, a.calls.split(",") if a.calls else None)
    tmp = None
    parent, commit = a.parent_lib, a.parent_commit
    if not parent and not a.parent_ref:
        raise SystemExit("--parent-lib or --parent-ref is required")
    if not commit and a.parent_ref:
        commit = subprocess.run(["git", "rev-parse", a.parent_ref], capture_output=True, text=True, cwd=ROOT).stdout.strip()
    if not commit:
        raise SystemExit("the parent's commit is not known: give --parent-commit with --parent-lib")
    if not parent:
        tmp = tempfile.TemporaryDirectory()
        parent = build_parent(a.parent_ref, tmp.name)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    if a.calls:
        cmd += ["--calls", a.calls]
    runs = {"parent": [], "this": []}
    for i in range(a.rounds):
        for which, lib in (("parent", parent), ("this", None)):
            runs[which].append(run(cmd, lib, a.timeout))
            print("round %d, %s: %.1f ms over all calls" % (i, which, sum(runs[which][-1]["ms"].values())), flush=True)
    names = list(runs["this"][0]["ms"])
    first = runs["parent"][0]["digests"]
    res = {"parent_commit": commit, "ncol_bits": NSMALL, "ncol_time": NBIG, "nlay": NLAY, "rounds": a.rounds, "steps": a.steps, "calls": {}}
    for n in names:
        par, this = stats([r["ms"][n] for r in runs["parent"]]), stats([r["ms"][n] for r in runs["this"]])
        res["calls"][n] = {"bits_equal": all(r["digests"][n] == first[n] for w in runs for r in runs[w]),
                           "parent_ms": par, "this_ms": this,
                           "overlaps_parent": this["min"] <= par["max"] and par["min"] <= this["max"],
                           "wholly_below_parent": this["max"] < par["min"], "wholly_above_parent": this["min"] > par["max"]}
        c = res["calls"][n]
        print("%-36s bits equal %-5s parent %.3f-%.3f ms, this %.3f-%.3f ms: %s"
              % (n, c["bits_equal"], par["min"], par["max"], this["min"], this["max"],
                 "above" if c["wholly_above_parent"] else "below" if c["wholly_below_parent"] else "overlaps"))
    res["all_bits_equal"] = all(c["bits_equal"] for c in res["calls"].values())
    res["none_wholly_above_parent"] = not any(c["wholly_above_parent"] for c in res["calls"].values())
    print("all bits equal:", res["all_bits_equal"], " none wholly above the parent:", res["none_wholly_above_parent"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
