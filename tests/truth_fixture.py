"""Readers of tests/golden/solver_truth_{sw,lw}.npz (tests/golden/make_golden_solver_truth.py writes them from
tests/solver_truth.py).  numpy only: the GPU suite reads the fixtures without mpmath."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAND2GPT = np.array([[1, 2], [3, 3]])
GPT2BAND = np.array([0, 0, 1])
_cache = {}


def _load(which):
    if which not in _cache:
        z = np.load(os.path.join(GOLDEN, "solver_truth_%s.npz" % which))
        arrays = {k: z[k] for k in z.files}
        meta = json.loads(str(arrays.pop("meta")))
        assert meta["band2gpt"] == BAND2GPT.tolist()
        for a in arrays.values():
            a.setflags(write=False)
        _cache[which] = (arrays, meta)
    return _cache[which]


def sw_meta():
    return _load("sw")[1]["sets"]


def lw_meta():
    return _load("lw")[1]["sets"]


def r32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32), dtype=np.float64)


def per_gpt(a):
    """(ncol, nband) -> (ng, ncol)."""
    return np.ascontiguousarray(a[:, GPT2BAND].T)


def sw_set(name, image="f64"):
    """(inputs, expected) of a shortwave set: inputs tau, ssa, g (3, nlay, ncol), mu0 (ncol), toa (3, ncol), alb_dir,
    alb_dif (ncol, 2) [, inc_dif (3, ncol), d_min (ncol)] -- for image "f32" rounded to float32 (held in float64);
    expected up, dn, dir (nlay + 1, ncol) [bnd_* (2, nlay + 1, ncol), gpt_* (3, nlay + 1, ncol)] of that image."""
    arrays, _ = _load("sw")
    pre = name + "."
    inp = {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre) and k.count(".") == 1}
    if image == "f32":
        inp = {k: r32(v) for k, v in inp.items()}
    pre = "%s.%s." % (name, image)
    exp = {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}
    assert exp, (name, image)
    return inp, exp


def lw_set(name, variant=None, image="f64"):
    """Inputs of a longwave set -- tau (3, nlay, ncol), lev_source (3, nlay + 1, ncol), sfc_emis (ncol, 2), sfc_source,
    inc_flux (3, ncol), plus lay / inc / dec as rte_lw takes them (lay the mean of the two level values, formed in the
    image's precision) -- and, with `variant` "tab 2 none f64" etc., the expected fluxes of that variant."""
    arrays, _ = _load("lw")
    pre = name + "."
    inp = {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre) and k.count(".") == 1}
    if variant is not None:
        image = variant.split()[3]
    if image == "f32":
        inp = {k: r32(v) for k, v in inp.items()}
    lev = inp["lev_source"]
    inp["inc"], inp["dec"] = np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1])
    if image == "f32":
        inp["lay"] = (0.5 * (inp["inc"].astype(np.float32) + inp["dec"].astype(np.float32))).astype(np.float64)
    else:
        inp["lay"] = 0.5 * (inp["inc"] + inp["dec"])
    inp["emis_gpt"] = per_gpt(inp["sfc_emis"])
    if variant is None:
        return inp
    q, n, i, im = variant.split()
    pre = "%s.%s%s.%s.%s." % (name, q, n, i, im)
    exp = {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}
    assert exp, (name, variant)
    return inp, exp


def exact_quadrature(n):
    """Gauss-Jacobi secants and weights (weight mu on [0, 1]) rounded to float64."""
    arrays, _ = _load("lw")
    return arrays["exact_Ds_%d" % n], arrays["exact_wts_%d" % n]


def flip(a, axis):
    """Reversed along `axis`, in fresh C-ordered memory (a length-1 axis would otherwise keep its negative stride)."""
    return np.flip(a, axis=axis).copy(order="C")
