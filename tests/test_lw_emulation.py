"""helpers.lw_emulate -- rte_lw_kernel's recurrence restated in numpy, which sets the single-precision flux bars of
tests/test_gpu_lw_f32.py -- run in float64 against the CPU oracle: it restates the same solver (no GPU needed)."""
import numpy as np
import pytest

import helpers


def _case(rng, ng, nlay, ncol):
    tau = rng.uniform(0, 2, (ng, nlay, ncol)) * rng.choice([1e-9, 1e-3, 1.0], size=(ng, nlay, ncol))
    lay, inc, dec = (rng.uniform(1, 9, (ng, nlay, ncol)) for _ in range(3))
    return dict(tau=tau, lay=lay, inc=inc, dec=dec, emis_gpt=rng.uniform(0.7, 1.0, (ng, ncol)),
                sfc=rng.uniform(1, 9, (ng, ncol)))


@pytest.mark.parametrize("ng,nlay,ncol,top_at_1,nmus,series3,thresh,inc,iso", [
    (7, 5, 9, True, 1, False, None, False, 0),
    (7, 60, 13, False, 3, True, None, True, 0),
    (5, 97, 6, True, 2, False, 1e-3, True, 1),     # overflow form: groups of 4 g-points
    (3, 137, 5, False, 4, True, 3e-4, False, 0),
])
def test_lw_emulation_in_float64_is_the_oracle(oracle_mod, ng, nlay, ncol, top_at_1, nmus, series3, thresh, inc, iso):
    rng = np.random.default_rng(nlay + ng)
    c = _case(rng, ng, nlay, ncol)
    incf = rng.uniform(0, 30, (ng, ncol)) if inc else None
    okw = {}
    if series3:
        okw["lw_series_terms"] = 3
    if thresh is not None:
        okw["lw_tau_thresh"] = thresh
    if iso:
        okw["lw_inc_flux_isotropic"] = iso
    opt = oracle_mod.solver_options(**okw)
    args = (c["tau"], c["lay"], c["inc"], c["dec"], c["emis_gpt"], c["sfc"])
    fu, fd = oracle_mod.rte_lw(*args, top_at_1=top_at_1, nmus=nmus, inc_flux=incf, options=opt)
    gu, gd = oracle_mod.rte_lw_gpt(*args, top_at_1=top_at_1, nmus=nmus, inc_flux=incf, options=opt)
    eu, ed, egu, egd = helpers.lw_emulate(*args, top_at_1=top_at_1, nmus=nmus, dtype=np.float64, series3=series3,
                                          tau_thresh=thresh, inc_flux=incf, inc_isotropic=bool(iso), per_gpt=True)
    assert np.max(np.abs(eu - fu)) < 1e-10 and np.max(np.abs(ed - fd)) < 1e-10
    assert np.max(np.abs(egu - gu)) < 1e-10 and np.max(np.abs(egd - gd)) < 1e-10
    assert np.min(fu) > 1.0
    # the float32 run is a different solver by a float32 amount: far from the float64 one, close to the oracle
    su, sd = helpers.lw_emulate(*args, top_at_1=top_at_1, nmus=nmus, dtype=np.float32, series3=series3, tau_thresh=thresh,
                                inc_flux=incf, inc_isotropic=bool(iso))
    d32 = max(np.max(np.abs(su - fu)), np.max(np.abs(sd - fd)))
    assert 1e-7 < d32 < 1e-2


def test_lw_seam_layers():
    assert helpers.lw_seam_layers(60, True) == [0]
    assert helpers.lw_seam_layers(33, True) == [0, 32] and helpers.lw_seam_layers(33, False) == [0, 32]
    assert helpers.lw_seam_layers(1, False) == [0]
    assert helpers.lw_seam_layers(137, True) == [0, 40, 41]           # nover = 41: walked 40 (ring) and 41 (registers)
    assert helpers.lw_seam_layers(137, False) == [95, 96, 136]
