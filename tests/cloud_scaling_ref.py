"""Numpy restatement of the sampled optical-depth scaling (ecckd_cloud_scaling_sample, ecckd_increment_scaled and the
lognormal table), written from the definitions in include/ecckd_hip.h ("In-cloud water variability") and from nothing
else, on top of ``mcica_helpers.draws``.  Every line of the definition is one IEEE float64 operation and numpy evaluates
them one by one, so the library's arrays are compared with ``array_equal``.

Arrays follow the package convention: ``cloud_frac`` and ``fsd`` are ``(nlay, ncol)``, the scaling ``(ngpt, nlay, ncol)``
float32, the mask ``(nlay, ncol)`` uint64."""
import numpy as np

import mcica_helpers as mh


def sample(cloud_frac, ngpt, values, fsd0, dfsd, fsd, overlap=mh.MAX_RAN, overlap_param=None, seed=0, col0=0):
    """``(scaling, mask)`` of ecckd_cloud_scaling_sample; ``fsd`` an ``(nlay, ncol)`` array or one number."""
    cf = np.asarray(cloud_frac, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64)
    nfsd, nq = v.shape
    nlay, ncol = cf.shape
    fsd = np.broadcast_to(np.asarray(fsd, dtype=np.float64), cf.shape)
    col = (np.arange(ncol, dtype=np.int64) + np.int64(col0)).astype(np.uint64)
    scaling = np.zeros((ngpt, nlay, ncol), dtype=np.float32)
    mask = np.zeros((nlay, ncol), dtype=np.uint64)
    bit = np.uint64(1) << np.arange(ngpt, dtype=np.uint64)
    r = np.zeros((ncol, ngpt))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for l in range(nlay):
            cloudy = cf[l] > 0
            if l == 0:
                a = np.zeros(ncol)
            else:
                both = cloudy & (cf[l - 1] > 0)
                a = np.where(both, 1.0 if overlap == mh.MAX_RAN else overlap_param[l - 1], 0.0)
            u, w = mh.draws(seed, col, l, ngpt, 0), mh.draws(seed, col, l, ngpt, 1)
            r = np.where(w < a[:, None], r, u)
            thresh = (1.0 - cf[l])[:, None]
            seen = (r >= thresh) & cloudy[:, None]
            mask[l] = np.bitwise_or.reduce(np.where(seen, bit, np.uint64(0)), axis=1)
            # the position inside the cloud and its bin
            p = (r - thresh) / cf[l][:, None]
            j = np.minimum(np.where(seen, p * float(nq), 0.0).astype(np.int64), nq - 1)
            # the two rows around the cell's FSD and the weight of the upper one
            x = (fsd[l] - fsd0) / dfsd
            low, high = ~(x > 0), x >= float(nfsd - 1)   # (a NaN is `low`)
            k = np.where(low, 0, np.where(high, nfsd - 2, np.where(low | high, 0.0, x).astype(np.int64)))
            wt = np.where(low, 0.0, np.where(high, 1.0, x - k.astype(np.float64)))
            v0, v1 = v[k[:, None], j], v[k[:, None] + 1, j]
            s = v0 + wt[:, None] * (v1 - v0)
            scaling[:, l, :] = np.where(seen, s, 0.0).astype(np.float32).T
    return scaling, mask


def scaled_tau(tau_band, scaling, band2gpt, ngpt):
    """``(ngpt, nlay, ncol)``: the band optical depth ``(nband, nlay, ncol)`` spread over the g-points times the scaling,
    in the precision of ``tau_band`` (one rounded product per cell: ecckd_increment_scaled's t2)."""
    import allsky_helpers as ah
    return ah.spread(tau_band, band2gpt, ngpt) * scaling.astype(tau_band.dtype)


def lognormal_mp(nfsd, fsd0, dfsd, nq, dps=40):
    """The bin means of the unit-mean lognormal distribution, evaluated with mpmath at ``dps`` digits and rounded to
    float64 once: entry j = nq * (Phi(z_{j+1} - sigma) - Phi(z_j - sigma)), sigma^2 = log(1 + f^2), z_j = Phi^-1(j / nq)."""
    import mpmath as mp
    with mp.workdps(dps):
        phi = lambda t: mp.erfc(-t / mp.sqrt(2)) / 2
        z = [None] + [mp.sqrt(2) * mp.erfinv(2 * mp.mpf(j) / nq - 1) for j in range(1, nq)] + [None]
        out = np.zeros((nfsd, nq))
        for k in range(nfsd):
            f = mp.mpf(fsd0) + k * mp.mpf(dfsd)
            sigma = mp.sqrt(mp.log(1 + f * f))
            edge = [mp.mpf(0)] + [phi(z[j] - sigma) for j in range(1, nq)] + [mp.mpf(1)]
            for j in range(nq):
                out[k, j] = float(nq * (edge[j + 1] - edge[j]))
    return out
