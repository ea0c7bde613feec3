"""Numpy restatement of the McICA cloud sampler (ecckd_cloud_mask_sample), written from the definition in
include/ecckd_hip.h and from nothing else: Philox4x32-10 (Salmon et al. 2011) keyed by (seed, global column, layer,
g-point), the rank-carrying generator of Raisanen et al. (2004), one uint64 word per (layer, column).  Everything is
integer arithmetic plus exact float64 operations, so the library's words are compared with ``array_equal``.

Arrays follow the package convention: ``cloud_frac`` is ``(nlay, ncol)``, ``overlap_param`` ``(nlay-1, ncol)``, the mask
``(nlay, ncol)`` uint64 with bit g = g-point g sees the layer's cloud."""
import numpy as np

MAX_RAN, EXP_RAN = 0, 1
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)

# (counter, key) -> output words: the known answers of the generator
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays holding 32-bit values) for counter words c0..c3 (broadcastable arrays) and
    the key (k0, k1) (Python ints)."""
    c = list(np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]   # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def draws(seed, col, lay, ngpt, stream):
    """u (stream 0) or v (stream 1) of the global columns ``col`` (array) in layer ``lay``: ``col.shape + (ngpt,)``."""
    seed = int(seed) & (2 ** 64 - 1)
    g = np.arange(ngpt, dtype=np.uint64)
    col = np.asarray(col).astype(np.uint64)[..., None]
    w = philox4x32_10(col & _LO, col >> _S32, np.uint64(lay), (g >> np.uint64(2)) | np.uint64(stream << 31),
                      seed & 0xFFFFFFFF, seed >> 32)
    pick = np.broadcast_to((g & np.uint64(3)).astype(np.intp), w[0].shape)
    x = np.choose(pick, w)
    return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def sample(cloud_frac, ngpt, overlap=MAX_RAN, overlap_param=None, seed=0, col0=0):
    """The mask ``(nlay, ncol)`` uint64 of ecckd_cloud_mask_sample."""
    cf = np.asarray(cloud_frac, dtype=np.float64)
    nlay, ncol = cf.shape
    col = (np.arange(ncol, dtype=np.int64) + np.int64(col0)).astype(np.uint64)
    mask = np.zeros((nlay, ncol), dtype=np.uint64)
    r = np.zeros((ncol, ngpt))
    bit = np.uint64(1) << np.arange(ngpt, dtype=np.uint64)
    with np.errstate(invalid="ignore"):
        for l in range(nlay):
            cloudy = cf[l] > 0
            if l == 0:
                a = np.zeros(ncol)
            else:
                both = cloudy & (cf[l - 1] > 0)
                a = np.where(both, 1.0 if overlap == MAX_RAN else overlap_param[l - 1], 0.0)
            u, v = draws(seed, col, l, ngpt, 0), draws(seed, col, l, ngpt, 1)
            r = np.where(v < a[:, None], r, u)
            bits = (r >= (1.0 - cf[l])[:, None]) & cloudy[:, None]
            mask[l] = np.bitwise_or.reduce(np.where(bits, bit, np.uint64(0)), axis=1)
    return mask


def unpack(mask, ngpt):
    """bool ``mask.shape + (ngpt,)``."""
    return ((np.asarray(mask, dtype=np.uint64)[..., None] >> np.arange(ngpt, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def masked_tau(tau_band, mask, band2gpt, ngpt):
    """``(ngpt, nlay, ncol)``: the band optical depth ``(nband, nlay, ncol)`` spread over the g-points, +0 where the
    g-point's bit is clear."""
    import allsky_helpers as ah
    bits = np.moveaxis(unpack(mask, ngpt), -1, 0)
    return np.where(bits, ah.spread(tau_band, band2gpt, ngpt), tau_band.dtype.type(0))
