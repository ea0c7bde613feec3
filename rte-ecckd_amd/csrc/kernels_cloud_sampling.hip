// kernels_cloud_sampling.hip -- McICA cloud sampling (Pincus et al. 2003): a per-g-point cloud mask drawn from the layer
// cloud fractions under maximum-random or exponential-random overlap, one 64-bit word per (column, layer), bit g =
// g-point g sees the layer's cloud.
//
// The definition is this project's own (include/ecckd_hip.h, ecckd_cloud_mask_sample): the rank-carrying generator of
// Raisanen et al. 2004 that RTE-RRTMGP's mo_cloud_sampling is built on, restated from the published description, with the
// random numbers made HERE by a counter-based generator (Philox4x32-10, Salmon et al. 2011) instead of read from an
// (ngpt,nlay,ncol) array of host-made randoms: the mask of a column depends on (seed, global column, layer, g-point) only,
// not on the launch shape, the block a host cuts its columns into or the GPU a column range is sharded to.  Everything is
// integer arithmetic plus exact fp64 operations (a draw is a 24-bit integer times 2^-24; 1 - cloud_frac is one rounded
// subtraction), so tests/mcica_helpers.py reproduces the words bit for bit.  Parity with RTE-RRTMGP is unpinned.
//
// Mapping (gfx950): lane = column, the thread walks the layers from the first to the last of the array and keeps the
// ranks of the g-points -- as their 24-bit integers -- in registers (NQ quads of four g-points: one Philox output each);
// one coalesced 8-byte load of cloud_frac and one coalesced 8-byte store of the word per (column, layer).  A clear layer
// costs nothing but its store; under maximum-random overlap a rank is drawn only where a cloud block starts (inside a
// block the correlation is 1 and `v < 1` always holds, so v is never made).  Not a roofline kernel: it writes 8 B per
// (column, layer) and does ~25 integer instructions per g-point of a cloudy layer (DESIGN section 5.5c has its time).
//
// The same ranks, read as the position of a sub-column inside the cloud, give the sampled optical-depth scaling of
// ecckd_cloud_scaling_sample (in-cloud water variability): cloud_scaling_sample_kernel, below the mask sampler.
#include "kernels.hpp"

namespace ecckd {
namespace {

constexpr int kSampleBlock = 64;   // one wave per block: 1e5 columns are 1563 blocks over 256 CUs

struct Philox4 { unsigned x[4]; };

// Philox4x32-10: counter (c0, c1, c2, c3), key (k0, k1)
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// The ranks r(l, g) * 2^24 of a cloudy layer from those of the layer above (`linked`: that layer was cloudy; alpha: the
// correlation with it, read under EXP_RAN only), for cloud_scaling_sample_kernel: the recurrence cloud_mask_sample_kernel
// spells in its own loop.  (Calling this from the mask kernel as well was tried: the same instructions in another order,
// and 4 more VGPRs in each of its EXP_RAN forms -- that kernel keeps its text and its figures.)
template <int NQ, bool EXP_RAN>
__device__ __forceinline__ void draw_ranks(unsigned (&rank)[NQ][4], int nq, bool linked, double alpha, unsigned c_lo, unsigned c_hi,
                                           unsigned l, unsigned k0, unsigned k1) {
  if (EXP_RAN || !linked) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q < nq) {
        const Philox4 u = philox4x32_10(c_lo, c_hi, l, (unsigned)q, k0, k1);
        if (EXP_RAN && linked) {
          const Philox4 v = philox4x32_10(c_lo, c_hi, l, (unsigned)q | 0x80000000u, k0, k1);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool keep = (double)(v.x[j] >> 8) * 0x1p-24 < alpha;
            rank[q][j] = keep ? rank[q][j] : u.x[j] >> 8;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) rank[q][j] = u.x[j] >> 8;
        }
      }
    }
  }
}

// NQ: quads of g-points held in registers (4 * NQ >= ngpt).  EXP_RAN: the correlation of adjacent cloudy layers is
// overlap_param(i, l-1) and v is drawn; else it is 1 (maximum-random).
template <int NQ, bool EXP_RAN>
__global__ void __launch_bounds__(kSampleBlock) cloud_mask_sample_kernel(int ncol, int nlay, int ngpt, const double *cloud_frac,
                                                                         const double *overlap_param, unsigned long long seed,
                                                                         long long col0, unsigned long long *mask) {
  const long i = (long)blockIdx.x * kSampleBlock + threadIdx.x;
  if (i >= ncol) return;
  const unsigned long long c = (unsigned long long)(col0 + i);
  const unsigned c_lo = (unsigned)c, c_hi = (unsigned)(c >> 32), k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  const int nq = (ngpt + 3) >> 2;   // (uniform)
  unsigned rank[NQ][4];             // r(l, g) * 2^24
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) rank[q][j] = 0u;
  bool prev_cloudy = false;
  for (int l = 0; l < nlay; ++l) {
    const double cf = cloud_frac[i + (long)ncol * l];
    const bool cloudy = cf > 0.;   // (a NaN is a clear layer)
    unsigned long long word = 0ull;
    if (cloudy) {
      // correlation of the rank with the layer above: 0 behind a clear layer (and in the first layer)
      const bool linked = prev_cloudy;
      [[maybe_unused]] double alpha = 0.;
      if (EXP_RAN && linked) alpha = overlap_param[i + (long)ncol * (l - 1)];
      const double thresh = 1. - cf;
      if (EXP_RAN || !linked) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          if (q < nq) {
            const Philox4 u = philox4x32_10(c_lo, c_hi, (unsigned)l, (unsigned)q, k0, k1);
            if (EXP_RAN && linked) {
              const Philox4 v = philox4x32_10(c_lo, c_hi, (unsigned)l, (unsigned)q | 0x80000000u, k0, k1);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const bool keep = (double)(v.x[j] >> 8) * 0x1p-24 < alpha;
                rank[q][j] = keep ? rank[q][j] : u.x[j] >> 8;
              }
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) rank[q][j] = u.x[j] >> 8;
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q < nq) {
          unsigned nib = 0u;
#pragma unroll
          for (int j = 0; j < 4; ++j) nib |= ((double)rank[q][j] * 0x1p-24 >= thresh ? 1u : 0u) << j;
          word |= (unsigned long long)nib << (4 * q);
        }
      }
      if (ngpt < 64) word &= (1ull << ngpt) - 1ull;   // bits ngpt..63 are 0
    }
    mask[i + (long)ncol * l] = word;
    prev_cloudy = cloudy;
  }
}

template <int NQ>
hipError_t launch_sample_nq(int ncol, int nlay, int ngpt, int exp_ran, const double *cloud_frac, const double *overlap_param,
                            unsigned long long seed, long long col0, unsigned long long *mask, hipStream_t s) {
  const unsigned blocks = (unsigned)(((long)ncol + kSampleBlock - 1) / kSampleBlock);
  if (exp_ran)
    hipLaunchKernelGGL((cloud_mask_sample_kernel<NQ, true>), dim3(blocks), dim3(kSampleBlock), 0, s, ncol, nlay, ngpt, cloud_frac,
                       overlap_param, seed, col0, mask);
  else
    hipLaunchKernelGGL((cloud_mask_sample_kernel<NQ, false>), dim3(blocks), dim3(kSampleBlock), 0, s, ncol, nlay, ngpt, cloud_frac,
                       overlap_param, seed, col0, mask);
  return hipGetLastError();
}

// Sampled optical-depth scaling (include/ecckd_hip.h, ecckd_cloud_scaling_sample): the same walk with the same ranks; a
// g-point that sees the cloud reads its rank as the position p inside the cloud, picks bin min(int(p * nq), nq - 1) of the
// table and interpolates between the two FSD rows around the cell's fsd -- every line one rounded fp64 operation, the
// result rounded to float once; a g-point that does not see it gets +0.  The stores are ngpt coalesced 4-byte rows per
// (column, layer): 256 B per wave and g-point.  fsd is read in cloudy layers only.
// LDS: the table (nfsd * nq doubles, at most kCloudOpticsLdsBytes) is staged by the block, else the two gathers of a seen
// g-point go through L2; the values, and so the bits, are the same.
// One wave walks all layers of its 64 columns.  The alternative -- 2 or 4 sub-blocks of layers per column block, each
// walking the layers above its share for the ranks alone -- was measured at 60 layers x 32 g-points (DESIGN section 5.5c,
// profiles/cloud_scaling_sampler_mappings.json): at 1e5 columns 0.23-0.25 against 0.26-0.27 ms under maximum-random overlap
// but 0.34-0.35 against 0.31-0.32 ms under exponential-random overlap (every prologue layer draws), at 1e6 columns
// slower under both; only a call of 2e4 columns gains (0.10 against 0.17 ms).  Not kept.
template <int NQ, bool EXP_RAN, bool LDS>
__global__ void __launch_bounds__(kSampleBlock) cloud_scaling_sample_kernel(const CloudScalingArgs a) {
  extern __shared__ double staged[];
  const int ncol = a.ncol, nlay = a.nlay, ngpt = a.ngpt, nbin = a.nq, nfsd = a.nfsd;
  if constexpr (LDS) {
    for (int t = threadIdx.x; t < nfsd * nbin; t += kSampleBlock) staged[t] = a.values[t];
    __syncthreads();
  }
  const double *values = LDS ? staged : a.values;
  const long i = (long)blockIdx.x * kSampleBlock + threadIdx.x;
  if (i >= ncol) return;
  const unsigned long long c = (unsigned long long)(a.col0 + i);
  const unsigned c_lo = (unsigned)c, c_hi = (unsigned)(c >> 32), k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
  const int nq = (ngpt + 3) >> 2;   // (uniform)
  unsigned rank[NQ][4];             // r(l, g) * 2^24
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) rank[q][j] = 0u;
  bool prev_cloudy = false;
  for (int l = 0; l < nlay; ++l) {
    const long cell = i + (long)ncol * l;
    const double cf = a.cloud_frac[cell];
    const bool cloudy = cf > 0.;   // (a NaN is a clear layer)
    float *const out = a.scaling + cell;
    const long plane = (long)ncol * nlay;
    unsigned long long word = 0ull;
    if (cloudy) {
      const bool linked = prev_cloudy;
      [[maybe_unused]] double alpha = 0.;
      if (EXP_RAN && linked) alpha = a.overlap_param[i + (long)ncol * (l - 1)];
      const double thresh = 1. - cf;
      draw_ranks<NQ, EXP_RAN>(rank, nq, linked, alpha, c_lo, c_hi, (unsigned)l, k0, k1);
      // the two rows around the cell's FSD and the weight of the upper one
      const double x = ((a.fsd ? a.fsd[cell] : a.fsd_const) - a.fsd0) / a.dfsd;
      int k = 0;
      double w = 0.;
      if (!(x > 0.)) { k = 0; w = 0.; }   // (a NaN lands here)
      else if (x >= (double)(nfsd - 1)) { k = nfsd - 2; w = 1.; }
      else { k = (int)x; w = x - (double)k; }
      const double *row = values + (long)k * nbin;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q < nq) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int g = 4 * q + j;
            if (g < ngpt) {
              const double r = (double)rank[q][j] * 0x1p-24;
              float s = 0.f;
              if (r >= thresh) {
                const double p = (r - thresh) / cf;
                int bin = (int)(p * (double)nbin);
                bin = bin < nbin - 1 ? bin : nbin - 1;
                const double v0 = row[bin], v1 = row[nbin + bin];
                s = (float)(v0 + w * (v1 - v0));
                word |= 1ull << g;
              }
              out[plane * g] = s;
            }
          }
        }
      }
    } else {
      for (int g = 0; g < ngpt; ++g) out[plane * g] = 0.f;
    }
    if (a.mask) a.mask[cell] = word;
    prev_cloudy = cloudy;
  }
}

template <int NQ>
hipError_t launch_scaling_nq(const CloudScalingArgs &a, hipStream_t s) {
  const unsigned blocks = (unsigned)(((long)a.ncol + kSampleBlock - 1) / kSampleBlock);
  const size_t bytes = sizeof(double) * (size_t)a.nfsd * (size_t)a.nq;
  const bool lds = bytes <= kCloudOpticsLdsBytes;
  typedef void (*K)(const CloudScalingArgs);
  const K k = a.exp_ran ? (lds ? cloud_scaling_sample_kernel<NQ, true, true> : cloud_scaling_sample_kernel<NQ, true, false>)
                        : (lds ? cloud_scaling_sample_kernel<NQ, false, true> : cloud_scaling_sample_kernel<NQ, false, false>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(kSampleBlock), lds ? bytes : 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_cloud_scaling_sample(const CloudScalingArgs &a, hipStream_t s) {
  if (a.ncol <= 0 || a.nlay <= 0) return hipSuccess;
  if (a.ngpt < 1 || a.ngpt > 64 || a.nfsd < 2 || a.nq < 1) return hipErrorInvalidValue;
  if (a.ngpt <= 32) return launch_scaling_nq<8>(a, s);
  if (a.ngpt <= 48) return launch_scaling_nq<12>(a, s);
  return launch_scaling_nq<16>(a, s);
}

hipError_t launch_cloud_mask_sample(int ncol, int nlay, int ngpt, int exp_ran, const double *cloud_frac, const double *overlap_param,
                                    unsigned long long seed, long long col0, unsigned long long *mask, hipStream_t s) {
  if (ncol <= 0 || nlay <= 0) return hipSuccess;
  if (ngpt < 1 || ngpt > 64) return hipErrorInvalidValue;
  // ranks in registers: 32 (the shipped 27- and 32-g models), 48 (36 g) or 64 of them
  if (ngpt <= 32) return launch_sample_nq<8>(ncol, nlay, ngpt, exp_ran, cloud_frac, overlap_param, seed, col0, mask, s);
  if (ngpt <= 48) return launch_sample_nq<12>(ncol, nlay, ngpt, exp_ran, cloud_frac, overlap_param, seed, col0, mask, s);
  return launch_sample_nq<16>(ncol, nlay, ngpt, exp_ran, cloud_frac, overlap_param, seed, col0, mask, s);
}

}  // namespace ecckd
