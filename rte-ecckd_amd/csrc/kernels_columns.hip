// kernels_columns.hip -- column compaction for the shortwave: select the daylit columns, gather a call's arrays to them,
// scatter the fluxes back with a fill value in the columns left out.
//
// No counterpart in the reference, whose shortwave driver computes the night columns with mu0 = 1 and zeroes them
// afterwards (ecckd_rfmip_sw.F90:103-108,143-145,156-161); a production host compacts in front of rte_sw.
//
// Mapping (gfx950): pure data movement, ordinary vector memory, no LDS beyond a block's four wave counts.
//  * Selection: three small launches.  (1) every block of 256 columns counts its daylit columns: one ballot + popcount per
//    wave, the four wave counts added through LDS.  (2) one block turns the block counts into exclusive offsets (shuffle scan
//    per wave, 256 counts per trip, a running carry) and stores the total.  (3) every block repeats its ballot and stores
//    column c at offset(block) + waves before + lanes before: output position k is the k-th daylit column whatever the
//    order in which blocks run -- no atomic counter anywhere.
//  * Gather: one thread per (inner, listed column), the inner index fastest, walking the outer index: stores are coalesced
//    along the list, loads go through the index (which ascends, so they are nearly so).  An index outside [0,ncol) is clamped.
//  * Scatter with fill: one thread per (inner, column of dst), so every element of dst is stored exactly once, in one pass
//    and coalesced; the thread finds its column in the ASCENDING list by bisection (log2(nday) loads that hit L2) and stores
//    the listed value or the fill.  A list entry outside [0,ncol) is never found, hence skipped; the list is only ever read at
//    positions [0,nday) and src only at listed positions, so no list content can make the kernel leave its arrays.
#include "kernels.hpp"

namespace ecckd {
namespace {

constexpr int kColBlock = 256;
constexpr int kColWaves = kColBlock / 64;
constexpr unsigned kColMinBlocks = 2048;   // blocks wanted in flight before a thread takes more than one outer index (not tuned)

// mu0 > mu0_min in double whatever the precision of mu0 (a NaN compares false: night)
template <typename real> __device__ __forceinline__ bool is_day(const real *mu0, int ncol, int c, double mu0_min) {
  return c < ncol && (double)mu0[c] > mu0_min;
}

template <typename real>
__global__ void __launch_bounds__(kColBlock) daylit_count_kernel(const real *mu0, int ncol, double mu0_min, int *block_count) {
  __shared__ int wave_count[kColWaves];
  const int c = blockIdx.x * kColBlock + threadIdx.x;
  const unsigned long long day = __ballot(is_day(mu0, ncol, c, mu0_min));
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(day);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int w = 0; w < kColWaves; ++w) n += wave_count[w];
    block_count[blockIdx.x] = n;
  }
}

// block_count(nblocks): counts in, exclusive offsets out; *total = their sum.  One block.
__global__ void __launch_bounds__(kColBlock) daylit_scan_kernel(int *block_count, int nblocks, int *total) {
  __shared__ int wave_sum[kColWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < nblocks; base += kColBlock) {
    const int i = base + threadIdx.x;
    const int v = i < nblocks ? block_count[i] : 0;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, chunk = 0;
    for (int w = 0; w < kColWaves; ++w) {
      if (w < wave) before += wave_sum[w];
      chunk += wave_sum[w];
    }
    if (i < nblocks) block_count[i] = carry + before + incl - v;
    carry += chunk;
    __syncthreads();   // (the next trip rewrites wave_sum)
  }
  if (threadIdx.x == 0) *total = carry;
}

template <typename real>
__global__ void __launch_bounds__(kColBlock) daylit_write_kernel(const real *mu0, int ncol, double mu0_min, const int *block_offset,
                                                                 int *day_index) {
  __shared__ int wave_count[kColWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * kColBlock + threadIdx.x;
  const bool mine = is_day(mu0, ncol, c, mu0_min);
  const unsigned long long day = __ballot(mine);
  if (lane == 0) wave_count[wave] = __popcll(day);
  __syncthreads();
  if (!mine) return;
  int at = block_offset[blockIdx.x] + __popcll(day & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) at += wave_count[w];
  day_index[at] = c;   // at < number of daylit columns <= ncol
}

__device__ __forceinline__ int clamp_column(int c, int ncol) { return c < 0 ? 0 : (c >= ncol ? ncol - 1 : c); }

// dst(i,k,o) = src(i,index(k),o)
template <typename T>
__global__ void __launch_bounds__(kColBlock) gather_columns_kernel(int ninner, int ncol, int nouter, int nday, const int *index,
                                                                   const T *src, T *dst) {
  const size_t dplane = (size_t)ninner * nday, splane = (size_t)ninner * ncol;
  const size_t q = (size_t)blockIdx.x * kColBlock + threadIdx.x;
  if (q >= dplane) return;
  const int k = (int)(q / ninner), i = (int)(q - (size_t)k * ninner);
  const size_t from = (size_t)clamp_column(index[k], ncol) * ninner + i;
  for (int o = blockIdx.y; o < nouter; o += gridDim.y) dst[(size_t)o * dplane + q] = src[(size_t)o * splane + from];
}

// dst(k,l) = src[index(k)*col_stride + l*lay_stride] (elements): a gas array as it crosses the ABI, to a dense (nday,nlay)
template <typename T>
__global__ void __launch_bounds__(kColBlock) gather_strided_kernel(int ncol, int nlay, int nday, const int *index, long long col_stride,
                                                                   long long lay_stride, const T *src, T *dst) {
  const int k = blockIdx.x * kColBlock + threadIdx.x;
  if (k >= nday) return;
  const long long from = (long long)clamp_column(index[k], ncol) * col_stride;
  for (int l = blockIdx.y; l < nlay; l += gridDim.y) dst[(size_t)l * nday + k] = src[from + (long long)l * lay_stride];
}

// dst(i,index(k),o) = src(i,k,o); dst(i,c,o) = fill for every column c the (ascending) list does not hold
template <typename T>
__global__ void __launch_bounds__(kColBlock) scatter_columns_kernel(int ninner, int ncol, int nouter, int nday, const int *index,
                                                                    const T *src, T *dst, T fill) {
  const size_t dplane = (size_t)ninner * ncol, splane = (size_t)ninner * nday;
  const size_t q = (size_t)blockIdx.x * kColBlock + threadIdx.x;
  if (q >= dplane) return;
  const int c = (int)(q / ninner), i = (int)(q - (size_t)c * ninner);
  int lo = 0, hi = nday;   // first position whose entry is not below c
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (index[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  const bool listed = lo < nday && index[lo] == c;
  const size_t from = (size_t)lo * ninner + i;
  for (int o = blockIdx.y; o < nouter; o += gridDim.y) dst[(size_t)o * dplane + q] = listed ? src[(size_t)o * splane + from] : fill;
}

// grid of `threads` threads along x, and along y as many walkers of the outer index as it takes to fill the device
dim3 column_grid(size_t threads, int nouter) {
  const size_t gx = (threads + kColBlock - 1) / kColBlock;
  size_t gy = gx >= kColMinBlocks ? 1 : (kColMinBlocks + gx - 1) / gx;
  if (gy > (size_t)nouter) gy = (size_t)nouter;
  return dim3((unsigned)gx, (unsigned)gy);
}

template <typename real>
hipError_t launch_daylit_t(const real *mu0, int ncol, double mu0_min, int *day_index, int *work, hipStream_t s) {
  const int nblocks = daylit_blocks(ncol);
  int *total = work, *block = work + 1;
  hipLaunchKernelGGL((daylit_count_kernel<real>), dim3(nblocks), dim3(kColBlock), 0, s, mu0, ncol, mu0_min, block);
  hipLaunchKernelGGL(daylit_scan_kernel, dim3(1), dim3(kColBlock), 0, s, block, nblocks, total);
  hipLaunchKernelGGL((daylit_write_kernel<real>), dim3(nblocks), dim3(kColBlock), 0, s, mu0, ncol, mu0_min, block, day_index);
  return hipGetLastError();
}

}  // namespace

int daylit_blocks(int ncol) { return (ncol + kColBlock - 1) / kColBlock; }
size_t daylit_work_bytes(int ncol) { return sizeof(int) * ((size_t)daylit_blocks(ncol) + 1); }

hipError_t launch_daylit_columns(const void *mu0, int f32, int ncol, double mu0_min, int *day_index, int *work, hipStream_t s) {
  if (ncol <= 0) return hipSuccess;
  return f32 ? launch_daylit_t(static_cast<const float *>(mu0), ncol, mu0_min, day_index, work, s)
             : launch_daylit_t(static_cast<const double *>(mu0), ncol, mu0_min, day_index, work, s);
}

hipError_t launch_gather_columns(int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *index, const void *src,
                                 void *dst, hipStream_t s) {
  if (elem_bytes != 4 && elem_bytes != 8) return hipErrorInvalidValue;
  if (ninner <= 0 || ncol <= 0 || nouter <= 0 || nday <= 0) return hipSuccess;
  const dim3 grid = column_grid((size_t)ninner * nday, nouter);
  if (elem_bytes == 8)
    hipLaunchKernelGGL((gather_columns_kernel<unsigned long long>), grid, dim3(kColBlock), 0, s, ninner, ncol, nouter, nday, index,
                       static_cast<const unsigned long long *>(src), static_cast<unsigned long long *>(dst));
  else
    hipLaunchKernelGGL((gather_columns_kernel<unsigned>), grid, dim3(kColBlock), 0, s, ninner, ncol, nouter, nday, index,
                       static_cast<const unsigned *>(src), static_cast<unsigned *>(dst));
  return hipGetLastError();
}

hipError_t launch_gather_strided(int ncol, int nlay, int elem_bytes, int nday, const int *index, long long col_stride,
                                 long long lay_stride, const void *src, void *dst, hipStream_t s) {
  if (elem_bytes != 4 && elem_bytes != 8) return hipErrorInvalidValue;
  if (ncol <= 0 || nlay <= 0 || nday <= 0) return hipSuccess;
  const dim3 grid = column_grid((size_t)nday, nlay);
  if (elem_bytes == 8)
    hipLaunchKernelGGL((gather_strided_kernel<unsigned long long>), grid, dim3(kColBlock), 0, s, ncol, nlay, nday, index, col_stride,
                       lay_stride, static_cast<const unsigned long long *>(src), static_cast<unsigned long long *>(dst));
  else
    hipLaunchKernelGGL((gather_strided_kernel<unsigned>), grid, dim3(kColBlock), 0, s, ncol, nlay, nday, index, col_stride,
                       lay_stride, static_cast<const unsigned *>(src), static_cast<unsigned *>(dst));
  return hipGetLastError();
}

hipError_t launch_scatter_columns(int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *index, const void *src,
                                  void *dst, double fill, hipStream_t s) {
  if (elem_bytes != 4 && elem_bytes != 8) return hipErrorInvalidValue;
  if (ninner <= 0 || ncol <= 0 || nouter <= 0) return hipSuccess;
  if (nday < 0) nday = 0;
  const dim3 grid = column_grid((size_t)ninner * ncol, nouter);
  if (elem_bytes == 8) {
    unsigned long long bits;
    __builtin_memcpy(&bits, &fill, 8);
    hipLaunchKernelGGL((scatter_columns_kernel<unsigned long long>), grid, dim3(kColBlock), 0, s, ninner, ncol, nouter, nday, index,
                       static_cast<const unsigned long long *>(src), static_cast<unsigned long long *>(dst), bits);
  } else {
    const float f = (float)fill;
    unsigned bits;
    __builtin_memcpy(&bits, &f, 4);
    hipLaunchKernelGGL((scatter_columns_kernel<unsigned>), grid, dim3(kColBlock), 0, s, ninner, ncol, nouter, nday, index,
                       static_cast<const unsigned *>(src), static_cast<unsigned *>(dst), bits);
  }
  return hipGetLastError();
}

}  // namespace ecckd
