// gas_fused_body.hpp -- the device code of the fused gas-optics kernels: the LDS layout, the pressure point, the item
// sequence and the body that walks tiles, segments and slab positions.  One definition for gas_fused_kernel
// (kernels_gas_fused.hip: every wave does all the work of its columns) and gas_roles_kernel (kernels_gas_roles.hip: tau
// waves and source waves share a block), so that both produce the same bits.  What the kernel computes and how it maps
// onto the machine is described at the top of kernels_gas_fused.hip.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <type_traits>

#include "kernels.hpp"
#include "wave_pair.hpp"

namespace ecckd {
namespace {

#ifndef ECCKD_FUSED_BLOCK
#define ECCKD_FUSED_BLOCK 512
#endif
constexpr int kBlock = ECCKD_FUSED_BLOCK;   // threads of a block = columns of a tile in the longwave mode; the others take kBlockSw
// The shortwave and tau-only modes (no Planck items: 162-185 VGPRs at two waves per SIMD) fit three waves per SIMD with few
// or no spills (168 VGPRs; 6-28 spilled registers in fp64, outside the loops; none in single precision): blocks of 768
// threads.  Same box, profiles/r03_ab_gas_blocks_f32.txt, r03_ab_gas_blocks2.txt: shortwave gas optics 1.29 -> 1.10 ms in
// fp64 and 1.17 -> 0.89 ms in fp32 at 1e5 columns, tau-only 7.38 -> 7.10 ms at 1e6.  The longwave shape cannot afford the
// registers (102 spilled: +10 %; single precision: no gain) and keeps 512.
#ifndef ECCKD_FUSED_BLOCK_SW
#define ECCKD_FUSED_BLOCK_SW 768
#endif
constexpr int kBlockSw = ECCKD_FUSED_BLOCK_SW;
#ifndef ECCKD_FUSED_SEG
#define ECCKD_FUSED_SEG 8
#endif
#ifndef ECCKD_FUSED_SEG_MAX
#define ECCKD_FUSED_SEG_MAX 64
#endif
// Tiles between two slab-range checks (pre-pass + block barriers).  kSeg sizes the grid (enough blocks for small
// column counts); the segment a block actually walks is TauArgs::seg = its whole tile range up to kSegMax -- measured at
// 1e6 columns: 4 / 8 / 16 / 32 tiles per segment = 13.51 / 13.27 / 13.06 / 12.92 ms.
constexpr int kSeg = ECCKD_FUSED_SEG;
constexpr int kSegMax = ECCKD_FUSED_SEG_MAX;

// Compile-time loop: f(integral_constant<int, I>) for I = I0 .. N-1, as straight-line code.  The
// item pipeline below must be fully unrolled (its buffer indices and item kinds are static);
// `#pragma unroll` silently gives up on a body this large.
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// Order of the items of a chunk.  Item INDICES are: [0, NLI) look_up_table gas (g-pair p, vmr plane h: index 2p + h),
// [NLI, NLI+NBI) bilinear slots, then NPI Planck items (g-pair p: index p).  Every g-pair ends
// in stores: tau once its last slot is in, three source planes per Planck item.  The sequence: all look_up_table
// items, then the bilinear items (slot outer, g-pair inner) with the Planck items spread between them.  Against all
// Planck items at the end (the stores of a chunk in one burst of 16-20 KiB per wave) that measured -0.4 % in fp64 and
// -5.5 % in fp32; g-pair-major order (four stores every tenth item) spilled 29 VGPRs in the 8-g-point double
// instantiation and measured equal in fp64, 2 % slower in fp32 (round 2, same box).
// seq_item(pos) = index of the item at position pos of the chunk's sequence; bil_slot / bil_pair decode a bilinear index.
constexpr int seq_item(int pos, int NLI, int NBI, int NPI) {
  if (NPI == 0 || pos < NLI) return pos;
  int r = pos - NLI, b = 0, k = 0;   // r-th item after the look_up_table items
  for (int q = 0;; ++q) {
    // Planck item k follows bilinear item ((2k+1)*NBI)/(2*NPI) - 1
    const bool planck_next = k < NPI && b >= ((2 * k + 1) * NBI) / (2 * NPI);
    if (q == r) return planck_next ? NLI + NBI + k : NLI + b;
    if (planck_next) ++k; else ++b;
  }
}
constexpr int bil_slot(int b, int NP2) { return b / NP2; }
constexpr int bil_pair(int b, int NP2) { return b % NP2; }

template <typename real> __device__ __forceinline__ real selmin(real a, real b) { return a < b ? a : b; }
template <typename real> __device__ __forceinline__ real selmax(real a, real b) { return a > b ? a : b; }

struct FLayout {
  int tb, red, bil, SB, lut, SL, pl, SP, total;
};

// NB  = bilinear slots the kernel reads per row (>= nbil; the slab is followed by a pad so that the
//       zero-weight slots read finite data).
// ngp = g-points per row in LDS: ng rounded up to the chunk size GC (the tail stays zero).
// ntp = Planck rows held in LDS (the whole table, or the window FusedArgs::pw).
// Offsets are in elements of the LDS storage type; `wide` = sizeof(arithmetic type) / sizeof(storage type) (2 for the
// fp32 image of an fp64 call): the reduction scratch holds arithmetic-type values.
__host__ __device__ inline FLayout f_layout(int ngp, int np, int nt, int nbil, int NB, int nv_lut, int R, int ntp, int wide = 1, int waves = kBlock / 64) {
  FLayout L;
  L.tb = 0;
  L.red = (np + 1) & ~1;
  L.bil = L.red + 4 * waves * wide;
  L.SB = nbil > 0 ? row_stride(nbil * ngp) : 2;
  L.lut = L.bil + R * nt * L.SB + NB * ngp;
  L.SL = nv_lut > 0 ? row_stride(ngp) : 2;
  L.pl = L.lut + (nv_lut > 0 ? R * nt * nv_lut * L.SL : 0) + ngp;
  L.SP = row_stride(ngp);
  L.total = L.pl + (ntp > 0 ? ntp * L.SP : 0);
  return L;
}

template <typename real> struct PPoint { int ip0; real pw0, pw1; };
template <typename real> __device__ __forceinline__ PPoint<real> pressure_point(real p0, real p1, real lp0, const UDivT<real> &dlp, int np) {
  const real log_pressure = log(real(0.5) * (p1 + p0));                      // :120
  real pressure_index = udiv(log_pressure - lp0, dlp);
  pressure_index = real(1) + selmax(real(0), selmin(pressure_index, (real)np - real(1.0001)));
  PPoint<real> r;
  r.ip0 = (int)pressure_index;
  r.pw1 = pressure_index - r.ip0;
  r.pw0 = real(1) - r.pw1;
  return r;
}

enum { MODE_TAU = 0, MODE_LW = 1, MODE_SW = 2 };
constexpr int fused_block(int mode) { return mode == MODE_LW ? kBlock : kBlockSw; }

// "gas_slab_f32" = auto.  The fp64 slab holds R = 3 pressure rows next to the Planck table, the float32 image R = 8; the
// widening costs 9 % where 3 rows do (measured, round 3: 13.6 against 12.6 ms at 1e6 columns) and saves a factor 3.4
// where the columns of a wave are spread over more rows than a slab position serves (surface pressures of 50-103 kPa
// shuffled over the columns: 11.1 -> 3.3 ms at 2e5 columns).  spread_probe_kernel counts, at the bottom layer of the
// call (where the spread is largest), the waves of 64 columns whose pressure indices span three values or more; more than
// one wave in kSpreadOneIn -> the float32 image.  Both forms give the same bits, so the choice only moves time.
constexpr int kSpreadOneIn = 24;

// sreal: type of the tables in LDS.  = real, or float under a double kernel: every table of the ecCKD files is float32 on
// disk (widened exactly on read, mo_simple_netcdf.F90:44-142), so the slab and the Planck table can be staged as the
// float32 they are -- half the LDS -- and widened again (v_cvt_f64_f32, exact) when they are used: the same bits.  The
// host checks that every value is float32-representable (FusedArgs::slab32).
#ifndef ECCKD_F64_WAVES
#define ECCKD_F64_WAVES 2
#endif
#ifndef ECCKD_F32_WAVES
#define ECCKD_F32_WAVES 2
#endif
// The Planck sources of one g-pair from the four table rows read for it (b[0], b[1]: the layer's rows, b[2], b[3]: those of
// level j+1): the one expression of the fast path, whichever wave evaluates it.
template <typename real, typename vec2>
__device__ __forceinline__ void planck_pair_values(const vec2 *b, const PlPoint<real> &qlay, const PlPoint<real> &ql1, real pi, real rpi,
                                                   real (&vl)[2], real (&v1)[2]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    vl[q] = div_pi(qlay.w0 * (real)b[0][q] + qlay.w1 * (real)b[1][q], pi, rpi);
    v1[q] = div_pi(ql1.w0 * (real)b[2][q] + ql1.w1 * (real)b[3][q], pi, rpi);
  }
}

// Threads of a block of the wave-roles form (kernels_gas_roles.hip): the eight tau waves of a 512-column tile and four
// source waves.
constexpr int kRolesThreads = 768;

// The body of gas_fused_kernel (kernels_gas_fused.hip) and of gas_roles_kernel (kernels_gas_roles.hip).  BLOCK = columns of
// a tile.  ROLES = false: BLOCK threads, every wave does all the work of its 64 columns.  ROLES = true (fp64 longwave,
// FULL, no ANYCLAMP, fp64 slab): kRolesThreads threads over the same tile, segment, slab and LDS image -- waves
// 0 .. BLOCK/64 - 1 ("tau waves") do what the tau-only mode does for their 64 columns and store tau; wave BLOCK/64 + s
// ("source wave" s) computes and stores the Planck sources of the columns of tau waves 2s and 2s + 1, so that both kinds
// walk the same 4 KiB pieces of the output planes.  Back-pressure from the store path then parks mostly waves that have no
// arithmetic to lose ("Wave roles").
template <typename real, int GC, int NB, bool FULL, bool ANYCLAMP, int MODE, typename sreal, int BLOCK, bool ROLES>
__device__ __forceinline__ void gas_fused_body(const FusedArgs &a) {
  static_assert(!ROLES || (MODE == MODE_LW && FULL && !ANYCLAMP && sizeof(real) == 8 && sizeof(sreal) == 8 && BLOCK == 512),
                "wave roles: the fp64 longwave shape over the fp64 slab");
  // kBlock: columns of a tile; kThreads: threads of the block (strides of the block-wide loops); kWaves: its waves
  constexpr int kBlock = BLOCK, kThreads = ROLES ? kRolesThreads : BLOCK, kWaves = kThreads / 64, kTauWaves = BLOCK / 64;
  // the Planck items ride in the item pipeline of every wave (the fused form), or are the source waves' alone
  constexpr bool kPlanckItems = MODE == MODE_LW && !ROLES;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  sreal *lds = reinterpret_cast<sreal *>(lds_raw);
  typedef sreal double2_t __attribute__((ext_vector_type(2)));   // (two consecutive g-points as they sit in LDS)
  typedef __attribute__((address_space(3))) const volatile sreal lds_cvd;
  typedef __attribute__((address_space(3))) const volatile double2_t lds_cvd2;
  lds_cvd *lv = (lds_cvd *)lds;
  // two consecutive g-points in one ds_read_b128 (ds_read_b64 for a float32 image)
  // (at a BYTE address plus a compile-time element offset, the immediate of the ds_read)
  typedef __attribute__((address_space(3))) const volatile char lds_cvc;
  auto ld2b = [&](int bytes, int elem) -> double2_t { return *(lds_cvd2 *)((lds_cvc *)lv + bytes + elem * (int)sizeof(sreal)); };
  constexpr int WIDE = (int)(sizeof(real) / sizeof(sreal));
  if (a.choose) {   // "gas_slab_f32" = auto: both forms are launched, the spread probe's count says which one works
    const bool want32 = (long)a.choose[0] * kSpreadOneIn > (long)a.choose_total;
    if (want32 != (WIDE == 2)) return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wcol = (tid & ~63) + wave_column(lane);   // column of this thread inside a tile
  // (wave roles: a source wave; wave-uniform, so the role branch is a scalar one)
  const bool src_role = ROLES && __builtin_amdgcn_readfirstlane(wave) >= kTauWaves;
  (void)src_role;
  (void)kTauWaves;
  const int j = blockIdx.y;
  const TauArgs &t = a.tau;
  const int ncol = t.ncol, nlay = t.nlay, ng = t.ng, np = t.np, nt = t.nt, R = t.R;
  const int nv_lut = t.lut >= 0 ? t.seq[t.lut].nv : 0;
  const int ntp = MODE == MODE_LW ? a.ntp : 0;
  const int PW = MODE == MODE_LW ? a.pw : 0;   // Planck rows staged in LDS: ntp (whole table) or a window
  const int ngp = (ng + GC - 1) / GC * GC;
  const FLayout L = f_layout(ngp, np, nt, t.nbil, NB, nv_lut, R, PW, WIDE, kWaves);
  real *redd = reinterpret_cast<real *>(lds + L.red);
  // The argument structs carry `double` pointers and scalars; in the single-precision
  // instantiation the pointers address float data (host side casts) and the scalars are rounded.
  auto P = [](const double *p) { return reinterpret_cast<const real *>(p); };
  auto Q = [](double *p) { return reinterpret_cast<real *>(p); };
  const UDivT<real> ud_dlp = make_udiv_t<real>(a.ud_dlp), ud_dt = make_udiv_t<real>(a.ud_dt);
  const UDivT<real> ud_dlv = make_udiv_t<real>(a.ud_dlv), ud_pdt = make_udiv_t<real>(a.ud_pdt);
  const real lp0 = (real)t.lp0, gw = (real)t.gw, pt0 = (real)a.pt0;

  // Everything a zero-weight slot (unused bilinear slot, absent look_up_table gas) can read must
  // be finite: clear the whole allocation once, the staged rows overwrite their part.
  for (int i = tid; i < L.total; i += kThreads) lds[i] = sreal(0);
  __syncthreads();
  for (int i = tid; i < np; i += kThreads) lds[L.tb + i] = (sreal)P(t.temperature)[i];
  int pw_lo = -1;   // first table row of the staged Planck window (-1: nothing staged yet)
  // per-column inputs: wave-uniform row pointers (this block's layer) + 32-bit per-lane byte offsets
  typedef __attribute__((address_space(1))) const char gcchar_t;
  typedef __attribute__((address_space(1))) const real greal_t;
  gcchar_t *slot_base[NB + 1];
  unsigned slot_cs[NB + 1];
#pragma unroll
  for (int s = 0; s <= NB; ++s) {
    const SlotArgs &e = a.slot[s < NB ? s : kTauPassGases];
    slot_base[s] = (gcchar_t *)(P(e.vmr) + (long)j * e.ls);
    slot_cs[s] = e.cs_bytes;
  }

  const long ntiles = ((long)ncol + kBlock - 1) / kBlock;
  const long t_begin = ntiles * blockIdx.x / gridDim.x;
  const long t_end = ntiles * (blockIdx.x + 1) / gridDim.x;
  int slab_lo = -1;
  const real *plev0 = P(t.plev) + (long)ncol * j, *plev1 = P(t.plev) + (long)ncol * (j + 1);
  const real pi = (real)3.14159265359f, rpi = real(1) / pi;   // :53
  // The Planck sources of column cc, g-point g, with the table rows read from global memory (any row, staged or not): what
  // a wave with a lane outside the staged rows stores, one g-point at a time.
  auto planck_from_global = [&](int g, long cc, const PlPoint<real> &qlay, const PlPoint<real> &ql1) {
    const long o = cc + (long)ncol * (j + (long)nlay * g);
    const real *pg = P(a.planck) + g;
    Q(a.lay_source)[o] = div_pi(qlay.w0 * pg[(long)qlay.row * ng] + qlay.w1 * pg[(long)(qlay.row + 1) * ng], pi, rpi);
    if (a.tlev) {   // level j+1 -> inc of this layer and dec of the next
      const real v1 = div_pi(ql1.w0 * pg[(long)ql1.row * ng] + ql1.w1 * pg[(long)(ql1.row + 1) * ng], pi, rpi);
      const long lgs = a.lev_gstride, ol = cc + (long)ncol * j + lgs * g;   // (the level arrays' own g-plane stride)
      Q(a.lev_source_inc)[ol] = v1;
      if (j + 1 < nlay && lgs == (long)ncol * nlay) Q(a.lev_source_dec)[ol + ncol] = v1;   // one level buffer: the same word
    }
  };

  const int seg_len = t.seg;
  for (long seg = t_begin; seg < t_end; seg += seg_len) {
    const long seg_end = seg + seg_len < t_end ? seg + seg_len : t_end;
    // ---- pre-pass: range of p0+p1 over the segment; the pressure index is monotone in it ----
    // ... and, when only a window of the Planck table is staged, the range of the temperatures that
    // index it (layer j and its two levels); the table row is monotone in T.
    const bool windowed = MODE == MODE_LW && PW < ntp;
    real smin = real(3.0e38), smax = -real(3.0e38), tmin = real(3.0e38), tmax = -real(3.0e38);
    for (long tile = seg; tile < seg_end; ++tile) {
      const long c = tile * kBlock + tid;
      if ((!ROLES || tid < kBlock) && c < ncol) {   // (the source waves hold no column of their own: their range stays empty)
        const real sp = plev1[c] + plev0[c];
        smin = selmin(smin, sp);
        smax = selmax(smax, sp);
        if (windowed) {
          const real tl = P(t.tlay)[c + (long)ncol * j];
          tmin = selmin(tmin, tl);
          tmax = selmax(tmax, tl);
          if (a.tlev) {
            const real ta = P(a.tlev)[c + (long)ncol * j], tb = P(a.tlev)[c + (long)ncol * (j + 1)];
            tmin = selmin(tmin, selmin(ta, tb));
            tmax = selmax(tmax, selmax(ta, tb));
          }
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      smin = selmin(smin, __shfl_xor(smin, o));
      smax = selmax(smax, __shfl_xor(smax, o));
      if (windowed) {
        tmin = selmin(tmin, __shfl_xor(tmin, o));
        tmax = selmax(tmax, __shfl_xor(tmax, o));
      }
    }
    __syncthreads();   // the previous segment's LDS reads are done
    if (lane == 0) { redd[4 * wave] = smin; redd[4 * wave + 1] = smax; redd[4 * wave + 2] = tmin; redd[4 * wave + 3] = tmax; }
    __syncthreads();
    smin = redd[0]; smax = redd[1]; tmin = redd[2]; tmax = redd[3];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      smin = selmin(smin, redd[4 * w]); smax = selmax(smax, redd[4 * w + 1]);
      tmin = selmin(tmin, redd[4 * w + 2]); tmax = selmax(tmax, redd[4 * w + 3]);
    }
    if (MODE == MODE_LW) {
      // rows [pw_lo, pw_lo + PW) of the Planck table; a lane needs rows r and r + 1
      int want = pw_lo;
      if (!windowed) {
        want = 0;
      } else if (tmin <= tmax) {
        const int rlo = planck_point<real>(tmin, pt0, ud_pdt, ntp).row, rhi = planck_point<real>(tmax, pt0, ud_pdt, ntp).row + 1;
        if (pw_lo < 0 || rlo < pw_lo || rhi > pw_lo + PW - 1) {
          // centre the range if it fits, else start at its low end (the rest takes the slow path)
          const int slack = PW - (rhi - rlo + 1);
          want = rlo - (slack > 0 ? slack / 2 : 0);
          want = want < 0 ? 0 : (want > ntp - PW ? ntp - PW : want);
        }
      } else if (pw_lo < 0) {
        want = 0;
      }
      if (want != pw_lo) {   // block-uniform: every thread holds the same reduced range
        pw_lo = want;
        for (int q = tid; q < PW * ng; q += kThreads) {
          const int r = q / ng, g = q - r * ng;
          lds[L.pl + r * L.SP + g] = (sreal)P(a.planck)[(long)(pw_lo + r) * ng + g];
        }
      }
    }
    int ipmin = 1, ipmax = 0;
    if (smin <= smax) {
      // same expression as pressure_point(): log(0.5*(p1+p0)); 0 + s == s exactly
      ipmin = pressure_point<real>(real(0), smin, lp0, ud_dlp, np).ip0;
      ipmax = pressure_point<real>(real(0), smax, lp0, ud_dlp, np).ip0;
    }
    // Entry `o` of the merged table (TauArgs::merge_*).  The slab staging and the tables-from-global-memory path both
    // go through this one expression: a column gets the same bits whichever path its wave takes.
    auto merged_coef = [&](long o) -> real {
      real v = (real)t.merge_mult[0] * P(t.seq[t.merge_seq[0]].coef)[o];
      for (int k = 1; k < t.nmerge; ++k) v = fma((real)t.merge_mult[k], P(t.seq[t.merge_seq[k]].coef)[o], v);
      return v;
    };
    auto stage_slab = [&](int lo) {   // pressure rows [lo, lo + R) of every active table -> LDS
      slab_lo = lo;
      const int rows_b = R * nt;
      const int items_b = rows_b * t.nbil;
      for (int q = wave; q < items_b; q += kWaves) {
        const int s = q % t.nbil, rb = q / t.nbil;
        const int ipl = rb % R, it = rb / R;
        const long row = (long)ng * ((slab_lo + ipl) + (long)np * it);
        // a row holds [g-point chunk][slot][GC g-points]: inside a chunk every (slot, g-point) is a compile-time
        // offset from the four corner addresses of the cell
        sreal *dst = lds + L.bil + rb * L.SB + s * GC;
        const int cs = t.nbil * GC;
        if (s == t.merge_slot) {   // sum_k mult_k * coefficient_k: the call-constant gases as one table
          // (never with a float32 image under a double kernel: the sums are not float32 numbers -- the host keeps the two apart)
          for (int g = lane; g < ng; g += 64) dst[(g / GC) * cs + g % GC] = (sreal)merged_coef(row + g);
        } else {
          const real *src = P(t.seq[t.bil_seq[s]].coef) + row;
          for (int g = lane; g < ng; g += 64) dst[(g / GC) * cs + g % GC] = (sreal)src[g];
        }
      }
      if (t.lut >= 0) {
        const real *coef = P(t.seq[t.lut].coef);
        const int rows_l = rows_b * nv_lut;
        for (int q = wave; q < rows_l; q += kWaves) {
          const int ipl = q % R, itv = q / R;
          const real *src = coef + (long)ng * ((slab_lo + ipl) + (long)np * itv);
          sreal *dst = lds + L.lut + q * L.SL;
          for (int g = lane; g < ng; g += 64) dst[g] = (sreal)src[g];
        }
      }
    };
    // A slab serves R - 1 consecutive values of the pressure index.  When the columns of the
    // segment span more (orography), the segment is walked once per slab POSITION: a wave handles
    // a tile in the pass whose position holds all of its lanes; a wave whose lanes straddle two
    // positions handles it once, in the pass of its lowest lane, through the slow path.
    const int span = R >= 2 ? R - 1 : 1;
    const int npos = (R >= 2 && ipmin <= ipmax) ? (ipmax - ipmin + span) / span : 1;
    for (int pos = 0; pos < npos; ++pos) {
    const int pos_lo = npos > 1 ? ipmin + pos * span : -0x40000000;   // pressure indices of this pass
    const int pos_hi = npos > 1 ? pos_lo + span - 1 : 0x40000000;
    if (pos > 0) __syncthreads();   // the previous pass's LDS reads are done
    if (R >= 2 && ipmin <= ipmax) {
      if (npos > 1) {
        const int lo = min(pos_lo - 1, np - R);
        if (lo != slab_lo) stage_slab(lo);
      } else if (!(slab_lo >= 0 && ipmin - 1 >= slab_lo && ipmax <= slab_lo + R - 1)) {
        stage_slab(min(ipmin - 1, np - R));
      }
    }
    __syncthreads();

    // The per-column inputs of a tile, one round of global loads: 14 values in the headline shape.
    // "gas_input_ahead": a wave issues the loads of its NEXT tile once the set-up of the tile in hand has consumed nx_*, and
    // holds the values across the chunk loops -- vector memory operations retire in order, so a load issued at the top of
    // a tile, after the previous tile's 64 stores, waits for all of them and then for its own round trip; issued a tile
    // ahead, only the first wait is left.  It pays while the values stay in registers (round 1: +1-2 %; with first-layer
    // code in the kernel every later attempt spilled and lost: DESIGN.md section 5.1, section 8), so it is compiled into
    // the 512-thread instantiations only -- the 768-thread ones sit at their cap of 168 VGPRs.  Beyond the last tile of
    // the loop the column is clamped (cc32): nothing is read out of bounds, and the values are dropped.
    constexpr bool kAhead = BLOCK == 512 && !ROLES;
    real nx_p0, nx_p1, nx_T, nx_W[NB], nx_vlut, nx_Tl1 = real(0);
    bool nx_loaded = false;   // nx_* hold the inputs of the tile about to start (wave-uniform)
    auto load_inputs = [&](long tile) {
      const long c = tile * kBlock + wcol;
      const unsigned cc32 = (unsigned)(c < ncol ? c : (long)ncol - 1);
      const unsigned co = cc32 * (unsigned)sizeof(real);
      auto at = [&](const real *row) { return *reinterpret_cast<greal_t *>((gcchar_t *)row + co); };
      nx_p0 = at(plev0); nx_p1 = at(plev1);
      nx_T = at(P(t.tlay) + (long)ncol * j);
#pragma unroll
      for (int s = 0; s < NB; ++s) nx_W[s] = *reinterpret_cast<greal_t *>(slot_base[s] + cc32 * slot_cs[s]);
      nx_vlut = *reinterpret_cast<greal_t *>(slot_base[NB] + cc32 * slot_cs[NB]);
      if (kPlanckItems && a.tlev) nx_Tl1 = at(P(a.tlev) + (long)ncol * (j + 1));
    };

    // Wave roles: a tile of source wave s = wave - kTauWaves.  It serves two sets of 64 columns, those of tau waves 2s and
    // 2s + 1, one after the other: tlay(j) and tlev(j+1) of both sets in one round of loads, then per set the two Planck
    // points and, g-pair by g-pair, four LDS reads, the expression of planck_pair_values and the paired stores to
    // lay_source and to level j+1 (FusedArgs::lev_gstride: one store into a level buffer, two into separate arrays, none
    // without tlev).  A set with columns beyond ncol stores lane by lane (store_pair's masked form); a set with a lane
    // outside the staged Planck window goes through planck_from_global, all its lanes at once; a set without columns is
    // skipped.  Nothing is carried from tile to tile (the tau waves sit at their register cap), and there is no barrier
    // in here.
    auto source_tile = [&](long tile) __attribute__((always_inline)) {
      if constexpr (ROLES) {
        constexpr int ES = (int)sizeof(sreal);
        const bool upper = lane >= 32;
        const unsigned plane = (unsigned)ncol * (unsigned)nlay, lplane = (unsigned)a.lev_gstride;
        const long plane2 = 2L * plane, plane2_lev = 2L * lplane;
        const bool has_next = j + 1 < nlay && lplane == plane;
        const int set0 = 2 * (__builtin_amdgcn_readfirstlane(wave) - kTauWaves);
        long cs[2];
        real Ts[2], Tls[2];
#pragma unroll
        for (int set = 0; set < 2; ++set) {
          cs[set] = tile * kBlock + (set0 + set) * 64 + wave_column(lane);
          const unsigned co = (unsigned)(cs[set] < ncol ? cs[set] : (long)ncol - 1) * (unsigned)sizeof(real);   // (clamped: never out of bounds)
          auto at = [&](const real *row) { return *reinterpret_cast<greal_t *>((gcchar_t *)row + co); };
          Ts[set] = at(P(t.tlay) + (long)ncol * j);
          Tls[set] = a.tlev ? at(P(a.tlev) + (long)ncol * (j + 1)) : real(0);
        }
#pragma unroll
        for (int set = 0; set < 2; ++set) {
          const long c = cs[set];
          const bool valid = c < ncol;
          if (!__any(valid)) continue;
          const long cc = valid ? c : (long)ncol - 1;
          PlPoint<real> qlay = planck_point<real>(Ts[set], pt0, ud_pdt, ntp);
          PlPoint<real> ql1 = a.tlev ? planck_point<real>(Tls[set], pt0, ud_pdt, ntp) : qlay;
          const int rmin = min(qlay.row, ql1.row), rmax = max(qlay.row, ql1.row);
          const bool inwin = rmin >= pw_lo && rmax + 1 <= pw_lo + PW - 1;
          if (!__any(valid && !inwin)) {
            // (a lane beyond ncol carries the rows of column ncol - 1, which may lie outside the window: it reads the
            // window's first rows instead -- finite values, never stored)
            qlay.off = inwin ? (qlay.row - pw_lo) * L.SP : 0;
            ql1.off = inwin ? (ql1.row - pw_lo) * L.SP : 0;
            int ap[4] = {ES * (L.pl + qlay.off), ES * (L.pl + qlay.off + L.SP), ES * (L.pl + ql1.off), ES * (L.pl + ql1.off + L.SP)};
            const unsigned coff = (unsigned)sizeof(real) * (unsigned)cc;
            const unsigned voff = (unsigned)sizeof(real) * ((unsigned)(c - (upper ? 1 : 0)) + (upper ? plane : 0u));
            const unsigned voff_lev = (unsigned)sizeof(real) * ((unsigned)(c - (upper ? 1 : 0)) + (upper ? lplane : 0u));
            real *w_lay = Q(a.lay_source) + (long)ncol * j;
            real *w_inc = a.tlev ? Q(a.lev_source_inc) + (long)ncol * j : nullptr;
            real *w_decn = a.tlev ? Q(a.lev_source_dec) + (long)ncol * (j + 1) : nullptr;    // has_next
            auto pairs = [&](auto masked_c) __attribute__((always_inline)) {
              constexpr bool masked = decltype(masked_c)::value;
              for (int gb = 0; gb < ngp; gb += GC) {
                asm volatile("" : "+v"(ap[0]), "+v"(ap[1]), "+v"(ap[2]), "+v"(ap[3]));
                static_for<0, GC / 2>([&](auto p_c) __attribute__((always_inline)) {
                  constexpr int g = 2 * decltype(p_c)::value;
                  const double2_t b[4] = {ld2b(ap[0], g), ld2b(ap[1], g), ld2b(ap[2], g), ld2b(ap[3], g)};
                  real vl[2], v1[2];
                  planck_pair_values<real>(b, qlay, ql1, pi, rpi, vl, v1);
                  store_pair<real>(w_lay, plane2, voff, coff, vl[0], vl[1], masked, valid);
                  if (a.tlev) {                                                    // :423-424
                    store_pair<real>(w_inc, plane2_lev, voff_lev, coff, v1[0], v1[1], masked, valid);
                    if (has_next) store_pair<real>(w_decn, plane2, voff, coff, v1[0], v1[1], masked, valid);
                  }
                });
#pragma unroll
                for (int q = 0; q < 4; ++q) ap[q] += ES * GC;
              }
            };
            if (!__all(valid)) pairs(std::true_type{}); else pairs(std::false_type{});
          } else {
            for (int g = 0; g < ng; ++g)
              if (valid) planck_from_global(g, cc, qlay, ql1);
          }
        }
      }
    };

    for (long tile = seg; tile < seg_end; ++tile) {
      // "gas_tile_sync": the waves of the block meet once per tile, so that they walk the tile's output planes (4 KiB per
      // plane and block, 512 B of it per wave) together instead of drifting apart over the segment.  Every wave passes
      // this barrier exactly once per (segment, slab position, tile), because it stands before anything a wave decides for
      // itself (the `own` early-out, fast / lowest, masked or unmasked chunk loop) and the trip counts of the three
      // enclosing loops are the same in every thread of the block:
      //   seg, seg_end <- t_begin, t_end (blockIdx.x, gridDim.x, ncol: block-uniform) and t.seg (kernel argument);
      //   npos         <- R (kernel argument) and ipmin, ipmax, which every thread computes with the same operations from
      //                   the same LDS words redd[0 .. 4 * kWaves) after the block barrier that follows their writes;
      //   the flag     <- a kernel argument (uniform over the grid).
      // No wave leaves the kernel before its last tile, and the early return of the "gas_slab_f32" = auto form above is
      // taken by whole grids.  A bare execution barrier: no LDS is exchanged here, so there is no fence and no wait for the
      // stores in flight -- in the code object the sequence is s_load_dword, s_waitcnt lgkmcnt(0), s_cmp, s_cbranch,
      // s_barrier in all 56 instantiations, no vmcnt wait.
      // The flag is read from the kernel-argument segment once per tile (the kernel's only argument starts at offset 0)
      // instead of from `a`: as one more scalar held over the tile loop it costs the register allocator, which already
      // spills 100-250 scalars here, 148 more spilled SGPRs over the instantiations, a VGPR in four of them and scratch in
      // two; re-read per tile, the listings stay where the parent's are (profiles/gas_tile_sync_kernel_resources_*.txt).
      // "gas_input_ahead" is read the same way, for the same reason.
      typedef __attribute__((address_space(4))) const char karg_c;
      typedef __attribute__((address_space(4))) const volatile int karg_i;
      {
        const int tile_sync = *(karg_i *)((karg_c *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(FusedArgs, tile_sync));
        if (tile_sync) __builtin_amdgcn_s_barrier();
      }
      // Wave roles.  The barrier above stands BEFORE the role branch, inside the one tile loop that all twelve waves walk:
      // a source wave passes it once per (segment, slab position, tile) exactly as a tau wave does -- the three trip counts
      // above do not depend on the wave -- also in the slab positions after the first, where it has nothing to do, in
      // tiles where its columns do not exist, and when its lanes take the global-memory form.  Neither role holds a
      // barrier of its own, source_tile() contains none, and the block barriers of the segment and slab-position loops
      // stand outside the tile loop, in code every wave runs.  No role returns before the last tile.
      if constexpr (ROLES) {
        if (src_role) {
          if (pos == 0) source_tile(tile);   // the sources do not depend on the slab: stored in the first position only
          continue;
        }
      }
      const long c = tile * kBlock + wcol;   // (see wave_column)
      const bool valid = c < ncol;
      const bool upper = lane >= 32;        // this lane stores plane g+1 of its column pair
      const long cc = c < ncol ? c : (long)ncol - 1;
      // ---- setup: one round of global loads (unless the previous trip issued them) ----
      if (!(kAhead && nx_loaded)) load_inputs(tile);
      nx_loaded = false;
      const real p0 = nx_p0, p1 = nx_p1, Tlayer = nx_T;
      real W[NB];        // per-slot vmr, then weight (:143-149); 0 for unused slots
#pragma unroll
      for (int s = 0; s < NB; ++s) W[s] = nx_W[s];
      real vlut = nx_vlut;
      const real Tl1 = nx_Tl1;

      const PPoint<real> pp = pressure_point<real>(p0, p1, lp0, ud_dlp, np);
      const int ip0 = pp.ip0;
      // Lanes this pass is responsible for: existing columns whose pressure index belongs to the slab
      // position of the pass (with a single position: every existing column).
      // (a lane whose pressure index lies outside the range the pre-pass found -- only a NaN pressure does
      // that: min/max skip it -- is assigned to the nearest position and sends its wave down the slow path:
      // its column comes out NaN like the oracle's, and no lane is ever dropped)
      const int ipq = ipmin <= ipmax ? (ip0 < ipmin ? ipmin : (ip0 > ipmax ? ipmax : ip0)) : ip0;
      const bool own = valid && ipq >= pos_lo && ipq <= pos_hi;
      if (!__any(own)) {   // nothing of this wave in this pass
        continue;
      }
      const bool lowest = !__any(valid && ipq < pos_lo);   // this is the pass of the wave's lowest lane
      const bool stray_wave = __any(valid && (ipq != ip0 || ipmin > ipmax));
      // (lanes of other passes are carried along with a clamped row: finite values, never stored)
      int ipl = ip0 - 1 - slab_lo;
      const bool inslab = (R >= 2) && slab_lo >= 0 && ipl >= 0 && ipl + 1 <= R - 1;
      ipl = ipl < 0 ? 0 : (ipl > R - 2 ? (R >= 2 ? R - 2 : 0) : ipl);

      const real t0 = pp.pw0 * (real)lds[L.tb + ip0 - 1] + pp.pw1 * (real)lds[L.tb + ip0];   // :131-132
      real temperature_index = udiv(Tlayer - t0, ud_dt);
      temperature_index = real(1) + selmax(real(0), selmin(temperature_index, (real)nt - real(1.0001)));
      const int it0 = (int)temperature_index;
      const real tw1 = temperature_index - it0;
      const real tw0 = real(1) - tw1;
      const real dp = p1 - p0;
      const real simple_weight = gw * dp;   // :143

      // corner weights, multiplied out once per cell
      const real a00 = tw0 * pp.pw0, a10 = tw0 * pp.pw1, a01 = tw1 * pp.pw0, a11 = tw1 * pp.pw1;
      real l000 = real(0), l100 = real(0), l010 = real(0), l110 = real(0), l001 = real(0), l101 = real(0), l011 = real(0), l111 = real(0);
      int iv0 = 1;
      if (t.lut >= 0) {   // :153-163
        const SeqGas &e = t.seq[t.lut];
        vlut = fma((real)a.slot[kTauPassGases].alpha, vlut, (real)a.slot[kTauPassGases].beta);
        const real log_vmr = log(selmax(vlut, (real)e.mf0));
        real vmr_index = udiv(log_vmr - (real)e.log_mf0, ud_dlv);
        vmr_index = real(1) + selmax(real(0), selmin(vmr_index, (real)e.nv - real(1.001)));
        iv0 = (int)vmr_index;
        const real vw1 = vmr_index - iv0, vw0 = real(1) - vw1;
        real wl = simple_weight * vlut;   // :148
        if (!ANYCLAMP) wl = wl < real(0) ? real(0) : wl;
        const real u0 = ANYCLAMP ? vw0 : wl * vw0, u1 = ANYCLAMP ? vw1 : wl * vw1;
        l000 = u0 * a00; l100 = u0 * a10; l010 = u0 * a01; l110 = u0 * a11;
        l001 = u1 * a00; l101 = u1 * a10; l011 = u1 * a01; l111 = u1 * a11;
        if (ANYCLAMP) vlut = wl;   // keep the weight; applied (and clamped) per g-point
      }
#pragma unroll
      for (int s = 0; s < NB; ++s) {
        const SlotArgs &e = a.slot[s];
        real x = simple_weight * fma((real)e.alpha, W[s], (real)e.beta);   // :143-149, see SlotArgs
        if (!ANYCLAMP) x = x < real(0) ? real(0) : x;   // od<0 -> 0 (:234-238) == weight<0 -> 0 for tables >= 0
        W[s] = x;
      }
      PlPoint<real> qlay{0, 0, real(0), real(0)}, ql1{0, 0, real(0), real(0)};
      bool inwin = true;
      if (kPlanckItems) {
        qlay = planck_point<real>(Tlayer, pt0, ud_pdt, ntp);
        // level j+1 serves lev_source_inc(:,j,:) AND lev_source_dec(:,j+1,:) (the same level: :419-424), so a
        // block evaluates ONE level per layer; the top level (lev_source_dec of layer 1) and the surface source
        // belong to no layer and are planck_edge_kernel's (kernels_planck.hip).
        ql1 = a.tlev ? planck_point<real>(Tl1, pt0, ud_pdt, ntp) : qlay;
        const int rmin = min(qlay.row, ql1.row), rmax = max(qlay.row, ql1.row);
        inwin = rmin >= pw_lo && rmax + 1 <= pw_lo + PW - 1;
        qlay.off = (qlay.row - pw_lo) * L.SP;
        ql1.off = (ql1.row - pw_lo) * L.SP;
      }
      const real moles = dp * gw;   // :313-314 (SW)
      // A wave with a lane that no slab position can serve (outside the Planck window, or no slab at
      // all) goes through the tables-from-global-memory path, all its lanes at once, in the pass of
      // its lowest lane.  Every other wave runs the item pipeline in each pass it owns lanes of:
      // all 64 lanes owned -> paired 16-byte stores, else the owned lanes store on their own.
      const bool slow_wave = __any(valid && !(inwin && R >= 2 && slab_lo >= 0)) || stray_wave;
      const bool fast = !slow_wave;
      const bool active = own && inslab;
      const bool masked_wave = !__all(active);
      const int ip0_ = ip0, it0_ = it0, iv0_ = iv0;

      if (kAhead) {   // nx_* are consumed: the next tile's inputs, ahead of this tile's stores
        const int ahead = *(karg_i *)((karg_c *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(FusedArgs, input_ahead));
        if (ahead) {
          load_inputs(tile + 1);
          nx_loaded = true;
        }
      }

      if (fast) {
        // The g-point work of a chunk is a static sequence of "items" of at most four 16-byte LDS
        // reads (two consecutive g-points each):
        //   look_up_table gas : (g-pair, vmr plane h)   4 corner reads, 8 FMAs  -> partial / final od
        //   bilinear slot     : (slot, g-pair)          4 corner reads, 10 FMAs
        //   Planck sources    : (g-pair)                layer + level j+1 (4 reads)
        // software-pipelined by hand: the reads of item i+1 are issued before the arithmetic of item
        // i.  Reads are volatile (kept in program order, never paired into ds_read2_b64) and every
        // item ends in an empty asm that pins its results, otherwise instruction selection floats
        // all arithmetic below all reads.  Four reads per item (not eight) keep the two read buffers
        // at 32 VGPRs.
        static_assert(GC % 4 == 0, "chunks are made of g-point pairs");
        constexpr int NP2 = GC / 2;                                  // g-pairs per chunk
        constexpr int NLI = 2 * NP2, NBI = NB * NP2;
        // LDS addresses (in elements): one register per corner row of the cell -- 4 for the bilinear slots, 8 for the
        // look_up_table gas, 4 for the Planck rows -- advanced once per chunk; everything
        // inside a chunk is an immediate offset of the ds_read.  (Until round 2 the slot offset s*ngp was a run-time
        // value: 80 v_add_u32 per chunk of eight g-points.)
        const int ob = L.bil + (ipl + R * (it0 - 1)) * L.SB;
        const int ol = t.lut >= 0 ? L.lut + (ipl + R * ((it0 - 1) + nt * (iv0 - 1))) * L.SL : L.bil;
        const int dPb = L.SB, dTb = R * L.SB;
        const int dPl = t.lut >= 0 ? L.SL : 0, dTl = t.lut >= 0 ? R * L.SL : 0, dVl = t.lut >= 0 ? R * nt * L.SL : 0;
        constexpr int ES = (int)sizeof(sreal);   // (the registers hold byte addresses)
        int ab[4] = {ES * ob, ES * (ob + dPb), ES * (ob + dTb), ES * (ob + dTb + dPb)};
        int al[8] = {ES * ol, ES * (ol + dPl), ES * (ol + dTl), ES * (ol + dTl + dPl),
                     ES * (ol + dVl), ES * (ol + dVl + dPl), ES * (ol + dVl + dTl), ES * (ol + dVl + dTl + dPl)};
        int ap[4] = {ES * (L.pl + qlay.off), ES * (L.pl + qlay.off + L.SP), ES * (L.pl + ql1.off), ES * (L.pl + ql1.off + L.SP)};
        const int cstride = ES * t.nbil * GC;   // a chunk of the bilinear row: [slot][GC]
        // Output addressing: a uniform plane pointer (SGPRs) plus ONE per-lane 32-bit byte
        // offset shared by all four arrays -- the lower half-wave writes column pairs of plane g, the upper
        // half-wave those of plane g+1 (see store_pair).  launch_gas_fused() checks that it fits 32 bits.
        const unsigned plane = (unsigned)ncol * (unsigned)nlay;
        const unsigned coff = (unsigned)sizeof(real) * (unsigned)cc;
        const unsigned voff = (unsigned)sizeof(real) * ((unsigned)(c - (upper ? 1 : 0)) + (upper ? plane : 0u));
        // running output pointers: (column 0, layer j, g-point 0), advanced by store_pair
        const long plane2 = 2L * plane;
        real *w_tau = Q(t.tau) + (long)ncol * j, *w_ssa = MODE == MODE_SW && t.ssa ? Q(t.ssa) + (long)ncol * j : nullptr;
        real *w_g = MODE == MODE_SW && t.ssa ? Q(t.g) + (long)ncol * j : nullptr;
        real *w_lay = kPlanckItems ? Q(a.lay_source) + (long)ncol * j : nullptr;
        // The level arrays have their own g-plane stride (FusedArgs::lev_gstride), so level j+1 is stored with its own
        // running pointer step and its own per-lane offset.  One level buffer (stride (nlay+1)*ncol, lev_source_inc ==
        // lev_source_dec + ncol): the store through w_inc IS lev_source_dec of layer j+1, and the second store goes.
        // (fp64 only: the single-precision instantiations keep separate arrays, and the code they had)
        constexpr bool kLevStride = MODE == MODE_LW && sizeof(real) == 8;
        const unsigned lplane = kLevStride ? (unsigned)a.lev_gstride : plane;
        const unsigned voff_lev = kLevStride ? (unsigned)sizeof(real) * ((unsigned)(c - (upper ? 1 : 0)) + (upper ? lplane : 0u)) : voff;
        const long plane2_lev = 2L * lplane;
        const bool has_next = j + 1 < nlay && lplane == plane;
        real *w_decn = kPlanckItems && a.tlev ? Q(a.lev_source_dec) + (long)ncol * (j + 1) : nullptr;    // has_next
        real *w_inc = kPlanckItems && a.tlev ? Q(a.lev_source_inc) + (long)ncol * j : nullptr;
        // Two copies of the chunk loop: with every lane owned (the common case) the stores are the
        // unconditional paired ones; the masked copy is for ragged waves and waves split between
        // slab positions.  A run-time flag instead costs a branch per store and ~2 % of the kernel.
        auto chunks = [&](auto masked_c) __attribute__((always_inline)) {
        constexpr bool masked = decltype(masked_c)::value;
        constexpr int NPI = kPlanckItems ? NP2 : 0;
        constexpr int NIT = NLI + NBI + NPI;
        for (int gb = 0; gb < ngp; gb += GC) {
          real acc[GC];
          // (never in the longwave mode: the Planck sources ride with the FIRST pass only.  Compiled out there, because
          // with these loads in the chunk loop the compiler keeps an s_waitcnt vmcnt(0) at the join below, at the top of
          // EVERY chunk, and on the common path that wait is for the previous chunk's stores to be acknowledged:
          // the stores of a chunk then never overlap the arithmetic of the next.  Found in the disassembly late in round 2.)
          if (MODE != MODE_LW && t.accumulate) {   // second and later passes of a model with more gases than one pass takes
            typedef __attribute__((address_space(1))) const char gcchar;
            typedef __attribute__((address_space(1))) const real greal;
#pragma unroll
            for (int g = 0; g < GC; ++g) {
              acc[g] = real(0);
              if (FULL || gb + g < ng) {
                // uniform plane pointer + one 32-bit per-lane offset (see store_pair)
                gcchar *pl = (gcchar *)(P(t.tau) + (long)ncol * (j + (long)nlay * (gb + g)));
                asm volatile("" : "+s"(pl));
                acc[g] = *reinterpret_cast<greal *>(pl + coff);
              }
            }
          } else {
#pragma unroll
            for (int g = 0; g < GC; ++g) acc[g] = real(0);
          }
          // (pinned: otherwise the address arithmetic is re-derived per read from the row indices)
          asm volatile("" : "+v"(ab[0]), "+v"(ab[1]), "+v"(ab[2]), "+v"(ab[3]));
          asm volatile("" : "+v"(al[0]), "+v"(al[1]), "+v"(al[2]), "+v"(al[3]), "+v"(al[4]), "+v"(al[5]), "+v"(al[6]), "+v"(al[7]));
          if (kPlanckItems) asm volatile("" : "+v"(ap[0]), "+v"(ap[1]), "+v"(ap[2]), "+v"(ap[3]));
          double2_t buf[2][4];
          real lutp[2] = {real(0), real(0)};
          static_for<0, NIT + 1>([&](auto pos_c) __attribute__((always_inline)) {
            constexpr int pos = decltype(pos_c)::value;                       // position in the sequence
            constexpr int it = pos < NIT ? seq_item(pos, NLI, NBI, NPI) : NIT;    // item read at this position
            // ---------------- issue the reads of item `it` ----------------
            if constexpr (it < NLI) {                       // look_up_table gas: g-points 2*pr, 2*pr+1, vmr plane h
              constexpr int g = 2 * (it / 2), h = it & 1;
              double2_t *b = buf[pos & 1];
              b[0] = ld2b(al[4 * h], g); b[1] = ld2b(al[4 * h + 1], g); b[2] = ld2b(al[4 * h + 2], g); b[3] = ld2b(al[4 * h + 3], g);
            } else if constexpr (it < NLI + NBI) {          // one bilinear slot, one g-pair
              constexpr int so = bil_slot(it - NLI, NP2) * GC + 2 * bil_pair(it - NLI, NP2);
              double2_t *b = buf[pos & 1];
              b[0] = ld2b(ab[0], so); b[1] = ld2b(ab[1], so); b[2] = ld2b(ab[2], so); b[3] = ld2b(ab[3], so);
            } else if constexpr (it < NIT) {                // Planck sources of one g-pair: layer and level j+1
              constexpr int g = 2 * (it - NLI - NBI);
              double2_t *b = buf[pos & 1];
              b[0] = ld2b(ap[0], g); b[1] = ld2b(ap[1], g);
              b[2] = ld2b(ap[2], g); b[3] = ld2b(ap[3], g);
            }
            // ---------------- arithmetic of item `it - 1` ----------------
            if constexpr (pos >= 1) {
              constexpr int pi_ = seq_item(pos - 1, NLI, NBI, NPI);       // the item read at the previous position
              const double2_t *b = buf[(pos - 1) & 1];
              if constexpr (pi_ < NLI) {
                const int g0 = 2 * (pi_ / 2);
                if ((pi_ & 1) == 0) {
#pragma unroll
                  for (int q = 0; q < 2; ++q) {
                    real v = l000 * (real)b[0][q];
                    v = fma(l100, (real)b[1][q], v); v = fma(l010, (real)b[2][q], v); v = fma(l110, (real)b[3][q], v);
                    asm volatile("" : "+v"(v));
                    lutp[q] = v;
                  }
                } else {
#pragma unroll
                  for (int q = 0; q < 2; ++q) {
                    real v = lutp[q];
                    v = fma(l001, (real)b[0][q], v); v = fma(l101, (real)b[1][q], v); v = fma(l011, (real)b[2][q], v);
                    v = fma(l111, (real)b[3][q], v);
                    if (ANYCLAMP) { v = vlut * v; v = v < real(0) ? real(0) : v; }
                    acc[g0 + q] = acc[g0 + q] + v;
                    asm volatile("" : "+v"(acc[g0 + q]));
                  }
                }
              } else if constexpr (pi_ < NLI + NBI) {
                constexpr int s = bil_slot(pi_ - NLI, NP2), g0 = 2 * bil_pair(pi_ - NLI, NP2);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                  real v = a00 * (real)b[0][q];
                  v = fma(a10, (real)b[1][q], v); v = fma(a01, (real)b[2][q], v); v = fma(a11, (real)b[3][q], v);
                  if (ANYCLAMP) { v = W[s] * v; v = v < real(0) ? real(0) : v; acc[g0 + q] = acc[g0 + q] + v; }
                  else acc[g0 + q] = fma(W[s], v, acc[g0 + q]);
                  asm volatile("" : "+v"(acc[g0 + q]));
                }
                // tau of the whole chunk is complete after its last bilinear item
                if (pi_ == NLI + NBI - 1) {
#pragma unroll
                  for (int g = 0; g < GC; g += 2) {
                    // planes of this pair that exist: both, or (g-point counts that are not a multiple of the chunk) only the
                    // first one -- then the half-wave that holds it stores alone -- or none
                    const int npl = FULL ? 2 : ng - (gb + g);
                    if (FULL || npl >= 1) {
                      if (MODE == MODE_SW) {
                        const real r0 = moles * P(t.rayleigh)[gb + g], r1 = moles * P(t.rayleigh)[gb + g + 1];   // :316
                        const real t0_ = acc[g] + r0, t1_ = acc[g + 1] + r1;                                 // :456
                        store_pair<real>(w_tau, plane2, voff, coff, t0_, t1_, masked, active, npl, upper);
                        if (t.ssa) {                                                                          // :459-460
                          store_pair<real>(w_ssa, plane2, voff, coff, r0 / t0_, r1 / t1_, masked, active, npl, upper);
                          store_pair<real>(w_g, plane2, voff, coff, real(0), real(0), masked, active, npl, upper);
                        }
                      } else {
                        store_pair<real>(w_tau, plane2, voff, coff, acc[g], acc[g + 1], masked, active, npl, upper);
                      }
                    }
                  }
                }
              } else {
                constexpr int g = 2 * (pi_ - NLI - NBI);
                const int npl = FULL ? 2 : ng - (gb + g);   // planes of this pair that exist (see the tau stores)
                real vl[2], v1[2];
                planck_pair_values<real>(b, qlay, ql1, pi, rpi, vl, v1);
                if (FULL || npl >= 1) {
                  store_pair<real>(w_lay, plane2, voff, coff, vl[0], vl[1], masked, active, npl, upper);
                  if (a.tlev) {                                                    // :423-424
                    store_pair<real>(w_inc, plane2_lev, voff_lev, coff, v1[0], v1[1], masked, active, npl, upper);
                    if (has_next) store_pair<real>(w_decn, plane2, voff, coff, v1[0], v1[1], masked, active, npl, upper);
                  }
                }
              }
            }
          });
#pragma unroll
          for (int q = 0; q < 4; ++q) ab[q] += cstride;
#pragma unroll
          for (int q = 0; q < 8; ++q) al[q] += ES * GC;
#pragma unroll
          for (int q = 0; q < 4; ++q) ap[q] += ES * GC;
        }
        };
        if (masked_wave) chunks(std::true_type{}); else chunks(std::false_type{});
      } else if (lowest) {
        // ---- a lane of this wave is outside the staged rows: tables from global memory ----
        // (the indices go through an opaque asm: otherwise the 64-bit address arithmetic of this
        // rare path is speculated above the branch and paid by every tile)
        int ip0 = ip0_, it0 = it0_, iv0 = iv0_;
        asm volatile("" : "+v"(ip0), "+v"(it0), "+v"(iv0));
        for (int g = 0; g < ng; ++g) {
          const long o = cc + (long)ncol * (j + (long)nlay * g);
          real acc = t.accumulate ? P(t.tau)[o] : real(0);
          if (t.lut >= 0) {
            const SeqGas &e = t.seq[t.lut];
            const real *cp = P(e.coef) + (long)ng * ((ip0 - 1) + (long)np * ((it0 - 1) + (long)nt * (iv0 - 1))) + g;
            const long dP = ng, dT = (long)ng * np, dV = (long)ng * np * nt;
            real v = l000 * cp[0];
            v = fma(l100, cp[dP], v);
            v = fma(l010, cp[dT], v);
            v = fma(l110, cp[dT + dP], v);
            v = fma(l001, cp[dV], v);
            v = fma(l101, cp[dV + dP], v);
            v = fma(l011, cp[dV + dT], v);
            v = fma(l111, cp[dV + dT + dP], v);
            if (ANYCLAMP) { v = vlut * v; v = v < real(0) ? real(0) : v; }
            acc = acc + v;
          }
#pragma unroll
          for (int s = 0; s < NB; ++s) {
            if (s < t.nbil) {
              const long o00 = (long)ng * ((ip0 - 1) + (long)np * (it0 - 1)) + g;
              const long dP = ng, dT = (long)ng * np;
              real c00, c10, c01, c11;
              if (s == t.merge_slot) {
                c00 = merged_coef(o00); c10 = merged_coef(o00 + dP); c01 = merged_coef(o00 + dT); c11 = merged_coef(o00 + dT + dP);
              } else {
                const real *cp = P(t.seq[t.bil_seq[s]].coef) + o00;
                c00 = cp[0]; c10 = cp[dP]; c01 = cp[dT]; c11 = cp[dT + dP];
              }
              real v = a00 * c00;
              v = fma(a10, c10, v);
              v = fma(a01, c01, v);
              v = fma(a11, c11, v);
              if (ANYCLAMP) { v = W[s] * v; v = v < real(0) ? real(0) : v; acc = acc + v; }
              else acc = fma(W[s], v, acc);
            }
          }
          if (valid) {
            if (MODE == MODE_SW) {
              const real ray = moles * P(t.rayleigh)[g];
              const real tt = acc + ray;
              Q(t.tau)[o] = tt;
              if (t.ssa) { Q(t.ssa)[o] = ray / tt; Q(t.g)[o] = real(0); }
            } else {
              Q(t.tau)[o] = acc;
            }
            if (kPlanckItems) planck_from_global(g, cc, qlay, ql1);
          }
        }
      }
    }
    }   // slab positions
  }
}

}  // namespace
}  // namespace ecckd
