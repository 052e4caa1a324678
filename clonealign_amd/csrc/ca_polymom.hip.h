// ca_polymom.hip.h -- the series form's forward moments as device bodies that two launches share:
//   * ca_poly.hip's own kernels k_poly_B / k_poly_red (the fallback order: launches of their own in front of the count-matrix stream), and
//   * the MOMENT ROLE of the count-matrix stream's launch (k_ys_mfma_mom / k_ys_mfma_ovf_mom, ca_kernels.hip.h): nmb + nred blocks of that launch, from block
//     index blk0 on, make the moments beside the stream's blocks -- two launches and their boundaries less per iteration.  blk0 = 0: in front of the stream's
//     blocks (they hold slots before the stream fills the chip); blk0 = the stream's block count: BEHIND them (CA_VAR_MOM_LAST), in the slots the stream leaves free.
// One copy of the arithmetic: every output sees the same additions in the same order whichever launch runs it (32 genes per partial, genes in order inside an
// accumulator; the reduction's lane stride over the partials, eight loads in flight, the wave tree), so the two orders give the same bits.
//
// Hand-over inside the merged launch (the idiom of ca_fwdbal.hip.h: device-scope atomics and tagged words, never a grid barrier).  Counted from blk0, blocks
// [0, nmb) make the partials, blocks [nmb, nmb + nred) reduce them.  A moment block stores its partials (and block 0 the header) with DEVICE-SCOPE atomic stores, every wave waits
// until its stores are acknowledged (s_waitcnt vmcnt(0)), the block meets at its barrier, and thread 0 stores this launch's tag into the block's flag word (a
// device-scope atomic store as well).  A reducer polls the flag words of ALL moment blocks with relaxed device-scope loads until they hold the tag, passes ONE
// device-scope acquire fence and its own barrier, and then reads header and partials with device-scope atomic loads.
//   Why a reducer on one XCD sees a partial written on another: the XCDs' L2s are not coherent with each other, but a device-scope store is written THROUGH its
//   XCD's L2 to the memory side (the fabric, which all XCDs share), and it is acknowledged -- the wave's vmcnt reaches zero -- only once it is there; the tag is
//   stored after every wave of the block has seen that.  A device-scope load is served from the memory side, not from a line the reader's L2 or the CU's L1 may
//   still hold of LAST iteration's slab, and the acquire fence drops such lines for good measure.  So flag == tag implies the partials of that block are at the
//   memory side, and the reads behind the acquire go there.  (No release fence on the writer's side: every handed-over byte is a write-through store, and a
//   fence would write back the whole L2 -- beside the stream's traffic, the cost the round-5 note on k_poly_B warned of.)
//   Why the wait ends, in either order of the grid: every block a reducer waits for has a LOWER index than the reducer (the reducers are the role's last blocks
//   wherever the role sits), and a moment block depends on nobody -- once dispatched it runs to its flag store whatever else is resident.  In front (blk0 = 0)
//   the moment blocks are the launch's first and are dispatched before anything can hold a slot against them.  Behind the stream's blocks (CA_VAR_MOM_LAST) a
//   moment block may QUEUE: every slot its XCD has can be taken by stream blocks, overflow blocks or reducers.  Stream and overflow blocks depend on nobody
//   either and leave after a bounded time, and the nred reducers are far fewer than the launch's slots, so they alone can never hold every slot: a queued moment
//   block is simply dispatched later, when a stream block of its XCD leaves, at the latest when the stream has drained -- a reducer then waits that much longer
//   (a few tens of microseconds), in a slot no stream block is waiting for, because every stream block was dispatched before the first block of the role.  The
//   argument needs no residency of the role and no order of dispatch beyond "a block that depends on nobody gets a slot when one frees".
//   Nothing else waits on the role inside the launch: the stream's and the overflow list's blocks read nothing it writes.  Its other outputs are read after the
//   launch's end whichever blocks made them last -- tabB and the header by the cell launch, the ranges ring (mirror) by a host decision four passes later, bad_word
//   and the error word at the host's next synchronisation, and xbits (reset by reducer 0 once every moment block has published) by the next update launch.
//   The wait is bounded all the same (timeout_ticks, the s_memrealtime clock): on expiry the block stores the sticky error word, takes no further part (tabB keeps
//   what it held) and the host reports CA_ERR_STATE at its next synchronisation (comm_check).
#pragma once
#include "ca_poly.h"

// shape of the moment role (lab builds override): gene groups a moment block makes one after the other, and reducer blocks.  Both blocks' kinds hold one of the
// stream's block slots for a few microseconds each: fewer of them delay fewer of the stream's blocks, more of them finish the chain sooner.
#ifndef CA_MOM_PER
#define CA_MOM_PER 1
#endif
#ifndef CA_MOM_NRED
#define CA_MOM_NRED 21
#endif
constexpr int CA_PM_GPB = 32;                        // genes per partial
constexpr int CA_PM_NO = (CA_PL_R + 1) * 16;         // outputs of a partial and bin: (k, column) -- draw A clones 0..7 | draw B clones 0..7
constexpr int CA_PM_MAXW = 8;                        // most waves of a block that runs the moment body

// what the moment body keeps in LDS: carved out of the stream's dynamic buffer where it rides (never extra static LDS there: that is added to EVERY block of the launch)
struct ca_pm_lds {
  double pw[CA_PM_GPB][CA_PL_R + 1];
  double Mg[CA_PM_GPB][16];
  int binof[CA_PM_GPB];
  unsigned int present[(CA_PL_NB + 31) / 32];
  float smn[CA_PM_MAXW], smx[CA_PM_MAXW], sxm[CA_PM_MAXW];
  int gave_up;
};

struct ca_pm_args {
  // the moments' inputs and outputs (k_poly_B's argument list)
  const float* V; unsigned int* xbits; const float* muA; const float* muB; const float* Lb; int G, C;
  ca_poly_hdr* hdr; double* part; unsigned int* bad_word; double* mirror; double seq;
  const float* xpart; int nx; const double* xglob; int nglob; double xadd;
  // the riding form only
  double* tabB;
  unsigned int* flags;               // [nmb] this launch's tag once the block's partials are published (the workspace starts zeroed)
  unsigned int tag;                  // never 0
  int ngrp, per, nmb, nred;          // gene groups (partials), groups per moment block, moment blocks = ceil(ngrp / per), reducer blocks
  int blk0;                          // the role's first block index in the launch: 0 = in front of the stream's blocks, nb_main = behind them (CA_VAR_MOM_LAST)
  unsigned long long timeout_ticks;  // bound of a reducer's wait (s_memrealtime, 100 MHz)
  unsigned int* err;                 // mapped host word: set when a wait ran out
};

__device__ __forceinline__ float ca_pm_wmax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float ca_pm_wmin(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
// the ranges of one parameter state, for the host's look ahead (ca_poly_guard in the engine): values first, the sequence number last
__device__ __forceinline__ void ca_poly_mirror_store(double* m, double seq, double xmax, double vlo, double vhi) {
  __hip_atomic_store(m + 1, xmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(m + 2, vlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(m + 3, vhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
  __hip_atomic_store(m, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <bool PUB>
__device__ __forceinline__ void ca_pm_st(double* p, double v) {
  if (PUB) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *p = v;
}

// ---- bin geometry (every block makes the same one: min / max are exact in any order) and the forward moments of gene groups grp0 .. grp0 + ngrp - 1 ----------
// part[group][b][k][col] partials (the 1 / k! inside the powers), summed in group order by ca_pm_red_body into tabB[b][k][col].
// TB: the block's threads -- 384 (one thread per output) in k_poly_B, the stream's 256 where the body rides (threads 0 .. 79 then take a second output: an output's
// additions are its own thread's, in gene order, either way).  `first`: this block writes the header and the host's mirror.  PUB: device-scope stores (see above).
template <int TB, bool PUB>
__device__ __forceinline__ void ca_pm_B_body(const ca_pm_args& a, int grp0, int ngrp, bool first, ca_pm_lds& s) {
  constexpr int R = CA_PL_R, NB = CA_PL_NB, GPB = CA_PM_GPB, NO = CA_PM_NO;
  static_assert(TB % 64 == 0 && TB / 64 <= CA_PM_MAXW && TB >= GPB, "block shape of the moment body");
  const float* __restrict__ V = a.V;
  const int G = a.G, C = a.C, nx = a.nx, nglob = a.nglob;
  const int t = threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  {   // (eight loads in flight: a load per iteration waited for the one before -- 0.5 us each)
    constexpr int U = 8;
    for (int g0_ = 0; g0_ < G; g0_ += TB * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { const int g = g0_ + u * TB + t; v[u] = V[g < G ? g : G - 1]; }
#pragma unroll
      for (int u = 0; u < U; ++u) { mn = fminf(mn, v[u]); mx = fmaxf(mx, v[u]); }
    }
  }
  float xm = 0.f;
  {
    constexpr int U = 4;
    for (int i0 = 0; i0 < nx; i0 += TB * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { const int i = i0 + u * TB + t; v[u] = a.xpart[i < nx ? i : nx - 1]; }
#pragma unroll
      for (int u = 0; u < U; ++u) xm = fmaxf(xm, v[u]);
    }
  }
  mn = ca_pm_wmin(mn); mx = ca_pm_wmax(mx); xm = ca_pm_wmax(xm);
  if ((t & 63) == 0) { s.smn[t >> 6] = mn; s.smx[t >> 6] = mx; s.sxm[t >> 6] = xm; }
  if (t < (NB + 31) / 32) s.present[t] = 0u;
  __syncthreads();
  mn = s.smn[0]; mx = s.smx[0]; xm = s.sxm[0];
#pragma unroll
  for (int w_ = 1; w_ < TB / 64; ++w_) { mn = fminf(mn, s.smn[w_]); mx = fmaxf(mx, s.smx[w_]); xm = fmaxf(xm, s.sxm[w_]); }
  double xmax = nx > 0 ? (double)xm : (double)__uint_as_float(*a.xbits);
  if (nglob > 0) { xmax = 0.0; for (int r = 0; r < nglob; ++r) xmax = fmax(xmax, a.xglob[r]); xmax += a.xadd; }   // (uniform; a handful of ranks)
  const double width = (double)mx - (double)mn;
  int nb = (int)ceil(xmax * width / (2.0 * CA_PL_A));
  nb = nb < 1 ? 1 : (nb > NB ? NB : nb);
  const double delta = width > 0.0 ? width / nb : 1.0;
  // All loadings equal -- W = 0 at the start of every fit -- is one bin of width one CENTRED on the common value: vlo half a bin below it, so that the centre
  // formula of the three kernels, vlo + (b + 0.5) delta, gives v_b = v exactly (a float minus and plus 0.5 in float64), every gene has v - v_b = 0 and the series
  // is its first term: any |x| is covered.  (With vlo AT the common value the centre lay 0.5 above the genes and nothing bounded |0.5 x| by CA_PL_A.)
  const double vlo = width > 0.0 ? (double)mn : (double)mn - 0.5;
  const int bad = !(xmax * (width > 0.0 ? delta : 0.0) * 0.5 <= CA_PL_A * 1.25) || !isfinite(xmax) || !isfinite(width);
  if (first && t == 0) {
    ca_poly_hdr* hdr = a.hdr;
    ca_pm_st<PUB>(&hdr->vlo, vlo); ca_pm_st<PUB>(&hdr->delta, delta); ca_pm_st<PUB>(&hdr->xmax, xmax);
    if (PUB) __hip_atomic_store(&hdr->nb, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else hdr->nb = nb;
    if (bad) { hdr->bad = 1; if (a.bad_word) __hip_atomic_store(a.bad_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }   // (the host looks at its next synchronisation)
    if (a.mirror) ca_poly_mirror_store(a.mirror, a.seq, xmax, (double)mn, (double)mx);   // (the host's look ahead gets the true range)
  }
  for (int gi = 0; gi < ngrp; ++gi) {
    if (gi > 0) {   // (the block's next group: its LDS tables are read no more)
      __syncthreads();
      if (t < (NB + 31) / 32) s.present[t] = 0u;
      __syncthreads();
    }
    // this group's genes: bin, powers of (v - v_b) over k!, the sixteen M columns
    const int g0 = (grp0 + gi) * GPB;
    if (t < GPB) {
      const int g = g0 + t;
      if (g < G) {
        const double v = (double)V[g];
        int b = (int)floor((v - vlo) / delta);
        b = b < 0 ? 0 : (b >= nb ? nb - 1 : b);
        s.binof[t] = b;
        atomicOr(&s.present[b >> 5], 1u << (b & 31));
        const double dv = v - (vlo + ((double)b + 0.5) * delta);
        double p = 1.0;
#pragma unroll
        for (int k = 0; k <= R; ++k) { s.pw[t][k] = p; p = p * dv * (1.0 / (double)(k + 1)); }   // (the reciprocals are compile-time constants)
        const double ma = (double)a.muA[g], mb = (double)a.muB[g];
        for (int c = 0; c < 8; ++c) {
          const double l = c < C ? (double)a.Lb[(int64_t)g * CA_CW + c] : 0.0;
          s.Mg[t][c] = ma * l; s.Mg[t][8 + c] = mb * l;
        }
      } else s.binof[t] = -1;
    }
    __syncthreads();
    const int ng = min(GPB, G - g0);
    double* mine = a.part + (int64_t)(grp0 + gi) * NB * NO;
    for (int o = t; o < NO; o += TB) {
      const int k = o >> 4, col = o & 15;
      // ONE pass over the group's genes for the first four bins (the usual case is one to three): four accumulators, genes in order
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      if (nb == 1) {   // (uniform: one bin, no selects)
#pragma unroll 8
        for (int i = 0; i < ng; ++i) a0 += s.pw[i][k] * s.Mg[i][col];
      } else {
#pragma unroll 4
        for (int i = 0; i < ng; ++i) {
          const double pr = s.pw[i][k] * s.Mg[i][col];
          const int bi = s.binof[i];
          a0 += bi == 0 ? pr : 0.0; a1 += bi == 1 ? pr : 0.0; a2 += bi == 2 ? pr : 0.0; a3 += bi == 3 ? pr : 0.0;
        }
      }
      ca_pm_st<PUB>(mine + 0 * NO + o, a0);
      if (nb > 1) ca_pm_st<PUB>(mine + 1 * NO + o, a1);
      if (nb > 2) ca_pm_st<PUB>(mine + 2 * NO + o, a2);
      if (nb > 3) ca_pm_st<PUB>(mine + 3 * NO + o, a3);
      for (int b = 4; b < nb; ++b) {          // (a wide exponent range)
        double acc = 0.0;
        if ((s.present[b >> 5] >> (b & 31)) & 1u)
          for (int i = 0; i < ng; ++i) acc += s.binof[i] == b ? s.pw[i][k] * s.Mg[i][col] : 0.0;
        ca_pm_st<PUB>(mine + (int64_t)b * NO + o, acc);
      }
    }
  }
}

// ---- fixed-order sums of the partials: one wave per output, lanes stride over the partials, then the wave's tree (same order every time) ----------------------
// mode 0: plain sum (tabB); mode 1: sum / k! with k = (j / C) % (R + 2) (tabQ = Q_k / k!).  Waves wave0, wave0 + nwave, ... of the outputs: WHICH wave sums an
// output does not enter its value.  DEV: the partials are read with device-scope loads (the riding form, see above).  PUB: the outputs are stored with
// device-scope stores -- blocks of the SAME launch read them behind a hand-over (ca_polygene.hip.h).
template <bool DEV, bool PUB = false>
__device__ __forceinline__ void ca_pm_red_body(const double* __restrict__ part, int nblk, int64_t stride, int nout, int mode, int C, double* __restrict__ out,
                                               int wave0, int nwave) {
  const int lane = threadIdx.x & 63;
  auto ld = [&](const double* p) -> double {
    if (DEV) return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return *p;
  };
  for (int j = wave0; j < nout; j += nwave) {
    // (up to eight loads in flight per lane: a miss to another XCD's data costs a microsecond, a chain of them is the kernel)
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int blk = lane + 64 * u; v[u] = blk < nblk ? ld(part + (int64_t)blk * stride + j) : 0.0; }
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) a += v[u];
    for (int blk = lane + 512; blk < nblk; blk += 64) a += ld(part + (int64_t)blk * stride + j);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) {
      if (mode == 1) {
        const int k = (j / C) % (CA_PL_R + 2);
        double f = 1.0;
        for (int i = 2; i <= k; ++i) f *= (double)i;
        a /= f;
      }
      ca_pm_st<PUB>(out + j, a);
    }
  }
}

// ---- the moment role of the count-matrix stream's launch: block blk < nmb + nred of the role (counted from a.blk0 by the caller) in a TB-thread launch,
// `lds` = the launch's dynamic buffer
template <int TB>
__device__ __forceinline__ void ca_pm_ride_block(const ca_pm_args& a, int blk, unsigned char* lds) {
  ca_pm_lds& s = *reinterpret_cast<ca_pm_lds*>(lds);
  const int t = threadIdx.x;
  if (blk < a.nmb) {
    const int grp0 = blk * a.per;
    ca_pm_B_body<TB, true>(a, grp0, min(a.per, a.ngrp - grp0), blk == 0, s);
    // every byte handed over was stored write-through (device-scope atomic stores): no release fence, whose write-back of the XCD's L2 would wait on the
    // stream's dirty lines -- the wave only waits until its own stores are acknowledged ...
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();      // ... every wave of the block has ...
    if (t == 0) __hip_atomic_store(a.flags + blk, a.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... and only then the block's tag
    return;
  }
  // a reducer: all moment blocks have lower indices; each runs to its flag store once dispatched, and none waits for a slot for ever (the header's argument)
  if (t == 0) s.gave_up = 0;
  __syncthreads();
  {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int i = t; i < a.nmb; i += TB) {
      while (__hip_atomic_load(a.flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != a.tag) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks) {
          __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          s.gave_up = 1;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // nothing read from here on comes from a line cached before the tags were seen
  __syncthreads();
  if (s.gave_up) return;  // (uniform: the sticky word is set, tabB keeps what it held, the host reports CA_ERR_STATE)
  const int r = blk - a.nmb;
  if (r == 0 && t == 0) *a.xbits = 0u;   // (its readers, the moment blocks, are complete: ready for the next state's maximum)
  const int nb = __hip_atomic_load(&a.hdr->nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ca_pm_red_body<true>(a.part, a.ngrp, (int64_t)CA_PL_NB * CA_PM_NO, nb * CA_PM_NO, 0, a.C, a.tabB, r * (TB / 64) + (t >> 6), a.nred * (TB / 64));
}
