// ca_eng_launch.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): one launch site per templated kernel family of the loop (matrix-core sweeps, fused forward sweeps and their riding streams, cell epilogues): the argument list once, the instantiation picked from the engine's picks.
//
// Each family: `..._t<...>` holds the family's one hipLaunchKernelGGL; `launch_...` maps the engine's picks to an instantiation.  The dispatch names exactly the
// combinations that exist (a cross product would add kernels, minutes of compile time and megabytes of code object); a pick that ca_eng_create.inc never makes
// falls to the last branch of its level.
inline ca_small_args no_small_args() { ca_small_args a; memset(&a, 0, sizeof(a)); return a; }

// calls f with the exponent dimension as a constant: 1 .. DMAX, any other D as DMAX
template <int DMAX, typename Fn>
int with_d(int D, Fn&& f) {
  static_assert(DMAX == 2 || DMAX == 4, "");
  if (D == 1) return f(std::integral_constant<int, 1>());
  if constexpr (DMAX == 2) return f(std::integral_constant<int, 2>());
  else {
    if (D == 2) return f(std::integral_constant<int, 2>());
    if (D == 3) return f(std::integral_constant<int, 3>());
    return f(std::integral_constant<int, 4>());
  }
}

// ---- k_bwd_mfma<TL, D, FRAC, C16, S2>: the matrix-core backward sweep ------------------------
// what rides on a sweep's first launch as extra block rows behind the sweep's own: a pending monitor pass's tail, the count-matrix stream's finishing sums
struct ca_bwdm_extra { ca_small_args tail; ca_yfin_args yfin; int rows; };
// one launch of the sweep: a sample (or both, S2), or a sample and a pair of clone chunks
struct ca_bwdm_ops {
  const unsigned short* coefq; const float* Lb; const float* mu; int sidx, first_s;
  const ca_bwdm_extra* extra;      // non-null: this launch is the sweep's first and carries the extra block rows
  const unsigned short* coefq1;    // C16 / S2: the third-part image of coef
  const float* mu1;                // S2: the second sample's mu
  bool frac, c16, s2, tl3;         // the form: two-part copy numbers, sixteen clones, both samples in one sweep, three gene tiles per wave
};
template <int TL, int DD, bool FRAC, bool C16, bool S2>
int bwd_mfma_t(ca_engine* h, const ca_bwdm_ops& o) {
  ca_yfin_args no_yfin;
  memset(&no_yfin, 0, sizeof(no_yfin));
  LAUNCH(h, CA_KERNEL_BWD,
         hipLaunchKernelGGL((k_bwd_mfma<TL, DD, FRAC, C16, S2>), dim3(cdiv(h->nwt, CA_TB / 64), h->csplit_m + (o.extra ? o.extra->rows : 0)), dim3(CA_TB),
                            (size_t)h->cchunk_m * 4 * DD * sizeof(float) * (S2 ? 2 : 1), h->stream, o.coefq, h->F, h->etamax2, o.Lb, o.mu, h->Vs, h->V, h->gpart,
                            h->dFpart, h->N, h->G, h->cchunk_m, h->S, o.sidx, o.first_s, o.extra ? 1 : 0, o.extra ? o.extra->tail : no_small_args(), h->csplit_m,
                            o.extra ? o.extra->yfin : no_yfin, o.coefq1, o.mu1));
  return CA_OK;
}
// D = 1, 2: CA_BWD_TL tiles per wave in every form, three in the plain form of small problems; D = 3, 4: the three-tile wave (CA_BWD_TL_D34), plain or two-part
int launch_bwd_mfma(ca_engine* h, int D, const ca_bwdm_ops& o) {
  return with_d<4>(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    if constexpr (DD <= 2) {
      if (o.c16) return bwd_mfma_t<CA_BWD_TL, DD, false, true, false>(h, o);
      if (o.s2) return o.frac ? bwd_mfma_t<CA_BWD_TL, DD, true, false, true>(h, o) : bwd_mfma_t<CA_BWD_TL, DD, false, false, true>(h, o);
      if (o.frac) return bwd_mfma_t<CA_BWD_TL, DD, true, false, false>(h, o);
      if (o.tl3) return bwd_mfma_t<3, DD, false, false, false>(h, o);
      return bwd_mfma_t<CA_BWD_TL, DD, false, false, false>(h, o);
    } else {
      return o.frac ? bwd_mfma_t<CA_BWD_TL_D34, DD, true, false, false>(h, o) : bwd_mfma_t<CA_BWD_TL_D34, DD, false, false, false>(h, o);
    }
  });
}

// ---- k_fwd_mfma<D>: the matrix-core forward sweep into Z partials (D = 1, 2) -----------------
int launch_fwd_mfma(ca_engine* h, const unsigned short* Mq, float* Zp, int split, int kchunk) {
  const dim3 grid(cdiv(h->N, (CA_TB / 64) * CA_FM_TL * 16), split);
  return with_d<2>(h->D, [&](auto d) -> int {
    LAUNCH(h, CA_KERNEL_FWD, hipLaunchKernelGGL((k_fwd_mfma<decltype(d)::value>), grid, dim3(CA_TB), 0, h->stream, h->F, h->etamax2, h->Vs, Mq, Zp, h->N, h->G, kchunk, h->nk32));
    return CA_OK;
  });
}

// ---- k_fwd_cell<D, TL, C16, S2F> / k_fwd_cell_mix<D, TL, 2, C16, S2F>: sweep + cell epilogue in one kernel: no Z partials, one launch ------
template <int D, int TL, bool C16, bool S2F>
int fwd_cell_t(ca_engine* h, const ca_cell_ptrs& cp) {
  LAUNCH(h, CA_KERNEL_FWD, hipLaunchKernelGGL((k_fwd_cell<D, TL, C16, S2F>), dim3(h->ncblk_f), dim3(CA_TB), 0, h->stream, h->F, h->etamax2, h->Vs, h->Mq, cp,
                                              h->alpha_u, h->cell_part, h->N, h->C, h->K, h->nk32));
  return CA_OK;
}
template <int D, int TL, bool C16, bool S2F>
int fwd_cell_mix_t(ca_engine* h, const ca_cell_ptrs& cp) {
  LAUNCH(h, CA_KERNEL_FWD, hipLaunchKernelGGL((k_fwd_cell_mix<D, TL, 2, C16, S2F>), dim3(h->ncblk_f), dim3(CA_TB), 0, h->stream, h->F, h->etamax2, h->Vs, h->Mq, cp,
                                              h->alpha_u, h->cell_part, h->N, h->C, h->K, h->nk32, h->fc_nbig));
  return CA_OK;
}
// one block shape (fc_nbig = 0) or two (k_fwd_cell_mix); TL 2 and 6 exist for D = 1 .. 4, every other TL for D = 1, 2
template <int TL, int DMAX, bool MIX>
int fwd_cell_tl(ca_engine* h, const ca_cell_ptrs& cp) {
  return with_d<DMAX>(h->D, [&](auto d) {
    if constexpr (MIX) return fwd_cell_mix_t<decltype(d)::value, TL, false, false>(h, cp);
    else return fwd_cell_t<decltype(d)::value, TL, false, false>(h, cp);
  });
}
// 9..16 clones (C16) and mc_samples = 2 with four draws (S2F): the two default block shapes, D = 1, 2
template <bool C16, bool S2F>
int fwd_cell_wide(ca_engine* h, const ca_cell_ptrs& cp) {
  return with_d<2>(h->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    if (h->fc_nbig > 0) return fwd_cell_mix_t<D, 6, C16, S2F>(h, cp);
    return h->fc_tl == 6 ? fwd_cell_t<D, 6, C16, S2F>(h, cp) : fwd_cell_t<D, 2, C16, S2F>(h, cp);
  });
}
int launch_fwd_cell(ca_engine* h, const ca_cell_ptrs& cp, bool s2f) {
  if (h->c16) return fwd_cell_wide<true, false>(h, cp);
  if (s2f) return fwd_cell_wide<false, true>(h, cp);
  if (h->fc_nbig > 0)
    switch (h->fc_tl) {
      case 4: return fwd_cell_tl<4, 2, true>(h, cp);
      case 5: return fwd_cell_tl<5, 2, true>(h, cp);
      case 8: return fwd_cell_tl<8, 2, true>(h, cp);
      default: return fwd_cell_tl<6, 4, true>(h, cp);   // (D = 3, 4: this shape and the 32-cell one only)
    }
  switch (h->fc_tl) {
    case 1: return fwd_cell_tl<1, 2, false>(h, cp);
    case 2: return fwd_cell_tl<2, 4, false>(h, cp);
    case 4: return fwd_cell_tl<4, 2, false>(h, cp);
    case 5: return fwd_cell_tl<5, 2, false>(h, cp);
    case 6: return fwd_cell_tl<6, 4, false>(h, cp);
    default: return fwd_cell_tl<8, 2, false>(h, cp);
  }
}

// ---- the count-matrix stream riding on the fused forward sweep's launch ----------------------
// Block order of a launch the count-matrix stream rides on (ca_yride_args / ca_ysride_args: nb_main stream units, nb_y with the overflow list's blocks; nf
// sweep blocks); returns the grid's block count.
// Interleave of the two kinds in dispatch order.  Blocks go round-robin over the 8 XCDs, so a period that divides 8 (the
// obvious even / odd split) puts ALL sweep blocks on four XCDs and all stream blocks on the other four; two sweep blocks per
// stream block mixes them on every CU: cfg-3 2795 -> 3008 it/s, 12.5k cells 10.9k -> 12.1k, cfg-2 16.3k -> 17.9k
// (profiles/r02_ab_ystream.txt section 8).
// Long-lived stream blocks lead the grid (ca_yride_args::pers) when there are at least two units of the matrix per CU: one
// such block per CU measured best (cfg-3, with the non-temporal stream: 2:1 interleave 3090, 256 blocks 3147, 341 / 512
// blocks 3008 / 2979, 192 / 128 blocks 2790 / 2320 it/s).  ca_options.ride_pattern < 0 sets the number, > 0 asks for the interleave (a << 8 | b).
template <typename RideArgs>
unsigned ride_pattern(const ca_engine* h, RideArgs& ya, int nf) {
  const int rp = h->opt.ride_pattern;
  ya.pat_a = 2; ya.pat_b = 1;
  if (rp > 0 && (rp >> 8) > 0 && (rp & 255) > 0) { ya.pat_a = rp >> 8; ya.pat_b = rp & 255; }
  if (rp < 0) ya.pers = std::min(-rp, ya.nb_main);
  else if (rp == 0 && ya.nb_main >= 2 * h->n_cu) ya.pers = h->n_cu;
  return ya.pers > 0 ? (unsigned)(ya.pers + nf + (ya.nb_y - ya.nb_main)) : (unsigned)(nf + ya.nb_y);
}

// k_fwd_cell_mix_y<D, TLB, 2>: the vector stream's blocks interleaved with the sweep's (D = 1, 2; 128-, 96- or 32-cell big blocks)
template <int D, int TLB>
int fwd_cell_mix_y_t(ca_engine* h, const ca_cell_ptrs& cp, ca_yride_args& ya) {
  const dim3 grid(ride_pattern(h, ya, h->ncblk_f));
  LAUNCH(h, CA_KERNEL_FWD, hipLaunchKernelGGL((k_fwd_cell_mix_y<D, TLB, 2>), grid, dim3(CA_TB), 0, h->stream, h->F, h->etamax2, h->Vs, h->Mq, cp, h->alpha_u,
                                              h->cell_part, h->N, h->C, h->K, h->nk32, h->fc_nbig, h->ncblk_f, ya));
  return CA_OK;
}
int launch_fwd_cell_mix_y(ca_engine* h, const ca_cell_ptrs& cp, ca_yride_args& ya) {
  return with_d<2>(h->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    if (h->fc_tl == 8) return fwd_cell_mix_y_t<D, 8>(h, cp, ya);
    if (h->fc_tl == 6) return fwd_cell_mix_y_t<D, 6>(h, cp, ya);
    return fwd_cell_mix_y_t<D, 2>(h, cp, ya);
  });
}

// (one piece in flight per wave: 128 VGPRs = four waves per SIMD like the vector stream's launch; two pieces, 162 VGPRs and
//  three waves, measured 2824 against 2869 it/s at cfg-3 -- profiles/r03_ab_ystream.txt)
#ifndef CA_YS_RIDE_DEPTH
#define CA_YS_RIDE_DEPTH 1   // (lab: pieces in flight per stream wave)
#endif
// k_fwd_cell_mix_ys<D, TLB, 2, DEPTH, C16, S2F, Y4>: the one-copy int8 matrix-core stream's blocks interleaved with the sweep's
template <int D, int TLB, bool C16, bool S2F, bool Y4>
int fwd_cell_mix_ys_t(ca_engine* h, const ca_cell_ptrs& cp, ca_ysride_args& ya) {
  const dim3 grid(ride_pattern(h, ya, h->ncblk_f));
  LAUNCH(h, CA_KERNEL_FWD, hipLaunchKernelGGL((k_fwd_cell_mix_ys<D, TLB, 2, CA_YS_RIDE_DEPTH, C16, S2F, Y4>), grid, dim3(CA_TB), 0, h->stream, h->F, h->etamax2, h->Vs,
                                              h->Mq, cp, h->alpha_u, h->cell_part, h->N, h->C, h->K, h->nk32, h->fc_nbig, h->ncblk_f, ya));
  return CA_OK;
}
// (the 4-bit image rides only with the series form's shapes: D = 1, no c16 / s2 -- ride_ys, ca_eng_create.inc)
template <int D, int TLB, bool C16, bool S2F>
int fwd_cell_mix_ys_y4(ca_engine* h, const ca_cell_ptrs& cp, ca_ysride_args& ya) {
  if constexpr (D == 1 && !C16 && !S2F) { if (h->ys4) return fwd_cell_mix_ys_t<D, TLB, C16, S2F, true>(h, cp, ya); }
  return fwd_cell_mix_ys_t<D, TLB, C16, S2F, false>(h, cp, ya);
}
// 96- and 32-cell big blocks: D = 1, 2 in the plain, the sixteen-clone and the four-draw form; 16-cell ones: the plain form only
template <int TLB>
int fwd_cell_mix_ys_tl(ca_engine* h, const ca_cell_ptrs& cp, ca_ysride_args& ya, bool c16, bool s2f) {
  return with_d<2>(h->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    if constexpr (TLB != 1) {
      if (c16) return fwd_cell_mix_ys_y4<D, TLB, true, false>(h, cp, ya);
      if (s2f) return fwd_cell_mix_ys_y4<D, TLB, false, true>(h, cp, ya);
    }
    return fwd_cell_mix_ys_y4<D, TLB, false, false>(h, cp, ya);
  });
}
int launch_fwd_cell_mix_ys(ca_engine* h, const ca_cell_ptrs& cp, ca_ysride_args& ya, bool s2f) {
  if (h->fc_tl == 6) return fwd_cell_mix_ys_tl<6>(h, cp, ya, h->c16, s2f);
  if (h->fc_tl == 1 && !h->c16) return fwd_cell_mix_ys_tl<1>(h, cp, ya, false, false);
  return fwd_cell_mix_ys_tl<2>(h, cp, ya, h->c16, s2f);
}

// k_fwd_bal_ys<1, TL, DEPTH, Y4>: small problems, one eight-wave sweep block per CU with bal_q = TL tiles each, left-over tiles spread gene-wise (ca_fwdbal.hip.h);
// the grid: sweep blocks, stream blocks (ba.stream_units units each), the overflow list's (its own block order: ya's interleave fields stay unset)
template <int TL, bool Y4>
int fwd_bal_ys_t(ca_engine* h, const ca_cell_ptrs& cp, const ca_bal_args& ba, const ca_ysride_args& ya) {
  const dim3 grid((unsigned)(h->n_cu + (ba.stream_units == 2 ? (ya.nb_main + 1) / 2 : ya.nb_main) + (ya.nb_y - ya.nb_main)));
  LAUNCH(h, CA_KERNEL_FWD, hipLaunchKernelGGL((k_fwd_bal_ys<1, TL, CA_YS_RIDE_DEPTH, Y4>), grid, dim3(CA_BAL_TB), 0, h->stream, h->F, h->etamax2, h->Vs, h->Mq, cp,
                                              h->alpha_u, h->cell_part, h->N, h->C, h->K, h->nk32, ba, ya));
  return CA_OK;
}
template <int TL>
int fwd_bal_ys_y4(ca_engine* h, const ca_cell_ptrs& cp, const ca_bal_args& ba, const ca_ysride_args& ya) {
  return h->ys4 ? fwd_bal_ys_t<TL, true>(h, cp, ba, ya) : fwd_bal_ys_t<TL, false>(h, cp, ba, ya);
}
int launch_fwd_bal_ys(ca_engine* h, const ca_cell_ptrs& cp, const ca_bal_args& ba, const ca_ysride_args& ya) {
  switch (h->bal_q) {
    case 1: return fwd_bal_ys_y4<1>(h, cp, ba, ya);
    case 2: return fwd_bal_ys_y4<2>(h, cp, ba, ya);
    case 3: return fwd_bal_ys_y4<3>(h, cp, ba, ya);
    case 4: return fwd_bal_ys_y4<4>(h, cp, ba, ya);
    case 5: return fwd_bal_ys_y4<5>(h, cp, ba, ya);
    default: return fwd_bal_ys_y4<6>(h, cp, ba, ya);
  }
}

// ---- cell epilogues over Z partials: CP = the clone count rounded up to a power of two lanes per cell ------
// k_cell_par<CP> (plain pass, up to 64 clones): Z partials of the vector sweeps, or of the paired matrix-core sweeps (pfwd)
template <int CP>
int cell_par_t(ca_engine* h, const float* ywp, int ywseg, int mode) {
  LAUNCH(h, CA_KERNEL_CELL,
         hipLaunchKernelGGL((k_cell_par<CP>), dim3(h->ncblk), dim3(CA_TB), 0, h->stream, h->pfwd ? h->pf_Z : h->Zpart, h->A, h->cn, h->s64, h->etamax2, h->glogit,
                            h->alpha_u, h->F, ywp, h->YW, h->coef, h->dgl, h->cell_part, h->N, h->C, h->S, h->D, h->K, h->pfwd ? h->pf_fsplit : h->gsplit,
                            h->nchunk, ywseg, mode, h->bwd_mfma ? h->coefq : nullptr, h->N16, h->pfwd ? 1 : 0, (int64_t)h->S * cdiv(h->nchunk, 2) * h->N16 * 32));
  return CA_OK;
}
inline int clone_lanes(const ca_engine* h) { int CP = 1; while (CP < h->C) CP <<= 1; return CP; }
int launch_cell_par(ca_engine* h, const float* ywp, int ywseg, int mode) {
  switch (clone_lanes(h)) {
    case 1: return cell_par_t<1>(h, ywp, ywseg, mode);
    case 2: return cell_par_t<2>(h, ywp, ywseg, mode);
    case 4: return cell_par_t<4>(h, ywp, ywseg, mode);
    case 8: return cell_par_t<8>(h, ywp, ywseg, mode);
    case 16: return cell_par_t<16>(h, ywp, ywseg, mode);
    case 32: return cell_par_t<32>(h, ywp, ywseg, mode);
    default: return cell_par_t<64>(h, ywp, ywseg, mode);
  }
}
// k_cell_fused<CP> (fused two-draw pass over Zpart2, up to 8 clones)
template <int CP>
int cell_fused_t(ca_engine* h, const ca_cell_ptrs& cp) {
  LAUNCH(h, CA_KERNEL_CELL, hipLaunchKernelGGL((k_cell_fused<CP>), dim3(h->ncblk), dim3(CA_TB), 0, h->stream, h->Zpart2, h->frow, cp, h->alpha_u, h->cell_part, h->N,
                                               h->C, h->D, h->K, h->fwd_mfma ? h->fsplit : h->gsplit));
  return CA_OK;
}
int launch_cell_fused(ca_engine* h, const ca_cell_ptrs& cp) {
  switch (clone_lanes(h)) {
    case 1: return cell_fused_t<1>(h, cp);
    case 2: return cell_fused_t<2>(h, cp);
    case 4: return cell_fused_t<4>(h, cp);
    default: return cell_fused_t<8>(h, cp);
  }
}

// ---- k_fit_mse<YT>: the squared-error sweep over the resident matrix in its storage (ca_fit_mse; never the 4-bit loop image) ----
// the list of used cells (sorted by clone, M entries), the clone-major table and the partial slabs of one call; TR list entries per wave
struct ca_mse_ops { const ca_mse_row* meta; const double* Et; double *cellpart, *genepart; int64_t M; int TR, nrb, nrg; };
template <typename YT>
int fit_mse_t(ca_engine* h, const ca_mse_ops& o) {
  LAUNCH(h, CA_KERNEL_YPASS, hipLaunchKernelGGL((k_fit_mse<YT>), dim3((unsigned)((int64_t)o.nrg * h->nseg)), dim3(CA_TB), 0, h->stream, (const YT*)h->Y, o.meta, o.Et,
                                                h->ovf_col, h->ovf_val, o.cellpart, o.genepart, o.M, h->G, h->Gp, h->nseg, o.nrb, o.TR));
  return CA_OK;
}
int launch_fit_mse(ca_engine* h, const ca_mse_ops& o) {
  if (h->ystore == CA_YSTORE_U8) return fit_mse_t<uint8_t>(h, o);
  if (h->ystore == CA_YSTORE_U16) return fit_mse_t<uint16_t>(h, o);
  return fit_mse_t<float>(h, o);
}

// ---- k_logexpr<YT>: the log-expression sweep over the resident matrix in its storage (ca_logexpr_sums; never the 4-bit loop image) ----
// the list of used cells (sorted by group), its nrg block pieces (none crosses a group boundary) and the two partial slabs of one call
struct ca_lx_ops { const ca_mse_row* meta; const ca_lx_blk* blk; double *part1, *part2; int nrg; };
template <typename YT>
int logexpr_t(ca_engine* h, const ca_lx_ops& o) {
  LAUNCH(h, CA_KERNEL_YPASS, hipLaunchKernelGGL((k_logexpr<YT>), dim3((unsigned)((int64_t)o.nrg * h->nseg)), dim3(CA_TB), 0, h->stream, (const YT*)h->Y, o.meta, o.blk,
                                                h->ovf_col, h->ovf_val, o.part1, o.part2, h->G, h->Gp, h->nseg));
  return CA_OK;
}
int launch_logexpr(ca_engine* h, const ca_lx_ops& o) {
  if (h->ystore == CA_YSTORE_U8) return logexpr_t<uint8_t>(h, o);
  if (h->ystore == CA_YSTORE_U16) return logexpr_t<uint16_t>(h, o);
  return logexpr_t<float>(h, o);
}

// ---- k_clone_ll<YT, NC> / k_clone_ll_z<NC>: the log-likelihood sweep over the resident matrix in its storage and the contraction beside it (ca_clone_loglik; never the 4-bit loop image) ----
// one batch of cells [n_lo, n_lo + n_cnt): the table of NC columns per gene and group (log E | V, zero padded) with its E = 0 masks, the partial slabs
struct ca_ll_ops { const double* tab; const unsigned* zmask; const double* lgtab; double *part, *lgpart; int64_t n_lo, n_cnt; int NC, ngrp; };
template <typename YT, int NC>
int clone_ll_t(ca_engine* h, const ca_ll_ops& o) {
  LAUNCH(h, CA_KERNEL_YPASS, hipLaunchKernelGGL((k_clone_ll<YT, NC>), dim3((unsigned)((int64_t)cdiv(o.n_cnt, CA_TB) * h->nseg), (unsigned)o.ngrp), dim3(CA_TB), 0, h->stream,
                                                (const YT*)h->Y, o.tab, o.zmask, o.lgtab, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, h->ovf_col, h->ovf_val, o.part, o.lgpart,
                                                h->N, o.n_lo, o.n_cnt, h->G, h->Gp, h->nseg));
  return CA_OK;
}
template <typename YT>
int clone_ll_nc(ca_engine* h, const ca_ll_ops& o) {
  if (o.NC == 8) return clone_ll_t<YT, 8>(h, o);
  if (o.NC == 16) return clone_ll_t<YT, 16>(h, o);
  return clone_ll_t<YT, 32>(h, o);
}
int launch_clone_ll(ca_engine* h, const ca_ll_ops& o) {
  if (h->ystore == CA_YSTORE_U8) return clone_ll_nc<uint8_t>(h, o);
  if (h->ystore == CA_YSTORE_U16) return clone_ll_nc<uint16_t>(h, o);
  return clone_ll_nc<float>(h, o);
}
// the contraction Z of one batch (D > 0): NC clone columns per group of the table E
struct ca_llz_ops { const double *Ut, *Vt, *Ez; double *zpart, *mpart; int64_t n_lo, n_cnt; int NC, ngrp, nzc; };
template <int NC>
int clone_ll_z_t(ca_engine* h, const ca_llz_ops& o) {
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_clone_ll_z<NC>), dim3((unsigned)cdiv(o.n_cnt, CA_TB), (unsigned)o.nzc, (unsigned)o.ngrp), dim3(CA_TB), 0, h->stream, o.Ut, o.Vt,
                                                o.Ez, o.zpart, o.mpart, o.n_lo, o.n_cnt, h->G, h->Gp));
  return CA_OK;
}
int launch_clone_ll_z(ca_engine* h, const ca_llz_ops& o) {
  if (o.NC == 8) return clone_ll_z_t<8>(h, o);
  if (o.NC == 16) return clone_ll_z_t<16>(h, o);
  return clone_ll_z_t<32>(h, o);
}
// ---- k_block_ll<YT, NC> / k_block_ll_z<NC>: the log-likelihood sweep by block of genes and the contraction beside it (ca_clone_loglik_by_block; never the 4-bit loop image) ----
// one batch of cells [n_lo, n_lo + n_cnt): k_clone_ll's table and masks, the run list (cuts, first run of every segment), the slab part[run][column][cell] of the nuse table columns in use + 2
struct ca_bll_ops { const double* tab; const unsigned* zmask; const double* lgtab; const int *rcut, *rseg; double* part; int64_t n_lo, n_cnt; int NC, ngrp, nuse; };
template <typename YT, int NC>
int block_ll_t(ca_engine* h, const ca_bll_ops& o) {
  LAUNCH(h, CA_KERNEL_YPASS, hipLaunchKernelGGL((k_block_ll<YT, NC>), dim3((unsigned)((int64_t)cdiv(o.n_cnt, CA_TB) * h->nseg), (unsigned)o.ngrp), dim3(CA_TB), 0, h->stream,
                                                (const YT*)h->Y, o.tab, o.zmask, o.lgtab, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, h->ovf_col, h->ovf_val, o.rcut, o.rseg, o.part,
                                                h->N, o.n_lo, o.n_cnt, h->G, h->Gp, h->nseg, o.nuse));
  return CA_OK;
}
template <typename YT>
int block_ll_nc(ca_engine* h, const ca_bll_ops& o) {
  if (o.NC == 8) return block_ll_t<YT, 8>(h, o);
  if (o.NC == 16) return block_ll_t<YT, 16>(h, o);
  return block_ll_t<YT, 32>(h, o);
}
int launch_block_ll(ca_engine* h, const ca_bll_ops& o) {
  if (h->ystore == CA_YSTORE_U8) return block_ll_nc<uint8_t>(h, o);
  if (h->ystore == CA_YSTORE_U16) return block_ll_nc<uint16_t>(h, o);
  return block_ll_nc<float>(h, o);
}
// the contraction Z of one batch by chunk (D > 0): NC clone columns per group of the table E, nzk chunks cut at label changes
struct ca_bllz_ops { const double *Ut, *Vt, *Ez; const int* zcut; double* zpart; int64_t n_lo, n_cnt; int NC, ngrp, nzk; };
template <int NC>
int block_ll_z_t(ca_engine* h, const ca_bllz_ops& o) {
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_block_ll_z<NC>), dim3((unsigned)((int64_t)cdiv(o.n_cnt, CA_TB) * o.nzk), (unsigned)o.ngrp), dim3(CA_TB), 0, h->stream, o.Ut, o.Vt,
                                                o.Ez, o.zcut, o.zpart, o.n_lo, o.n_cnt, h->Gp, o.nzk, h->C));
  return CA_OK;
}
int launch_block_ll_z(ca_engine* h, const ca_bllz_ops& o) {
  if (o.NC == 8) return block_ll_z_t<8>(h, o);
  if (o.NC == 16) return block_ll_z_t<16>(h, o);
  return block_ll_z_t<32>(h, o);
}
// ---- k_pair_ll<YT>: the pair-mixture sweep over the resident matrix in its storage (ca_clone_pair_loglik with D > 0; never the 4-bit loop image) ----
// one batch of cells [n_lo, n_lo + n_cnt): E compact [G][C], the cells' log Z and base sums (k_pair_cell), the weights, the batch's rows of the output [n_cnt][MW]
struct ca_pll_ops { const double *Ec, *lzc, *base, *wts; double* out; int64_t n_lo, n_cnt; int W, MW; };
template <typename YT>
int pair_ll_t(ca_engine* h, const ca_pll_ops& o) {
  LAUNCH(h, CA_KERNEL_YPASS, hipLaunchKernelGGL((k_pair_ll<YT>), dim3((unsigned)cdiv(o.n_cnt, CA_TB / 64), (unsigned)cdiv(o.MW, 64)), dim3(CA_TB), 0, h->stream, (const YT*)h->Y, o.Ec,
                                                o.lzc, o.base, h->s64, o.wts, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, h->ovf_col, h->ovf_val, o.out, o.n_lo, o.n_cnt, h->G,
                                                h->Gp, h->nseg, h->C, o.W, o.MW));
  return CA_OK;
}
int launch_pair_ll(ca_engine* h, const ca_pll_ops& o) {
  if (h->ystore == CA_YSTORE_U8) return pair_ll_t<uint8_t>(h, o);
  if (h->ystore == CA_YSTORE_U16) return pair_ll_t<uint16_t>(h, o);
  return pair_ll_t<float>(h, o);
}
// ---- k_mix_list<YT> / k_mix_rounds: the compacted list of a batch's rows and the projected-Newton rounds over it (ca_clone_mixture, every D; never the 4-bit loop image) ----
// one batch of cells [n_lo, n_lo + n_cnt): E compact [G][C], the cells' log Z and base sums (k_pair_cell), the list slabs [n_cnt][Gp] (gene, y, r, r^2 / y) and
// counts, the batch's rows of the start (null: uniform), the batch's rows of the outputs
struct ca_mix_ops { const double *Ec, *lzc, *base, *start; int* lg; double *ly, *lr, *lq; int* ln; double *w, *g, *mll, *bnd; int* rnd; int64_t n_lo, n_cnt; int max_iter; double tol; };
template <typename YT>
int mix_list_t(ca_engine* h, const ca_mix_ops& o) {
  LAUNCH(h, CA_KERNEL_YPASS, hipLaunchKernelGGL((k_mix_list<YT>), dim3((unsigned)cdiv(o.n_cnt, CA_TB / 64)), dim3(CA_TB), 0, h->stream, (const YT*)h->Y,
                                                h->n_ovf > 0 ? h->ovf_rowptr : nullptr, h->ovf_col, h->ovf_val, o.lg, o.ly, o.ln, o.n_lo, o.n_cnt, h->G, h->Gp, h->nseg));
  return CA_OK;
}
int launch_mix(ca_engine* h, const ca_mix_ops& o) {
  if (h->ystore == CA_YSTORE_U8) CACK(mix_list_t<uint8_t>(h, o));
  else if (h->ystore == CA_YSTORE_U16) CACK(mix_list_t<uint16_t>(h, o));
  else CACK(mix_list_t<float>(h, o));
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_mix_rounds, dim3((unsigned)cdiv(o.n_cnt, CA_TB / 64)), dim3(CA_TB), 0, h->stream, o.Ec, o.lzc, o.base, h->s64, o.lg, o.ly, o.lr,
                                                o.lq, o.ln, o.start, o.w, o.g, o.mll, o.bnd, o.rnd, o.n_lo, o.n_cnt, h->Gp, h->C, o.max_iter, o.tol));
  return CA_OK;
}
// ---- k_dm_ll<YT>: the Dirichlet-multinomial sweep over the resident matrix in its storage (ca_clone_loglik_dm, every D; never the 4-bit loop image) ----
// one batch of cells [n_lo, n_lo + n_cnt): E compact [G][C], the cells' log Z, max of eta and heads (k_dm_cell), the concentrations, the padded factors (null: D = 0),
// the batch's rows of the output [n_cnt][CK]; ysmall: the largest integer count on the product route (0: none)
struct ca_dml_ops { const double *Ec, *lzc, *mrow, *head, *conc, *Ut, *Vt; double* out; int64_t n_lo, n_cnt; int K, CK, ysmall; };
template <typename YT>
int dm_ll_t(ca_engine* h, const ca_dml_ops& o) {
  LAUNCH(h, CA_KERNEL_YPASS, hipLaunchKernelGGL((k_dm_ll<YT>), dim3((unsigned)cdiv(o.n_cnt, CA_TB / 64), (unsigned)cdiv(o.CK, 64)), dim3(CA_TB), 0, h->stream, (const YT*)h->Y, o.Ec,
                                                o.lzc, o.mrow, o.head, o.conc, o.Ut, o.Vt, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, h->ovf_col, h->ovf_val, o.out, o.n_lo, o.n_cnt,
                                                h->G, h->Gp, h->nseg, h->C, o.K, o.CK, o.ysmall));
  return CA_OK;
}
int launch_dm_ll(ca_engine* h, const ca_dml_ops& o) {
  if (h->ystore == CA_YSTORE_U8) return dm_ll_t<uint8_t>(h, o);
  if (h->ystore == CA_YSTORE_U16) return dm_ll_t<uint16_t>(h, o);
  return dm_ll_t<float>(h, o);
}
// ---- k_boot_build / k_boot_prod<YT, EXPSRC, NT> / k_boot_zero<YT> / k_boot_finish / k_boot_reduce: one chunk of replicates of ca_clone_loglik_reweighted on one batch of cells (never the 4-bit loop image) ----
// the call's weights [R][G], E compact and the padded factors; the chunk's right-hand sides (B1: nc1 columns, B2: nc2, Z0 at D = 0) for the replicates
// [r0, r0 + rc); the batch's slabs and outputs; the list of genes with a zero of E and its masks (nz entries of nw words; flags holds rcp replicates a cell)
struct ca_boot_ops { const double *W, *Ec, *Ut, *Vt; double *B1, *B2, *Z0, *part, *zpart, *mpart, *llb, *sb; const int* zg; const unsigned* zm; unsigned* flags;
                     int64_t n_lo, n_cnt; int r0, rc, rcp, nw, nz, D, nzc, nc1, nc2; };
int launch_boot_build(ca_engine* h, const ca_boot_ops& o) {
  const int nb_tab = cdiv((int64_t)h->Gp * (o.nc1 + (o.D > 0 ? o.nc2 : 0)), CA_TB), nb_z0 = o.D > 0 ? 0 : cdiv((int64_t)o.rc * h->C, CA_TB);
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_boot_build, dim3((unsigned)(nb_tab + nb_z0)), dim3(CA_TB), 0, h->stream, o.Ec, o.W, o.B1, o.D > 0 ? o.B2 : nullptr, o.Z0, o.r0, o.rc,
                                                h->G, h->Gp, h->C, o.nc1, o.nc2, nb_tab));
  return CA_OK;
}
// the product: exps = false, the resident rows against B1 into part; exps = true (D > 0), exp(eta - m) against B2 into zpart / mpart
template <typename YT, bool EXPSRC, int NT>
int boot_prod_t(ca_engine* h, const ca_boot_ops& o, int ngroups) {
  const int ncol = EXPSRC ? o.nc2 : o.nc1;
  LAUNCH(h, EXPSRC ? CA_KERNEL_OTHER : CA_KERNEL_YPASS,
         hipLaunchKernelGGL((k_boot_prod<YT, EXPSRC, NT>), dim3((unsigned)cdiv(o.n_cnt, 16 * (CA_TB / 64)), (unsigned)o.nzc, (unsigned)ngroups), dim3(CA_TB), 0, h->stream,
                            (const YT*)h->Y, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, h->ovf_col, h->ovf_val, o.Ut, o.Vt, EXPSRC ? o.B2 : o.B1, EXPSRC ? o.zpart : o.part,
                            EXPSRC ? o.mpart : nullptr, o.n_lo, o.n_cnt, h->G, h->Gp, ncol));
  return CA_OK;
}
// groups of CA_BOOT_NT column tiles (group z takes the tiles from z NT on); a product of at most four tiles -- a short last chunk of replicates -- takes the
// four-tile instantiation
template <typename YT, bool EXPSRC>
int boot_prod_nt(ca_engine* h, const ca_boot_ops& o) {
  const int tiles = (EXPSRC ? o.nc2 : o.nc1) / 16;
  if (tiles <= 4) return boot_prod_t<YT, EXPSRC, 4>(h, o, 1);
  return boot_prod_t<YT, EXPSRC, CA_BOOT_NT>(h, o, cdiv(tiles, CA_BOOT_NT));
}
int launch_boot_prod(ca_engine* h, const ca_boot_ops& o, bool exps) {
  if (exps) return boot_prod_nt<float, true>(h, o);   // (never reads Y)
  if (h->ystore == CA_YSTORE_U8) return boot_prod_nt<uint8_t, false>(h, o);
  if (h->ystore == CA_YSTORE_U16) return boot_prod_nt<uint16_t, false>(h, o);
  return boot_prod_nt<float, false>(h, o);
}
template <typename YT>
int boot_zero_t(ca_engine* h, const ca_boot_ops& o) {
  LAUNCH(h, CA_KERNEL_YPASS, hipLaunchKernelGGL((k_boot_zero<YT>), dim3((unsigned)cdiv(o.n_cnt * o.rc * o.nw, CA_TB)), dim3(CA_TB), 0, h->stream, (const YT*)h->Y, o.W, o.zg, o.zm, o.flags,
                                                o.n_lo, o.n_cnt, o.r0, o.rc, o.rcp, o.nw, o.nz, h->G, h->Gp));
  return CA_OK;
}
int launch_boot_zero(ca_engine* h, const ca_boot_ops& o) {
  if (h->ystore == CA_YSTORE_U8) return boot_zero_t<uint8_t>(h, o);
  if (h->ystore == CA_YSTORE_U16) return boot_zero_t<uint16_t>(h, o);
  return boot_zero_t<float>(h, o);
}
// ll_r and s_r of the chunk, then the chunk's replicates added into the call's votes and shares (the pointers at the batch's first row)
int launch_boot_finish(ca_engine* h, const ca_boot_ops& o, const double* lp, int* votes, double* psum, double* psq) {
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_boot_finish, dim3((unsigned)cdiv(o.n_cnt * o.rc, CA_TB)), dim3(CA_TB), 0, h->stream, o.part, o.zpart, o.mpart, o.Z0,
                                                o.nz > 0 ? o.flags : nullptr, o.llb, o.sb, o.n_cnt, o.rc, o.rcp, o.nw, h->C, o.D, o.nzc, o.nc1, o.nc2));
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_boot_reduce, dim3((unsigned)cdiv(o.n_cnt, CA_TB)), dim3(CA_TB), 0, h->stream, o.llb, lp, votes, psum, psq, o.n_lo, o.n_cnt, o.rc, h->C));
  return CA_OK;
}

// ---- k_proj_mom<NC, K> / k_proj_step<K>: one round of ca_project_cells on one batch of cells (neither reads the count matrix) ----
// the moments' operands: U = [psi | x] and V = [W | beta] padded to CA_LL_DMAX factors, E in groups of NC clone columns, the frozen flags, the chunk slabs
struct ca_pm_ops { const double *Ut, *Vt, *Ez; const unsigned char* frozen; double *zpart, *mpart; int64_t n_lo, n_cnt; int K, NC, ngrp, nzc; };
template <int NC, int K>
int proj_mom_t(ca_engine* h, const ca_pm_ops& o) {
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_proj_mom<NC, K>), dim3((unsigned)cdiv(o.n_cnt, CA_TB), (unsigned)o.nzc, (unsigned)o.ngrp), dim3(CA_TB), 0, h->stream, o.Ut, o.Vt,
                                                o.Ez, o.frozen, o.zpart, o.mpart, o.n_lo, o.n_cnt, h->G, h->Gp));
  return CA_OK;
}
int launch_proj_mom(ca_engine* h, const ca_pm_ops& o) {   // (sixteen clones per group only where the accumulators of eight leave room: K <= 1)
  if (o.K == 0) return o.NC == 8 ? proj_mom_t<8, 0>(h, o) : proj_mom_t<16, 0>(h, o);
  if (o.K == 1) return o.NC == 8 ? proj_mom_t<8, 1>(h, o) : proj_mom_t<16, 1>(h, o);
  return proj_mom_t<8, 2>(h, o);
}
// the round's finisher (final = 0) or the closing evaluation (final = 1)
struct ca_ps_ops { const double *zpart, *mpart, *A, *B, *lp; double* Ut; unsigned char *frozen, *conv; int* rounds; double *ll, *probs, *obj; int64_t n_lo, n_cnt; int K, nzc, nmt, round, final; double tol, max_step; };
template <int K>
int proj_step_t(ca_engine* h, const ca_ps_ops& o) {
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_proj_step<K>), dim3((unsigned)cdiv(o.n_cnt, CA_TB)), dim3(CA_TB), 0, h->stream, o.zpart, o.mpart, o.A, o.B, o.lp, h->s64, o.Ut, o.frozen,
                                                o.rounds, o.conv, o.ll, o.probs, o.obj, o.n_lo, o.n_cnt, h->C, o.nzc, o.nmt, o.round, o.final, o.tol, o.max_step));
  return CA_OK;
}
int launch_proj_step(ca_engine* h, const ca_ps_ops& o) {
  if (o.K == 0) return proj_step_t<0>(h, o);
  if (o.K == 1) return proj_step_t<1>(h, o);
  return proj_step_t<2>(h, o);
}

// ---- k_ev_mom<NS, K, FULL> and the finishers of ca_clone_evidence on one batch of cells (none reads the count matrix) ----
// Slots per group from the register budget (DESIGN section 7): Newton rounds (all moments) eight clones at K = 1 and four at K = 2, the quadrature pass (Z0 only)
// sixteen (clone, node) slots at K = 1 and eight at K = 2.
// the batch's operands: x in U's last columns, V = [W | beta] padded, E compact [Gp][C], the slots' psi, the pairs' states, the chunk slabs
struct ca_evm_ops { const double *Ut, *Vt, *Ec, *ps; const unsigned char* fz; double *zpart, *mpart; int64_t n_lo, n_cnt; int K, Q, nslot, nzc; bool full; };
template <int NS, int K, bool FULL>
int ev_mom_t(ca_engine* h, const ca_evm_ops& o) {
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_ev_mom<NS, K, FULL>), dim3((unsigned)cdiv(o.n_cnt, CA_TB), (unsigned)o.nzc, (unsigned)cdiv(o.nslot, NS)), dim3(CA_TB), 0, h->stream,
                                                o.Ut, o.Vt, o.Ec, o.ps, o.fz, o.zpart, o.mpart, o.n_lo, o.n_cnt, h->G, h->C, o.Q, o.nslot));
  return CA_OK;
}
int launch_ev_mom(ca_engine* h, const ca_evm_ops& o) {
  if (o.full) return o.K == 1 ? ev_mom_t<8, 1, true>(h, o) : ev_mom_t<4, 2, true>(h, o);
  return o.K == 1 ? ev_mom_t<16, 1, false>(h, o) : ev_mom_t<8, 2, false>(h, o);   // (sixteen slots at K = 2 spill: 32 psi registers beside the 32 of m and Z0)
}
// the per-pair state of a batch: psi of the clones, state, rounds, converged, f*, H, laplace, evidence; the quadrature's nodes, weights and node psi
struct ca_evs_ops { const double *zpart, *mpart, *A, *B, *Ut, *nodes, *wts; double *ps, *pq; unsigned char *fz, *conv; int* rounds; double *fstar, *Hm, *lap, *ev;
                    int64_t n_lo, n_cnt; int K, Q, nzc, round, final; double tol, max_step; };
template <int K>
int ev_fin_t(ca_engine* h, const ca_evs_ops& o, int what) {
  const dim3 grid((unsigned)cdiv(o.n_cnt * h->C, CA_TB));
  if (what == 0)
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_ev_init<K>), grid, dim3(CA_TB), 0, h->stream, o.A, o.Ut, o.ps, o.fz, o.rounds, o.conv, o.fstar, o.Hm, o.ev, o.lap, o.n_lo, o.n_cnt, h->C));
  else if (what == 1)
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_ev_step<K>), grid, dim3(CA_TB), 0, h->stream, o.zpart, o.mpart, o.A, o.B, o.Ut, h->s64, o.ps, o.fz, o.rounds, o.conv, o.fstar, o.Hm,
                                                  o.n_lo, o.n_cnt, h->C, o.nzc, o.round, o.final, o.tol, o.max_step));
  else if (what == 2)
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_ev_nodes<K>), grid, dim3(CA_TB), 0, h->stream, o.ps, o.fz, o.fstar, o.Hm, o.nodes, o.pq, o.lap, o.n_cnt, h->C, o.Q));
  else
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL((k_ev_reduce<K>), grid, dim3(CA_TB), 0, h->stream, o.zpart, o.mpart, o.A, o.B, o.Ut, h->s64, o.pq, o.fz, o.fstar, o.lap, o.nodes, o.wts,
                                                  o.ev, o.n_lo, o.n_cnt, h->C, o.Q, o.nzc));
  return CA_OK;
}
enum { CA_EV_INIT = 0, CA_EV_STEP = 1, CA_EV_NODES = 2, CA_EV_REDUCE = 3 };
int launch_ev_fin(ca_engine* h, const ca_evs_ops& o, int what) { return o.K == 1 ? ev_fin_t<1>(h, o, what) : ev_fin_t<2>(h, o, what); }

// ---- k_simulate: one launch over a list of work items of ca_simulate_counts (no engine: the call owns its stream) ----
// The search table's plan for G genes: S = genes per LDS entry (1: the whole table in LDS), whether the row's histogram fits in LDS beside it, the LDS bytes.
struct ca_sim_plan { int S, nco, hist_lds; size_t lds; };
inline ca_sim_plan sim_plan(int G) {
  ca_sim_plan p;
  p.hist_lds = (size_t)G * 4 + 8 * (size_t)cdiv(G, 64) <= CA_SIM_LDS ? 1 : 0;   // (it must fit beside a table of one entry per 64 genes)
  const size_t room = CA_SIM_LDS - (p.hist_lds ? (size_t)G * 4 : 0);
  p.S = 1;
  while (8 * (size_t)cdiv(G, p.S) > room) p.S *= 2;
  p.nco = cdiv(G, p.S);
  p.lds = 8 * (size_t)p.nco + (p.hist_lds ? (size_t)G * 4 : 0);
  return p;
}
struct ca_sim_ops { const double *Et, *Vt, *U; const int32_t* clone; const int64_t* total; const ca_sim_item* items; double* cumg; int32_t* Y; int64_t n_items; int G, D;
                    ca_sim_plan plan; uint64_t seed, draw, q0; };
inline hipError_t launch_simulate(hipStream_t stream, const ca_sim_ops& o) {
  hipLaunchKernelGGL(k_simulate, dim3((unsigned)o.n_items), dim3(CA_SIM_TB), o.plan.lds, stream, o.Et, o.Vt, o.U, o.clone, o.total, o.items, o.plan.S > 1 ? o.cumg : nullptr, o.Y,
                     o.G, o.D, o.plan.S, o.plan.nco, o.plan.hist_lds, (uint32_t)o.seed, (uint32_t)(o.seed >> 32), o.draw, o.q0);
  return hipGetLastError();
}

// ---- k_predictive: one launch over a batch of cells of ca_predictive_stats, `blocks` blocks walking them with the grid's stride (no engine: the call owns its stream) ----
struct ca_pred_ops { const double *Et, *Vt, *U; const int32_t* clone; const int64_t* total; const double* lgtab; double *cum_blk, *lw_blk; int32_t* row_blk; double* ll;
                     unsigned long long* T; int64_t n_cnt; int blocks, G, C, D, n_rep; ca_sim_plan plan; uint64_t seed, draw0, q0; };
inline hipError_t launch_predictive(hipStream_t stream, const ca_pred_ops& o) {
  hipLaunchKernelGGL(k_predictive, dim3((unsigned)o.blocks), dim3(CA_SIM_TB), o.plan.lds, stream, o.Et, o.Vt, o.U, o.clone, o.total, o.lgtab, o.plan.S > 1 ? o.cum_blk : nullptr,
                     o.lw_blk, o.row_blk, o.ll, o.T, o.n_cnt, o.G, o.C, o.D, o.plan.S, o.plan.nco, o.plan.hist_lds, (uint32_t)o.seed, (uint32_t)(o.seed >> 32), o.draw0, o.n_rep, o.q0);
  return hipGetLastError();
}

// ---- k_predmom_loge / k_predmom_cell / k_predmom_gene<D> / k_predmom_finish: the launches of ca_predictive_moments on one batch of cells (no engine: the call owns its stream) ----
// the call's tables (E, log E and V transposed, the running sums acc [3][C][G]) and the batch's arrays: the cells' inputs, what the cell phase leaves for the
// gene phase (m, Z), the list of cells with counts by clone, its strips, the first strip of every clone, the strip sums
struct ca_predmom_ops { const double *Et, *Vt, *U; double* lEt; const int32_t* clone; const int64_t* total; double *w_blk, *m, *z, *mean, *var; const int32_t *list, *first;
                        const ca_pm_strip* strips; double *genepart, *acc; int64_t n_cnt; int blocks, nstrips, G, C, D; bool w_lds; };
inline hipError_t launch_predmom_loge(hipStream_t stream, const ca_predmom_ops& o) {
  const int64_t n = (int64_t)o.C * o.G;
  hipLaunchKernelGGL(k_predmom_loge, dim3((unsigned)cdiv(n, CA_PM_TB)), dim3(CA_PM_TB), 0, stream, o.Et, o.lEt, n);
  return hipGetLastError();
}
inline hipError_t launch_predmom_cell(hipStream_t stream, const ca_predmom_ops& o) {
  hipLaunchKernelGGL(k_predmom_cell, dim3((unsigned)o.blocks), dim3(CA_PM_TB), o.w_lds ? (size_t)o.G * sizeof(double) : 0, stream, o.Et, o.lEt, o.Vt, o.U, o.clone, o.total,
                     o.w_lds ? nullptr : o.w_blk, o.m, o.z, o.mean, o.var, o.n_cnt, o.G, o.D);
  return hipGetLastError();
}
template <int D>
hipError_t predmom_gene_t(hipStream_t stream, const ca_predmom_ops& o) {
  const int gtiles = cdiv(o.G, CA_PM_TB);
  hipLaunchKernelGGL((k_predmom_gene<D>), dim3((unsigned)((int64_t)gtiles * o.nstrips)), dim3(CA_PM_TB), 0, stream, o.Et, o.Vt, o.U, o.total, o.m, o.z, o.list, o.strips, o.genepart,
                     o.G, gtiles);
  return hipGetLastError();
}
inline hipError_t launch_predmom_gene(hipStream_t stream, const ca_predmom_ops& o) {   // (V's row of a gene lives in registers: one instantiation per D = 1 .. CA_LL_DMAX)
  switch (o.D) {
    case 1: return predmom_gene_t<1>(stream, o);
    case 2: return predmom_gene_t<2>(stream, o);
    case 3: return predmom_gene_t<3>(stream, o);
    case 4: return predmom_gene_t<4>(stream, o);
    case 5: return predmom_gene_t<5>(stream, o);
    case 6: return predmom_gene_t<6>(stream, o);
    case 7: return predmom_gene_t<7>(stream, o);
    default: return predmom_gene_t<8>(stream, o);
  }
}
inline hipError_t launch_predmom_finish(hipStream_t stream, const ca_predmom_ops& o) {
  hipLaunchKernelGGL(k_predmom_finish, dim3((unsigned)cdiv((int64_t)o.C * o.G, CA_PM_TB)), dim3(CA_PM_TB), 0, stream, o.genepart, o.first, o.acc, o.G, o.C);
  return hipGetLastError();
}

// ---- k_cnp_cell / k_cnp_gene<JB> / k_cnp_block / k_cnp_finish: the launches of ca_copy_number_profile on one batch of cells (no engine: the call owns its stream) ----
// the call's tables (E and V transposed, mu, kappa, in per-gene mode their products mk [J][G], the running sums acc [C][J][W], W = G or B; in block mode the run list, `full` [C][B] and `same` [C][J][B]) and
// the batch's arrays: the cells' inputs, m and Z, the shares [cells][2][B], the list of cells with counts by clone, its strips, the first strip of every clone, the strip sums
struct ca_cnp_ops { const double *Et, *Vt, *U, *mu, *kappa, *mk; const int32_t* clone; const int64_t* total; double *w_blk, *m, *z, *share; const int32_t *list, *first, *run_gene, *run_first;
                    const unsigned char *full, *same; const ca_pm_strip* strips; double *part, *acc; int64_t n_cnt; int blocks, nstrips, G, C, D, J, B; bool w_lds, by_block; };
inline hipError_t launch_cnp_cell(hipStream_t stream, const ca_cnp_ops& o) {
  hipLaunchKernelGGL(k_cnp_cell, dim3((unsigned)o.blocks), dim3(CA_PM_TB), o.w_lds ? (size_t)o.G * sizeof(double) : 0, stream, o.Et, o.Vt, o.U, o.clone, o.total,
                     o.w_lds ? nullptr : o.w_blk, o.m, o.z, o.mu, o.by_block ? o.run_gene : nullptr, o.run_first, o.full, o.share, o.n_cnt, o.G, o.D, o.B);
  return hipGetLastError();
}
template <int JB>
hipError_t cnp_gene_t(hipStream_t stream, const ca_cnp_ops& o) {
  const int gtiles = cdiv(o.G, CA_PM_TB);
  hipLaunchKernelGGL((k_cnp_gene<JB>), dim3((unsigned)((int64_t)gtiles * o.nstrips)), dim3(CA_PM_TB), 0, stream, o.Et, o.Vt, o.U, o.total, o.m, o.z, o.list, o.strips, o.mk, o.part,
                     o.G, o.D, o.J, gtiles);
  return hipGetLastError();
}
inline hipError_t launch_cnp_sum(hipStream_t stream, const ca_cnp_ops& o) {   // (the accumulators live in registers: one instantiation per bucket of J)
  if (o.by_block) {
    const int tiles = cdiv(o.J * o.B, CA_PM_TB);
    hipLaunchKernelGGL(k_cnp_block, dim3((unsigned)((int64_t)tiles * o.nstrips)), dim3(CA_PM_TB), 0, stream, o.share, o.total, o.list, o.strips, o.kappa, o.same, o.part, o.B, o.J, tiles);
    return hipGetLastError();
  }
  return o.J <= 4 ? cnp_gene_t<4>(stream, o) : o.J <= 8 ? cnp_gene_t<8>(stream, o) : cnp_gene_t<16>(stream, o);
}
inline hipError_t launch_cnp_finish(hipStream_t stream, const ca_cnp_ops& o) {
  const int64_t JW = (int64_t)o.J * (o.by_block ? o.B : o.G);
  hipLaunchKernelGGL(k_cnp_finish, dim3((unsigned)cdiv(JW * o.C, CA_PM_TB)), dim3(CA_PM_TB), 0, stream, o.part, o.first, o.acc, JW, o.C);
  return hipGetLastError();
}

// ---- k_sep_loge / k_sep_build / k_boot_prod<float, true, NT> / k_sep_scale / k_sep_merge / k_sep_finish: the launches of ca_clone_separability on one batch of cells (no engine: the call owns its stream) ----
// the call's tables (e and log e [Gp][C], the padded factors Vt [Gp][CA_LL_DMAX]); the right-hand side B [Gp][W] of the columns [c_lo, c_lo + W); the batch's padded
// factors Ut, its slabs (part, mpart, the chunks' scales wk, the shift m), the merged rows R [n_cnt][ncolp] and the five outputs
struct ca_sep_ops { const double *Ec, *Vt, *Ut; double *lE, *B, *part, *mpart, *wk, *m, *R, *logZ, *excl, *m1, *m2, *m3; int64_t n_cnt; int G, Gp, C, nzc, ncol, ncolp, c_lo, W; };
inline hipError_t launch_sep_loge(hipStream_t stream, const ca_sep_ops& o) {
  const int64_t n = (int64_t)o.Gp * o.C;
  hipLaunchKernelGGL(k_sep_loge, dim3((unsigned)cdiv(n, CA_TB)), dim3(CA_TB), 0, stream, o.Ec, o.lE, n);
  return hipGetLastError();
}
inline hipError_t launch_sep_build(hipStream_t stream, const ca_sep_ops& o) {
  hipLaunchKernelGGL(k_sep_build, dim3((unsigned)cdiv((int64_t)o.Gp * o.W, CA_TB)), dim3(CA_TB), 0, stream, o.Ec, o.lE, o.B, o.c_lo, o.W, o.ncol, o.G, o.Gp, o.C);
  return hipGetLastError();
}
// the bootstrap's exponent product on the call's own stream: groups of CA_BOOT_NT column tiles, the four-tile instantiation for at most four (boot_prod_nt's rule)
template <int NT>
hipError_t sep_prod_t(hipStream_t stream, const ca_sep_ops& o, int ngroups) {
  hipLaunchKernelGGL((k_boot_prod<float, true, NT>), dim3((unsigned)cdiv(o.n_cnt, 16 * (CA_TB / 64)), (unsigned)o.nzc, (unsigned)ngroups), dim3(CA_TB), 0, stream, (const float*)nullptr,
                     (const int64_t*)nullptr, (const int*)nullptr, (const float*)nullptr, o.Ut, o.Vt, (const double*)o.B, o.part, o.mpart, (int64_t)0, o.n_cnt, o.G, o.Gp, o.W);
  return hipGetLastError();
}
inline hipError_t launch_sep_prod(hipStream_t stream, const ca_sep_ops& o) {
  const int tiles = o.W / 16;
  return tiles <= 4 ? sep_prod_t<4>(stream, o, 1) : sep_prod_t<CA_BOOT_NT>(stream, o, cdiv(tiles, CA_BOOT_NT));
}
inline hipError_t launch_sep_scale(hipStream_t stream, const ca_sep_ops& o) {
  hipLaunchKernelGGL(k_sep_scale, dim3((unsigned)cdiv(o.n_cnt, CA_TB)), dim3(CA_TB), 0, stream, (const double*)o.mpart, o.wk, o.m, o.n_cnt, o.nzc);
  return hipGetLastError();
}
inline hipError_t launch_sep_merge(hipStream_t stream, const ca_sep_ops& o) {
  hipLaunchKernelGGL(k_sep_merge, dim3((unsigned)cdiv(o.n_cnt * o.W, CA_TB)), dim3(CA_TB), 0, stream, (const double*)o.part, (const double*)o.wk, o.R, o.n_cnt, o.nzc, o.c_lo, o.W, o.ncolp);
  return hipGetLastError();
}
inline hipError_t launch_sep_finish(hipStream_t stream, const ca_sep_ops& o) {
  hipLaunchKernelGGL(k_sep_finish, dim3((unsigned)cdiv(o.n_cnt * o.C * o.C, CA_TB)), dim3(CA_TB), 0, stream, (const double*)o.R, (const double*)o.m, o.logZ, o.excl, o.m1, o.m2, o.m3, o.n_cnt,
                     o.C, o.ncolp);
  return hipGetLastError();
}
