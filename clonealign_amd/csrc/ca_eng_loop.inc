// ca_eng_loop.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): the loop: count-matrix products per parameter state, backward / update halves, plain and fused passes (sweeps or series form), the host's waits, eps staging.
// The side stream's products: the row products (YW, psi.(YW) partials) are done at ev_ywdone, everything (also Y^T psi)
// at ev_ydone.  all = false waits for the row products only (the backward sweep's ELBO tail needs nothing else).
int wait_y(ca_engine* h, bool all) {
  if (all) {
    if (h->y_pending) HIPCK(h, hipStreamWaitEvent(h->stream, h->ev_ydone, 0));
    h->y_pending = false; h->yw_pending = false;
  } else if (h->yw_pending) {
    HIPCK(h, hipStreamWaitEvent(h->stream, h->ev_ywdone, 0));
    h->yw_pending = false;
  }
  return CA_OK;
}

// After a merged update (k_update_merged) the per-cell exponent bound of the stepped state has not been made: the fused forward sweep's
// blocks make it themselves (ca_cell_ptrs::vmm_part); every OTHER consumer of etamax2 calls this first (the two small kernels of setup).
int make_etamax(ca_engine* h) {   // (from the block ranges of V' in vmm_part)
  if (h->D > 0) {
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_vmm_final, dim3(1), dim3(64), 0, h->stream, h->vmm_part, h->vmm, h->ngblk, h->D));
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_etamax, dim3(cdiv(h->N, CA_TB)), dim3(CA_TB), 0, h->stream, h->F, h->vmm, h->etamax2, h->N, h->D));
  }
  h->em_stale = false;
  return CA_OK;
}
int ensure_etamax(ca_engine* h) {
  if (!h->em_stale) return CA_OK;
  return make_etamax(h);
}

// ---- derived state that depends on the parameters only (not on eps) -------------------------
int refresh_derived(ca_engine* h) {
  CACK(wait_y(h, true));
  h->y_defer = false;   // a deferred side-stream Y pass would not be ordered after this parameter change: redo it in line
  h->pre_valid = false;
  h->ys_steps = -1;     // arbitrary parameter change: the fixed-point exponents are taken from exact maxima again
  h->ys_quant_ready = false;
  if (h->D > 0) LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_vprep, dim3(h->ngblk), dim3(CA_TB), 0, h->stream, h->V, h->Vs, h->vmm_part, h->G, h->D));
  CACK(make_etamax(h));
  h->gaux_slot = -1;
  h->ycache_valid = false;
  h->yfin_pending = false; h->ycol_pending = false;
  h->look_valid = false;
  h->poly_fresh = false;
  h->poly_seq_base = h->poly_seq + 1;   // (an arbitrary parameter change: ranges seen before it say nothing)
  h->poly_xmax_ready = false;
  h->poly_xglob_steps = -1;
  return CA_OK;
}

// The overflow list's share of a stream launch (counts above 255): its per-entry work rides as extra blocks -- the cell side into one extra strip of YWpart
// (YWextra, behind the stream's own strips), the gene side into the chunk sums the finisher adds per gene.  All zero without a list.
ca_ovf_args ovf_args(ca_engine* h, float* YWextra) {
  ca_ovf_args ovf;
  memset(&ovf, 0, sizeof(ovf));
  if (h->n_ovf > 0) {
    ovf.nb_rows = cdiv(h->N, CA_TB); ovf.nb_chunks = cdiv(h->n_ovf_chunk, CA_TB / 64);
    ovf.rowptr = h->ovf_rowptr; ovf.col = h->ovf_col; ovf.val = h->ovf_val; ovf.YWextra = YWextra;
    ovf.chunk_start = h->ovf_chunk_start; ovf.row2 = h->ovf_row2; ovf.val2 = h->ovf_val2; ovf.csum = h->ovf_csum; ovf.nchunk = h->n_ovf_chunk;
  }
  return ovf;
}
// The finishing sums over a stream's float partial slabs: column sums of YTpart's `rows` row groups (+ the overflow list's chunk sums per gene) into red_y, laid out
// [Gp][K] (first G rows used); YW = sum of YWpart's `nseg` strips (+ the overflow list's) and the psi.(YW) partials of the ELBO.  As a struct they ride as extra blocks
// of the backward sweep (k_bwd_mfma) or of the series form's cell launch; launch_yfinish is the same sums as a launch of their own (k_yfinish = k_colsum's blocks +
// k_yw_dot's).
ca_yfin_args yfin_args(ca_engine* h, int rows, int nseg) {
  ca_yfin_args a;
  memset(&a, 0, sizeof(a));
  a.ncol = cdiv((int64_t)h->Gp * h->K, 64); a.nrow = h->n_yw;
  a.part = h->YTpart; a.out = h->red + h->off_y; a.rows = rows; a.ld = (int64_t)h->Gp * h->K; a.cols = h->Gp * h->K; a.G = h->G;
  if (h->n_ovf > 0) { a.col_chunk_ptr = h->ovf_col_chunk_ptr; a.csum = h->ovf_csum; }
  a.YWpart = h->YWpart; a.nseg = nseg + (h->n_ovf > 0 ? 1 : 0); a.F = h->F; a.D = h->D; a.N = h->N; a.YW = h->YW; a.yw_part = h->yw_part;
  return a;
}
// (cols_only: the column sums alone -- the row jobs of this stream launch are done, CA_VAR_GENE_RIDE)
int launch_yfinish(ca_engine* h, int rows, int nseg, bool cols_only = false) {
  ca_yfin_args a = yfin_args(h, rows, nseg);
  if (cols_only) a.nrow = 0;
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_yfinish, dim3(a.ncol + a.nrow), dim3(1024), 0, h->stream, a.part, a.out, a.rows, a.ld, a.cols, a.col_chunk_ptr,
                                                a.csum, h->K, a.G, a.ncol, a.YWpart, a.nseg, a.F, a.D, a.N, a.YW, a.yw_part));
  return CA_OK;
}

// The same two products on the int8 matrix cores (ca_ymfma.hip.h), both from ONE tiled copy through the transposing LDS read (k_ys_mfma; K = 1): a quantiser launch (fixed-point images of W and
// psi; exact maxima by a separate pass only for the first state after a reset, afterwards bounded from the previous state's),
// the stream, the finisher.  Three launches, like the VALU stream's.
// Arguments of the quantiser for the current parameters (slot ys_slot).  lagged = true: the exponents are bounded from the previous
// state's maxima (`steps` Adam steps ago) -- possible up to 4 steps back; else the caller runs k_ym_absmax first (exact maxima).
ca_ysq_args ys_quant_args(ca_engine* h, int steps, bool* lagged) {
  ca_ysq_args a;
  memset(&a, 0, sizeof(a));
  const int s0 = h->ys_slot, s1 = (s0 + 1) % 3;
  a.nblk = h->ys_nq;
  a.V = h->V; a.Dv = h->D; a.G = h->G; a.GS = h->Gp / 64; a.F = h->F; a.Df = h->D; a.N = h->N; a.NS = h->ys_N64 / 64;
  *lagged = steps >= 0 && steps <= 4 && h->ys_step_bound > 0.f;
  if (*lagged) {
    a.amax_in = h->ys_amaxp + (int64_t)s0 * h->ys_ncap * 2; a.n_in = h->ys_namax[s0];
    a.slack_w = a.slack_p = (float)steps * h->ys_step_bound;
  } else {
    a.amax_in = reinterpret_cast<const float*>(h->ys_amax); a.n_in = 1;
  }
  a.amax_out = h->ys_amaxp + (int64_t)s1 * h->ys_ncap * 2;
  h->ys_namax[s1] = h->ys_nq;   // (what a run of the quantiser's own blocks leaves; the merged update overrides it)
  a.exps = h->ys_exps + 2 * s0; a.Wr = h->Wr; a.Pr = h->Pr; a.Wsum = h->Wsum; a.Psum = h->Psum;
  return a;
}
// quantiser of the one-copy stream as launches of its own (first pass after a reset, call-by-call API); inside the loop it rides
// on k_adam_cell (train_update) and this is a no-op
int ys_quant(ca_engine* h) {
  if (h->ys_quant_ready) return CA_OK;
  bool lagged = false;
  ca_ysq_args a = ys_quant_args(h, h->ys_steps, &lagged);
  if (!lagged) {
    HIPCK(h, hipMemsetAsync(h->ys_amax, 0, 2 * sizeof(unsigned), h->stream));
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_ym_absmax, dim3(cdiv(std::max<int64_t>(h->N, h->G), CA_YM_TB)), dim3(CA_YM_TB), 0, h->stream,
                                                  h->V, h->D, (int64_t)h->G, h->F, h->D, h->N, 1, h->ys_amax));
  }
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_ys_quant, dim3(a.nblk), dim3(CA_YM_TB), 0, h->stream, a));
  return CA_OK;
}
// (with the 4-bit image the body reads neither Wsum nor Psum -- no bias to undo; the quantiser still writes them, a few KB per pass)
ca_ys_io ys_io(ca_engine* h) {
  ca_ys_io io;
  io.Wr = h->Wr; io.Pr = h->Pr; io.Wsum = h->Wsum; io.Psum = h->Psum; io.exps = h->ys_exps + 2 * h->ys_slot;
  io.YWpart = h->YWpart; io.YTpart = h->YTpart;
  io.esc_off = h->ys4 ? h->esc_off : nullptr; io.esc = h->ys4 ? h->esc : nullptr;
  io.perm = nullptr;
  return io;
}
ca_ovf_args ys_ovf(ca_engine* h) { return ovf_args(h, h->YWpart + (int64_t)h->ys_nseg * h->N); }
// finisher of the one-copy stream: the vector stream's own (k_yfinish) over the float partial slabs the stream left
// (ycol_pending: the series form's cell launch has run the row jobs, the column jobs were to ride on its merged way back, which has not been queued -- the consumer
//  that comes first gets them as a launch: k_yfinish's column blocks, bitwise the riding waves' sums)
int yfin_flush(ca_engine* h) {
  if (h->ycol_pending && !h->yfin_pending) {
    h->ycol_pending = false;
    return launch_yfinish(h, h->ys_nrg, h->ys_nseg, true);
  }
  h->ycol_pending = false;
  if (!h->yfin_pending) return CA_OK;
  h->yfin_pending = false;
  return launch_yfinish(h, h->ys_nrg, h->ys_nseg);
}
// the stream's slabs are complete (launch issued): finisher now, or left pending for the backward sweep that follows in the loop;
// advances the quantiser's slot ring
int ys_finish(ca_engine* h, bool defer = false) {
  h->yfin_pending = true; h->ycol_pending = false;
  if (!defer) CACK(yfin_flush(h));
  h->ys_slot = (h->ys_slot + 1) % 3;   // (the only place the ring advances: ca_ystream_parts finds the launch's exponents one slot back)
  h->ys_launched = true;
  h->ys_steps = 0;
  h->ys_quant_ready = false;
  h->ycache_valid = true;
  return CA_OK;
}
// (h->mom_args set: the series form's forward moments ride as blocks of this launch, ca_polymom.hip.h -- taken here, so that the caller can tell.  The grid is
//  [role][stream][overflow] with pm->blk0 = 0 and [stream][role][overflow] with pm->blk0 = nb_main: the same block count, the kernels map the index)
// (N2 > 0: the 2-bit / 4-bit image, its escape list and its gene order in place of the 4-bit image's -- CA_VAR_Y2; everything else of the launch as it is)
template <bool Y4, int N2 = 0>
void launch_ys(ca_engine* h) {
  constexpr int lds = Y4 ? CA_YS4_LDS_BYTES : CA_YS_LDS_BYTES;
  ca_ys_io yio = ys_io(h);
  const uint8_t* Yimg = h->Ys;
  if (N2 > 0) { Yimg = h->Ys2; yio.esc_off = h->esc2_off; yio.esc = h->esc2; yio.perm = h->y2_perm; }
  const int nb_main = h->ys_nrg * h->ys_nseg;
  const ca_pm_args* pm = h->mom_args;
  h->mom_args = nullptr;
  const int nmom = pm ? pm->nmb + pm->nred : 0;
  if (h->n_ovf > 0) {   // (the overflow list's blocks behind the stream's)
    const ca_ovf_args ovf = ys_ovf(h);
    const dim3 grid(nmom + nb_main + ovf.nb_rows + ovf.nb_chunks);
    if (pm) {
      ca_pm_args pmo = *pm;
      if (h->mom_last && h->mom_ovf_first) pmo.blk0 += ovf.nb_rows + ovf.nb_chunks;   // (lab: the overflow list's blocks between the stream's and the role)
      hipLaunchKernelGGL((k_ys_mfma_ovf_mom<Y4, N2>), grid, dim3(CA_YM_TB), lds, h->stream, Yimg, yio, h->N, h->Gp, h->ys_RS, nb_main, ovf, h->F, h->V, h->D, pmo);
    }
    else hipLaunchKernelGGL((k_ys_mfma_ovf<Y4, N2>), grid, dim3(CA_YM_TB), lds, h->stream, Yimg, yio, h->N, h->Gp, h->ys_RS, nb_main, ovf, h->F, h->V, h->D);
  } else {
    if (pm) hipLaunchKernelGGL((k_ys_mfma_mom<Y4, N2>), dim3(nmom + nb_main), dim3(CA_YM_TB), lds, h->stream, Yimg, yio, h->N, h->Gp, h->ys_RS, *pm);
    else hipLaunchKernelGGL((k_ys_mfma<Y4, N2>), dim3(nb_main), dim3(CA_YM_TB), lds, h->stream, Yimg, yio, h->N, h->Gp, h->ys_RS);
  }
}
int ycache_ys(ca_engine* h) {
  CACK(ys_quant(h));
  if (h->ys4 && h->ys_n2 == 6) LAUNCH(h, CA_KERNEL_YPASS, (launch_ys<true, 6>(h)));
  else if (h->ys4 && h->ys_n2 == 5) LAUNCH(h, CA_KERNEL_YPASS, (launch_ys<true, 5>(h)));
  else if (h->ys4) LAUNCH(h, CA_KERNEL_YPASS, launch_ys<true>(h));
  else LAUNCH(h, CA_KERNEL_YPASS, launch_ys<false>(h));
  const bool defer = h->ys_defer_next;
  h->ys_defer_next = false;
  return ys_finish(h, defer);
}

// Y.W and Y^T.psi for the current parameters (once per parameter state, SURVEY.md §7.3)
int ensure_ycache(ca_engine* h) {
  if (h->y_defer) {   // deferred side-stream start (train_tail): ordered after the parameter update by ev_params
    h->y_defer = false;
    HIPCK(h, hipStreamWaitEvent(h->stream2, h->ev_params, 0));
    std::swap(h->stream, h->stream2);
    h->on_side = true;
    const int rc = ensure_ycache(h);
    h->on_side = false;
    std::swap(h->stream, h->stream2);
    CACK(rc);
    HIPCK(h, hipEventRecord(h->ev_ydone, h->stream2));
    h->y_pending = true;
    HIPCK(h, hipEventRecord(h->ev_ywdone, h->stream2));   // (no earlier point: the row products are finished by the stream's last launch)
    h->yw_pending = true;
    return CA_OK;
  }
  if (h->ycache_valid || h->K == 0) { h->ycache_valid = true; return yfin_flush(h); }
  h->yfin_pending = false; h->ycol_pending = false;
  if (h->y_ys) return ycache_ys(h);
  dim3 grid((unsigned)((int64_t)h->nrg * h->nseg));
  // entries above 255: one extra "segment" of YW and one extra term of Y^T psi; their per-entry work rides on the
  // first stream launch, the per-gene sums on the column-sum launch
  const ca_ovf_args ovf = ovf_args(h, h->YWpart + (int64_t)h->nseg * h->N * h->K);
  ca_ovf_args none;
  memset(&none, 0, sizeof(none));
  const ca_ypass_ops fit = {h->F, h->D, h->V, h->YWpart, h->YTpart, h->K};
  for (int koff = 0; koff < h->K; koff += 4) {
    const int kk = std::min(4, h->K - koff);
    CACK(prof_begin(h, CA_KERNEL_YPASS));
    const ca_ovf_args& o = koff == 0 ? ovf : none;
    ypass<0>(h, fit, koff, kk, grid, o);
    HIPCK(h, hipGetLastError());
    CACK(prof_end(h));
  }
  // YTpart is [nrb][Gp*K]: column sums over the row blocks (+ the overflow list's chunk sums per gene); ytpsi is laid
  // out [Gp][K] (first G rows used).  Row side: YW = sum of the strips, and the psi.(YW) partials of the ELBO (the fused
  // loop's cell epilogue leaves both to this).  One launch for both (launch_yfinish).
  if (!h->on_side) {
    CACK(launch_yfinish(h, h->nrg, h->nseg));
  } else {
    // on the side stream, beside the forward sweep, the two finishers stay two small launches: the merged one's 1024-thread
    // blocks need sixteen free wave slots at once and took 64 us to get through a GPU the sweep has filled (profiles/r02_v1_timeline.txt)
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_colsum, dim3(cdiv((int64_t)h->Gp * h->K, 64)), dim3(1024), 0, h->stream,
                                                  h->YTpart, h->red + h->off_y, h->nrg, (int64_t)h->Gp * h->K, h->Gp * h->K,
                                                  h->n_ovf > 0 ? h->ovf_col_chunk_ptr : nullptr, h->n_ovf > 0 ? h->ovf_csum : nullptr, h->K, h->G));
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_yw_dot, dim3(h->n_yw), dim3(CA_TB), 0, h->stream, h->YWpart,
                                                  h->nseg + (h->n_ovf > 0 ? 1 : 0), h->F, h->D, h->K, h->N, h->YW, h->yw_part));
  }
  h->ycache_valid = true;
  return CA_OK;
}

// Backward half of a train pass.  Needs: coef / dgl from the cell epilogue, mu of the same eps, red[0..3+C) cell sums.
// cell_sums_global: red[0..3+C) was already all-reduced by the monitor pass that produced it (fused path).

// arguments of the O(K + C) body (ca_final_small_body): monitor form (apply = 0, ELBO out) or train form
ca_small_args small_args(ca_engine* h, const double* gene_part, int apply, float lr_t, double* elbo_dst, bool reduce_cells) {
  ca_small_args a;
  a.enabled = 1;
  a.red = h->red; a.gene_part = gene_part; a.ngblk = h->ngblk;
  a.vchi = h->vchi; a.alpha_u = h->alpha_u; a.m_v = h->m_v; a.v_v = h->v_v; a.m_a = h->m_a; a.v_a = h->v_a; a.g_v = h->g_v; a.g_a = h->g_a;
  a.elbo_out = elbo_dst; a.terms_out = h->terms_dev;
  a.G = h->G; a.C = h->C; a.K = h->K; a.apply = apply;
  a.lr_t = lr_t; a.b1 = (float)h->opt.beta1; a.b2 = (float)h->opt.beta2; a.aeps = (float)h->opt.adam_eps;
  a.vmm_part = h->vmm_part; a.vmm = h->vmm; a.D = h->D;
  a.dir_const = h->dir_const;
  a.cell_part = reduce_cells ? h->cell_part : nullptr; a.ncblk = h->ncblk;
  a.host_out = nullptr; a.host_flag = nullptr; a.host_seq = 0; a.reduce_only = 0;
  a.yw_part = nullptr; a.n_yw = 0;
  a.ee_part = nullptr; a.n_ee = 0;
  a.vchi_out = nullptr; a.alpha_out = nullptr;
  if (!apply && elbo_dst && h->host_seq_next && h->host_dev) {   // monitor pass inside ca_run: mirror the ELBO to the host
    a.host_out = h->host_dev + 32;
    a.host_flag = reinterpret_cast<unsigned long long*>(h->host_dev + 33);
    a.host_seq = h->host_seq_next;
    h->host_seq_next = 0;
  }
  return a;
}
// Reduce a pending monitor tail's cell partials (and psi.(YW) partials) for a sharded run: red[0 .. 3 + C) local sums,
// ready for the all-reduce.  The Y stream (side stream) must have delivered the psi.(YW) partials first.
int mon_tail_local_sums(ca_engine* h) {
  if (!h->mon_tail.enabled || !h->mon_tail.cell_part) return CA_OK;
  CACK(wait_y(h, false));
  ca_small_args r = h->mon_tail;
  r.reduce_only = 1; r.host_out = nullptr;
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_final_small, dim3(1), dim3(CA_TB), 0, h->stream, r));
  h->mon_tail.cell_part = nullptr; h->mon_tail.yw_part = nullptr;
  return CA_OK;
}
// a fused monitor pass leaves its ELBO assembly for the next train pass's per-gene kernel; if none is coming, run it now
int flush_mon_tail(ca_engine* h) {
  if (!h->mon_tail.enabled) return CA_OK;
  CACK(wait_y(h, false));
  if (h->mon_tail.yw_part) CACK(yfin_flush(h));
  if (is_sharded(h) && (h->mon_tail.cell_part || h->mon_tail_local)) {   // local sums (unless the forward made them), then the (3 + C)-double all-reduce of a monitor pass
    CACK(mon_tail_local_sums(h));
    CACK(allreduce(h, h->red, 3 + h->C));
    h->mon_tail_local = false;
  }
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_final_small, dim3(1), dim3(CA_TB), 0, h->stream, h->mon_tail));
  h->mon_tail.enabled = 0;
  return CA_OK;
}

#ifndef CA_BWD_TL3_MAXN
#define CA_BWD_TL3_MAXN 18432   // cells up to which the backward sweep takes three gene tiles per wave (see create_impl)
#endif
// backward half of a train pass: the sweep, the column sums of its partials and the cross-shard reduction.  Changes no
// variable, so ca_run may issue it before it knows whether the loop goes on (train_bwd_speculative).
int train_bwd(ca_engine* h, const float* mu32, bool cell_sums_global) {
  const int W_ = h->S + h->D;
  bool merged = false, ride_ar = false;
  ca_ar_ride ride;
  if (h->poly_fresh) {   // the backward moments of this look-ahead half are in the workspace: per-gene sums straight into red (no slabs, no column sums)
    h->poly_fresh = false;
    h->fold_now = false;
    // CA_VAR_GENE_RIDE: the reduction of those moments is not queued yet where this pass takes the merged way back (fused_pass decided); it comes with the per-gene
    // pass below, and so do the stream's column jobs if they are still pending.  (Sharded since the forward half, which cannot happen inside a fit: the launch now.)
    const bool merged_back = h->red_pending && gene_ride_merges(h);
    if (h->red_pending && !merged_back) HIPCK(h, ca_poly_reduce(h->stream, &h->pws, h->N, h->C, nullptr, nullptr, nullptr, 0, h->F, nullptr, 0, 1));
    h->red_pending = false;
    ca_yfin_args back_cols;
    memset(&back_cols, 0, sizeof(back_cols));
    if (merged_back && h->ycol_pending && !h->yfin_pending) { back_cols = yfin_args(h, h->ys_nrg, h->ys_nseg); back_cols.nrow = 0; h->ycol_pending = false; }
    CACK(yfin_flush(h));
    // a pending monitor pass's tail (reduction of the cell partials into red -- which this pass's alpha step reads --, psi.(YW) sum, ELBO assembly) rides as
    // an extra block of the per-gene launch, as it does on the matrix-core way back; sharded it is a collective of its own
    ca_small_args bwd_tail = no_small_args();
    if (is_sharded(h)) {
      // Cell-sharded (round 6, late): ONE collective per iteration, as on the sweeps.  What travels: the pending monitor pass's local cell sums, Y^T psi, the
      // backward moments Q (the per-gene gradients follow from the global Q on every rank alike) and every rank's max |psi| -- the prefix of `red` up to off_g.
      // Then the per-gene launch; the monitor pass's assembly rides on the update launch.
      bool local_sums = false;
      if (h->mon_tail.enabled && h->mon_tail.cell_part) { CACK(mon_tail_local_sums(h)); local_sums = true; }   // (red[0 .. 3 + C): this rank's sums)
      else if (h->mon_tail.enabled && h->mon_tail_local) local_sums = true;                                      // (... made on the forward's reduction launch)
      h->mon_tail_local = false;
      CACK(wait_y(h, true));
      if (!h->poly_xslot_pending)
        HIPCK(h, ca_poly_xslot(h->stream, h->poly_xmax_ready ? h->poly_xpart : nullptr, (int)cdiv(h->N, CA_TB), h->F, h->N, h->red + h->off_x, h->opt.rank,
                               std::max(h->opt.world, 1)));
      h->poly_xslot_pending = false;
      const int64_t skip = (cell_sums_global && !local_sums) ? 3 + h->C : 0;   // (a flushed monitor pass left the cell sums global already)
      CACK(allreduce(h, h->red + skip, h->off_g - skip));
      h->poly_xglob_steps = 0;
      CACK(prof_begin(h, CA_KERNEL_BWD));
      const hipError_t e = ca_poly_backward(h->stream, &h->pws, h->V, mu32, h->Lb, h->G, h->C, h->red + h->off_g, nullptr);
      HIPCK(h, e);
      CACK(prof_end(h));
      h->poly_df = true;
      h->ycache_valid = false;   // red_y now holds the GLOBAL sum
      return CA_OK;
    }
    else if (h->mon_tail.enabled && h->mon_tail.cell_part && h->upd_merge && h->opt.reserved[1] != 6) {
      // Two stages, like the sweeps' split tail: the block sums of the cell partials (and of the psi.(YW) partials, complete since the cell launch) ride HERE, beside
      // the per-gene blocks -- 5 us against their 6 --; the sums over the gene blocks and the fp64 chains of the assembly ride on the update launch's monitor block,
      // under its own 12 us.  Whole in this launch the body took 11 us and was the launch (rocprofv3: k_final_small 11.3 us alone, k_poly_gene 6.3).
      CACK(wait_y(h, false));
      bwd_tail = h->mon_tail;
      bwd_tail.reduce_only = 1; bwd_tail.host_out = nullptr;
      h->mon_tail.cell_part = nullptr; h->mon_tail.yw_part = nullptr;   // (second stage: the assembly from red and the gene partials)
    }
    else if (h->mon_tail.enabled) { CACK(wait_y(h, false)); bwd_tail = h->mon_tail; h->mon_tail.enabled = 0; }   // (reserved[1] = 6: whole, lab)
    CACK(prof_begin(h, CA_KERNEL_BWD));
    hipError_t e;
    if (merged_back) {
      if (++h->gene_tag == 0u) h->gene_tag = 1u;
      // (0.5 s: every reducer a gene block waits for has a lower block index and depends on nobody in the launch, ca_polygene.hip.h)
      e = ca_poly_backward_merged(h->stream, &h->pws, h->V, mu32, h->Lb, h->G, h->C, h->red + h->off_g, &bwd_tail, back_cols.ncol > 0 ? &back_cols : nullptr,
                                  h->poly_nb_ub, h->gene_tag, 50000000ull, reinterpret_cast<unsigned int*>(h->host_dev + 44));
    } else e = ca_poly_backward(h->stream, &h->pws, h->V, mu32, h->Lb, h->G, h->C, h->red + h->off_g, &bwd_tail);
    HIPCK(h, e);
    CACK(prof_end(h));
    h->poly_df = true;
  } else
  if (h->bwd_mfma) {
    h->poly_df = false;
    const int xb = cdiv(h->nwt, CA_TB / 64);
    // A pending monitor pass's tail rides on the sweep as one extra block (its fp64 chains hide under 130 us of sweep):
    // whole when unsharded; sharded, only the local sums of the cell / psi.(YW) partials -- ONE all-reduce per iteration
    // then carries them together with this pass's gene sums and the ELBO is assembled after it (k_final_gene's extra
    // block, or ca_run's flush).  Both need the Y stream's psi.(YW) partials: the side stream is awaited here, one
    // kernel later than the cell epilogue that used to need it.
    // The riding count-matrix stream's finishing sums are further extra blocks of this launch.  The pending monitor tail needs one of
    // them (the psi.(YW) partials), so it moves on to the per-gene kernel's extra block (train_update) when they ride here.
    ca_yfin_args yfin;
    memset(&yfin, 0, sizeof(yfin));
    // Sharded over the peer-to-peer transport (round 4): the stream's finisher rides here as it does unsharded, the psi.(YW) partial sum a
    // pending monitor pass needs is added to its cell sum INSIDE the all-reduce's launch, and so are the column sums of this sweep's
    // slabs -- fwd, bwd, all-reduce, update: four launches where there were six.  Other transports keep the launches.
    ride_ar = is_sharded(h) && p2p_ride_ok(h, h->red_n);
    if (h->ycol_pending) CACK(yfin_flush(h));   // (column sums a series pass left for a merged way back that never came: this sweep's update reads them)
    if (is_sharded(h) && !ride_ar) CACK(yfin_flush(h));   // (the tail's local sums go into this pass's all-reduce, so they stay here)
    if (h->yfin_pending) { yfin = yfin_args(h, h->ys_nrg, h->ys_nseg); h->yfin_pending = false; }
    ca_small_args bwd_tail = no_small_args();
    bool split_tail = false;
    if (h->mon_tail.enabled && h->mon_tail.cell_part) {
      CACK(wait_y(h, false));   // the psi.(YW) partials; the column products may still be streaming beside this sweep
      bwd_tail = h->mon_tail;
      merged = is_sharded(h);
      if (merged) { bwd_tail.reduce_only = 1; bwd_tail.host_out = nullptr; }
      if (merged && ride_ar && yfin.nrow > 0 && bwd_tail.yw_part) {   // the partials are made by this very launch: their sum rides in the all-reduce
        ride.yw_part = bwd_tail.yw_part; ride.n_yw = bwd_tail.n_yw; ride.yw_index = 0;
        bwd_tail.yw_part = nullptr;
      }
      // the psi.(YW) partials are being made by this very launch: the cell partials are reduced here, the rest of the tail
      // (their sum, the assembly) follows on the per-gene kernel's extra block
      split_tail = !merged && yfin.nrow > 0 && bwd_tail.yw_part != nullptr;
      if (split_tail) { bwd_tail.reduce_only = 1; bwd_tail.host_out = nullptr; bwd_tail.yw_part = nullptr; }
    }
    const int nextra = (bwd_tail.enabled || yfin.nrow) ? 1 + cdiv(yfin.ncol, CA_TB / 64) + yfin.nrow : 0;
    const ca_bwdm_extra extra = {bwd_tail, yfin, cdiv(nextra, xb)};   // (rows: extra block rows behind the sweep's)
    // mc_samples = 2 (round 4): both samples in ONE sweep (k_bwd_mfma<.., S2>: one exp per (cell, gene) for the two of them)
    const bool s2b = h->s2f && h->S == 2 && !h->c16;
    ca_bwdm_ops o;
    memset(&o, 0, sizeof(o));
    if (h->bwd_pairs) {
      // 17..32 clones, or 9..16 with mc_samples >= 2: the sixteen-clone form once per sample and pair of clone chunks, accumulating into the same partials
      // (the copy numbers of the pair: Lb + 2 pair G 8, a chunk of zeros behind an odd last one; coef: one image per sample and pair, k_cell_par)
      // an odd last chunk stands alone: the eight-clone form on its own image (k_cell_par wrote it in that layout)
      for (int s = 0; s < h->S; ++s)
        for (int pr = 0; pr < h->bwd_pairs; ++pr) {
          const bool lone = (h->nchunk & 1) && pr == h->bwd_pairs - 1;
          o.coefq = h->coefq + ((int64_t)s * h->bwd_pairs + pr) * h->N16 * 32; o.Lb = h->Lb + (int64_t)pr * 2 * h->G * CA_CW; o.mu = mu32 + (int64_t)s * h->G;
          o.sidx = s; o.first_s = pr == 0 ? 1 : 0; o.extra = (s == 0 && pr == 0) ? &extra : nullptr;
          o.c16 = !lone;
          o.coefq1 = lone ? nullptr : h->coefq + ((int64_t)(h->S + s) * h->bwd_pairs + pr) * h->N16 * 32;   // (the third-part image of this sample and pair)
          CACK(launch_bwd_mfma(h, h->D == 1 ? 1 : 2, o));
        }
    } else {
      o.Lb = h->Lb; o.first_s = 1; o.frac = h->bwd_frac; o.c16 = h->c16; o.s2 = s2b; o.tl3 = h->bwd_tl == 3;
      if ((h->D == 1 || h->D == 2) && (s2b || h->c16)) o.coefq1 = h->coefq + h->N16 * 32;   // (C16: the third-part image, S = 1)
      if ((h->D == 1 || h->D == 2) && s2b) o.mu1 = mu32 + h->G;
      for (int s = 0; s < (s2b ? 1 : h->S); ++s) {
        o.coefq = h->coefq + (int64_t)s * h->N16 * 32; o.mu = mu32 + (int64_t)s * h->G; o.sidx = s; o.extra = s == 0 ? &extra : nullptr;
        CACK(launch_bwd_mfma(h, h->D, o));   // (D = 3, 4: the three-tile wave)
      }
    }
    if (bwd_tail.enabled) {
      if (merged) { h->mon_tail.cell_part = nullptr; h->mon_tail.yw_part = nullptr; }   // local sums done; assembly still pending
      else if (split_tail) h->mon_tail.cell_part = nullptr;
      else h->mon_tail.enabled = 0;
    }
    // (summing the sweep's partials inside k_final_gene instead -- one thread per gene, csplit_m loads in a row -- was
    //  slower than this parallel launch at 100k cells: 2219 -> 2190 it/s; small unsharded problems fold it: fold_gsum)
    h->fold_now = h->fold_gsum && !is_sharded(h);
    if (ride_ar) { ride.gpart = h->gpart; ride.nslice = h->csplit_m; ride.fold_n = (int64_t)h->G * W_; }
    else if (!h->fold_now)
      LAUNCH(h, CA_KERNEL_OTHER,
             hipLaunchKernelGGL(k_colsum, dim3(cdiv((int64_t)h->G * W_, 64)), dim3(1024), 0, h->stream, h->gpart,
                                h->red + h->off_g, h->csplit_m, (int64_t)h->G * W_, h->G * W_));
  } else {
    h->fold_now = false;
    h->poly_df = false;
    CACK(yfin_flush(h));
    CACK(flush_mon_tail(h));
    for (int s = 0; s < h->S; ++s)
      for (int ch = 0; ch < h->nchunk; ++ch) {
        BwdArgs a;
        a.coef = h->coef + ((int64_t)s * h->nchunk + ch) * h->N * CA_CW;
        a.F = h->F; a.em = h->etamax2;
        a.Lb = h->Lb + (int64_t)ch * h->G * CA_CW;
        a.mu = mu32 + (int64_t)s * h->G;
        a.Vs = h->Vs; a.V = h->V; a.gpart = h->gpart; a.dFpart = h->dFpart;
        a.N = h->N; a.G = h->G; a.cchunk = h->cchunk; a.D = h->D; a.S = h->S; a.sidx = s;
        a.first_s = (ch == 0); a.first = (s == 0 && ch == 0);
        const int nc = std::min(CA_CW, h->C - ch * CA_CW);
        LAUNCH(h, CA_KERNEL_BWD, launch_bwd(h->RG, nc, dim3(cdiv(h->ntile, CA_TB / 64), h->csplit), h->stream, a));
      }
    LAUNCH(h, CA_KERNEL_OTHER,
           hipLaunchKernelGGL(k_colsum, dim3(cdiv((int64_t)h->G * W_, 64)), dim3(1024), 0, h->stream, h->gpart,
                              h->red + h->off_g, h->csplit, (int64_t)h->G * W_, h->G * W_));
  }
  // the Y stream's results (Y^T psi in red_y, the psi.(YW) partials) are first needed from here on
  CACK(wait_y(h, true));
  // sharded loop: a pending monitor pass's cell sums travel with this pass's gene sums -- ONE all-reduce per iteration;
  // the ELBO is assembled after it (k_final_gene's extra block, or ca_run's flush)
  // (series-capable engines: the gene sums are the LAST part of the buffer and the ranks' max |psi| travel too, see ca_engine::off_q)
  if (h->poly && is_sharded(h)) {
    HIPCK(h, ca_poly_xslot(h->stream, h->poly_xmax_ready ? h->poly_xpart : nullptr, (int)cdiv(h->N, CA_TB), h->F, h->N, h->red + h->off_x, h->opt.rank,
                           std::max(h->opt.world, 1)));
    h->poly_xglob_steps = 0;
    h->poly_xslot_pending = false;
  }
  const int64_t skip = (cell_sums_global && !merged) ? 3 + h->C : 0;
  ride.fold_lo = h->off_g - skip;
  CACK(allreduce(h, h->red + skip, h->red_n - skip, ride_ar ? &ride : nullptr));
  if (is_sharded(h)) h->ycache_valid = false;   // red_y now holds the GLOBAL sum
  return CA_OK;
}

// update half: per-gene / per-cell gradients from the reduced sums, Adam when `apply`
// will the update half of a train pass take the one-launch form (k_update_merged)?  (the loop has announced the next eps pair, the fused forward
// sweep that follows can make the exponent bound itself, K >= 1)
inline bool update_merges(const ca_engine* h, int apply, const double* elbo_dst) {
  const int64_t mB = h->s2 ? 2 * h->hint_A + 1 : h->hint_B;
  return apply && h->upd_merge && !elbo_dst && h->pre_ok && h->hint_A >= 0 && mB >= 0 && h->fused_ok && h->gene_part_alt && h->fwd_cell && h->K > 0;
}
// the next fused pass's per-gene prologue for eps draws A and B, riding on the update (ca_pre_args): into the alternate partial buffers, fused_pass swaps them in
ca_pre_args pre_args(const ca_engine* h, int64_t A, int64_t B) {
  ca_pre_args pre;
  memset(&pre, 0, sizeof(pre));
  pre.nblk = h->ngblk;
  pre.loc = h->loc; pre.ls = h->ls; pre.epsA = h->eps_dev + A * (int64_t)h->G; pre.epsB = h->eps_dev + B * (int64_t)h->G;
  pre.colsum = h->colsum; pre.Lb = h->Lb; pre.V = h->V; pre.YtX = h->YtX; pre.muA = h->mu32; pre.muB = h->s2 ? h->mu32 + h->G : h->mu32B; pre.Mb = h->Mb2;
  pre.s2 = h->s2 ? 1 : 0;
  pre.gene_partA = h->gene_part_alt; pre.gene_partB = h->gene_partB_alt; pre.Mq = h->fwd_mfma ? h->Mq : nullptr;
  pre.G = h->G; pre.D = h->D; pre.K = h->K; pre.mrow = h->frow; pre.C = h->C;
  return pre;
}
// The int8 count-matrix stream's quantiser for the state an Adam step is about to produce, as extra blocks of the update's launch (W and psi are final there):
// possible when the exponents can be bounded from the maxima of the state before (`ys_steps` steps ago, + this one).  nblk = 0: it does not ride (ys_quant runs it).
ca_ysq_args ys_quant_ride(ca_engine* h) {
  ca_ysq_args a;
  memset(&a, 0, sizeof(a));
  if (!h->y_ys || h->K == 0 || h->ys_quant_ready) return a;
  bool lagged = false;
  const ca_ysq_args q = ys_quant_args(h, h->ys_steps >= 0 ? h->ys_steps + 1 : -1, &lagged);
  if (!lagged) return a;
  h->ys_quant_ready = true;
  return q;
}
// psi is final: the Y pass for the new parameters goes to the side stream from HERE (its launches are issued by the
// next pass, so the main stream is not left waiting for the host to get through them), and what the update still has to run
// (k_adam_cell -- q(z) logits, exponent bound, the O(K + C) update and the next pass's per-gene prologue: 12-16 us) is its head
// start over the next forward sweep.  The Y stream needs one: letting the sweep and the Y kernel start together
// cost 18 % (2219 -> 1825 it/s; the sweep's blocks take the CUs first).  Not when the stream rides on the sweep's launch.
int defer_y_to_side(ca_engine* h) {
  if (!h->async_y || h->K == 0 || h->ride_ok || h->ride_ys) return CA_OK;
  HIPCK(h, hipEventRecord(h->ev_params, h->stream));
  h->y_defer = true;
  return CA_OK;
}
// bookkeeping after an applied Adam step (both forms of the update).  xmax_ready: the launch left max |psi| of the stepped state per 256-cell piece (ca_merge_args::xpart)
void adam_stepped(ca_engine* h, bool xmax_ready) {
  if (h->ys_steps >= 0) h->ys_steps += 1;
  h->b1p *= (float)h->opt.beta1;
  h->b2p *= (float)h->opt.beta2;
  h->adam_steps += 1;
  h->poly_xmax_ready = xmax_ready;
  if (h->poly_xglob_steps >= 0) h->poly_xglob_steps += 1;
  h->ycache_valid = false;
  h->yfin_pending = false; h->ycol_pending = false;
  h->look_valid = false;
  if (h->poly && h->y_ys && h->K > 0) h->poly_y_defer = true;   // series form: the next series pass sends the count-matrix products of the stepped state to the side stream
}
int train_update(ca_engine* h, const float* eps, int apply, double* elbo_dst) {
  const int N256 = cdiv(h->N, CA_TB);
  float lr_t = 0.f;
  if (apply) {
    // lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), float32 like TF's _prepare()/_apply_dense
    lr_t = (float)h->opt.learning_rate * sqrtf(1.f - h->b2p) / (1.f - h->b1p);
  }
  // A pending monitor pass's ELBO is assembled by one extra block of the per-gene kernel (ca_final_small_body: the
  // reduction of the cell / psi.(YW) partials unless train_bwd did it for the all-reduce, then the assembly) BEFORE the
  // O(K + C) update, which rides on the per-cell kernel the same way.
  CACK(yfin_flush(h));   // (nothing pending when a backward sweep preceded)
  ca_small_args mon = no_small_args();
  if (h->mon_tail.enabled) { mon = h->mon_tail; h->mon_tail.enabled = 0; }
  // psi's own step: extra blocks of the per-gene kernel (it needs the sweep's dF partials and YW, nothing per-gene)
  ca_psi_args psi;
  memset(&psi, 0, sizeof(psi));
  if (h->K > 0) {
    psi.nblk = N256; psi.F = h->F; psi.YW = h->YW; psi.dFpart = h->dFpart; psi.m_psi = h->m_psi; psi.v_psi = h->v_psi; psi.g_psi = h->g_psi;
    psi.N = h->N; psi.D = h->D; psi.K = h->K; psi.ntile = h->poly_df ? 1 : h->bwd_mfma ? cdiv(h->nwt, CA_TB / 64) : h->ntile;
  }
  h->pre_valid = false;
  // Round 4: the whole update half in ONE launch (k_update_merged) whenever the loop has announced the next eps pair, the fused forward
  // sweep that follows can make the exponent bound itself (fwd_cell) and K >= 1 -- see the kernel.  Everything else (call-by-call API,
  // the last step of a run, the VALU / two-kernel forward paths) keeps the two launches below.
  {
    int64_t mA = h->hint_A, mB = h->hint_B;
    if (h->s2) { mA = 2 * h->hint_A; mB = mA + 1; }
    if (update_merges(h, apply, elbo_dst)) {
      ca_merge_args mg;
      memset(&mg, 0, sizeof(mg));
      h->gate_armed = false;
      if (h->gate_req && h->host_dev) {   // ca_run: wait on the device for the host's decision (every block but the monitor block)
        // (the gate word and the error word each in a cache line of their own: doubles 32 / 33 are the ELBO and its flag, which the host spins on)
        // (pinned doubles: 32 / 33 the ELBO and its flag, which the host spins on; 40 the fatal word; 48 the host's answer; 56 the relay's verdict)
        mg.gate = reinterpret_cast<const unsigned long long*>(h->host_dev + 48); mg.gate_seq = ++h->gate_seq;
        mg.gate_ack = reinterpret_cast<unsigned long long*>(h->host_dev + 56);
        mg.gate_err = reinterpret_cast<unsigned long long*>(h->host_dev + 40);
        mg.gate_local = h->gate_local;
        mg.gate_timeout = h->gate_ticks;   // the RELAY's patience (s_memrealtime ticks, 100 MHz): ~1 ms, then the launch stores nothing and the host re-queues it
        h->gate_armed = true;
        h->gate_t0 = std::chrono::steady_clock::now();   // (before the launch below: the relay's clock starts no earlier)
      }
      h->gate_req = false;
      mg.pre = pre_args(h, mA, mB);
      mg.ysq = ys_quant_ride(h);   // the int8 stream's images of the stepped W and psi (exponents from the lagged maxima, as on k_adam_cell)
      if (mg.ysq.nblk) {
        mg.ysq.nblk = h->ngblk + N256;
        h->ys_namax[(h->ys_slot + 1) % 3] = h->ngblk + N256;   // one pair per gene block, then one per psi block
      }
      mg.tail = small_args(h, h->gene_part, 1, lr_t, nullptr, false);
      mg.tail.terms_out = nullptr;                 // (the pending monitor pass's block of this launch owns the ELBO terms)
      mg.tail.vmm_part = nullptr; mg.tail.vmm = nullptr;   // the range of V' is the next sweep's business
      mg.tail.vchi_out = h->vchi_alt; mg.tail.alpha_out = h->alpha_u_alt;
      mg.glogit = h->glogit; mg.dgl = h->dgl; mg.m_gl = h->m_gl; mg.v_gl = h->v_gl; mg.C = h->C; mg.ncell = N256;
      if (!h->vmm_at_ready) {   // first merged update of this engine: both range buffers at (+inf, -inf); from here on every launch resets the next one's
        int init[32];
        for (int i = 0; i < 32; ++i) init[i] = (i & 8) ? (int)0x807FFFFF /* ca_f2ord(-inf) */ : (int)0x7F800000 /* ca_f2ord(+inf) */;
        HIPCK(h, hipMemcpyAsync(h->vmm_at, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));   // (the source is on this stack frame)
        h->vmm_at_ready = true;
      }
      mg.vmm_at = h->vmm_at + 16 * h->vmm_at_idx; mg.vmm_at_next = h->vmm_at + 16 * (1 - h->vmm_at_idx);
      mg.xpart = (h->poly && h->K == 1 && h->D == 1 && h->opt.reserved[1] != 5) ? h->poly_xpart : nullptr;   // (reserved[1] = 5: k_poly_xmax as a launch of its own, lab)
      // the sweep-independent part of the per-gene gradient: left by the prologue that made this pass's eps draw (if it was a merged
      // update's, with the parameters still the ones it saw), and made for the next train pass's draw by this launch's prologue
      mg.aux_ld = h->G;
      const int64_t this_draw = (eps - h->eps_dev) / (int64_t)h->G;
      mg.aux_in = (h->S == 1 && h->gaux_slot >= 0 && h->gaux_slot == this_draw) ? h->gaux + (int64_t)h->gaux_idx * 5 * h->G : nullptr;
      mg.aux_out = h->S == 1 ? h->gaux + (int64_t)(1 - h->gaux_idx) * 5 * h->G : nullptr;
      LAUNCH(h, CA_KERNEL_OTHER,
             hipLaunchKernelGGL(k_update_merged, dim3(h->ngblk + (mon.enabled ? 1 : 0) + 1 + cdiv(psi.nblk, 4) + cdiv(N256, 4)), dim3(CA_UM_TB), 0, h->stream,
                                h->red + h->off_g, h->red + h->off_y, eps, h->colsum, h->YtX, h->vchi, h->loc, h->ls, h->V, h->m_loc, h->v_loc,
                                h->m_ls, h->v_ls, h->m_V, h->v_V, h->g_loc, h->g_ls, h->g_V, h->Vs, h->vmm_part, h->G, h->S, h->D, h->K, lr_t,
                                (float)h->opt.beta1, (float)h->opt.beta2, (float)h->opt.adam_eps, mon, h->ngblk, psi,
                                h->fold_now ? h->gpart : nullptr, h->csplit_m, mg));
      h->fold_now = false;
      CACK(defer_y_to_side(h));   // (2- / 4-byte storage, K != 1)
      std::swap(h->vchi, h->vchi_alt);
      std::swap(h->alpha_u, h->alpha_u_alt);
      h->em_stale = true;
      h->vmm_at_idx = 1 - h->vmm_at_idx;   // (the buffer this launch filled is the other one from now on: vmm_at_cur below)
      h->gaux_idx = 1 - h->gaux_idx; h->gaux_slot = h->S == 1 ? mB : -1;
      h->pre_valid = true; h->pre_A = mA; h->pre_B = mB;
      h->hint_A = h->hint_B = -1;
      adam_stepped(h, mg.xpart != nullptr);   // (max |psi| came with the update: the series form's next moment launches need no k_poly_xmax in front)
      return CA_OK;
    }
  }
  if (apply) h->gaux_slot = -1;   // the per-gene parameters change without a prologue that leaves the next step's sweep-independent part
  LAUNCH(h, CA_KERNEL_OTHER,
         hipLaunchKernelGGL(k_final_gene, dim3(h->ngblk + (mon.enabled ? 1 : 0) + psi.nblk), dim3(CA_TB), 0, h->stream, h->red + h->off_g,
                            h->red + h->off_y, eps, h->colsum, h->YtX, h->vchi, h->loc, h->ls, h->V, h->m_loc, h->v_loc, h->m_ls,
                            h->v_ls, h->m_V, h->v_V, h->g_loc, h->g_ls, h->g_V, h->Vs, h->vmm_part, h->G, h->S, h->D, h->K, apply,
                            lr_t, (float)h->opt.beta1, (float)h->opt.beta2, (float)h->opt.adam_eps, mon, h->ngblk, psi,
                            h->fold_now ? h->gpart : nullptr, h->csplit_m));
  h->fold_now = false;
  if (apply) CACK(defer_y_to_side(h));   // (the per-cell kernel below is the Y pass's head start over the next forward sweep)
  // the next fused pass's per-gene prologue, when the loop has announced its eps slots: extra blocks of the per-cell kernel
  ca_pre_args pre;
  memset(&pre, 0, sizeof(pre));
  // (the hints are PASS slots; two samples per pass for mc_samples = 2)
  int64_t hA = h->hint_A, hB = h->hint_B;
  if (h->s2) { hA = 2 * h->hint_A; hB = hA + 1; }
  if (apply && h->pre_ok && h->hint_A >= 0 && hB >= 0 && h->fused_ok && h->gene_part_alt) pre = pre_args(h, hA, hB);
  // the int8 count-matrix stream's quantiser for the state this step produces: extra blocks of the same launch (W and psi are
  // final since k_final_gene), exponents bounded from the maxima of the state before (`ys_steps` steps ago, + this one)
  ca_ysq_args ysq;
  memset(&ysq, 0, sizeof(ysq));
  if (apply) ysq = ys_quant_ride(h);
  LAUNCH(h, CA_KERNEL_OTHER,
         hipLaunchKernelGGL(k_adam_cell, dim3(N256 + 1 + pre.nblk + ysq.nblk), dim3(CA_TB), 0, h->stream, h->F, h->glogit, h->dgl, h->m_gl, h->v_gl,
                            h->N, h->C, h->D, apply, lr_t, (float)h->opt.beta1, (float)h->opt.beta2, (float)h->opt.adam_eps,
                            h->vmm_part, h->ngblk, h->etamax2, small_args(h, h->gene_part, apply ? 1 : 0, lr_t, elbo_dst, false),
                            N256, pre, ysq));
  if (pre.nblk) { h->pre_valid = true; h->pre_A = hA; h->pre_B = hB; }
  h->hint_A = h->hint_B = -1;
  if (apply) adam_stepped(h, false);   // (V', its range and etamax2 were refreshed inside the step's own kernels)
  return CA_OK;
}

int train_tail(ca_engine* h, const float* eps, const float* mu32, int apply, double* elbo_dst, bool cell_sums_global) {
  CACK(train_bwd(h, mu32, cell_sums_global));
  return train_update(h, eps, apply, elbo_dst);
}

// One evaluation of the model for the eps of device slot `eps_slot`.
//   mode CA_MODE_ELBO : forward only, ELBO -> elbo_dst        (`sess$run(elbo)`)
//   mode CA_MODE_GINIT: forward only, overwrite the q(z) logits (`gamma_init`)
//   mode CA_MODE_TRAIN: forward + backward (+ Adam when apply)  (`sess$run(train)`)
int run_pass(ca_engine* h, int64_t eps_slot, int mode, int apply, double* elbo_dst) {
  const float* eps = h->eps_dev + eps_slot * (int64_t)h->S * h->G;
  h->poly_fresh = false;   // (a plain pass makes its own forward half: backward moments left by an unused look-ahead are nobody's)
  h->poly_y_defer = false;   // (... and runs its count-matrix pass in line, as ever: the deferral was for a series pass)
  CACK(flush_mon_tail(h));
  CACK(ensure_etamax(h));
  if (mode != CA_MODE_TRAIN) h->hint_A = h->hint_B = -1;
  h->pre_valid = false;   // this pass rewrites mu32 and the current per-gene partials
  LAUNCH(h, CA_KERNEL_OTHER,
         hipLaunchKernelGGL(k_gene_pre, dim3(h->ngblk), dim3(CA_TB), 0, h->stream, h->loc, h->ls, eps, h->colsum, h->Lb, h->V,
                            h->D, h->K, h->YtX, h->mu32, h->Mb, h->gene_part, h->G, h->S, h->nchunk, CA_CW, 0, CA_CW));
  CACK(ensure_ycache(h));
  if (h->pfwd) {
    // the pass's S x nchunk slices of M two to a sixteen-column matrix-core sweep (round 6; mc_samples = 3: two sweeps where there were three vector sweeps
    // of 1.4x the time each; 20 clones: two where there were three)
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_mq_pairs, dim3(h->ngblk, h->S * h->nchunk), dim3(CA_TB), 0, h->stream, h->Mb, h->pf_Mq, h->G, h->nk32));
    for (int pr = 0; pr < h->pf_npair; ++pr) {
      const unsigned short* mq = h->pf_Mq + (int64_t)pr * h->nk32 * 1024;
      float* zp = h->pf_Z + (int64_t)pr * h->pf_fsplit * h->N * 16;
      CACK(launch_fwd_mfma(h, mq, zp, h->pf_fsplit, h->pf_kchunk));
    }
  } else
  for (int s = 0; s < h->S; ++s)
    for (int ch = 0; ch < h->nchunk; ++ch) {
      const int nc = std::min(CA_CW, h->C - ch * CA_CW);
      const float* M = h->Mb + ((int64_t)s * h->nchunk + ch) * h->G * CA_CW;
      // Zpart [S][gsplit][nchunk][N][8]: the kernel strides its split index by N*8, so pass per-(s,ch) bases
      // laid out as [s][ch][split][N][8]
      float* Zp = h->Zpart + (((int64_t)s * h->nchunk + ch) * h->gsplit) * h->N * CA_CW;
      LAUNCH(h, CA_KERNEL_FWD, launch_fwd(nc, h->D, dim3(cdiv(h->N, CA_TB * kFwdR), h->gsplit), h->stream, h->F, h->etamax2, h->Vs, M, Zp, h->N, h->G, h->gchunk));
    }
  CACK(wait_y(h, true));   // the cell epilogue is the first consumer of YW / Y^T psi
  // (matrix-core products arrive as finished row sums: one "strip", already in YW)
  const bool yw_done = h->y_ys;
  const float* ywp = yw_done ? h->YW : h->YWpart;
  const int ywseg = yw_done ? 1 : h->nseg + (h->n_ovf > 0 ? 1 : 0);
  if (h->C <= 64) {
    CACK(launch_cell_par(h, ywp, ywseg, mode));
  } else {
    LAUNCH(h, CA_KERNEL_CELL,
           hipLaunchKernelGGL(k_cell, dim3(h->ncblk), dim3(CA_TB), 0, h->stream, h->Zpart, h->A, h->cn, h->s64, h->etamax2, h->glogit,
                              h->alpha_u, h->F, ywp, h->YW, h->coef, h->dgl, h->scratch, h->cell_part, h->N, h->C, h->S, h->D,
                              h->K, h->gsplit, h->nchunk, ywseg, mode));
  }
  if (mode == CA_MODE_GINIT) return CA_OK;
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_reduce_part, dim3(3 + h->C), dim3(CA_TB), 0, h->stream, h->cell_part, h->red, h->ncblk, 3 + h->C));
  if (mode == CA_MODE_TRAIN) return train_tail(h, eps, h->mu32, apply, elbo_dst, false);
  CACK(allreduce(h, h->red, 3 + h->C));
  LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_final_small, dim3(1), dim3(CA_TB), 0, h->stream,
                                                small_args(h, h->gene_part, 0, 0.f, elbo_dst, false)));
  return CA_OK;
}

// Series form or sweeps for the pass about to be queued?  See ca_engine::poly_ring.  *use_series = the decision; *mirror / *seq = where and under which
// number this pass leaves its own ranges (the series form's first launch does; a pass that takes the sweeps queues the two tiny range launches itself,
// poly_ranges_for_sweeps).
#define CA_POLY_LAG 4
int poly_wait_entry(ca_engine* h, uint64_t want, double out[3]) {
  volatile double* e = h->poly_ring + (want % 16) * 4;
  unsigned spins = 0;
  auto t_next = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::seconds(20);
  while (e[0] != (double)want) {
    if ((++spins & 0x3FFu) == 0 && std::chrono::steady_clock::now() >= t_next) {
      t_next = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
      const hipError_t q = hipStreamQuery(h->stream);
      if (q != hipSuccess && q != hipErrorNotReady) HIPCK(h, q);
      if ((q == hipSuccess && e[0] != (double)want) || std::chrono::steady_clock::now() >= t_end) {
        h->err = "internal: the ranges of an earlier pass never reached the host (series form's look ahead)";
        return CA_ERR_STATE;
      }
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  out[0] = e[1]; out[1] = e[2]; out[2] = e[3];
  return CA_OK;
}
// Where max |psi| of the current state comes from for the series form's ranges.  Unsharded: the merged update's per-piece maxima where current, else a launch.
// Cell-sharded (round 6, late): every rank must use the SAME number -- the bin geometry, hence the moments every rank computes for itself, and the host's
// series-or-sweeps decision follow from it.  The ranks' maxima travel in the fit's one collective per iteration (slots at off_x, ca_poly_xslot) for the state
// BEFORE that iteration's update; the state after it is covered by adding what one Adam step can move a variable.  Where the slots hold nothing current (a new
// engine, a restart, a set_param, a cancelled update) they are refreshed by a small collective of their own: every rank gets there together, the decisions
// up to this point having been the same on all of them.
struct ca_xsrc { const float* xpart; int nx; const double* xglob; int nglob; double xadd; };
inline double poly_step_bound(const ca_engine* h) {
  // no Adam step moves a variable further (ca_adam_step_bound: the bound the int8 stream's lagged exponents rest on too; > 0 wherever the series form exists, create_impl)
  return h->adam_bound * 1.0001;
}
int poly_xsrc(ca_engine* h, ca_xsrc* x) {
  memset(x, 0, sizeof(*x));
  const int nx = (int)cdiv(h->N, CA_TB);
  if (is_sharded(h)) {
    const int W = std::max(h->opt.world, 1);
    if (h->poly_xglob_steps < 0 || h->poly_xglob_steps > 1) {
      HIPCK(h, ca_poly_xslot(h->stream, h->poly_xmax_ready ? h->poly_xpart : nullptr, nx, h->F, h->N, h->red + h->off_x, h->opt.rank, W));
      CACK(allreduce(h, h->red + h->off_x, W));
      h->poly_xglob_steps = 0;
      h->poly_xslot_pending = false;
    }
    x->xglob = h->red + h->off_x; x->nglob = W; x->xadd = (double)h->poly_xglob_steps * poly_step_bound(h);
  } else if (h->poly_xmax_ready) { x->xpart = h->poly_xpart; x->nx = nx; }
  return CA_OK;
}
int poly_guard(ca_engine* h, bool* use_series, double** mirror, double* seq, bool* ranges_queued) {
  const uint64_t s = h->poly_seq + 1;
  *ranges_queued = false;
  *mirror = h->poly_ring_dev + (s % 16) * 4;
  *seq = (double)s;
  double r[3];
  int steps;
  if (s < h->poly_seq_base + CA_POLY_LAG) {
    // the first passes after the ranges became unknown (a new engine, a restart, a set_param): this state's own ranges, now -- the one wait for the device
    // the look ahead ever makes; the passes behind it count their steps from the base entry
    if (s == h->poly_seq_base) {
      ca_xsrc xs;
      CACK(poly_xsrc(h, &xs));
      HIPCK(h, ca_poly_ranges(h->stream, &h->pws, h->V, h->F, h->G, h->N, *mirror, *seq, xs.xpart, xs.nx, xs.xglob, xs.nglob, xs.xadd));
      *ranges_queued = true;
      h->poly_steps_at[s % 16] = h->adam_steps;
    }
    CACK(poly_wait_entry(h, h->poly_seq_base, r));
    steps = (int)(h->adam_steps - h->poly_steps_at[h->poly_seq_base % 16]);
  } else {
    CACK(poly_wait_entry(h, s - CA_POLY_LAG, r));
    steps = (int)(h->adam_steps - h->poly_steps_at[(s - CA_POLY_LAG) % 16]);
  }
  *use_series = ca_poly_covers(r[0], r[1], r[2], steps, poly_step_bound(h));
  h->poly_nb_ub = *use_series ? ca_poly_nb_ahead(r[0], r[1], r[2], steps, poly_step_bound(h)) : 0;   // (sizes the merged way back's grid, enters no result)
  h->poly_seq = s;
  h->poly_steps_at[s % 16] = h->adam_steps;
  return CA_OK;
}

// Monitor pass for eps slot A fused with the forward half of the NEXT train pass (eps slot B): one sweep,
// one exp per (cell, gene) for both (same parameters, R/inference-tflow.R:401,403 of consecutive iterations).
int fused_pass(ca_engine* h, int64_t slotA, int64_t slotB, double* elbo_dst, double* elbo_dstB = nullptr, int64_t trainA = -1) {
  // trainA >= 0 (mc_samples = 2, h->s2f): slotA / slotB are the monitor pass's two samples, trainA / trainA + 1 the next train pass's -- four draws, one sweep
  const bool s2f = trainA >= 0;
  const float* epsA = h->eps_dev + slotA * (int64_t)h->G;
  const float* epsB = h->eps_dev + slotB * (int64_t)h->G;
  if (elbo_dstB) CACK(flush_mon_tail(h));   // pair sweeps come from outside the loop: nothing may be left pending
  if (h->pre_valid && h->pre_A == slotA && h->pre_B == slotB) {   // the train pass before this one already ran the prologue
    std::swap(h->gene_part, h->gene_part_alt);
    std::swap(h->gene_partB, h->gene_partB_alt);
  } else {
    LAUNCH(h, CA_KERNEL_OTHER,
           hipLaunchKernelGGL(k_gene_pre_fused, dim3(h->ngblk), dim3(CA_TB), 0, h->stream, h->loc, h->ls, epsA, epsB, h->colsum, h->Lb,
                              h->V, h->D, h->K, h->YtX, h->mu32, h->s2 ? h->mu32 + h->G : h->mu32B, h->Mb2, h->gene_part, h->gene_partB, h->G,
                              h->frow, h->C, h->fwd_mfma ? h->Mq : nullptr, h->s2 ? 1 : 0));
  }
  if (s2f) {   // the train pair's prologue: second operand image, mu of both samples where the backward sweeps read it (the monitor pair's mu is nobody's)
    const float* epsTA = h->eps_dev + trainA * (int64_t)h->G;
    LAUNCH(h, CA_KERNEL_OTHER,
           hipLaunchKernelGGL(k_gene_pre_fused, dim3(h->ngblk), dim3(CA_TB), 0, h->stream, h->loc, h->ls, epsTA, epsTA + h->G, h->colsum, h->Lb,
                              h->V, h->D, h->K, h->YtX, h->mu32, h->mu32 + h->G, h->Mb2, h->gene_partB, h->gene_partB, h->G,
                              h->frow, h->C, h->Mq + (int64_t)h->nk32 * 1024, 1));
  }
  h->pre_valid = false;
  // the Y products of this parameter state: riding on the sweep's own launch (below), or from the side stream / in line
  h->poly_fresh = false;   // (backward moments of an earlier, unused look-ahead half are nobody's from here on)
  // (sharded: the ranks see different cells; they decide alike because max |psi| is the global one, poly_xsrc -- up to 256 ranks, a slot per rank)
  bool series = h->poly && !s2f && !elbo_dstB && !h->fwd_gate && (!is_sharded(h) || h->opt.world <= CA_TB);
  double* pl_mirror = nullptr; double pl_seq = 0.0;
  if (series) {
    bool queued = false;
    CACK(poly_guard(h, &series, &pl_mirror, &pl_seq, &queued));
    if (!series && !queued) {   // (the sweeps take this pass: its ranges all the same)
      ca_xsrc xs;
      CACK(poly_xsrc(h, &xs));
      HIPCK(h, ca_poly_ranges(h->stream, &h->pws, h->V, h->F, h->G, h->N, pl_mirror, pl_seq, xs.xpart, xs.nx, xs.xglob, xs.nglob, xs.xadd));
    }
    if (series) h->n_series += 1; else h->n_series_fallback += 1;
  }
  const bool ride = (h->ride_ok || h->ride_ys) && !h->ycache_valid && h->fwd_cell && !h->y_defer && !h->y_pending && !series;   // (the series form has no sweep launch to ride on)
  if (!ride && !series) CACK(ensure_ycache(h));   // (series: placed between its own launches, below)
  ca_cell_ptrs cp;
  cp.A = h->A; cp.cn = h->cn; cp.s64 = h->s64; cp.etamax2 = h->etamax2; cp.glogit = h->glogit; cp.F = h->F;
  cp.coef = h->coef; cp.dgl = h->dgl; cp.coefq = h->bwd_mfma ? h->coefq : nullptr;
  cp.vmm_at = nullptr; cp.etamax_w = nullptr;
  cp.gate = nullptr; cp.gate_go = 0ull;
  if (h->fwd_gate) {
    if (!(h->fwd_cell && ride && h->ride_ys) || !h->gate_local) { h->err = "internal: a forward sweep queued ahead of the host's decision must be the one-launch form"; return CA_ERR_STATE; }
    cp.gate = h->gate_local; cp.gate_go = (h->gate_seq << 1) | 1ull;
  }
  // (the series form needs no exponent bound: after a merged update it stays stale until a pass that wants it asks, ensure_etamax)
  if (series) {}
  else if (h->em_stale && h->fwd_cell && h->D > 0) { cp.vmm_at = h->vmm_at + 16 * (1 - h->vmm_at_idx); cp.etamax_w = h->etamax2; h->em_stale = false; }
  else CACK(ensure_etamax(h));
  cp.ee_partB = (elbo_dstB && h->fwd_cell) ? h->ee_partB : nullptr;
  cp.s2 = h->s2 ? 1 : 0; cp.N16 = h->N16;
  int cell_blocks = h->ncblk;
  if (series) {
    // Z of both draws from the moments of M over gene bins (ca_poly.hip), the same cell epilogue, d/dF and the backward moments in one pass over
    // the CELLS: no cells x genes sweep.  The count-matrix products of this state run as their own launch (in line).
    // Order: the forward moments ride as the first blocks of the count-matrix stream's launch (CA_VAR_MOM_RIDE, below); where they cannot, their launches come
    // FIRST, on an empty device, and the stream's launch behind them (lab, poly_side: on the side stream beside the cell launch, deferred since the update).
    cp.etamax2 = h->poly_zero; cp.coefq = nullptr; cp.vmm_at = nullptr; cp.etamax_w = nullptr;   // (the zeros: read only with CA_VAR_CELL_LEAN off)
    ca_xsrc xs_m;
    CACK(poly_xsrc(h, &xs_m));
    // Lab (ca_options.reserved[1] = 4): the moment launches on a high-priority side stream BESIDE the count-matrix stream's launch, the cell launch waiting for both.
    // Measured level with the in-line order (cfg-3: 185.3 against 184.7 us per iteration): beside the stream's HBM traffic the chain of latencies takes 75 us instead
    // of 20 -- still hidden --, but the two cross-stream dependencies cost the critical path 5 us each (rocprofv3 timeline: 7.6 us from the update's end to the
    // stream's start, 5.8 us from the stream's end to the cell launch).  In line, max |psi| comes with the update (ca_merge_args::xbits): two launches, 14 us.
    const bool moments_aside = h->opt.reserved[1] == 4 && h->stream3 && h->ev_poly0 && !h->ycache_valid && !h->poly_side && !h->y_pending;
    if (moments_aside) {
      HIPCK(h, hipEventRecord(h->ev_poly0, h->stream));
      HIPCK(h, hipStreamWaitEvent(h->stream3, h->ev_poly0, 0));
      std::swap(h->stream, h->stream3);
    }
    // CA_VAR_MOM_RIDE: the moments as the moment role of the count-matrix stream's launch (ca_polymom.hip.h) -- the stream reads the count matrix and the W / psi
    // images, the moments V, mu, L and max |psi|: neither reads what the other writes, and as blocks of one launch they need no event between them.  Wherever this
    // pass launches no stream in line (its products are cached, or go to a side stream), or max |psi| would need a launch of its own, the moments keep theirs.
    hipError_t e = hipSuccess;
    ca_pm_args pm;
    const bool mom_rides = h->mom_ride && h->y_ys && !h->ycache_valid && !h->poly_side && !moments_aside && !h->y_defer && !h->y_pending && h->host_dev &&
                           ((xs_m.xpart && xs_m.nx > 0) || (xs_m.xglob && xs_m.nglob > 0));
    if (mom_rides) {
      memset(&pm, 0, sizeof(pm));
      const int nglob = xs_m.xglob ? xs_m.nglob : 0;
      pm.V = h->V; pm.xbits = h->pws.xbits; pm.muA = h->mu32; pm.muB = h->mu32B; pm.Lb = h->Lb; pm.G = h->G; pm.C = h->C;
      pm.hdr = h->pws.hdr; pm.part = h->pws.partB; pm.bad_word = reinterpret_cast<unsigned int*>(h->host_dev + 42); pm.mirror = pl_mirror; pm.seq = pl_seq;
      pm.xpart = xs_m.xpart; pm.nx = (nglob || !xs_m.xpart) ? 0 : xs_m.nx; pm.xglob = xs_m.xglob; pm.nglob = nglob; pm.xadd = xs_m.xadd;
      pm.tabB = h->pws.tabB; pm.flags = h->pws.mflags;
      if (++h->mom_tag == 0u) h->mom_tag = 1u;
      pm.tag = h->mom_tag;
      pm.ngrp = h->pws.n_gene_blocks; pm.per = h->mom_per; pm.nmb = (int)cdiv(pm.ngrp, pm.per); pm.nred = h->mom_nred;
      pm.blk0 = h->mom_last ? h->ys_nrg * h->ys_nseg : 0;   // (CA_VAR_MOM_LAST: behind the stream's blocks, in front of the overflow list's; else the launch's first blocks)
      pm.timeout_ticks = 50000000ull;   // 0.5 s: every block a reducer waits for depends on nobody and at worst queues for a slot until stream blocks leave (ca_polymom.hip.h)
      pm.err = reinterpret_cast<unsigned int*>(h->host_dev + 43);
      h->mom_args = &pm;
    } else {
      CACK(prof_begin(h, CA_KERNEL_FWD));
      e = ca_poly_moments(h->stream, &h->pws, h->V, h->F, h->mu32, h->mu32B, h->Lb, h->G, h->N, h->C,
                          h->host_dev ? reinterpret_cast<unsigned int*>(h->host_dev + 42) : nullptr, pl_mirror, pl_seq,
                          xs_m.xpart, xs_m.nx, xs_m.xglob, xs_m.nglob, xs_m.xadd);
      int pe = (e == hipSuccess) ? prof_end(h) : CA_OK;   // (both events of the pair on the stream the chain ran on)
      if (moments_aside) {
        if (e == hipSuccess) e = hipEventRecord(h->ev_poly1, h->stream);
        std::swap(h->stream, h->stream3);
      }
      HIPCK(h, e);
      CACK(pe);
    }
    if (h->poly_side && h->poly_y_defer && !h->ycache_valid) {
      h->poly_y_defer = false;
      HIPCK(h, hipEventRecord(h->ev_params, h->stream));
      h->y_defer = true;
    }
    // (the stream's finisher stays in line behind it: on the side stream beside the cell launch its 1024-thread blocks got through late -- 198 against 187 us
    //  per iteration at cfg-3, 110 against 102 at 50k x 3k x 6)
    // ... nor as its own launch in line (5.4 us and a gap): its jobs ride as extra blocks -- the row jobs behind the cell launch's cell blocks, in the slots the
    // blocks with one pass fewer leave (a finisher block is that kernel with its 207 - 241 VGPRs: it cannot run beside two cell blocks on a CU); the column jobs,
    // whose sums nobody reads before the update, on the launch that follows (CA_VAR_GENE_RIDE; off: behind the cell blocks too, as they were)
    h->ys_defer_next = h->y_ys && !h->ycache_valid && h->opt.reserved[1] != 3;   // (reserved[1] = 3: the finisher as a launch of its own, lab)
    const int yrc = ensure_ycache(h);
    const bool mom_left = h->mom_args != nullptr;
    h->mom_args = nullptr;   // (pm leaves scope with this pass)
    CACK(yrc);
    if (mom_left) { h->err = "internal: the series form's moments were to ride on a count-matrix stream launch that was not made"; return CA_ERR_STATE; }
    h->ys_defer_next = false;
    ca_yfin_args yfin_ride;
    memset(&yfin_ride, 0, sizeof(yfin_ride));
    const bool yfin_rides = h->yfin_pending;
    if (yfin_rides) { yfin_ride = yfin_args(h, h->ys_nrg, h->ys_nseg); h->yfin_pending = false; }
    if (moments_aside) HIPCK(h, hipStreamWaitEvent(h->stream, h->ev_poly1, 0));
    CACK(prof_begin(h, CA_KERNEL_FWD));
    // cell-sharded: what the iteration's collective needs from this rank besides the moments -- the monitor pass's local block sums (red[0 .. 3 + C)) and the
    // rank's max |psi| slot -- rides on the moments' reduction launch (two extra blocks) instead of two small launches in front of the collective
    ca_small_args ltail = no_small_args();
    const bool sh = is_sharded(h) && h->tail_fuse && yfin_rides;   // (yfin_rides: the psi.(YW) partials are made by this very cell launch)
    if (sh) {
      ltail = small_args(h, h->gene_part, 0, 0.f, nullptr, true);
      ltail.ncblk = h->pws.n_cell_blocks;
      if (h->K > 0) { ltail.yw_part = h->yw_part; ltail.n_yw = h->n_yw; }
      ltail.reduce_only = 1; ltail.host_out = nullptr;
    }
    // CA_VAR_GENE_RIDE: the column jobs go with the reduction -- with the merged way back that train_bwd queues (unsharded), else as extra blocks of k_poly_red here
    const bool cols_move = yfin_rides && h->gene_cols;   // (the measured rule of create_impl: not at 100 000 cells, where the cell launch hides them)
    const bool merges = gene_ride_merges(h);
    ca_yfin_args yfin_cols = yfin_ride;
    if (cols_move) yfin_ride.ncol = 0;
    e = ca_poly_cells(h->stream, &h->pws, h->N, h->C, h->K, &cp, h->alpha_u, h->cell_part, h->dFpart, yfin_rides ? &yfin_ride : nullptr, h->cell_lean, h->cell_mfma, h->cell_edge);
    // the ONE place that decides where the reduction of the backward moments runs: here, as a launch (with the sharded fit's riders), or inside train_bwd's launch
    h->red_pending = merges;
    if (merges) h->ycol_pending = cols_move;
    else if (e == hipSuccess)
      e = ca_poly_reduce(h->stream, &h->pws, h->N, h->C, cols_move ? &yfin_cols : nullptr, sh ? &ltail : nullptr, h->poly_xmax_ready ? h->poly_xpart : nullptr,
                         (int)cdiv(h->N, CA_TB), h->F, sh ? h->red + h->off_x : nullptr, h->opt.rank, std::max(h->opt.world, 1));
    h->mon_tail_local = sh;   // (the tail set up below starts with its local sums made)
    if (sh) { h->poly_xslot_pending = true; h->poly_xglob_steps = -1; }   // (the slots hold THIS rank's number until the collective has summed them)
    HIPCK(h, e);
    CACK(prof_end(h));
    cell_blocks = h->pws.n_cell_blocks;
    h->poly_fresh = true;
  } else
  if (h->fwd_cell && ride && h->ride_ys) {   // the one-copy int8 matrix-core stream's blocks interleaved with the sweep's
    cell_blocks = h->ncblk_f;
    CACK(ys_quant(h));
    ca_ysride_args ya;
    memset(&ya, 0, sizeof(ya));
    ya.Ys = h->Ys; ya.io = ys_io(h); ya.F = h->F; ya.V = h->V; ya.Df = h->D;
    ya.Gp = h->Gp; ya.RS = h->ys_RS; ya.nb_main = h->ys_nrg * h->ys_nseg; ya.nb_y = ya.nb_main;
    ya.ovf = ys_ovf(h);
    ya.nb_y += ya.ovf.nb_rows + ya.ovf.nb_chunks;
    if (h->fwd_bal && !s2f) {   // small problems: one eight-wave sweep block per CU, left-over tiles spread gene-wise (ca_fwdbal.hip.h)
      ca_bal_args ba;
      memset(&ba, 0, sizeof(ba));
      ba.nb = h->n_cu; ba.r = h->bal_r; ba.nchunk = h->bal_nchunk; ba.xw = h->bal_xw;
      cell_blocks = h->n_cu;   // (a row of block partials per block that runs an epilogue)
      if (++h->bal_tag == 0u) h->bal_tag = 1u;
      ba.tag = h->bal_tag;
      ba.timeout_ticks = 50000000ull;   // 0.5 s: every chunk a block waits for was dispatched before it and is made first
      ba.err = reinterpret_cast<unsigned int*>(h->host_dev + 41);
      // stream units per stream block: one (four live waves beside the sweep block's eight) while the stream still ends inside the sweep, else two
      // (measured, 8192 ... 25 000 cells x 5000 genes: one unit per block is 2-4 us per iteration faster at every size, gpurun_out/r5/stair_units.txt;
      //  ride_pattern = 2 asks for two)
      ba.stream_units = h->opt.ride_pattern == 2 ? 2 : 1;
      CACK(launch_fwd_bal_ys(h, cp, ba, ya));
    } else CACK(launch_fwd_cell_mix_ys(h, cp, ya, s2f));
    CACK(ys_finish(h, h->yfin_split && (!is_sharded(h) || p2p_ride_ok(h, h->red_n))));
  } else if (h->fwd_cell && ride) {   // ... and the Y stream's blocks interleaved with the sweep's in the same grid
    cell_blocks = h->ncblk_f;
    ca_yride_args ya;
    memset(&ya, 0, sizeof(ya));
    ya.Y = (const uint8_t*)h->Y; ya.F = h->F; ya.Dstride = h->D; ya.V = h->V; ya.YWpart = h->YWpart; ya.YTpart = h->YTpart;
    ya.G = h->G; ya.Gp = h->Gp; ya.nseg = h->nseg; ya.nrb = h->nrb; ya.TR = h->TR;
    ya.nb_main = h->nrg * h->nseg; ya.nb_y = ya.nb_main;
    ya.ovf = ovf_args(h, h->YWpart + (int64_t)h->nseg * h->N * h->K);
    ya.nb_y += ya.ovf.nb_rows + ya.ovf.nb_chunks;
    CACK(launch_fwd_cell_mix_y(h, cp, ya));
    CACK(launch_yfinish(h, h->nrg, h->nseg));   // the stream's finishers, in line behind the launch they rode on
    h->ycache_valid = true;
  } else if (h->fwd_cell) {   // sweep + cell epilogue in one kernel: no Z partials, one launch
    cell_blocks = h->ncblk_f;
    CACK(launch_fwd_cell(h, cp, s2f));
  } else {
  if (h->fwd_mfma) {
    CACK(launch_fwd_mfma(h, h->Mq, h->Zpart2, h->fsplit, h->fkchunk));
  } else {
    LAUNCH(h, CA_KERNEL_FWD, launch_fwd_fused(h->C, h->D, dim3(cdiv(h->N, CA_TB * kFwdR), h->gsplit), h->stream, h->F, h->etamax2,
                                              h->Vs, h->Mb2, h->Zpart2, h->N, h->G, h->gchunk));
  }
  {
    // (no wait for the side stream here: this epilogue does not touch the Y stream's products -- k_yw_dot does)
    CACK(launch_cell_fused(h, cp));
  }
  }
  // The ELBO assembly (reduction of the cell partials and of k_yw_dot's psi.(YW) partials, then the O(K + C) body) is
  // left pending: it rides on the per-gene kernel of the train pass that completes this look-ahead (train_update), after
  // the single all-reduce of that pass when sharded (train_bwd); ca_run and the odd ends flush it (flush_mon_tail).
  h->mon_tail = small_args(h, h->gene_part, 0, 0.f, elbo_dst, true);
  h->mon_tail.ncblk = cell_blocks;
  if (h->K > 0) { h->mon_tail.yw_part = h->yw_part; h->mon_tail.n_yw = h->n_yw; }
  if (series && h->mon_tail_local) { h->mon_tail.cell_part = nullptr; h->mon_tail.yw_part = nullptr; }   // (sharded series: red[0 .. 3 + C) holds this rank's sums already)
  else h->mon_tail_local = false;
  if (!h->tail_fuse) CACK(flush_mon_tail(h));
  if (cp.ee_partB) {
    // pair sweep (ca_final_elbo): both draws are monitor passes of the same parameters.  ELBO A as usual, then ELBO B from
    // the same red[1 ..] (prior, entropy and sum-gamma terms do not depend on the draw), its own cell sum of the expected
    // log-likelihood and its own per-gene partials.
    CACK(flush_mon_tail(h));
    ca_small_args b = small_args(h, h->gene_partB, 0, 0.f, elbo_dstB, false);
    b.ee_part = h->ee_partB; b.n_ee = cell_blocks;
    if (h->K > 0) { b.yw_part = h->yw_part; b.n_yw = h->n_yw; }
    LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_final_small, dim3(1), dim3(CA_TB), 0, h->stream, b));
    h->look_valid = false;   // no train pass follows: the second draw's coef / d logits are by-products
    return CA_OK;
  }
  h->look_valid = true;
  h->look_slot = s2f ? trainA + 1 : slotB;
  h->bwd_ready = false;
  return CA_OK;
}

// Train pass whose forward half was already done by fused_pass(.., slotB): backward sweep + Adam.
int train_from_lookahead(ca_engine* h, int64_t slot) {
  // (s2: `slot` is the PASS, its two samples are draws 2 slot and 2 slot + 1 and the look-ahead bookkeeping is in draws)
  const int64_t want = h->s2 ? 2 * slot + 1 : slot;
  if (!h->look_valid || h->look_slot != want) { h->err = "internal: no look-ahead forward for this eps slot"; return CA_ERR_STATE; }
  h->look_valid = false;
  const bool have_bwd = h->bwd_ready && h->bwd_slot == want;
  h->bwd_ready = false;
  if (!have_bwd) CACK(train_bwd(h, h->s2 ? h->mu32 : h->mu32B, true));
  return train_update(h, h->eps_dev + slot * (int64_t)h->S * h->G, 1, nullptr);
}

// ca_run: issue the backward half of the NEXT train pass (its forward half came with the monitor pass just queued)
// before the host reads that monitor pass's ELBO, so the read-back and the stop test run beside the sweep instead of
// draining the GPU every iteration.  If the loop stops, the sweep's scratch results are simply never used.
int train_bwd_speculative(ca_engine* h) {
  if (!h->look_valid) return CA_OK;
  CACK(train_bwd(h, h->s2 ? h->mu32 : h->mu32B, true));
  h->bwd_ready = true;
  h->bwd_slot = h->look_slot;
  return CA_OK;
}
// ca_run: the monitor pass's O(K + C) body mirrors its ELBO into pinned host memory and raises a sequence flag
// (ca_small_args::host_*); the host spins on the flag instead of draining a stream, so whatever was queued behind
// the monitor pass (the speculative backward sweep) keeps the GPU busy.  Falls back to a plain read-back when the
// stream runs dry without the flag (mirror unavailable) and surfaces stream errors.
int wait_host_elbo(ca_engine* h, unsigned long long seq, const double* dev, double* out) {
  if (!h->host_dev) return read_doubles(h, dev, out, 1);
  volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(h->host_pinned + 33);
  // (the stream is asked only when the flag is overdue: a hipStreamQuery behind freshly queued work makes the runtime put a
  //  marker packet into the queue, and the update half's first launch then started 5.8 us late in EVERY iteration of ca_run --
  //  the "unexplained gap" of round 1; host API trace in profiles/r02_ab_ystream.txt section 7)
  unsigned spins = 0;
  auto t_next = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
  while (*flag != seq) {
    if ((++spins & 0x3FFu) == 0 && std::chrono::steady_clock::now() >= t_next) {
      t_next = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) {
        if (*flag == seq) break;
        return read_doubles(h, dev, out, 1);
      }
      if (q != hipErrorNotReady) HIPCK(h, q);
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  *out = *reinterpret_cast<volatile double*>(h->host_pinned + 32);
  return comm_check(h);
}

// monitor pass on eps slot m; with next >= 0 (and the fused path available) also the forward half of the train
// pass on slot `next`, which train_pass() then completes
int monitor_pass(ca_engine* h, int64_t m, int64_t next, double* elbo_dst) {
  if (h->fused_ok && h->s2) {   // mc_samples = 2: the pass's two samples in the two column halves
    // ... and the next train pass's two samples in a second operand set of the same sweep (round 4), or the sweep alone
    if (h->s2f && next >= 0 && next != m) return fused_pass(h, 2 * m, 2 * m + 1, elbo_dst, nullptr, 2 * next);
    CACK(fused_pass(h, 2 * m, 2 * m + 1, elbo_dst));
    h->look_valid = false;
    return CA_OK;
  }
  if (h->fused_ok && next >= 0) return fused_pass(h, m, next, elbo_dst);
  if (h->fused_ok && h->c16) {   // (9..16 clones have no plain matrix-core pass: the fused sweep with this draw in both roles)
    CACK(fused_pass(h, m, m, elbo_dst));
    h->look_valid = false;
    return CA_OK;
  }
  return run_pass(h, m, CA_MODE_ELBO, 0, elbo_dst);
}
int train_pass(ca_engine* h, int64_t slot) {
  if (h->look_valid && h->look_slot == (h->s2 ? 2 * slot + 1 : slot)) return train_from_lookahead(h, slot);
  if (h->fused_ok && (h->c16 || h->s2) && (h->bwd_mfma || !is_sharded(h))) {   // its forward half: the same sweep with this pass's draw(s)
    if (h->c16) CACK(flush_mon_tail(h));   // (9..16 clones: a pending tail is a real monitor pass's)
    h->mon_tail.enabled = 0;   // (mc_samples = 2: a tail still pending belongs to a ca_iterate pass whose ELBO nobody reads; ca_run has flushed its own)
    CACK(h->s2 ? fused_pass(h, 2 * slot, 2 * slot + 1, h->terms_dev + 3) : fused_pass(h, slot, slot, h->terms_dev + 3));   // (the monitor role's ELBO is scratch)
    return train_from_lookahead(h, slot);
  }
  return run_pass(h, slot, CA_MODE_TRAIN, 1, nullptr);
}

int ensure_eps_cap(ca_engine* h, int64_t draws) {
  if (draws <= h->eps_cap) return CA_OK;
  float* p = nullptr;
  HIPCK(h, hipMalloc((void**)&p, (size_t)draws * h->S * h->G * sizeof(float)));
  if (h->eps_dev) {
    SYNC(h);
    HIPCK(h, hipFree(h->eps_dev));
    h->dev_bytes -= h->eps_cap * (int64_t)h->S * h->G * 4;
  }
  h->eps_dev = p;
  h->eps_cap = draws;
  h->dev_bytes += draws * (int64_t)h->S * h->G * 4;
  return CA_OK;
}
int ensure_elbo_cap(ca_engine* h, int64_t n) {
  if (n <= h->elbo_cap) return CA_OK;
  double* p = nullptr;
  HIPCK(h, hipMalloc((void**)&p, (size_t)n * sizeof(double)));
  if (h->elbo_dev) {
    SYNC(h);
    HIPCK(h, hipFree(h->elbo_dev));
  }
  h->elbo_dev = p;
  h->elbo_cap = n;
  return CA_OK;
}

// The pinned staging buffer of the eps stream, at least `bytes` long and free to be refilled: the copy that last read it has completed BEFORE it is freed,
// regrown or written.
int stage_reserve(ca_engine* h, size_t bytes) {
  if (h->ev_stage) HIPCK(h, hipEventSynchronize(h->ev_stage));
  if (bytes > h->eps_stage_bytes) {
    if (h->eps_stage) HIPCK(h, hipHostFree(h->eps_stage));
    h->eps_stage = nullptr; h->eps_stage_bytes = 0;
    HIPCK(h, hipHostMalloc((void**)&h->eps_stage, bytes));
    h->eps_stage_bytes = bytes;
  }
  return CA_OK;
}
// put `n_draws` draws on the device: from the caller's stream, or generated (built-in Philox stream)
int stage_eps(ca_engine* h, const float* eps_stream, int64_t have, int64_t need) {
  const int64_t per = (int64_t)h->S * h->G;
  h->look_valid = false;   // the staged eps slots are about to change
  h->gaux_slot = -1;
  CACK(ensure_eps_cap(h, std::max<int64_t>(need, 1)));
  const size_t bytes = (size_t)need * per * sizeof(float);
  if (eps_stream) {
    if (have < need) {
      h->err = "eps stream too short: need " + std::to_string(need) + " draws, got " + std::to_string(have);
      return CA_ERR_INVALID;
    }
    // Through the engine's pinned staging buffer, stream-ordered, WITHOUT draining the stream: a copy from the caller's pageable
    // memory followed by a synchronisation left the GPU idle for ~250 us at the start of every call (kernel trace of the
    // driver's 20-step command: 4 % of its time).
    CACK(stage_reserve(h, bytes));
    memcpy(h->eps_stage, eps_stream, bytes);
  } else {
    // counter-based stream: draws are independent, so a long run's worth (2 + 2 max_iter draws) is generated by several
    // host threads -- same values whatever the thread count -- straight into a pinned staging buffer the engine keeps
    // (pageable memory cost 1.5 ms of copy for 8 MB; with 16 threads the 402 draws of a default fit took 3.3 ms in all)
    CACK(stage_reserve(h, bytes));
    float* out = h->eps_stage;
    const int64_t nt = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(need / 4, 48), (int64_t)std::thread::hardware_concurrency() / 2));
    if (nt > 1 && need * per >= (1 << 16)) {
      std::vector<std::thread> pool;
      const uint64_t seed = h->opt.seed, base = h->draw;
      for (int64_t t = 0; t < nt; ++t)
        pool.emplace_back([=]() { for (int64_t d = t; d < need; d += nt) ca_philox::normal_draw(seed, base + d, per, out + d * per); });
      for (auto& th : pool) th.join();
    } else {
      for (int64_t d = 0; d < need; ++d) ca_philox::normal_draw(h->opt.seed, h->draw + d, per, out + d * per);
    }
    h->draw += need;
  }
  // the copy, and behind it the event the next call waits for before it touches the buffer
  HIPCK(h, hipMemcpyAsync(h->eps_dev, h->eps_stage, bytes, hipMemcpyHostToDevice, h->stream));
  if (!h->ev_stage) HIPCK(h, hipEventCreateWithFlags(&h->ev_stage, hipEventDisableTiming));
  HIPCK(h, hipEventRecord(h->ev_stage, h->stream));
  return CA_OK;
}
