// ca_eng_create.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): create_impl: buffers, decomposition picks (every threshold measured: DESIGN.md section 5), setup sums; find_param.

// ---- CA_VAR_MOM_LAST: where the moment role of the count-matrix stream's launch goes (ca_polymom.hip.h) -- pure functions of numbers the engine has ------------
// In front of the stream's blocks the role's nmb + nred blocks take slots first, and as many stream blocks as the grid then exceeds one round of slots by start only
// when a block of the role leaves: the launch ends that much later (3.75 us at cfg-3, profiles/r14_mom_last_before.txt).  Behind the stream's blocks every stream
// block is resident from the start and the role runs in the slots the stream leaves free.  What that is worth is set by the role's own chain of memory latencies,
// which beside the stream's traffic runs several times slower than on an empty device (profiles/r14_mom_last_ab.txt):
//   * the role's shape behind the stream: as many gene groups per moment block as make the moment blocks fit ONE round of the free slots of every XCD (blocks are
//     dealt round-robin over the XCDs) -- a block then scans V and max|psi| once for its groups, where several rounds of one-group blocks scan them once per block --
//     and twice the reducers, which cost no stream block a slot there.  At cfg-3 (44 free slots, 5 per XCD): 4 groups per block, 40 blocks, 42 reducers.  Measured
//     at cfg-3 against one group and 21 reducers behind the stream: 4 groups -1.6 us, 42 reducers -1.0 us, both -2.8 us per iteration; 2 groups +1.3 us.
//   * the order is kept as it was (false) where nothing would be displaced (the stream's blocks and the role fit one round of slots together: the orders are
//     equivalent), where an XCD would have no free slot beside its stream blocks, where one round would need more than CA_ML_MAX_PER groups per block, and where the
//     stream's estimated time is below CA_ML_MIN_STREAM_US: the role's chain in that shape ends about as late as a 52 us stream (cfg-3: the launch 1.5 - 2 us
//     longer than the stream alone instead of 3.75), and later than a shorter one -- behind a 29 us stream (50k x 5k) it is level with the order in front or slower,
//     behind an 18 us stream (25k x 5k) 4 - 9 us slower.
// The stream's time from its stored bytes: fixed + bytes / rate, fitted to k_ys_mfma_ovf<true> alone at 25k / 50k / 100k x 5k (17.66 / 29.42 / 52.20 us).
constexpr double CA_ML_STREAM_FIXED_US = 6.6;
constexpr double CA_ML_STREAM_BYTES_PER_US = 5.62e6;
constexpr double CA_ML_MIN_STREAM_US = 45.0;   // between the 29.4 us stream where the order does not pay and the 52.2 us stream where it does
constexpr int CA_ML_MAX_PER = 4;               // the most gene groups per moment block that was measured
struct ca_mom_last_in {
  int slots;            // resident blocks of this kernel with its dynamic LDS: occupancy x n_cu, asked of the runtime
  int n_cu;             // XCDs = n_cu / 32 on this part
  int nb_stream, nb_ovf;   // the stream's blocks; the overflow list's (behind the role: they take no slot from it and do not enter the pick)
  int ngrp, nred;       // gene groups (32 genes each); reducer blocks with the role in front
  int64_t image_bytes;  // stored image bytes the launch reads
};
inline int ca_mom_last_free(const ca_mom_last_in& a) { return std::max(a.slots - a.nb_stream, 0); }
inline int ca_mom_last_free_x(const ca_mom_last_in& a) {   // free slots of the XCD with the most stream blocks
  const int xcd = std::max(a.n_cu / 32, 1);
  return a.slots / xcd - cdiv(a.nb_stream, xcd);
}
// gene groups per moment block behind the stream: the fewest with which every XCD's moment blocks fit its free slots at once (0: no XCD-wide free slot)
inline int ca_mom_last_per(const ca_mom_last_in& a) {
  const int xcd = std::max(a.n_cu / 32, 1), free_x = ca_mom_last_free_x(a);
  if (free_x < 1) return 0;
  return std::max(1, cdiv(a.ngrp, free_x * xcd));
}
inline bool ca_mom_last_pick(const ca_mom_last_in& a) {
  if (a.nb_stream + a.ngrp + a.nred <= a.slots) return false;
  const int per = ca_mom_last_per(a);
  if (per < 1 || per > CA_ML_MAX_PER) return false;
  return CA_ML_STREAM_FIXED_US + (double)a.image_bytes / CA_ML_STREAM_BYTES_PER_US >= CA_ML_MIN_STREAM_US;
}

// ---- CA_VAR_Y2: the host's share of the 2-bit / 4-bit image (ca_ymfma.hip.h) -- a pure function of the per-gene counts k_y2_hist leaves (ca_y2_plan in the C ABI) --------
// Per 512-gene segment the genes sorted by their stored counts >= 3, ascending, ties by gene index (padded genes count 0); the list of N2 narrow blocks holds the
// counts >= 3 of the genes in them and the counts >= 15 of the others.  N2 without force: the larger of 6 and 5 (the values the stream is instantiated for) whose
// list is at most 1 in 256 of the matrix's counts -- the 4-bit image's budget --, else 0.
constexpr int CA_Y2_NS[2] = {6, 5};
// the matrix size (padded counts N64 x Gp) from which the image is picked: between 25k x 5k (1.28e8), where the forced image gains 1.5 us per iteration of 64 -- about
// the spread of a run --, and 50k x 5k (2.56e8), where it gains 4.5 of 81; 100k x 5k gains 8.8 of 109.7 (profiles/r18_y2_ab.txt)
constexpr double CA_Y2_MIN_COUNTS = 2.0e8;
inline int ca_y2_plan_impl(const int32_t* cnt3, const int32_t* cnt15, int Gp, int64_t counts, int force_n2, uint16_t* perm, uint16_t* pos, int64_t* n_esc) {
  const int nseg = Gp / CA_YS_GW;
  int64_t e15 = 0, e3[CA_YS_GW / 64 + 1];   // e3[b]: what the list grows by when blocks 0 .. b-1 are narrow
  for (int b = 0; b <= CA_YS_GW / 64; ++b) e3[b] = 0;
  std::vector<int> idx(CA_YS_GW);
  for (int s = 0; s < nseg; ++s) {
    const int32_t* c3 = cnt3 + (size_t)s * CA_YS_GW;
    const int32_t* c15 = cnt15 + (size_t)s * CA_YS_GW;
    for (int i = 0; i < CA_YS_GW; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return c3[a] < c3[b]; });
    for (int i = 0; i < CA_YS_GW; ++i) {
      perm[(size_t)s * CA_YS_GW + i] = (uint16_t)idx[i];
      pos[(size_t)s * CA_YS_GW + idx[i]] = (uint16_t)i;
      e15 += c15[idx[i]];
      e3[i / 64 + 1] += (int64_t)c3[idx[i]] - c15[idx[i]];
    }
  }
  for (int b = 1; b <= CA_YS_GW / 64; ++b) e3[b] += e3[b - 1];
  int n2 = 0;
  if (force_n2 > 0) n2 = force_n2 < CA_YS_GW / 64 ? force_n2 : CA_YS_GW / 64 - 1;
  else
    for (int k = 0; k < 2 && n2 == 0; ++k)
      if ((e15 + e3[CA_Y2_NS[k]]) * 256 <= counts) n2 = CA_Y2_NS[k];
  *n_esc = e15 + e3[n2];
  return n2;
}

int create_impl(ca_engine* h, const ca_problem* p) {
  const int N = (int)h->N; (void)N;
  HIPCK(h, hipSetDevice(h->device));
  hipDeviceProp_t prop;
  HIPCK(h, hipGetDeviceProperties(&prop, h->device));
  h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIPCK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  // (a low-priority side stream, or s_setprio 3 in the sweep, only moves the Y stream's time out from under the sweep:
  //  measured 2090 -> 2100 and 2090 -> 1730 it/s; the cell epilogue waits for it either way)
  HIPCK(h, hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
  HIPCK(h, hipEventCreateWithFlags(&h->ev_params, hipEventDisableTiming));
  HIPCK(h, hipEventCreateWithFlags(&h->ev_ydone, hipEventDisableTiming));
  {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
    if (hipStreamCreateWithPriority(&h->stream3, hipStreamNonBlocking, hi) != hipSuccess) { (void)hipGetLastError(); h->stream3 = nullptr; }
  }
  HIPCK(h, hipEventCreateWithFlags(&h->ev_poly0, hipEventDisableTiming));
  HIPCK(h, hipEventCreateWithFlags(&h->ev_poly1, hipEventDisableTiming));
  HIPCK(h, hipEventCreateWithFlags(&h->ev_ywdone, hipEventDisableTiming));
  // side stream for the count-matrix products: pays from ~4e7 counts up (12.5k x 5k: 9543 it/s against 9207 in line;
  // 10k x 2k: 10917 against 13017 -- two cross-stream events per iteration cost more than the overlap returns)
  h->async_y = variant_on(h, CA_VAR_ASYNC_Y, "CA_ASYNC_Y") &&
               ((double)h->N * (double)h->G >= 4e7 || variantx_on(h, CA_VARX_ASYNC_SMALL, "CA_ASYNC_SMALL"));
  HIPCK(h, hipHostMalloc((void**)&h->host_pinned, 64 * sizeof(double)));
  memset(h->host_pinned, 0, 64 * sizeof(double));
  if (hipHostGetDevicePointer((void**)&h->host_dev, h->host_pinned, 0) != hipSuccess) { h->host_dev = nullptr; (void)hipGetLastError(); }
  h->mon_tail = no_small_args();
  h->tail_fuse = variant_on(h, CA_VAR_TAIL_FUSE, "CA_TAIL_FUSE");
  h->pre_ok = variant_on(h, CA_VAR_PRE, "CA_PRE");
  h->upd_merge = h->tail_fuse && h->pre_ok && variant_on(h, CA_VAR_UPDATE_MERGE, "CA_UPDATE_MERGE");
  h->p2p_ride = h->tail_fuse && variant_on(h, CA_VAR_P2P_RIDE, "CA_P2P_RIDE");
  h->run_gate = h->upd_merge && variant_on(h, CA_VAR_RUN_GATE, "CA_RUN_GATE");
  {   // the device's wall clock (s_memrealtime) in ticks per microsecond, asked of the runtime instead of assumed (ADVICE r5)
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) == hipSuccess && khz >= 1000) h->ticks_per_us = (double)khz / 1000.0;
    else (void)hipGetLastError();
  }
  h->gate_ticks = (unsigned long long)(h->ticks_per_us * (double)(h->opt.gate_timeout_us > 0 ? h->opt.gate_timeout_us : 1000));
  h->run_fwd = h->run_gate && variantx_on(h, CA_VARX_RUN_FWD, "CA_RUN_FWD");   // opt-in: see the header (no runtime call may block between a gated launch and its answer)
  h->pair_elbo = variant_on(h, CA_VAR_PAIR_ELBO, "CA_PAIR_ELBO");
  CACK(h->sp_in ? upload_y_sparse(h, p, h->sp_in) : upload_y(h, p));
  const int G = h->G, C = h->C, K = h->K, P = h->P, S = h->S, D = h->D;
  const int64_t Nn = h->N;
  h->nchunk = cdiv(C, CA_CW);
  h->ngblk = cdiv(G, CA_TB);
  {
    int CP = 1;
    while (CP < C) CP <<= 1;
    h->ncblk = (C <= 64) ? std::min(cdiv(Nn, CA_TB / CP), 16 * 256) : cdiv(Nn, CA_TB);   // k_cell_par: grid-stride over groups of CA_TB / CP cells
  }
  // ---- sweep decomposition
  const int target_blocks = 8 * h->n_cu;
  // one full round of resident blocks (8 x 256 threads per CU) when the cell blocks alone do not fill the chip
  const int nfb = cdiv(Nn, CA_TB * kFwdR);
  // enough blocks for ~one resident round, but never more than 16 gene slices: every slice adds an N x 16 float
  // partial that the cell epilogue has to read back (at 12.5k cells 78 slices cost 2x the sweep itself)
  h->gsplit = std::max(1, std::min(std::min(target_blocks / std::max(nfb, 1), 16), std::max(1, G / 64)));
  h->gsplit = std::max(h->gsplit, cdiv(G, 1024));      // LDS slice: at most 1024 genes x (8 + D) floats = 64 KB
  if (const int t = tune_val(h, CA_TUNE_GSPLIT, "CA_GSPLIT")) h->gsplit = std::max(std::max(1, t), cdiv(G, 1024));   // tuning override
  h->gchunk = cdiv(G, h->gsplit);
  h->gsplit = cdiv(G, h->gchunk);
  // genes per lane of the backward sweep: more genes amortise the per-cell wave reduction (tools/bwd_lab2.hip)
  h->RG = G >= 1024 ? 4 : 1;   // RG = 8 measured equal in the engine (272 vs 276 us): kept selectable, not default
  if (const int r = tune_val(h, CA_TUNE_RG, "CA_RG")) { if (r == 1 || r == 4 || r == 8) h->RG = r; }
  h->ntile = cdiv(G, 64 * h->RG);
  const int gblocks = cdiv(h->ntile, CA_TB / 64);
  h->csplit = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(target_blocks, gblocks), std::max<int64_t>(1, Nn / 64)));
  if (const int t = tune_val(h, CA_TUNE_CSPLIT, "CA_CSPLIT")) h->csplit = std::max(1, t);   // tuning override
  h->cchunk = (Nn + h->csplit - 1) / h->csplit;
  h->csplit = cdiv(Nn, h->cchunk);
  h->TR = 128;
  const int tr_set = tune_val(h, CA_TUNE_TR, "CA_TR");
  if (tr_set) h->TR = std::min(128, std::max(1, tr_set));   // tuning override (k_ypass keeps psi of <= 128 rows)
  h->nrb = cdiv(Nn, h->TR);
  while (!tr_set && (int64_t)h->nrb * h->nseg < 4 * h->n_cu && h->TR > 32) { h->TR /= 2; h->nrb = cdiv(Nn, h->TR); }
  h->nrg = cdiv(h->nrb, CA_TB / 64);
  // ---- constants
  std::vector<double> Lrm((size_t)G * C), logL((size_t)G * C);
  std::vector<float> Lb((size_t)(h->nchunk + (h->nchunk & 1)) * G * CA_CW, 0.f);   // (an odd number of clone chunks: a chunk of zeros completes the last pair)
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < C; ++c) {
      const double v = p->L[hidx(p->layout, g, c, G, C)];
      Lrm[(size_t)g * C + c] = v;
      logL[(size_t)g * C + c] = std::log(v);
      Lb[((size_t)(c / CA_CW) * G + g) * CA_CW + (c % CA_CW)] = (float)v;
    }
  CACK(dalloc(h, &h->Lb, (int64_t)Lb.size()));
  CACK(upload_f(h, h->Lb, Lb));
  double* logL_dev = nullptr; double* extra_dev = nullptr;
  HIPCK(h, hipMalloc((void**)&logL_dev, logL.size() * sizeof(double)));
  HIPCK(h, hipMemcpy(logL_dev, logL.data(), logL.size() * sizeof(double), hipMemcpyHostToDevice));
  if (p->extra_loglik) {
    std::vector<double> ex((size_t)Nn * C);
    for (int64_t n = 0; n < Nn; ++n)
      for (int c = 0; c < C; ++c) ex[(size_t)n * C + c] = p->extra_loglik[hidx(p->layout, n, c, Nn, C)];
    HIPCK(h, hipMalloc((void**)&extra_dev, ex.size() * sizeof(double)));
    HIPCK(h, hipMemcpy(extra_dev, ex.data(), ex.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  CACK(dalloc(h, &h->A, Nn * C));
  CACK(dalloc(h, &h->cn, Nn));
  CACK(dalloc(h, &h->s64, Nn));
  CACK(dalloc(h, &h->s32, Nn));
  CACK(dalloc(h, &h->colsum, G));
  if (h->ystore == CA_YSTORE_U8) launch_prep<uint8_t>(h, logL_dev, extra_dev);
  else if (h->ystore == CA_YSTORE_U16) launch_prep<uint16_t>(h, logL_dev, extra_dev);
  else launch_prep<float>(h, logL_dev, extra_dev);
  HIPCK(h, hipGetLastError());
  SYNC(h);
  hipFree(logL_dev);
  if (extra_dev) hipFree(extra_dev);
  // ---- variables (:240-272)
  // matrix-core backward sweep: D = K + P from 1 to 4 (eta is D multiply-adds on the vector unit, the matrix-core products do not depend on D; three and four
  // latent dimensions + covariates take the three-tile wave -- their per-gene accumulators grow with D -- in the main form only: up to eight clones, one
  // sample per sweep), one clone chunk or the C16 form
  {
    bool exact = true;
    for (double v : Lrm) {
      const float f = (float)v;
      uint32_t u; memcpy(&u, &f, 4);
      if ((double)f != v || (u & 0xFFFFu) != 0) { exact = false; break; }
    }
    h->bwd_frac = !exact;   // copy numbers that are not bf16-exact: the sweep's two-part form (k_bwd_mfma<.., FRAC>)
    // 9..16 clones (two clone chunks): the sweep's C16 form, integer copy numbers only (fractional ones would need 48 operand slots)
    // 17..32 clones, or 9..16 with mc_samples >= 2 (round 6): the same form once per pair of clone chunks and sample, accumulating (bwd_pairs, set below)
    h->bwd_mfma = (D == 1 || D == 2 || ((D == 3 || D == 4) && h->nchunk == 1)) && (h->nchunk == 1 || (h->nchunk <= 4 && exact)) &&
                  variant_on(h, CA_VAR_BWD_MFMA, "CA_BWD_MFMA");
    h->N16 = (Nn + 15) / 16 * 16;
    if (h->bwd_mfma) {
      // Gene tiles per wave.  Four amortise the coef operand best (cfg-3: 111.6 us against 122.5 with three, although three fit four waves per SIMD);
      // a small problem has too few wave jobs at four (cfg-2: 32 of them, eight blocks across) and gains from three: cfg-2 39.3 -> 37.5 us per
      // iteration, 12.5k x 5k 63.7 -> 62.6; 25k cells 91.2 -> 95.1 (profiles/r05_small_shapes.txt section 9).  Main variant only.
      h->bwd_tl = (Nn <= CA_BWD_TL3_MAXN && !h->c16 && exact && S == 1 && h->nchunk == 1 && variant_on(h, CA_VAR_BWD_TL3, "CA_BWD_TL3")) ? 3 : CA_BWD_TL;
      if (D >= 3) h->bwd_tl = CA_BWD_TL_D34;
      h->nwt = cdiv(G, h->bwd_tl * 16);
      const int xb = cdiv(h->nwt, CA_TB / 64);
      {
        // resident blocks per CU from the compiler's register count (LDS, 16 B per cell of the slice, is not the limit
        // at the slice lengths this produces); one or two full rounds instead of "about 8 blocks per CU"
        int per_cu = 4;
        const void* bfn = D == 4 ? (const void*)k_bwd_mfma<CA_BWD_TL_D34, 4, false> : D == 3 ? (const void*)k_bwd_mfma<CA_BWD_TL_D34, 3, false>
                        : h->bwd_tl == 3 ? (D == 1 ? (const void*)k_bwd_mfma<3, 1, false> : (const void*)k_bwd_mfma<3, 2, false>)
                                         : (D == 1 ? (const void*)k_bwd_mfma<CA_BWD_TL, 1, false> : (const void*)k_bwd_mfma<CA_BWD_TL, 2, false>);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bfn, CA_TB, 16 * 1024) != hipSuccess || per_cu < 1)
          per_cu = 4;
        (void)hipGetLastError();
        const int smax = (int)std::max<int64_t>(1, std::min<int64_t>(Nn / 256, cdiv(2 * (int64_t)per_cu * h->n_cu, xb)));
        h->csplit_m = pick_split(xb, (int64_t)per_cu * h->n_cu, smax, 1e-4);
      }
      if (const int t = tune_val(h, CA_TUNE_CSPLIT_M, "CA_CSPLIT_M")) h->csplit_m = std::max(1, t);
      // mc_samples = 2: the two-sample sweep keeps a second set of d/dF slices in LDS; where that would leave fewer than three blocks per CU
      // (more than 48 KB a block) the cell slices are halved -- two whole rounds where there was one -- with or without the variant
      if (S == 2 && (int64_t)2 * 4 * (((Nn + h->csplit_m - 1) / h->csplit_m + 15) / 16 * 16) * D * 4 > 48 * 1024) h->csplit_m *= 2;
      h->csplit_m = (int)std::max<int64_t>(h->csplit_m, (Nn * D * (S == 2 ? 2 : 1) + 4079) / 4080);   // LDS: [samples x] 4 waves x cchunk x D floats <= 64 KB
      h->cchunk_m = ((Nn + h->csplit_m - 1) / h->csplit_m + 15) / 16 * 16;
      h->csplit_m = cdiv(Nn, h->cchunk_m);
      // fold the column sums of the sweep's partials into the per-gene kernel: a launch and its gap less.  Up to 32k cells in round 2
      // (the fold's loads went out eight at a time, one column after the other: slower than the k_colsum launch above that);
      // with both columns from one load and twenty slices in flight it is level or ahead wherever the slice count is the one
      // resident round (cfg-3 +0.3 %, 50k cells +0.6 %, 200k +0.2 %); long shards with many more slices keep the launch
      h->fold_gsum = (Nn <= 32768 || (h->csplit_m <= 64 && S + D == 2) || variantx_on(h, CA_VARX_FOLD_ALWAYS, "CA_FOLD_ALWAYS")) && S + D <= 12 && h->tail_fuse &&
                     variant_on(h, CA_VAR_FOLD_GSUM, "CA_FOLD_GSUM");
      // (zero-filled: the slots of a missing last chunk stay zero; two or more clone chunks: a second image of the same size behind the first for the third part)
      CACK(dalloc(h, &h->coefq, (int64_t)S * cdiv(h->nchunk, 2) * h->N16 * 32 * (h->nchunk >= 2 ? 2 : 1)));
    }
  }
  CACK(dalloc(h, &h->F, h->N16 * std::max(D, 1)));
  CACK(dalloc(h, &h->m_psi, Nn * std::max(K, 1)));
  CACK(dalloc(h, &h->v_psi, Nn * std::max(K, 1)));
  CACK(dalloc(h, &h->g_psi, Nn * std::max(K, 1)));
  CACK(dalloc(h, &h->glogit, Nn * C));
  CACK(dalloc(h, &h->m_gl, Nn * C));
  CACK(dalloc(h, &h->v_gl, Nn * C));
  CACK(dalloc(h, &h->dgl, Nn * C));
  CACK(dalloc(h, &h->V, (int64_t)G * std::max(D, 1)));
  CACK(dalloc(h, &h->m_V, (int64_t)G * std::max(D, 1)));
  CACK(dalloc(h, &h->v_V, (int64_t)G * std::max(D, 1)));
  CACK(dalloc(h, &h->g_V, (int64_t)G * std::max(D, 1)));
  CACK(dalloc(h, &h->Vs, (int64_t)cdiv(G, 32) * 32 * std::max(D, 1)));   // padded to whole 32-gene k-steps (last gene replicated)
  CACK(dalloc(h, &h->loc, G)); CACK(dalloc(h, &h->ls, G));
  CACK(dalloc(h, &h->m_loc, G)); CACK(dalloc(h, &h->v_loc, G));
  CACK(dalloc(h, &h->m_ls, G)); CACK(dalloc(h, &h->v_ls, G));
  CACK(dalloc(h, &h->g_loc, G)); CACK(dalloc(h, &h->g_ls, G));
  CACK(dalloc(h, &h->vchi, std::max(K, 1))); CACK(dalloc(h, &h->m_v, std::max(K, 1))); CACK(dalloc(h, &h->v_v, std::max(K, 1)));
  CACK(dalloc(h, &h->g_v, std::max(K, 1)));
  CACK(dalloc(h, &h->alpha_u, C)); CACK(dalloc(h, &h->m_a, C)); CACK(dalloc(h, &h->v_a, C)); CACK(dalloc(h, &h->g_a, C));
  CACK(dalloc(h, &h->vchi_alt, std::max(K, 1))); CACK(dalloc(h, &h->alpha_u_alt, C));
  CACK(dalloc(h, &h->vmm_at, 32));
  CACK(dalloc(h, &h->gate_local, 2));
  CACK(dalloc(h, &h->gaux, (int64_t)2 * 5 * G));
  {
    std::vector<float> Fh((size_t)Nn * std::max(D, 1), 0.f);
    if (D > 0) {
      for (int64_t n = 0; n < Nn; ++n) {
        for (int k = 0; k < K; ++k) Fh[(size_t)n * D + k] = (float)p->psi0[hidx(p->layout, n, k, Nn, K)];
        for (int q = 0; q < P; ++q) Fh[(size_t)n * D + K + q] = (float)p->X[hidx(p->layout, n, q, Nn, P)];
      }
    }
    CACK(upload_f(h, h->F, Fh));
    std::vector<float> l0((size_t)G);
    if (p->loc0)   // else: filled below from the data (device form of mu_guess, R/inference-tflow.R:220-235)
      for (int g = 0; g < G; ++g) l0[g] = (float)p->loc0[g];
    CACK(upload_f(h, h->loc, l0));
  }
  // ---- pass buffers
  CACK(dalloc(h, &h->mu32, (int64_t)S * G));
  CACK(dalloc(h, &h->Mb, (int64_t)S * h->nchunk * G * CA_CW));
  // 9..16 clones (c16): the fused machinery with ONE draw per sweep in all sixteen operand columns -- only in its default form
  // (matrix-core sweeps, sweep + cell epilogue in one kernel); otherwise such problems take the plain passes as before
  h->c16 = S == 1 && C > CA_CW && C <= 2 * CA_CW && (D == 1 || D == 2) && h->bwd_mfma && h->tail_fuse &&
           variant_on(h, CA_VAR_FWD_MFMA, "CA_FWD_MFMA") && variant_on(h, CA_VAR_FWD_CELL, "CA_FWD_CELL");
  // mc_samples = 2 (s2): the two column halves carry the two SAMPLES of one pass; same conditions, up to eight clones
  h->s2 = S == 2 && C <= CA_CW && (D == 1 || D == 2) && h->bwd_mfma && h->tail_fuse &&
          variant_on(h, CA_VAR_FWD_MFMA, "CA_FWD_MFMA") && variant_on(h, CA_VAR_FWD_CELL, "CA_FWD_CELL");
  h->fused_ok = ((S == 1 && (C <= CA_CW || h->c16)) || h->s2) && variant_on(h, CA_VAR_FUSED, "CA_FUSED");
  if (!h->fused_ok) { h->c16 = false; h->s2 = false; }
  if (h->nchunk >= 2 && !h->c16) {
    // (with the fused loop switched off by hand the plain passes stay what they were: vector sweeps both ways)
    if (h->bwd_mfma && S * h->nchunk >= 3 && variant_on(h, CA_VAR_FUSED, "CA_FUSED")) h->bwd_pairs = cdiv(h->nchunk, 2);
    else h->bwd_mfma = false;
  }
  // plain passes with their forward contraction on the matrix cores: shapes the fused loop does not take (not: the fused loop switched off by hand)
  h->pfwd = !h->fused_ok && S * h->nchunk >= 3 && (D == 1 || D == 2) && C <= 64 && variant_on(h, CA_VAR_FUSED, "CA_FUSED") && variant_on(h, CA_VAR_FWD_MFMA, "CA_FWD_MFMA");
  if (h->pfwd) {
    h->pf_npair = cdiv(S * h->nchunk, 2);
    h->nk32 = cdiv(G, 32);
    const int cblocks = cdiv(Nn, (CA_TB / 64) * CA_FM_TL * 16);
    int per_cu = 4;
    const void* fn = (D == 1) ? (const void*)k_fwd_mfma<1> : (const void*)k_fwd_mfma<2>;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, CA_TB, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    (void)hipGetLastError();
    h->pf_fsplit = pick_split(cblocks, (int64_t)per_cu * h->n_cu, std::max(1, std::min(16, h->nk32 / CA_FM_KC)), 0.02);
    h->pf_kchunk = cdiv(h->nk32, h->pf_fsplit);
    h->pf_fsplit = cdiv(h->nk32, h->pf_kchunk);
    CACK(dalloc(h, &h->pf_Mq, (int64_t)h->pf_npair * h->nk32 * 1024));   // zero-filled: padding genes, missing columns and a missing last slice stay 0
    CACK(dalloc(h, &h->pf_Z, (int64_t)h->pf_npair * h->pf_fsplit * Nn * 16));
  }
  if (h->s2) h->pair_elbo = false;   // (two draws per sweep need two column halves of their own)
  if (h->fused_ok) {
    h->frow = (2 * C <= 8) ? 8 : 16;
    // matrix-core forward sweep: D = K + P in {1, 2} in every form; D in {3, 4} (round 6) as the sweep + cell epilogue kernel in its two default block shapes,
    // beside the matrix-core backward sweep.  The count-matrix stream then runs as a launch of its own, in line: riding on the D = 3 sweep (160-190 registers a
    // wave) the int8 stream's blocks wait for whole sweep blocks to retire -- measured 514 us for the merged launch against 140 + 96 apart (100k x 5k x 8, K = 1, P = 2)
    const bool d34 = (D == 3 || D == 4) && S == 1 && C <= CA_CW && h->bwd_mfma && h->tail_fuse && variant_on(h, CA_VAR_FWD_CELL, "CA_FWD_CELL");
    h->fwd_mfma = (D == 1 || D == 2 || d34) && variant_on(h, CA_VAR_FWD_MFMA, "CA_FWD_MFMA");
    h->fwd_cell = h->fwd_mfma && h->tail_fuse && variant_on(h, CA_VAR_FWD_CELL, "CA_FWD_CELL");
    {
      // cells per block of k_fwd_cell: 16 * TL -- measured, not derived.  96-cell blocks (fewest re-reads of the B operand
      // from L2) as soon as there is one full round of them, the launch then carries a second, 32-cell block size for the
      // cells that do not fill a whole round (k_fwd_cell_mix, below).  With that, TL = 6 is best or within 1 % of the best of
      // {4, 5, 6} from 35k to 400k cells (35k: 6310 / 6207 / 6046 it/s for 6 / 5 / 4; 50k: 5012 / 4916 / 4951; 70k: 3499 /
      // 3459 / 3523; 100k: 2691 / 2594 / 2625); 128-cell blocks never won (200k: 1346 vs 1363, 400k: 609 vs 638 it/s).
      // Small shards: 32-cell blocks, or CUs are left with one block or none (25k: 7619 / 7443 / 6701 for TL = 2 / 4 / 6
      // without the second block size, 7535 for 6 with it).
      // (16-cell blocks, fc_tl = 1, were tried for shards below 16k cells -- twice the waves per SIMD -- and lost: 12.5k cells
      //  39 us against 35, every block re-reads the B operand)
      h->fc_tl = (h->fwd_cell && cdiv(Nn, 64) < 2 * h->n_cu) ? 2 : 6;
      // fewer 32-cell blocks than CUs: 16-cell blocks, where the int8 stream rides (round 3, with this round's kernels: 6250 cells
      // 17.2k -> 18.8k it/s; at 12.5k cells and at 10k x 2k they still lose, 13.7k vs 14.2k and 21.7k vs 22.1k)
      if (h->fwd_cell && h->fc_tl == 2 && cdiv(Nn, 32) < h->n_cu && h->ystore == CA_YSTORE_U8 && K == 1 && D <= 2 && !h->c16 && h->fused_ok &&
          variant_on(h, CA_VAR_Y_MFMA1, "CA_Y_MFMA1") && variant_on(h, CA_VAR_Y_RIDE, "CA_Y_RIDE"))
        h->fc_tl = 1;   // (only where the int8 stream will ride: the other streams' merged kernels exist for 32- and 96-cell blocks)
      if (const int t = tune_val(h, CA_TUNE_FC_TL, "CA_FC_TL")) { if (t == 1 || t == 2 || t == 4 || t == 5 || t == 6 || t == 8) h->fc_tl = t; }
      if ((h->c16 || h->s2 || D >= 3) && h->fc_tl != 2) h->fc_tl = 6;   // (the two-operand-set kernels -- sixteen clones, four draws of mc_samples = 2 -- exist for the two default block shapes)
      if (h->s2 && !h->fwd_cell) { h->s2 = false; h->fused_ok = false; }
      h->ncblk_f = cdiv(Nn, 16 * h->fc_tl);
      // two block sizes in one launch (k_fwd_cell_mix)
      if (h->fwd_cell && (h->fc_tl == 4 || h->fc_tl == 5 || h->fc_tl == 6 || h->fc_tl == 8) && D >= 1 && D <= 4) {
        // measured at 100k cells (1042 blocks of 96): 1024 big + 53 small 2706 it/s, 768 + 821: 2682, 512 + 1589: 2669, all big
        // 2642 -- what pays is every CU getting the same number of big blocks, so: whole multiples of the CU count in big
        // blocks, the remainder (less than one big block per CU) in small ones
        int nbig = (h->ncblk_f / h->n_cu) * h->n_cu;
        if (const int t = tune_val(h, CA_TUNE_FC_NBIG, "CA_FC_NBIG")) nbig = t < 0 ? 0 : t;
        if (nbig > 0 && h->ncblk_f > nbig) {
          h->fc_nbig = nbig;
          h->ncblk_f = nbig + cdiv(Nn - (int64_t)nbig * 16 * h->fc_tl, 32);
        }
      }
    }
    int zsplit = h->gsplit;
    if (h->fwd_mfma) {
      h->frow = 16;
      h->nk32 = cdiv(G, 32);
      const int cblocks = cdiv(Nn, (CA_TB / 64) * CA_FM_TL * 16);
      {
        int per_cu = 4;
        const void* fn = (D == 1) ? (const void*)k_fwd_mfma<1> : (const void*)k_fwd_mfma<2>;   // (D = 3, 4 never take this kernel: a guide for the slice count only)
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, CA_TB, 0) != hipSuccess || per_cu < 1) per_cu = 4;
        (void)hipGetLastError();
        // every gene slice adds an N x 16 float partial (written here, re-read by the cell epilogue): ~2 % of the sweep
        h->fsplit = pick_split(cblocks, (int64_t)per_cu * h->n_cu, std::max(1, std::min(16, h->nk32 / CA_FM_KC)), 0.02);
      }
      if (const int t = tune_val(h, CA_TUNE_FSPLIT, "CA_FSPLIT")) h->fsplit = std::max(1, std::min(t, h->nk32));
      h->fkchunk = cdiv(h->nk32, h->fsplit);
      h->fsplit = cdiv(h->nk32, h->fkchunk);
      zsplit = h->fsplit;
      CACK(dalloc(h, &h->Mq, (int64_t)h->nk32 * 2 * 64 * 8 * ((h->c16 || h->s2) ? 2 : 1)));   // zero-filled: padding genes and columns stay 0 (9..16 clones: one image per draw)
    } else {
      CACK(dalloc(h, &h->Mb2, (int64_t)G * h->frow));
    }
    CACK(dalloc(h, &h->mu32B, G));
    CACK(dalloc(h, &h->gene_partB, (int64_t)h->ngblk * (3 + K)));
    CACK(dalloc(h, &h->gene_part_alt, (int64_t)h->ngblk * (3 + K)));
    CACK(dalloc(h, &h->gene_partB_alt, (int64_t)h->ngblk * (3 + K)));
    if (!h->fwd_cell) CACK(dalloc(h, &h->Zpart2, (int64_t)zsplit * Nn * h->frow));   // k_fwd_cell keeps Z in the block
  }
  // The side stream accompanies the cell-kernel path only.  Round 5, found by a parity run at 150k cells x 18 clones: with the plain passes (more than sixteen
  // clones, D >= 3, K = 0 ...) the loop's pipelining (deferred monitor tail, prologue hand-over, gated update) and the side stream's deferred start are not ordered
  // against each other -- ca_run's ELBOs from the second iteration on were wrong by 1e-4 ... 1e-1 and differed from run to run, silently, from 4e7 counts up
  // (below that the Y pass runs in line; the suite's side-stream cases all take the cell kernel).  Those shapes run the Y pass in line at every size.
  if (!h->fwd_cell) h->async_y = false;
  if (verbose(h))
    fprintf(stderr, "[clonealign_hip] N=%lld G=%d C=%d D=%d n_cu=%d gsplit=%d gchunk=%d csplit=%d fused=%d fwd_mfma=%d fsplit=%d fkchunk=%d "
            "bwd_mfma=%d csplit_m=%d cchunk_m=%lld nwt=%d fwd_cell=%d fc_tl=%d fc_nbig=%d ncblk_f=%d ystore=%d async_y=%d\n", (long long)Nn, G, C, D, h->n_cu, h->gsplit,
            h->gchunk, h->csplit, (int)h->fused_ok, (int)h->fwd_mfma, h->fsplit, h->fkchunk, (int)h->bwd_mfma, h->csplit_m,
            (long long)h->cchunk_m, h->nwt, (int)h->fwd_cell, h->fc_tl, h->fc_nbig, h->ncblk_f, h->ystore, (int)h->async_y);
  CACK(dalloc(h, &h->vmm, 2 * std::max(D, 1)));
  CACK(dalloc(h, &h->vmm_part, (int64_t)h->ngblk * 2 * std::max(D, 1)));
  CACK(dalloc(h, &h->etamax2, h->N16));
  CACK(dalloc(h, &h->gene_part, (int64_t)h->ngblk * (3 + K)));
  CACK(dalloc(h, &h->Zpart, (int64_t)S * h->gsplit * h->nchunk * Nn * CA_CW));
  CACK(dalloc(h, &h->coef, (int64_t)S * h->nchunk * Nn * CA_CW));
  CACK(dalloc(h, &h->scratch, Nn * C));
  const int64_t n_cpart = std::max(std::max(h->ncblk, h->ncblk_f), h->n_cu);   // (balanced sweep: one block per CU)
  CACK(dalloc(h, &h->cell_part, n_cpart * (3 + C)));
  // The series form of the contraction (ca_poly.hip) where it is measured faster than the sweeps: the count-matrix stream then runs as a launch of its own
  // (in line) and the rest is O(N + G) work in five small launches.  What the sweeps cost grows with N G, the series form with N and with a fixed chain of
  // launches (about 35 us), so the pick is a gene count per cell count: G >= 2000 + 2.5e7 / N (tools/series_time.py, late round 6, us per iteration sweeps /
  // series: 100k x 5k x 8 253 / 171; 50k x 3k x 6 107 / 89; 32k x 5k 110 / 86; 25k x 5k 92 / 78; 12.5k x 5k 63 / 59; 10k x 5k x 4 56 / 50; ties at 8192 x 5k and
  // 16k x 3k; losses below: 20k x 2k 55 / 59, 40k x 1k 58 / 67, 10k x 2k x 4 38 / 47).  The first form of the round needed 32k cells and 1.4e8 counts.
  // CA_VAR_SERIES switches the pick off, CA_VARX_SERIES forces the form at any size (tests; profiles/r06_series.txt).
#ifdef CA_SERIES_ALWAYS
  const bool series_auto = true;   // (shake-out builds: every eligible shape through the series form, whole GPU suite)
#else
  // (a rank of a cell-sharded fit pays one launch more per iteration -- the collective sits between the moments' reduction and the per-gene launch -- where the
  //  sweeps' collective rides in their launches: measured as a rank over the peer-to-peer transport, tools/shard_seq_time.py, us per iteration sweeps / series:
  //  12.5k x 5k x 8 69 / 72; 25k x 5k 96 / 94; 50k x 5k 149 / 126 -- so the rank's own cell count has to carry three times as much)
  const bool series_auto = Nn >= 6000 && (double)G >= 2000.0 + (h->opt.world > 1 ? 7.5e7 : 2.5e7) / (double)Nn;
#endif
  h->adam_bound = ca_adam_step_bound(h->opt.learning_rate, h->opt.beta1, h->opt.beta2);
  // (poly_shape: what does not depend on the rank's own cell count -- the same on every rank of a sharded fit)
  // (Adam settings without a step bound, beta1^2 >= beta2: no series form -- its look ahead counts on one)
  h->poly_shape = ca_poly_ok(D, S, C) && h->fused_ok && !h->c16 && !h->s2 && K == 1 && h->adam_bound > 0 &&
                  (variant_on(h, CA_VAR_SERIES, "CA_SERIES") || variantx_on(h, CA_VARX_SERIES, "CA_SERIES_ON"));
  h->poly = h->poly_shape && ((series_auto && variant_on(h, CA_VAR_SERIES, "CA_SERIES")) || variantx_on(h, CA_VARX_SERIES, "CA_SERIES_ON"));
  if (h->poly) {
    int CPp = 1;
    while (CPp < C) CPp <<= 1;
    const int per_cu = (h->opt.reserved[0] >= 1 && h->opt.reserved[0] <= 8) ? h->opt.reserved[0] : 2;   // (ca_options.reserved[0]: cell blocks per CU of the series form, lab)
    const int ncb = (int)std::min<int64_t>(cdiv(Nn, CA_TB / CPp), (int64_t)per_cu * h->n_cu);   // (<= ncblk: cell_part has a row for each)
    h->poly_side = h->opt.reserved[1] == 1;   // (ca_options.reserved[1] = 1: the count-matrix stream on the side stream beside the cell launch; default in line)
    const size_t wb = ca_poly_workspace_bytes(G, ncb);
    CACK(dalloc(h, &h->poly_mem, (int64_t)wb));
    HIPCK(h, hipMemsetAsync(h->poly_mem, 0, wb, h->stream));
    ca_poly_bind(&h->pws, h->poly_mem, G, ncb);
    HIPCK(h, hipHostMalloc((void**)&h->poly_ring, 16 * 4 * sizeof(double), hipHostMallocMapped));
    memset(h->poly_ring, 0, 16 * 4 * sizeof(double));
    if (hipHostGetDevicePointer((void**)&h->poly_ring_dev, h->poly_ring, 0) != hipSuccess) { (void)hipGetLastError(); h->poly = false; }
    CACK(dalloc(h, &h->poly_xpart, cdiv(Nn, CA_TB)));
    CACK(dalloc(h, &h->poly_zero, Nn));
    HIPCK(h, hipMemsetAsync(h->poly_zero, 0, (size_t)Nn * sizeof(float), h->stream));
  }
  CACK(dalloc(h, &h->ee_partB, n_cpart));
  CACK(dalloc(h, &h->gpart, (int64_t)std::max(h->csplit, h->csplit_m) * G * (S + D)));
  CACK(dalloc(h, &h->dFpart, (int64_t)std::max(h->ntile, h->nwt) * Nn * std::max(D, 1)));
  CACK(dalloc(h, &h->YWpart, (int64_t)(h->nseg + 1) * Nn * std::max(K, 1)));
  CACK(dalloc(h, &h->YTpart, (int64_t)(h->nrb + 1) * h->Gp * std::max(K, 1)));
  CACK(dalloc(h, &h->YW, Nn * std::max(K, 1)));
  h->n_yw = cdiv(Nn, CA_TB);
  CACK(dalloc(h, &h->yw_part, h->n_yw));
  CACK(dalloc(h, &h->ytpsi, (int64_t)h->Gp * std::max(K, 1)));
  // ---- count-matrix products on the int8 matrix cores, both from ONE tiled copy (k_ys_mfma, ca_ymfma.hip.h): K = 1, 1-byte storage
  // (the stream's buffer loads carry 32-bit byte offsets inside a strip: RS <= 512 cells x Gp bytes, and 16 N bytes of psi's image -- far inside 2^31 below these bounds)
  if (h->ystore == CA_YSTORE_U8 && K == 1 && h->Gp < (1 << 21) && Nn < ((int64_t)1 << 26) && variant_on(h, CA_VAR_Y_MFMA1, "CA_Y_MFMA1")) {
    h->ys_N64 = (Nn + 63) / 64 * 64;
    h->ys_nseg = h->Gp / CA_YS_GW;                  // Gp is a multiple of 1024
    // strips of RS cells per wave: about one resident round of blocks (3 per CU), at least 64 cells
    h->ys_RS = 64;
    while (h->ys_RS < 512 && cdiv(Nn, 4 * h->ys_RS) * h->ys_nseg > 4 * h->n_cu) h->ys_RS *= 2;
    h->ys_nrg = cdiv(Nn, 4 * h->ys_RS);
    // the loop image at 4 bits per count (CA_VAR_Y4): by default for the series form only (its stream is a launch of its own; the sweeps' riding
    // forms keep the 1-byte body) and where the escape list (stored counts >= 15) is at most 1 in 256 counts -- the shapes measured, at about
    // 1 in 370 (profiles/r07_*); CA_VARX_Y4 forces it at any shape and fraction.  A deterministic function of the shape and the matrix (int
    // offsets: below 2^31 counts)
    const bool y4_force = variantx_on(h, CA_VARX_Y4, "CA_Y4_ON") || variantx_on(h, CA_VARX_Y2, "CA_Y2_ON");   // (a forced 2-bit / 4-bit image needs the 4-bit one beside it)
    if (variant_on(h, CA_VAR_Y4, "CA_Y4") && (h->poly || y4_force) && (double)Nn * (double)h->Gp < 2.0e9) {
      const int64_t nkeys = (int64_t)h->ys_nrg * h->ys_nseg * 4 * h->ys_RS;
      CACK(dalloc(h, &h->esc_off, nkeys + 1));
      const int64_t nw = Nn * h->ys_nseg;
      hipLaunchKernelGGL(k_esc_count, dim3(cdiv(nw * 64, CA_YM_TB)), dim3(CA_YM_TB), 0, h->stream, (const uint8_t*)h->Y, Nn, h->Gp, h->ys_nseg, h->ys_RS,
                         h->esc_off);
      hipLaunchKernelGGL(k_esc_scan, dim3(1), dim3(1024), 0, h->stream, h->esc_off, nkeys);
      HIPCK(h, hipGetLastError());
      int total = 0;
      HIPCK(h, hipMemcpyAsync(&total, h->esc_off + nkeys, sizeof(int), hipMemcpyDeviceToHost, h->stream));
      SYNC(h);
      h->n_esc = total;
      h->ys4 = h->n_esc * 256 <= Nn * (int64_t)h->G || y4_force;
      if (!h->ys4) {   // the offsets were the last allocation: returned, nothing of the 4-bit image stays resident
        HIPCK(h, hipFree(h->esc_off));
        h->allocs.pop_back();
        h->dev_bytes -= 4 * (nkeys + 1);
        h->esc_off = nullptr;
      } else {
        CACK(dalloc(h, &h->esc, h->n_esc));
        hipLaunchKernelGGL(k_esc_fill, dim3(cdiv(nw * 64, CA_YM_TB)), dim3(CA_YM_TB), 0, h->stream, (const uint8_t*)h->Y, Nn, h->Gp, h->ys_nseg, h->ys_RS,
                           h->esc_off, h->esc);
        HIPCK(h, hipGetLastError());
      }
    }
    CACK(dalloc(h, &h->Ys, h->ys_N64 * h->Gp / (h->ys4 ? 2 : 1)));
    uint8_t *wr = nullptr, *pr = nullptr;
    CACK(dalloc(h, &wr, (int64_t)(h->Gp / 64) * 1024));
    CACK(dalloc(h, &pr, (h->ys_N64 / 64) * 1024));
    h->Wr = (uint4*)wr; h->Pr = (uint4*)pr;
    CACK(dalloc(h, &h->Wsum, (int64_t)(h->Gp / 64) * 4));
    CACK(dalloc(h, &h->Psum, (h->ys_N64 / 64) * 4));
    CACK(dalloc(h, &h->YWpart, (int64_t)(std::max(h->nseg, h->ys_nseg) + 1) * Nn));      // (replaces the vector stream's smaller slabs)
    CACK(dalloc(h, &h->YTpart, (int64_t)(std::max(h->nrb, h->ys_nrg) + 1) * h->Gp));
    CACK(dalloc(h, &h->ys_exps, 6));
    CACK(dalloc(h, &h->ys_amax, 2));
    h->ys_nq = cdiv((int64_t)(h->Gp / 64) + h->ys_N64 / 64, CA_YM_TB / 64);
    h->ys_ncap = std::max(h->ys_nq, h->ngblk + cdiv(Nn, CA_TB)) + 2;
    CACK(dalloc(h, &h->ys_amaxp, (int64_t)3 * h->ys_ncap * 2));
    if (h->ys4)
      hipLaunchKernelGGL(k_pack_y4, dim3(cdiv(h->ys_N64 * (h->Gp / 32), CA_YM_TB)), dim3(CA_YM_TB), 0, h->stream, (const uint8_t*)h->Y, (uint4*)h->Ys, Nn,
                         h->ys_N64, h->Gp);
    else
      hipLaunchKernelGGL(k_bias_y, dim3(cdiv(h->ys_N64 * (h->Gp / 16), CA_YM_TB)), dim3(CA_YM_TB), 0, h->stream, (const uint8_t*)h->Y, (uint4*)h->Ys, Nn,
                         h->ys_N64, h->Gp);
    HIPCK(h, hipGetLastError());
    // the 2-bit / 4-bit image beside the 4-bit one (CA_VAR_Y2), for the series form's own stream launch: from the resident u8 matrix, whatever the ingest was
    if (h->ys4 && h->poly && variant_on(h, CA_VAR_Y2, "CA_Y2")) {
      const bool y2_force = variantx_on(h, CA_VARX_Y2, "CA_Y2_ON");
      const int lab_n2 = (h->opt.reserved[0] >> 8) & 15;   // (ca_options.reserved[0], bits 8 up, lab: N2 of a forced image, 5 or 6)
      if (y2_force || (double)h->ys_N64 * (double)h->Gp >= CA_Y2_MIN_COUNTS) {
        int* hist = nullptr;
        CACK(dalloc(h, &hist, 2 * (int64_t)h->Gp));
        hipLaunchKernelGGL(k_y2_hist, dim3(cdiv(h->Gp / 4, CA_YM_TB), (unsigned)cdiv(Nn, 64)), dim3(CA_YM_TB), 0, h->stream, (const uint8_t*)h->Y, Nn, h->Gp, hist);
        HIPCK(h, hipGetLastError());
        std::vector<int32_t> hc(2 * (size_t)h->Gp);
        HIPCK(h, hipMemcpyAsync(hc.data(), hist, hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        SYNC(h);
        std::vector<uint16_t> perm(h->Gp), pos(h->Gp);
        int64_t ne = 0;
        const int n2 = ca_y2_plan_impl(hc.data(), hc.data() + h->Gp, h->Gp, Nn * (int64_t)h->G, y2_force ? (lab_n2 == 5 || lab_n2 == 6 ? lab_n2 : 6) : 0, perm.data(), pos.data(), &ne);
        if (n2 > 0 && ne < ((int64_t)1 << 31)) {
          CACK(dalloc(h, &h->y2_perm, (int64_t)h->Gp));
          CACK(dalloc(h, &h->y2_pos, (int64_t)h->Gp));
          HIPCK(h, hipMemcpyAsync(h->y2_perm, perm.data(), (size_t)h->Gp * 2, hipMemcpyHostToDevice, h->stream));
          HIPCK(h, hipMemcpyAsync(h->y2_pos, pos.data(), (size_t)h->Gp * 2, hipMemcpyHostToDevice, h->stream));
          const int64_t nkeys = (int64_t)h->ys_nrg * h->ys_nseg * 4 * h->ys_RS, nw = Nn * h->ys_nseg;
          CACK(dalloc(h, &h->esc2_off, nkeys + 1));
          hipLaunchKernelGGL(k_esc_count, dim3(cdiv(nw * 64, CA_YM_TB)), dim3(CA_YM_TB), 0, h->stream, (const uint8_t*)h->Y, Nn, h->Gp, h->ys_nseg, h->ys_RS,
                             h->esc2_off, (const uint4*)h->y2_pos, n2);
          hipLaunchKernelGGL(k_esc_scan, dim3(1), dim3(1024), 0, h->stream, h->esc2_off, nkeys);
          HIPCK(h, hipGetLastError());
          int total = 0;
          HIPCK(h, hipMemcpyAsync(&total, h->esc2_off + nkeys, sizeof(int), hipMemcpyDeviceToHost, h->stream));
          SYNC(h);
          if ((int64_t)total != ne) { h->err = "2-bit image: the device's escape count differs from the host plan's"; return CA_ERR_STATE; }
          h->n_esc2 = total;
          CACK(dalloc(h, &h->esc2, h->n_esc2));
          hipLaunchKernelGGL(k_esc_fill, dim3(cdiv(nw * 64, CA_YM_TB)), dim3(CA_YM_TB), 0, h->stream, (const uint8_t*)h->Y, Nn, h->Gp, h->ys_nseg, h->ys_RS,
                             h->esc2_off, h->esc2, (const uint4*)h->y2_pos, n2);
          const int64_t sb = n2 * 1024 + (8 - n2) * 2048, ib = (h->ys_N64 / 64) * h->ys_nseg * sb;
          CACK(dalloc(h, &h->Ys2, ib));
          hipLaunchKernelGGL(k_pack_y2, dim3(cdiv(ib / 16, CA_YM_TB)), dim3(CA_YM_TB), 0, h->stream, (const uint8_t*)h->Y, (uint4*)h->Ys2, Nn, h->ys_N64, h->Gp, n2,
                             h->y2_perm);
          HIPCK(h, hipGetLastError());
          SYNC(h);   // (the host's vectors were the copies' sources)
          h->ys_n2 = n2;
          h->y_dev_bytes += ib + 4 * h->n_esc2 + 4 * (nkeys + 1) + 4 * (int64_t)h->Gp;
        }
      }
    }
    if (h->adam_bound > 0) h->ys_step_bound = (float)(1.02 * h->adam_bound);   // (ca_adam_step_bound; none: the quantiser never runs on lagged maxima)
    h->y_ys = true;
    h->y_dev_bytes += h->ys4 ? h->ys_N64 * h->Gp / 2 + 4 * h->n_esc + 4 * ((int64_t)h->ys_nrg * h->ys_nseg * 4 * h->ys_RS + 1) : h->ys_N64 * h->Gp;
  }
  // the series form's forward moments ride on its in-line count-matrix stream's launch (CA_VAR_MOM_RIDE, ca_polymom.hip.h): wherever that stream exists and runs in
  // line -- every shape measured gains or is level (profiles/r11_mom_ride_ab.txt); a pass that launches no stream keeps the moments' own launches (run_fused)
  h->mom_ride = h->poly && h->y_ys && !h->poly_side && h->host_dev && variant_on(h, CA_VAR_MOM_RIDE, "CA_MOM_RIDE");
  // ... behind the stream's blocks where ca_mom_last_pick (above) says so (CA_VAR_MOM_LAST), or wherever they ride (CA_VARX_MOM_LAST); off: in front, as before
  if (h->mom_ride) {
    ca_mom_last_in ml;
    int per_cu = 0;
    // (the slots of the launch that runs: the form with the overflow list's blocks where there is a list, the stream's dynamic LDS of the image in use)
    const hipError_t oe = h->ys4 ? (h->n_ovf > 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ys_mfma_ovf_mom<true>, CA_YM_TB, CA_YS4_LDS_BYTES)
                                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ys_mfma_mom<true>, CA_YM_TB, CA_YS4_LDS_BYTES))
                                 : (h->n_ovf > 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ys_mfma_ovf_mom<false>, CA_YM_TB, CA_YS_LDS_BYTES)
                                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ys_mfma_mom<false>, CA_YM_TB, CA_YS_LDS_BYTES));
    if (oe != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }   // (no answer: no free slot is known of, the rule keeps the order as it was)
    ml.slots = per_cu * h->n_cu; ml.n_cu = h->n_cu;
    ml.nb_stream = h->ys_nrg * h->ys_nseg;
    ml.nb_ovf = h->n_ovf > 0 ? cdiv(Nn, CA_TB) + cdiv(h->n_ovf_chunk, CA_TB / 64) : 0;
    ml.ngrp = h->pws.n_gene_blocks; ml.nred = CA_MOM_NRED;
    ml.image_bytes = h->ys_N64 * h->Gp / (h->ys4 ? 2 : 1);
    h->mom_free_slots = ca_mom_last_free(ml);
    h->mom_last = variantx_on(h, CA_VARX_MOM_LAST, "CA_MOM_LAST_ON") || (variant_on(h, CA_VAR_MOM_LAST, "CA_MOM_LAST") && ca_mom_last_pick(ml));
    if (h->opt.variant_off & CA_VAR_MOM_LAST) h->mom_last = false;   // (off is off: the launch as it was, block for block, whatever else is asked)
    if (h->mom_last) {   // the role's shape behind the stream (above); forced where no XCD-wide free slot exists: the shape it has in front
      const int per = ca_mom_last_per(ml);
      h->mom_per = per < 1 ? CA_MOM_PER : std::min(per, CA_ML_MAX_PER);
      h->mom_nred = 2 * CA_MOM_NRED;
      const int lab = (h->opt.reserved[1] & ~0xFF) ? h->opt.reserved[1] >> 8 : 0;   // (ca_options.reserved[1], bits 8 up, lab: groups per moment block | 16: the reducers of the order in front | 32: overflow blocks in front of the role)
      if (lab & 15) h->mom_per = lab & 15;
      if (lab & 16) h->mom_nred = CA_MOM_NRED;
      h->mom_ovf_first = (lab & 32) != 0;
    }
  }
  // the series form's cell launch without the memory and LDS-crossbar round trips inside its passes (CA_VAR_CELL_LEAN, ca_poly.hip): wherever the series form runs
  h->cell_lean = h->poly && variant_on(h, CA_VAR_CELL_LEAN, "CA_CELL_LEAN");
  // ... and with its backward moments gathered by fp64 MFMA per wave instead of the thread-owned chain between two block barriers (CA_VAR_CELL_MFMA): likewise
  h->cell_mfma = h->poly && variant_on(h, CA_VAR_CELL_MFMA, "CA_CELL_MFMA");
  // ... and, for that form alone, with its head's loads issued at once and its block end as one parking step (CA_VAR_CELL_EDGE): the same bits
  h->cell_edge = h->poly && h->cell_lean && h->cell_mfma && variant_on(h, CA_VAR_CELL_EDGE, "CA_CELL_EDGE");
  // ... and the way back from it: the stream's column jobs off the cell launch, reduction + per-gene pass + column jobs as one launch (CA_VAR_GENE_RIDE,
  // ca_polygene.hip.h); which order a pass takes is decided where it is queued (gene_ride_merges: a cell-sharded fit keeps the two launches)
  h->gene_ride = h->poly && variant_on(h, CA_VAR_GENE_RIDE, "CA_GENE_RIDE");
  // ... and whether the stream's column jobs leave the cell launch with it.  Measured (profiles/r22_tail_ab.txt (B), merged launch alone against merged launch + moved
  // columns, alternating): 25k / 50k x 5k x 8 and 50k x 3k x 6 gain 2.0 - 2.4 us per iteration from the move (cell launch 16.7 -> 14.1 and 20.1 -> 18.2 us), 12.5k is
  // level, and at 100 000 cells (x 8 and x 4 clones) the move LOSES 0.3 - 0.7: there the cell launch is no shorter without them (28.3 us either way) and they sit at
  // the end of the way back, in front of the update that reads their sums.  The rule is the cell count between the measured shapes; what decides it inside the cell
  // launch -- which block ends it -- has not been stamped (DESIGN section 10).  ca_options.reserved[1] = 7 / 8 (lab) keeps / moves them whatever the rule says.
  h->gene_cols = h->gene_ride && (h->opt.reserved[1] == 8 || (h->opt.reserved[1] != 7 && Nn <= CA_GENE_COLS_MAXN));
  // the Y stream rides on the forward sweep's launch: 1-byte storage, K = 1, the fused sweep with its default block shapes
  h->ride_ok = h->ystore == CA_YSTORE_U8 && K == 1 && D <= 2 && h->fused_ok && !h->c16 && h->fwd_cell && (h->fc_tl == 6 || h->fc_tl == 8 || (h->fc_tl == 2 && h->fc_nbig == 0)) &&
               !h->y_ys && variant_on(h, CA_VAR_Y_RIDE, "CA_Y_RIDE");
  const bool tl1_ok = h->fc_tl == 1 && h->fc_nbig == 0 && !h->c16;
  h->ride_ys = h->y_ys && (!h->ys4 || (h->poly && D == 1 && !h->c16 && !h->s2)) && D <= 2 && h->fused_ok && h->fwd_cell && (h->fc_tl == 6 || tl1_ok || (h->fc_tl == 2 && h->fc_nbig == 0)) &&
               variant_on(h, CA_VAR_Y_RIDE, "CA_Y_RIDE");
  h->yfin_split = h->ride_ys && h->bwd_mfma && h->tail_fuse && variant_on(h, CA_VAR_YFIN_RIDE, "CA_YFIN_RIDE");
  // The int8 one-copy stream either rides or runs in line: as a launch of its own on the SIDE stream (variant y_ride off at 4e7 counts and more) its parameter
  // images -- rewritten by the update launch -- are not ordered against that stream (tools/fuzz_large.py --wide: 22 165 x 4734 x 3, trace 6e-5 off).  Not a
  // default path (1-byte storage with K = 1 rides); the side stream stays for the vector streams of 2- / 4-byte storage and K != 1, which the large runs confirm.
  if (h->y_ys && !h->ride_ys) h->async_y = false;
  {   // balanced forward sweep (ca_fwdbal.hip.h): one to six whole tiles per CU, the int8 stream riding, eight clones at most, one latent dimension
    const int tiles = cdiv(Nn, 16), qb = tiles / std::max(h->n_cu, 1), rb = tiles - qb * h->n_cu;
    // ... and at least 96 k-steps of 32 genes: with eight waves per block a wave of cfg-2 (2000 genes, 63 k-steps) has eight k-steps, the two
    // pipeline fills of a block that also sweeps a chunk cost more than the balance returns (10k x 2k x 4: 42.7 against 39.3 us per iteration)
    h->fwd_bal = h->ride_ys && !h->c16 && !h->s2 && D == 1 && C <= 8 && qb >= 1 && qb <= 6 && h->nk32 >= 96 && h->host_dev && variant_on(h, CA_VAR_FWD_BAL, "CA_FWD_BAL");
    if (h->fwd_bal) {
      // left-over tiles: gene chunks swept by the sweep blocks beside their own tiles (us per iteration at 12 500 / 25 000 / 10 240 / 14 336 cells, i.e. 14 / 27 /
      // 128 / 128 left-over tiles: chunks 63.6 / 95.1 / 57.3 / 68.0, four-wave sweep 65.0 / 98.7 / 58.5 / 69.3; profiles/r05_small_shapes.txt)
      h->bal_q = qb; h->bal_r = rb;
      h->bal_nchunk = rb > 0 ? std::min(CA_BAL_MAXCHUNK, h->n_cu / rb) : 0;
      CACK(dalloc(h, &h->bal_xw, std::max<int64_t>(1, (int64_t)rb * h->bal_nchunk * 512)));
    }
  }
  // mc_samples = 2, four draws per sweep: where the sweep is the cell kernel and the stream either rides as the int8 stream or not at all
  h->s2f = h->s2 && h->fused_ok && h->fwd_cell && (h->fc_tl == 2 || h->fc_tl == 6) && (h->ride_ys || !h->ride_ok) && variant_on(h, CA_VAR_S2_FUSE, "CA_S2_FUSE");
  // The layout has to be the same on every rank (the collective's length follows from it), and the pick of the form depends on the rank's own cell count (shards
  // differ by a cell): a rank of a sharded fit takes the series layout whenever the SHAPE allows the form; when the transport is up the ranks agree on the pick
  // (setup_global_sums) and go back to the classic layout together where not every rank picked the form.
  h->layout_series = h->poly || (h->poly_shape && h->opt.world > 1);
  if (h->layout_series) {   // (K = 1, D = 1, S = 1)
    h->off_y = 3 + C;
    h->off_q = h->off_y + (int64_t)h->Gp * K;
    h->off_x = h->off_q + (int64_t)CA_PL_NB * (CA_PL_R + 2) * 8;
    h->off_g = h->off_x + std::max(h->opt.world, 1);
    h->red_n = h->off_g + (int64_t)G * (S + D);
    CACK(dalloc(h, &h->red, h->red_n));
    if (h->poly) h->pws.tabQ = h->red + h->off_q;   // (the backward moments are reduced in place: sharded, they travel in the collective)
  } else {
  h->off_g = 3 + C;
  h->off_y = h->off_g + (int64_t)G * (S + D);
  h->red_n = h->off_y + (int64_t)G * K;
  CACK(dalloc(h, &h->red, h->off_y + (int64_t)h->Gp * std::max(K, 1)));   // Y^T psi lands here directly ([Gp][K] rows, first G reduced)
  }
  CACK(dalloc(h, &h->terms_dev, 4));
  CACK(ensure_elbo_cap(h, 64));
  CACK(ensure_eps_cap(h, 1));
  // ---- column sums and Y^T X via the streaming kernel with all-ones factors (a block's four strips are summed in float32, the cross-strip
  //      sum is fp64: exact for integer counts while a block's partial stays below 2^24 -- u8 bytes always do, and their overflow excess is added in double
  //      below; u16 counts over 512 cells and f32 counts above 65535 need not, and colsum is then good to float32 rounding, 6e-8 relative)
  {
    // colsum: run ypass with K' = 1, psi == 1, W == 0 on temporary factor buffers
    const int cols = 1 + ((K > 0) ? P : 0);
    // loc0 == NULL: one more column with factor 1 / rowMeans(Y) gives mu_guess_g = mean_n(y_ng / mean_g' y_ng') (:220-235,
    // data_init_mu = TRUE), and loc0 = safe_inverse_softplus(mu_guess) (:262, :6-11).  The weights go through float32 and
    // the strip sums are fp32 (1e-7 relative on an initial value).
    const int cols_all = cols + (p->loc0 ? 0 : 1);
    std::vector<double> srow;
    if (!p->loc0) {
      srow.resize((size_t)Nn);
      HIPCK(h, hipMemcpyAsync(srow.data(), h->s64, (size_t)Nn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      SYNC(h);
    }
    std::vector<double> cs((size_t)G, 0.0), ytx((size_t)G * std::max(P, 1), 0.0);
    float *Ft = nullptr, *Vt = nullptr, *YWp = nullptr, *YTp = nullptr; double* yt = nullptr;
    HIPCK(h, hipMalloc((void**)&Ft, (size_t)Nn * sizeof(float)));
    HIPCK(h, hipMalloc((void**)&Vt, (size_t)G * sizeof(float)));
    HIPCK(h, hipMalloc((void**)&YWp, (size_t)h->nseg * Nn * sizeof(float)));
    HIPCK(h, hipMalloc((void**)&YTp, (size_t)h->nrb * h->Gp * sizeof(float)));
    HIPCK(h, hipMalloc((void**)&yt, (size_t)h->Gp * sizeof(double)));
    HIPCK(h, hipMemsetAsync(Vt, 0, (size_t)G * sizeof(float), h->stream));
    std::vector<float> col((size_t)Nn);
    for (int j = 0; j < cols_all; ++j) {
      if (j >= cols) for (int64_t n = 0; n < Nn; ++n) col[n] = (float)((double)G / srow[(size_t)n]);
      else for (int64_t n = 0; n < Nn; ++n) col[n] = j == 0 ? 1.f : (float)p->X[hidx(p->layout, n, j - 1, Nn, P)];
      HIPCK(h, hipMemcpyAsync(Ft, col.data(), (size_t)Nn * sizeof(float), hipMemcpyHostToDevice, h->stream));
      dim3 grid((unsigned)((int64_t)h->nrg * h->nseg));
      ca_ovf_args no_ovf;
      memset(&no_ovf, 0, sizeof(no_ovf));
      ypass<0>(h, ca_ypass_ops{Ft, 1, Vt, YWp, YTp, 1}, 0, 1, grid, no_ovf);
      HIPCK(h, hipGetLastError());
      hipLaunchKernelGGL(k_colsum, dim3(cdiv(h->Gp, 64)), dim3(1024), 0, h->stream, YTp, yt, h->nrg, (int64_t)h->Gp, h->Gp);
      std::vector<double> tmp((size_t)G);
      HIPCK(h, hipMemcpyAsync(tmp.data(), yt, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      SYNC(h);
      for (int64_t e = 0; e < h->n_ovf; ++e)   // overflow list, fixed (cell, gene) order
        tmp[h->h_ocol[e]] += (double)h->h_oval[e] * (double)col[h->h_orow[e]];
      if (j >= cols) {
        if (h->opt.world > 1) h->mu_part = tmp;   // a shard: the guess over ALL cells is completed when the transport is set (setup_global_sums)
        std::vector<float> l0((size_t)G);
        for (int g = 0; g < G; ++g) {
          const double mu = tmp[g] / (double)Nn;
          l0[g] = (float)(std::log(1.0 - std::exp(-std::fabs(mu))) + std::max(mu, 0.0));
        }
        CACK(upload_f(h, h->loc, l0));
      } else if (j == 0) cs = tmp;
      else for (int g = 0; g < G; ++g) ytx[(size_t)g * P + (j - 1)] = tmp[g];
    }
    hipFree(Ft); hipFree(Vt); hipFree(YWp); hipFree(YTp); hipFree(yt);
    CACK(upload_d(h, h->colsum, cs));
    CACK(dalloc(h, &h->YtX, (int64_t)G * std::max(P, 1)));
    CACK(upload_d(h, h->YtX, ytx));
  }
  CACK(dalloc(h, &h->loc_init, G));
  HIPCK(h, hipMemcpyAsync(h->loc_init, h->loc, (size_t)G * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  h->dir_const = -((double)C * std::lgamma(1.0 / (double)C) - std::lgamma(1.0));
  h->b1p = (float)h->opt.beta1;
  h->b2p = (float)h->opt.beta2;
  CACK(refresh_derived(h));
  SYNC(h);
  return CA_OK;
}

struct ParamRef {
  float* f = nullptr; double* d = nullptr;
  int64_t rows = 0, cols = 0, stride = 0, off = 0;  // logical rows x cols; device element (r,c) at r*stride + off + c
  int xform = 0;  // 0 none, 1 softplus, 2 row softmax, 3 exp, 4 softmax (vector)
  bool matrix = false;
};

bool find_param(ca_engine* h, const std::string& n, bool grad, ParamRef& r) {
  const int64_t N = h->N; const int G = h->G, C = h->C, K = h->K, P = h->P, D = h->D;
  if (n == "loc" || n == "mu") { r.f = grad ? h->g_loc : h->loc; r.rows = G; r.cols = 1; r.stride = 1; r.xform = (n == "mu") ? 1 : 0; return !(grad && n == "mu"); }
  if (n == "ls") { r.f = grad ? h->g_ls : h->ls; r.rows = G; r.cols = 1; r.stride = 1; return true; }
  if (n == "gamma_logits" || n == "clone_probs") { r.f = grad ? h->dgl : h->glogit; r.rows = N; r.cols = C; r.stride = C; r.matrix = true; r.xform = (n == "clone_probs") ? 2 : 0; return !(grad && n == "clone_probs"); }
  if (n == "alpha_unconstr" || n == "alpha") { r.f = grad ? h->g_a : h->alpha_u; r.rows = C; r.cols = 1; r.stride = 1; r.xform = (n == "alpha") ? 4 : 0; return !(grad && n == "alpha"); }
  if (n == "v" || n == "chi") { r.f = grad ? h->g_v : h->vchi; r.rows = K; r.cols = 1; r.stride = 1; r.xform = (n == "chi") ? 3 : 0; return !(grad && n == "chi"); }
  if (n == "psi") { r.f = grad ? h->g_psi : h->F; r.rows = N; r.cols = K; r.stride = grad ? K : D; r.matrix = true; return true; }
  if (n == "W") { r.f = grad ? h->g_V : h->V; r.rows = G; r.cols = K; r.stride = D; r.matrix = true; return true; }
  if (n == "beta") { r.f = grad ? h->g_V : h->V; r.rows = G; r.cols = (D > 0) ? P : 0; r.stride = D; r.off = K; r.matrix = true; return true; }
  if (n == "s" && !grad) { r.d = h->s64; r.rows = N; r.cols = 1; r.stride = 1; return true; }
  return false;
}

