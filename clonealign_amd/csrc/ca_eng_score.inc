// ca_eng_score.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): C ABI, the scoring family -- the calls that score the resident count matrix under a fitted model: the per-cell, per-clone log-likelihood (ca_clone_loglik), under a mixture of two clones (ca_clone_pair_loglik), the maximum-likelihood mixture of all clones (ca_clone_mixture), Dirichlet-multinomial (ca_clone_loglik_dm), by block of genes (ca_clone_loglik_by_block), the per-cell MAP psi of cells outside a fit (ca_project_cells), the clone evidence with psi integrated out (ca_clone_evidence), with the genes reweighted for every replicate of a bootstrap (ca_clone_loglik_reweighted).
// All of them read the matrix, the row sums and the overflow list only: no wait for the loop's side stream, no variable, Adam slot or draw index changes.  Their
// inputs and outputs cover the local cells, so a sharded handle needs no sums from its peers; it still takes part in ONE small collective, the verdict on the
// input (a non-finite U is local), so that every rank returns the same code instead of one of them leaving the others waiting.
// The scaffolding they share is written once: the owner of a call's device memory (ca_call_mem, ca_eng_state.inc), and here the operands of the sweep and of the contraction (ll_operands),
// the verdict (agree_on_verdict), the batch size (cells_per_batch), the outputs' layout (ca_rows_out).
extern "C++" {   // (templates: this part sits inside the C ABI's extern "C" block)
namespace {
// The verdict on the input, agreed across the ranks of a sharded handle: a rank whose own input is fine learns here that another rank's is not.
int agree_on_verdict(ca_engine* h, std::string& bad) {
  if (!is_sharded(h)) return CA_OK;
  std::vector<double> pack{bad.empty() ? 0.0 : 1.0};   // [ranks whose input was refused]
  ca_call_mem mem(h);
  double* scratch = mem.alloc<double>(1);
  if (mem.rc != CA_OK) return mem.rc;
  CACK(allreduce_host_vec(h, pack, scratch));
  if (pack[0] != 0.0 && bad.empty()) bad = "another rank refused its input";
  return CA_OK;
}

// cells per batch, so that the batch's slabs (per_cell bytes each) stay within the budget: whole blocks, at least one (a cell's values do not depend on its batch)
int64_t cells_per_batch(int64_t cells, int64_t per_cell, int64_t budget) { return std::min<int64_t>(cells, std::max<int64_t>(CA_TB, (budget / per_cell) / CA_TB * CA_TB)); }
constexpr int64_t CA_LL_BUDGET = (int64_t)1 << 28;   // a quarter of a gigabyte

// A [rows][cols] output the device writes row-major: p is where the copies land -- the caller's array itself when the handle's layout is row-major, a temporary
// that finish() puts into the caller's layout otherwise.
struct ca_rows_out {
  double* dst; int64_t rows, cols; bool colmaj;
  std::vector<double> tmp;
  double* p;
  ca_rows_out(const ca_engine* h, double* dst_, int64_t rows_, int64_t cols_)
      : dst(dst_), rows(dst_ ? rows_ : 0), cols(cols_), colmaj(h->layout == CA_COL_MAJOR), tmp(colmaj ? (size_t)(rows * cols) : 0), p(colmaj ? tmp.data() : dst) {}
  void finish() {
    if (!colmaj) return;
    for (int64_t n = 0; n < rows; ++n)
      for (int64_t j = 0; j < cols; ++j) dst[hidx(CA_COL_MAJOR, n, j, rows, cols)] = tmp[(size_t)(n * cols + j)];
  }
};

// The table of the log-likelihood sweep (k_clone_ll): per gene the columns [log E of the clones | V], in groups of NC columns, zero padded; where E = 0 the
// entry is 0 and the gene's mask has the bit.  logz0[c] = log sum_g E[g][c].  Returns the refusal, or "".
std::string ll_sweep_table(ca_engine* h, const double* E, const double* V, int D, int NC, int ngrp, std::vector<double>& tab, std::vector<unsigned>& zmask, std::vector<double>& logz0) {
  const int G = h->G, Gp = h->Gp, C = h->C;
  std::string bad;
  std::vector<double> col((size_t)G);
  tab.assign((size_t)ngrp * Gp * NC, 0.0); logz0.assign((size_t)C, 0.0); zmask.assign((size_t)ngrp * Gp, 0u);
  for (int c = 0; c < C && bad.empty(); ++c) {
    const int grp = c / NC, cc = c % NC;
    for (int g = 0; g < G; ++g) {
      const double v = E[hidx(h->layout, g, c, G, C)];
      if (!std::isfinite(v) || v < 0.0) { bad = "expected expression has a negative or non-finite entry (gene " + std::to_string(g) + ", clone " + std::to_string(c) + ")"; break; }
      col[(size_t)g] = v;
      if (v > 0.0) tab[((size_t)grp * Gp + g) * NC + cc] = std::log(v);
      else zmask[(size_t)grp * Gp + g] |= 1u << cc;
    }
    if (!bad.empty()) break;
    const double sum = pairwise_sum(col.data(), 0, G);
    if (!std::isfinite(sum) || sum == 0.0) { bad = "expected expression of clone " + std::to_string(c) + " sums to " + std::to_string(sum) + " over the genes"; break; }
    logz0[(size_t)c] = std::log(sum);
  }
  for (int g = 0; g < G && D > 0 && bad.empty(); ++g)
    for (int d = 0; d < D; ++d) {
      const double v = V[hidx(h->layout, g, d, G, D)];
      if (!std::isfinite(v)) { bad = "V has a non-finite entry (gene " + std::to_string(g) + ", factor " + std::to_string(d) + ")"; break; }
      tab[((size_t)((C + d) / NC) * Gp + g) * NC + (C + d) % NC] = v;
    }
  return bad;
}

// What a scoring call asks of its inputs.  The cells' factor block is [u[0] | u[1]], D columns together: U itself, or psi_start | X; a part without values is
// zeros, and a non-finite entry is refused as "<name> has a non-finite entry (cell n, <unit> k)".
struct ca_u_part { const double* v; int cols; const char* name; const char* unit; };
struct ca_ll_req {
  const double *E, *V; int D;
  ca_u_part u[2];
  int64_t c_lo, c_cnt;   // the cell range
  bool lgc;              // the lgamma(k + 1) table
  bool factors;          // Ut, Vt (and Ez) even at D = 0
  int NZ;                // E in groups of NZ clone columns (Ez); 0: none
  bool compact;          // E compact (Ec)
};
// The operands: the sweep's table in groups of NC columns with its masks and logz0, U and V padded to CA_LL_DMAX factors, E as asked, the lgamma table; `bad`
// is the first problem in the order range, E, V, the cells' block by cell (or "").  Vt, Ez and Ec are filled only when nothing is wrong.
struct ca_ll_operands {
  int NC, ngrp, nct;
  std::vector<double> tab, logz0, Ut /*[N][CA_LL_DMAX]*/, Vt /*[Gp][CA_LL_DMAX]*/, Ez /*[ngz][Gp][NZ]*/, Ec /*[Gp][C]*/, lgt;
  std::vector<unsigned> zmask;
  std::string bad;
};
void ll_operands(ca_engine* h, const ca_ll_req& q, ca_ll_operands& o) {
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C, D = q.D;
  const int ncol = C + D;
  o.NC = ncol <= 8 ? 8 : ncol <= 16 ? 16 : 32; o.ngrp = cdiv(ncol, o.NC); o.nct = o.ngrp * o.NC;
  std::string& bad = o.bad;
  if (q.c_lo < 0 || q.c_cnt < 0 || q.c_lo > N || q.c_cnt > N - q.c_lo)
    bad = "the cell range [" + std::to_string(q.c_lo) + ", " + std::to_string(q.c_lo) + " + " + std::to_string(q.c_cnt) + ") is outside [0, " + std::to_string(N) + "]";
  if (bad.empty()) bad = ll_sweep_table(h, q.E, q.V, D, o.NC, o.ngrp, o.tab, o.zmask, o.logz0);
  const bool fac = q.factors || D > 0;
  if (fac && bad.empty()) {
    o.Ut.assign((size_t)N * CA_LL_DMAX, 0.0);
    for (int64_t n = 0; n < N && bad.empty(); ++n) {
      int at = 0;
      for (const ca_u_part& p : q.u) {
        for (int k = 0; k < p.cols && p.v && bad.empty(); ++k) {
          const double v = p.v[hidx(h->layout, n, k, N, p.cols)];
          if (!std::isfinite(v)) bad = std::string(p.name) + " has a non-finite entry (cell " + std::to_string(n) + ", " + p.unit + " " + std::to_string(k) + ")";
          o.Ut[(size_t)n * CA_LL_DMAX + at + k] = v;
        }
        at += p.cols;
      }
    }
  }
  if (q.lgc) { o.lgt.resize(CA_LL_LGTAB); for (int k = 0; k < CA_LL_LGTAB; ++k) o.lgt[(size_t)k] = std::lgamma((double)k + 1.0); }
  if (!bad.empty()) return;
  const int NZ = fac ? q.NZ : 0, ngz = NZ ? cdiv(C, NZ) : 0;
  if (fac) o.Vt.assign((size_t)Gp * CA_LL_DMAX, 0.0);
  if (NZ) o.Ez.assign((size_t)ngz * Gp * NZ, 0.0);
  if (q.compact) o.Ec.assign((size_t)Gp * C, 0.0);
  for (int g = 0; g < G; ++g) {
    for (int d = 0; d < D; ++d) o.Vt[(size_t)g * CA_LL_DMAX + d] = q.V[hidx(h->layout, g, d, G, D)];
    for (int c = 0; c < C && (NZ || q.compact); ++c) {
      const double v = q.E[hidx(h->layout, g, c, G, C)];
      if (NZ) o.Ez[((size_t)(c / NZ) * Gp + g) * NZ + c % NZ] = v;
      if (q.compact) o.Ec[(size_t)g * C + c] = v;
    }
  }
}
// the operands on the device (null where one is empty)
struct ca_ll_dev { double *tab, *logz0, *Ut, *Vt, *Ez, *Ec, *lgt; unsigned* zm; };
ca_ll_dev upload_operands(ca_call_mem& mem, const ca_ll_operands& o) {
  auto up = [&](const std::vector<double>& v) { return v.empty() ? nullptr : mem.upload(v); };
  ca_ll_dev d;
  d.tab = up(o.tab); d.logz0 = up(o.logz0); d.Ut = up(o.Ut); d.Vt = up(o.Vt); d.Ez = up(o.Ez); d.Ec = up(o.Ec); d.lgt = up(o.lgt);
  d.zm = mem.upload(o.zmask);
  return d;
}
// the sweep of one batch against the table: part[segment][cell][column], lgpart[segment][cell]
int sweep_batch(ca_engine* h, const ca_ll_operands& op, const ca_ll_dev& dev, double* part, double* lgpart, int64_t n_lo, int64_t n_cnt) {
  ca_ll_ops o;
  o.tab = dev.tab; o.zmask = dev.zm; o.lgtab = dev.lgt; o.part = part; o.lgpart = lgpart; o.n_lo = n_lo; o.n_cnt = n_cnt; o.NC = op.NC; o.ngrp = op.ngrp;
  return launch_clone_ll(h, o);
}

// p_y_on_c (R/inference-tflow.R:288-296) at a fit's point estimates on the resident matrix: ll[n][c] for every cell and clone (include/clonealign_hip.h has the
// formula and the rules).
// ONE body serves ca_clone_loglik and ca_clone_pair_loglik: the pair call runs the same launches over its cell range -- its ll is ca_clone_loglik's bit for bit,
// and the pair-independent pieces (sum y eta, the lgamma sum, log Z) are those launches' -- and then, per batch, k_pair_cell and k_pair_ll (D > 0) or the
// table sweep of k_clone_ll with k_pair_tab_finish (D = 0).  ca_clone_loglik_dm is a third caller: after the same launches, per batch, k_dm_cell and k_dm_ll (every D).
// ca_clone_mixture is a fourth: after the same launches, per batch, k_pair_cell (log Z and base, every D), k_mix_list and k_mix_rounds (ca_k_mixture.hip.h).
struct ca_pair_req { const double* weights; int W; double* pair_ll; };   // the pair part of a call: W weights in (0, 1), the output cell_cnt x (M W)
struct ca_dm_req { const double* conc; int K; double* dm_ll; };          // the Dirichlet-multinomial part of a call: K concentrations > 0, the output cell_cnt x (C K)
// the mixture part of a call (ca_clone_mixture): the start (cell_cnt x C on the simplex, or null: uniform), the rounds' settings, the outputs (grad may be null)
struct ca_mix_req { const double* start; int max_iter; double tol; double *weights, *grad, *mix_ll, *bound; int32_t* rounds; };
int clone_ll_impl(ca_engine* h, const char* who, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, int64_t c_lo, int64_t c_cnt, double* ll,
                  const ca_pair_req* pq, const ca_dm_req* dq = nullptr, const ca_mix_req* mq = nullptr) {
  const std::string pre = std::string(who) + ": ";
  if (D < 0 || D > CA_LL_DMAX) { h->err = pre + "D = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]"; return CA_ERR_INVALID; }   // (the same on every rank: no collective)
  if (D > 0 && (!U || !V)) { h->err = pre + "D = " + std::to_string(D) + " needs both U (cells x D) and V (genes x D)"; return CA_ERR_INVALID; }
  const int G = h->G, Gp = h->Gp, C = h->C, nseg = h->nseg;
  const int W = pq ? pq->W : 0;
  if (pq) {   // (the same on every rank as well)
    if (C < 2) { h->err = pre + "C = " + std::to_string(C) + " clones: a pair needs at least 2"; return CA_ERR_INVALID; }
    if (W < 1 || W > CA_PLL_WMAX) { h->err = pre + "n_weights = " + std::to_string(W) + " is outside [1, " + std::to_string(CA_PLL_WMAX) + "]"; return CA_ERR_INVALID; }
    if (!pq->weights) { h->err = pre + "weights is NULL"; return CA_ERR_INVALID; }
    for (int i = 0; i < W; ++i)
      if (!std::isfinite(pq->weights[i]) || !(pq->weights[i] > 0.0 && pq->weights[i] < 1.0)) {
        h->err = pre + "weight " + std::to_string(i) + " is " + std::to_string(pq->weights[i]) + ": not inside the open interval (0, 1)";
        return CA_ERR_INVALID;
      }
  }
  const int K = dq ? dq->K : 0, CK = C * K;
  double phi_max = 0.0;
  if (dq) {   // (the same on every rank as well)
    if (K < 1 || K > CA_DM_KMAX) { h->err = pre + "n_conc = " + std::to_string(K) + " is outside [1, " + std::to_string(CA_DM_KMAX) + "]"; return CA_ERR_INVALID; }
    if (!dq->conc) { h->err = pre + "conc is NULL"; return CA_ERR_INVALID; }
    for (int i = 0; i < K; ++i) {
      const double v = dq->conc[i];
      if (!std::isfinite(v) || !(v > 0.0)) { h->err = pre + "concentration " + std::to_string(i) + " is " + std::to_string(v) + ": not finite and > 0"; return CA_ERR_INVALID; }
      if (v > CA_DM_PHI_MAX) { h->err = pre + "concentration " + std::to_string(i) + " is above 1e300: lgamma of it overflows"; return CA_ERR_INVALID; }
      phi_max = std::max(phi_max, v);
    }
  }
  if (mq) {   // (the same on every rank as well; the start's rows are the rank's own and join the verdict below)
    if (C > CA_MIX_CMAX) { h->err = pre + "C = " + std::to_string(C) + " clones: a mixture takes at most " + std::to_string(CA_MIX_CMAX); return CA_ERR_INVALID; }
    if (mq->max_iter < 0) { h->err = pre + "max_iter = " + std::to_string(mq->max_iter) + " is negative"; return CA_ERR_INVALID; }
    if (!std::isfinite(mq->tol) || mq->tol < 0.0) { h->err = pre + "tol_nats = " + std::to_string(mq->tol) + " is negative or not finite"; return CA_ERR_INVALID; }
  }
  HIPCK(h, hipSetDevice(h->device));
  const int MP = C * (C - 1) / 2, MW = MP * W;
  // the contraction's operands (D > 0): E in groups of NZ clone columns; the pair and Dirichlet-multinomial parts read E compact
  const int NZ = C <= 8 ? 8 : C <= 16 ? 16 : 32, ngz = cdiv(C, NZ), nzt = ngz * NZ, nzc = cdiv(G, CA_LL_ZCHUNK);
  ca_ll_operands op;
  ll_operands(h, ca_ll_req{E, V, D, {{U, D, "U", "factor"}, {nullptr, 0, "", ""}}, c_lo, c_cnt, with_const != 0, false, NZ, pq != nullptr || dq != nullptr || mq != nullptr}, op);
  std::string& bad = op.bad;
  const int nct = op.nct;
  // the pair part's operands; for D = 0 the table log(A P_ga + B P_gb) of M W columns in groups of NP, its both-zero masks and the slots' shifts
  // lz = min(log Z_a, log Z_b)
  ca_ll_operands pt;   // (the table route's sweep: tab, zmask, NC, ngrp)
  pt.NC = MW <= 8 ? 8 : MW <= 16 ? 16 : 32; pt.ngrp = pq ? cdiv(MW, pt.NC) : 0; pt.nct = pt.ngrp * pt.NC;
  const int NP = pt.NC, nctp = pt.nct;
  std::vector<double> wts, slot_lz, cv;   // (cv: the concentrations of a Dirichlet-multinomial call)
  if (dq) cv.assign(dq->conc, dq->conc + K);
  if (pq && bad.empty()) {
    wts.assign(pq->weights, pq->weights + W);
    if (D == 0) {
      pt.tab.assign((size_t)pt.ngrp * Gp * NP, 0.0); pt.zmask.assign((size_t)pt.ngrp * Gp, 0u); slot_lz.assign((size_t)MW, 0.0);
      int j = 0;
      for (int a = 0; a < C; ++a)
        for (int b = a + 1; b < C; ++b)
          for (int wi = 0; wi < W; ++wi, ++j) {
            const double lz = std::min(op.logz0[(size_t)a], op.logz0[(size_t)b]), w = wts[(size_t)wi];
            const double A = w * std::exp(lz - op.logz0[(size_t)a]), B = (1.0 - w) * std::exp(lz - op.logz0[(size_t)b]);
            slot_lz[(size_t)j] = lz;
            const int grp = j / NP, jc = j % NP;
            for (int g = 0; g < G; ++g) {
              const double v = std::fma(A, op.Ec[(size_t)g * C + a], B * op.Ec[(size_t)g * C + b]);
              if (v > 0.0) pt.tab[((size_t)grp * Gp + g) * NP + jc] = std::log(v);
              else pt.zmask[(size_t)grp * Gp + g] |= 1u << jc;
            }
          }
    }
  }
  std::vector<double> st;   // (the start of a mixture call, row-major)
  if (mq && mq->start && bad.empty()) {
    st.resize((size_t)(c_cnt * C));
    for (int64_t i = 0; i < c_cnt && bad.empty(); ++i) {
      double sum = 0.0;
      for (int c = 0; c < C; ++c) {
        const double v = mq->start[hidx(h->layout, i, c, c_cnt, C)];
        if (!std::isfinite(v) || v < 0.0) { bad = "start has a negative or non-finite entry (cell " + std::to_string(c_lo + i) + ", clone " + std::to_string(c) + ")"; break; }
        st[(size_t)(i * C + c)] = v;
        sum += v;
      }
      if (bad.empty() && !(std::fabs(sum - 1.0) <= 1e-9)) bad = "the start of cell " + std::to_string(c_lo + i) + " sums to " + std::to_string(sum) + ": off 1 by more than 1e-9";
    }
  }
  CACK(agree_on_verdict(h, bad));
  if (!bad.empty()) { h->err = pre + bad; return CA_ERR_INVALID; }
  if (c_cnt == 0) return CA_OK;
  // cells in batches, so that the partial slabs stay below a quarter of a gigabyte; a mixture call adds its list slab, up to Gp entries of (gene, y, r, r^2 / y) a cell
  const int64_t mix_cell = mq ? ((int64_t)3 * C + 3) * (int64_t)sizeof(double) + (int64_t)Gp * (3 * (int64_t)sizeof(double) + (int64_t)sizeof(int)) + 2 * (int64_t)sizeof(int) : 0;
  const int64_t per_cell = mix_cell + ((int64_t)nseg * (nct + 1) + (D > 0 ? (int64_t)nzc * (nzt + 1) : 0) + (pq ? (int64_t)C + 1 + MW + (D == 0 ? (int64_t)nseg * nctp : 0) : 0) + (dq ? (int64_t)C + 1 + K + CK : 0)) * (int64_t)sizeof(double);
  const int64_t NB = cells_per_batch(c_cnt, per_cell, CA_LL_BUDGET);
  ca_rows_out o_ll(h, ll, c_cnt, C), o_pair(h, pq ? pq->pair_ll : nullptr, c_cnt, MW), o_dm(h, dq ? dq->dm_ll : nullptr, c_cnt, CK);
  ca_rows_out o_mw(h, mq ? mq->weights : nullptr, c_cnt, C), o_mg(h, mq ? mq->grad : nullptr, c_cnt, C);
  ca_call_mem mem(h);
  const ca_ll_dev dev = upload_operands(mem, op);
  double* part = mem.alloc<double>((int64_t)nseg * NB * nct);
  double* lgpart = with_const ? mem.alloc<double>((int64_t)nseg * NB) : nullptr;
  double* zpart = D > 0 ? mem.alloc<double>((int64_t)nzc * NB * nzt) : nullptr;
  double* mpart = D > 0 ? mem.alloc<double>((int64_t)nzc * NB) : nullptr;
  double* ll_d = mem.alloc<double>(h->N * C);
  double* lzc_d = pq || dq || mq ? mem.alloc<double>(NB * C) : nullptr;
  double *wts_d = nullptr, *slz_d = nullptr, *base_d = nullptr, *ppart = nullptr, *pll_d = nullptr;
  ca_ll_dev ptd{};
  if (pq) {
    wts_d = mem.upload(wts);
    if (D == 0) { ptd.tab = mem.upload(pt.tab); ptd.zm = mem.upload(pt.zmask); slz_d = mem.upload(slot_lz); ppart = mem.alloc<double>((int64_t)nseg * NB * nctp); }
    base_d = mem.alloc<double>(NB);
    pll_d = mem.alloc<double>(NB * MW);
  }
  double *conc_d = nullptr, *mrow_d = nullptr, *head_d = nullptr, *dll_d = nullptr;
  if (dq) {
    conc_d = mem.upload(cv);
    mrow_d = mem.alloc<double>(NB);
    head_d = mem.alloc<double>(NB * K);
    dll_d = mem.alloc<double>(NB * CK);
  }
  ca_mix_ops mx{};
  const double* st_d = nullptr;
  if (mq) {
    if (!st.empty()) st_d = mem.upload(st);
    base_d = mem.alloc<double>(NB);
    mx.lg = mem.alloc<int>(NB * Gp); mx.ly = mem.alloc<double>(NB * Gp); mx.lr = mem.alloc<double>(NB * Gp); mx.lq = mem.alloc<double>(NB * Gp); mx.ln = mem.alloc<int>(NB);
    mx.w = mem.alloc<double>(NB * C); mx.g = mem.alloc<double>(NB * C); mx.mll = mem.alloc<double>(NB); mx.bnd = mem.alloc<double>(NB); mx.rnd = mem.alloc<int>(NB);
    mx.Ec = dev.Ec; mx.lzc = lzc_d; mx.base = base_d; mx.max_iter = mq->max_iter; mx.tol = mq->tol;
  }
  if (mem.rc != CA_OK) return mem.rc;
  for (int64_t n_lo = c_lo; n_lo < c_lo + c_cnt; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, c_lo + c_cnt - n_lo);
    CACK(sweep_batch(h, op, dev, part, lgpart, n_lo, n_cnt));
    if (D > 0) {
      ca_llz_ops z;
      z.Ut = dev.Ut; z.Vt = dev.Vt; z.Ez = dev.Ez; z.zpart = zpart; z.mpart = mpart; z.n_lo = n_lo; z.n_cnt = n_cnt; z.NC = NZ; z.ngrp = ngz; z.nzc = nzc;
      CACK(launch_clone_ll_z(h, z));
    }
    if (ll) {
      hipLaunchKernelGGL(k_clone_ll_finish, dim3((unsigned)cdiv(n_cnt * C, CA_TB)), dim3(CA_TB), 0, h->stream, part, lgpart, zpart, mpart, dev.logz0, dev.Ut, h->s64, ll_d, n_lo, n_cnt, C,
                         (int)D, (int)nseg, nct, nzc, nzt);
      HIPCK(h, hipGetLastError());
    }
    if (pq) {
      hipLaunchKernelGGL(k_pair_cell, dim3((unsigned)cdiv(n_cnt * (C + 1), CA_TB)), dim3(CA_TB), 0, h->stream, part, lgpart, zpart, mpart, dev.logz0, dev.Ut, h->s64, lzc_d, base_d, n_lo, n_cnt,
                         C, (int)D, (int)nseg, nct, nzc, nzt);
      HIPCK(h, hipGetLastError());
      if (D > 0) {
        ca_pll_ops p;
        p.Ec = dev.Ec; p.lzc = lzc_d; p.base = base_d; p.wts = wts_d; p.out = pll_d; p.n_lo = n_lo; p.n_cnt = n_cnt; p.W = W; p.MW = MW;
        CACK(launch_pair_ll(h, p));
      } else {   // the table route: no lgamma sum here (base has it)
        CACK(sweep_batch(h, pt, ptd, ppart, nullptr, n_lo, n_cnt));
        hipLaunchKernelGGL(k_pair_tab_finish, dim3((unsigned)cdiv(n_cnt * MW, CA_TB)), dim3(CA_TB), 0, h->stream, ppart, base_d, slz_d, h->s64, pll_d, n_lo, n_cnt, MW, (int)nseg, nctp);
        HIPCK(h, hipGetLastError());
      }
      HIPCK(h, hipMemcpyAsync(o_pair.p + (size_t)(n_lo - c_lo) * MW, pll_d, (size_t)n_cnt * MW * sizeof(double), hipMemcpyDeviceToHost, h->stream));   // (in stream order: before the next batch overwrites it)
    }
    if (mq) {   // log Z and base are the pair part's (k_pair_cell, every D: logz0 at D = 0), then the list and the rounds
      hipLaunchKernelGGL(k_pair_cell, dim3((unsigned)cdiv(n_cnt * (C + 1), CA_TB)), dim3(CA_TB), 0, h->stream, part, lgpart, zpart, mpart, dev.logz0, dev.Ut, h->s64, lzc_d, base_d, n_lo, n_cnt,
                         C, (int)D, (int)nseg, nct, nzc, nzt);
      HIPCK(h, hipGetLastError());
      mx.start = st_d ? st_d + (size_t)(n_lo - c_lo) * C : nullptr; mx.n_lo = n_lo; mx.n_cnt = n_cnt;
      CACK(launch_mix(h, mx));
      const size_t row = (size_t)(n_lo - c_lo);   // (the copies run in stream order: before the next batch overwrites the buffers)
      HIPCK(h, hipMemcpyAsync(o_mw.p + row * C, mx.w, (size_t)n_cnt * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      if (mq->grad) HIPCK(h, hipMemcpyAsync(o_mg.p + row * C, mx.g, (size_t)n_cnt * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCK(h, hipMemcpyAsync(mq->mix_ll + row, mx.mll, (size_t)n_cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCK(h, hipMemcpyAsync(mq->bound + row, mx.bnd, (size_t)n_cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCK(h, hipMemcpyAsync(mq->rounds + row, mx.rnd, (size_t)n_cnt * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    }
    if (dq) {
      hipLaunchKernelGGL(k_dm_cell, dim3((unsigned)cdiv(n_cnt * (C + K), CA_TB)), dim3(CA_TB), 0, h->stream, lgpart, zpart, mpart, dev.logz0, h->s64, conc_d, lzc_d, mrow_d, head_d, n_lo,
                         n_cnt, C, K, (int)D, (int)nseg, nzc, nzt);
      HIPCK(h, hipGetLastError());
      ca_dml_ops p;
      p.Ec = dev.Ec; p.lzc = lzc_d; p.mrow = mrow_d; p.head = head_d; p.conc = conc_d; p.Ut = D > 0 ? dev.Ut : nullptr; p.Vt = dev.Vt; p.out = dll_d; p.n_lo = n_lo; p.n_cnt = n_cnt;
      p.K = K; p.CK = CK; p.ysmall = phi_max <= CA_DM_PHI_PROD ? CA_DM_YSMALL : 0;
      CACK(launch_dm_ll(h, p));
      HIPCK(h, hipMemcpyAsync(o_dm.p + (size_t)(n_lo - c_lo) * CK, dll_d, (size_t)n_cnt * CK * sizeof(double), hipMemcpyDeviceToHost, h->stream));   // (in stream order: before the next batch overwrites it)
    }
  }
  if (ll) HIPCK(h, hipMemcpyAsync(o_ll.p, ll_d + (size_t)c_lo * C, (size_t)c_cnt * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipStreamSynchronize(h->stream));
  o_ll.finish(); o_pair.finish(); o_dm.finish(); o_mw.finish(); o_mg.finish();
  return CA_OK;
}
}  // namespace
}  // extern "C++"

int ca_clone_loglik(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, double* ll) {
  if (!h || !E || !ll) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  return clone_ll_impl(h, "ca_clone_loglik", E, U, V, D, with_const, 0, h->N, ll, nullptr);
}

// The log-likelihood of the resident cells [cell_lo, cell_lo + cell_cnt) under every mixture of two clones and every weight of the grid (a heterotypic doublet;
// include/clonealign_hip.h has the formula and the rules).  ca_clone_loglik's launches, then the pair's own.
int ca_clone_pair_loglik(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, const double* weights, int32_t n_weights, int64_t cell_lo,
                         int64_t cell_cnt, double* ll, double* pair_ll) {
  if (!h) return CA_ERR_INVALID;
  if (!E || !pair_ll) { h->err = std::string("ca_clone_pair_loglik: ") + (!E ? "E" : "pair_ll") + " is NULL"; return CA_ERR_INVALID; }
  CA_NOT_IN_RUN(h);
  ca_pair_req pq{weights, (int)n_weights, pair_ll};
  return clone_ll_impl(h, "ca_clone_pair_loglik", E, U, V, D, with_const, cell_lo, cell_cnt, ll, &pq);
}

// The maximum-likelihood mixture of all clones for each of the resident cells [cell_lo, cell_lo + cell_cnt): simplex weights by projected Newton, with a certified
// bound in nats (include/clonealign_hip.h has the formulas, the round and the rules; ca_k_mixture.hip.h the kernels).  ca_clone_loglik's launches, k_pair_cell's
// log Z and base, then the list and the rounds.
int ca_clone_mixture(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, const double* start, int32_t max_iter, double tol_nats,
                     int64_t cell_lo, int64_t cell_cnt, double* ll, double* weights, double* grad, double* mix_ll, double* bound_nats, int32_t* rounds) {
  if (!h) return CA_ERR_INVALID;
  {
    const char* null_arg = !E ? "E" : !weights ? "weights" : !mix_ll ? "mix_ll" : !bound_nats ? "bound_nats" : !rounds ? "rounds" : nullptr;
    if (null_arg) { h->err = std::string("ca_clone_mixture: ") + null_arg + " is NULL"; return CA_ERR_INVALID; }
  }
  CA_NOT_IN_RUN(h);
  ca_mix_req mq{start, (int)max_iter, tol_nats, weights, grad, mix_ll, bound_nats, rounds};
  return clone_ll_impl(h, "ca_clone_mixture", E, U, V, D, with_const, cell_lo, cell_cnt, ll, nullptr, nullptr, &mq);
}

// The Dirichlet-multinomial log-likelihood of the resident cells [cell_lo, cell_lo + cell_cnt) under every clone at every concentration of the grid (overdispersed
// cell scoring; include/clonealign_hip.h has the formula and the rules, ca_k_dmll.hip.h the kernel).  ca_clone_loglik's launches (ll, the lgamma sums, log Z and
// the max of eta are theirs), then its own.
int ca_clone_loglik_dm(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, const double* conc, int32_t n_conc, int64_t cell_lo,
                       int64_t cell_cnt, double* ll, double* dm_ll) {
  if (!h) return CA_ERR_INVALID;
  if (!E || !conc || !dm_ll) { h->err = std::string("ca_clone_loglik_dm: ") + (!E ? "E" : !conc ? "conc" : "dm_ll") + " is NULL"; return CA_ERR_INVALID; }
  CA_NOT_IN_RUN(h);
  ca_dm_req dq{conc, (int)n_conc, dm_ll};
  return clone_ll_impl(h, "ca_clone_loglik_dm", E, U, V, D, with_const, cell_lo, cell_cnt, ll, nullptr, &dq);
}

// The sufficient statistics of ca_clone_loglik by block of genes for the resident cells [cell_lo, cell_lo + cell_cnt) (include/clonealign_hip.h has the formulas and
// the rules; ca_k_blockll.hip.h the kernels).  The table, the masks and the lgamma table are ca_clone_loglik's.  The host turns the labelling into the RUN LIST
// (maximal ranges of consecutive genes with one label, cut again at the segment boundaries), the chunk list of the contraction (the same ranges cut at every
// CA_LL_ZCHUNK genes of the axis) and the lists block -> runs, block -> chunks in ascending gene order.  The slab is n_runs x cells x (C + D + 2) doubles, so the
// cell batch follows from a fixed byte budget: a chromosome-sorted axis (n_runs about n_blocks + nseg) takes the usual batch, a fully interleaved labelling
// (n_runs = G) small ones.
int ca_clone_loglik_by_block(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, const int32_t* block_of_gene, int32_t n_blocks,
                             int64_t c_lo, int64_t c_cnt, double* A, double* logZ, double* s, double* lg) {
  if (!h) return CA_ERR_INVALID;
  const std::string pre = "ca_clone_loglik_by_block: ";
  {
    const char* null_arg = !E ? "E" : !block_of_gene ? "block_of_gene" : !A ? "A" : !logZ ? "logZ" : !s ? "s" : (with_const && !lg) ? "lg (with_const != 0)" : nullptr;
    if (null_arg) { h->err = pre + null_arg + " is NULL"; return CA_ERR_INVALID; }
  }
  CA_NOT_IN_RUN(h);
  if (D < 0 || D > CA_LL_DMAX) { h->err = pre + "D = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]"; return CA_ERR_INVALID; }   // (the same on every rank: no collective)
  if (D > 0 && (!U || !V)) { h->err = pre + "D = " + std::to_string(D) + " needs both U (cells x D) and V (genes x D)"; return CA_ERR_INVALID; }
  if (n_blocks < 1) { h->err = pre + "n_blocks = " + std::to_string(n_blocks) + " is below 1"; return CA_ERR_INVALID; }
  const int G = h->G, C = h->C, nseg = h->nseg, B = n_blocks;
  for (int g = 0; g < G; ++g)
    if (block_of_gene[g] < 0 || block_of_gene[g] >= B) {
      h->err = pre + "block_of_gene[" + std::to_string(g) + "] = " + std::to_string(block_of_gene[g]) + " is outside [0, " + std::to_string(B) + ")";
      return CA_ERR_INVALID;
    }
  HIPCK(h, hipSetDevice(h->device));
  const int ncol = C + D;
  const int NZ = C <= 8 ? 8 : C <= 16 ? 16 : 32, ngz = cdiv(C, NZ);
  ca_ll_operands op;
  ll_operands(h, ca_ll_req{E, V, D, {{U, D, "U", "factor"}, {nullptr, 0, "", ""}}, c_lo, c_cnt, with_const != 0, false, NZ, false}, op);
  CACK(agree_on_verdict(h, op.bad));
  if (!op.bad.empty()) { h->err = pre + op.bad; return CA_ERR_INVALID; }
  if (c_cnt == 0) return CA_OK;
  // the run list and the chunk list: cuts where the label changes, and at the segment boundaries (runs) or at every CA_LL_ZCHUNK genes (chunks)
  const int segw = 64 * h->VEC;
  std::vector<int> rcut, rseg((size_t)nseg + 1, 0), zcut, run_blk, zk_blk;
  for (int g = 0; g < G; ++g) {
    const bool change = g == 0 || block_of_gene[g] != block_of_gene[g - 1];
    if (g % segw == 0) rseg[(size_t)(g / segw)] = (int)rcut.size();
    if (change || g % segw == 0) { rcut.push_back(g); run_blk.push_back(block_of_gene[g]); }
    if (change || g % CA_LL_ZCHUNK == 0) { zcut.push_back(g); zk_blk.push_back(block_of_gene[g]); }
  }
  const int n_runs = (int)rcut.size(), nzk = (int)zcut.size();
  rseg[(size_t)nseg] = n_runs;
  rcut.push_back(G); rcut.push_back(INT32_MAX);   // (the kernel reads one entry past the run it has just finished)
  zcut.push_back(G);
  // block -> its runs / chunks in ascending gene order (a counting sort keeps the order)
  auto by_block = [&](const std::vector<int>& blk, std::vector<int>& ptr, std::vector<int>& list) {
    ptr.assign((size_t)B + 1, 0); list.resize(blk.size());
    for (int b : blk) ++ptr[(size_t)b + 1];
    for (int b = 0; b < B; ++b) ptr[(size_t)b + 1] += ptr[(size_t)b];
    std::vector<int> at(ptr.begin(), ptr.end() - 1);
    for (size_t i = 0; i < blk.size(); ++i) list[(size_t)at[(size_t)blk[i]]++] = (int)i;
  };
  std::vector<int> brp, bruns, bzp, bzk;
  by_block(run_blk, brp, bruns);
  by_block(zk_blk, bzp, bzk);
  // D = 0: log Z of a block does not depend on the cell -- a float64 sum over the block's genes in ascending order, -inf where it is 0 (an empty block included)
  std::vector<double> logz0b;
  if (D == 0) {
    std::vector<double> sum((size_t)B * C, 0.0);
    for (int g = 0; g < G; ++g)
      for (int c = 0; c < C; ++c) sum[(size_t)block_of_gene[g] * C + c] += E[hidx(h->layout, g, c, G, C)];
    logz0b.resize(sum.size());
    for (size_t i = 0; i < sum.size(); ++i) logz0b[i] = sum[i] > 0.0 ? std::log(sum[i]) : -INFINITY;
  }
  // cells in batches under the byte budget: the two slabs and the batch's outputs
  const int64_t BC = (int64_t)B * C;
  const int64_t per_cell = ((int64_t)n_runs * (ncol + 2) + (D > 0 ? (int64_t)nzk * (C + 1) : 0) + 2 * BC + 2 * B) * (int64_t)sizeof(double);
  const int64_t NB = cells_per_batch(c_cnt, per_cell, CA_BLL_BUDGET);
  ca_rows_out oA(h, A, c_cnt, BC), oZ(h, logZ, c_cnt, BC), oS(h, s, c_cnt, B), oL(h, with_const ? lg : nullptr, c_cnt, B);
  ca_call_mem mem(h);
  const ca_ll_dev dev = upload_operands(mem, op);
  const int *rcut_d = mem.upload(rcut), *rseg_d = mem.upload(rseg), *brp_d = mem.upload(brp), *bruns_d = mem.upload(bruns);
  const int *zcut_d = nullptr, *bzp_d = nullptr, *bzk_d = nullptr;
  const double* lzb_d = nullptr;
  if (D > 0) { zcut_d = mem.upload(zcut); bzp_d = mem.upload(bzp); bzk_d = mem.upload(bzk); }
  else lzb_d = mem.upload(logz0b);
  double* part = mem.alloc<double>((int64_t)n_runs * (ncol + 2) * NB);   // (the columns in use: the padding of the last group is not stored)
  double* zpart = D > 0 ? mem.alloc<double>((int64_t)nzk * (C + 1) * NB) : nullptr;
  double *A_d = mem.alloc<double>(NB * BC), *Z_d = mem.alloc<double>(NB * BC), *S_d = mem.alloc<double>(NB * B), *L_d = with_const ? mem.alloc<double>(NB * B) : nullptr;
  if (mem.rc != CA_OK) return mem.rc;
  for (int64_t n_lo = c_lo; n_lo < c_lo + c_cnt; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, c_lo + c_cnt - n_lo);
    ca_bll_ops o;
    o.tab = dev.tab; o.zmask = dev.zm; o.lgtab = dev.lgt; o.rcut = rcut_d; o.rseg = rseg_d; o.part = part; o.n_lo = n_lo; o.n_cnt = n_cnt; o.NC = op.NC; o.ngrp = op.ngrp; o.nuse = ncol;
    CACK(launch_block_ll(h, o));
    if (D > 0) {
      ca_bllz_ops z;
      z.Ut = dev.Ut; z.Vt = dev.Vt; z.Ez = dev.Ez; z.zcut = zcut_d; z.zpart = zpart; z.n_lo = n_lo; z.n_cnt = n_cnt; z.NC = NZ; z.ngrp = ngz; z.nzk = nzk;
      CACK(launch_block_ll_z(h, z));
    }
    hipLaunchKernelGGL(k_block_ll_finish, dim3((unsigned)cdiv(n_cnt * BC, CA_TB)), dim3(CA_TB), 0, h->stream, part, zpart, lzb_d, dev.Ut, brp_d, bruns_d, bzp_d, bzk_d, A_d, Z_d, S_d, L_d,
                       n_lo, n_cnt, (int)B, C, (int)D);
    HIPCK(h, hipGetLastError());
    const size_t row = (size_t)(n_lo - c_lo);   // (the copies run in stream order: before the next batch overwrites the buffers)
    HIPCK(h, hipMemcpyAsync(oA.p + row * BC, A_d, (size_t)(n_cnt * BC) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(oZ.p + row * BC, Z_d, (size_t)(n_cnt * BC) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(oS.p + row * B, S_d, (size_t)(n_cnt * B) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (with_const) HIPCK(h, hipMemcpyAsync(oL.p + row * B, L_d, (size_t)(n_cnt * B) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCK(h, hipStreamSynchronize(h->stream));
  oA.finish(); oZ.finish(); oS.finish(); oL.finish();
  return CA_OK;
}

extern "C++" {
namespace {
// What ca_project_cells and ca_clone_evidence share before their rounds.  The refusal of K, P or the iteration's settings, or "" (the same on every rank: no collective):
std::string newton_args_refusal(int K, int P, const double* V, const double* X, int max_iter, double tol, double max_step) {
  const int D = K + P;
  if (K < 0 || K > CA_PROJ_KMAX) return "K = " + std::to_string(K) + " is outside [0, " + std::to_string(CA_PROJ_KMAX) + "] (the device limit of the moment kernel)";
  if (P < 0 || D > CA_LL_DMAX) return "K + P = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]";
  if (D > 0 && !V) return "K + P = " + std::to_string(D) + " needs V (genes x (K + P))";
  if (P > 0 && !X) return "P = " + std::to_string(P) + " needs X (cells x P)";
  if (max_iter < 0) return "max_iter = " + std::to_string(max_iter) + " is negative";
  if (!(tol > 0.0) || !std::isfinite(tol)) return "tol = " + std::to_string(tol) + " is not a positive finite number";
  if (!(max_step > 0.0) || !std::isfinite(max_step)) return "max_step = " + std::to_string(max_step) + " is not a positive finite number";
  return "";
}
// and the ONE sweep over the matrix of a batch: k_clone_ll against [log E | V], then k_proj_sums (A, B and the constant)
int sweep_sums_batch(ca_engine* h, const ca_ll_operands& op, const ca_ll_dev& dev, double* part, double* lgpart, double* A_d, double* B_d, int D, int64_t n_lo, int64_t n_cnt) {
  CACK(sweep_batch(h, op, dev, part, lgpart, n_lo, n_cnt));
  hipLaunchKernelGGL(k_proj_sums, dim3((unsigned)cdiv(n_cnt * (h->C + D), CA_TB)), dim3(CA_TB), 0, h->stream, part, lgpart, h->s64, A_d, B_d, n_lo, n_cnt, h->C, D, (int)h->nseg, op.nct);
  HIPCK(h, hipGetLastError());
  return CA_OK;
}
}  // namespace
}  // extern "C++"

// Per-cell MAP psi and the clone posterior at it for the resident cells under a fit's gene-level parameters (include/clonealign_hip.h has the algorithm and the
// rules).  ONE sweep over the matrix (k_clone_ll against [log E | V]: A, B and the constant), then rounds of two launches that never read it, queued back to
// back; every few rounds the host reads the frozen flags and stops queuing when no cell is left -- freezing is per cell, so WHEN the host looks changes no result.
int ca_project_cells(ca_handle h, const double* E, const double* V, int32_t K, int32_t P, const double* X, const double* log_prior, const double* psi_start,
                     int32_t with_const, int32_t max_iter, double tol, double max_step, double* psi, double* ll, double* clone_probs, double* objective,
                     int32_t* rounds, uint8_t* converged) {
  if (!h || !E || !ll || !clone_probs || !objective || !rounds || !converged || (K > 0 && !psi)) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  const int D = K + P;
  auto refuse = [&](const std::string& why) { h->err = "ca_project_cells: " + why; return CA_ERR_INVALID; };
  { const std::string why = newton_args_refusal(K, P, V, X, max_iter, tol, max_step); if (!why.empty()) return refuse(why); }
  const int poll_set = (with_const >> 8) & 0xFF, poll = poll_set ? poll_set : 4;   // rounds between two looks at the frozen flags (255: practically never)
  const bool lgc = (with_const & 1) != 0;
  HIPCK(h, hipSetDevice(h->device));
  const int64_t N = h->N; const int G = h->G, C = h->C, nseg = h->nseg;
  // the moments' operands: U = [psi | x] and V padded to CA_LL_DMAX factors, E in groups of NZ clone columns
  const int NM = 1 + K + K * (K + 1) / 2;
  const int NZ = (K <= 1 && C > 8) ? 16 : 8, ngz = cdiv(C, NZ), nmt = ngz * NZ * NM, nzc = cdiv(G, CA_LL_ZCHUNK);
  ca_ll_operands op;
  ll_operands(h, ca_ll_req{E, V, D, {{psi_start, K, "psi_start", "factor"}, {X, P, "X", "covariate"}}, 0, N, lgc, true, NZ, false}, op);
  std::string& bad = op.bad;
  std::vector<double> lp;
  if (log_prior && bad.empty()) {
    lp.resize((size_t)N * C);
    for (int64_t n = 0; n < N && bad.empty(); ++n)
      for (int c = 0; c < C; ++c) {
        const double v = log_prior[hidx(h->layout, n, c, N, C)];
        if (std::isnan(v) || v == HUGE_VAL) { bad = "log_prior has a NaN or +inf entry (cell " + std::to_string(n) + ", clone " + std::to_string(c) + "); -inf excludes a clone"; break; }
        lp[(size_t)n * C + c] = v;
      }
  }
  CACK(agree_on_verdict(h, bad));
  if (!bad.empty()) return refuse(bad);
  if (N == 0) return CA_OK;
  // cells in batches, so that the partial slabs stay below a quarter of a gigabyte
  const int64_t NB = cells_per_batch(N, ((int64_t)nseg * (op.nct + 1) + (int64_t)nzc * (nmt + 1)) * (int64_t)sizeof(double), CA_LL_BUDGET);
  ca_rows_out o_ll(h, ll, N, C), o_pr(h, clone_probs, N, C);
  std::vector<double> o_u((size_t)N * CA_LL_DMAX);
  std::vector<int> o_rd((size_t)N);
  std::vector<unsigned char> fr((size_t)NB);
  ca_call_mem mem(h);
  const ca_ll_dev dev = upload_operands(mem, op);
  const double* lp_d = log_prior ? mem.upload(lp) : nullptr;
  double* part = mem.alloc<double>((int64_t)nseg * NB * op.nct);
  double* lgpart = lgc ? mem.alloc<double>((int64_t)nseg * NB) : nullptr;
  double *zpart = mem.alloc<double>((int64_t)nzc * NB * nmt), *mpart = mem.alloc<double>((int64_t)nzc * NB);
  double *A_d = mem.alloc<double>(N * C), *B_d = mem.alloc<double>(N * CA_LL_DMAX), *ll_d = mem.alloc<double>(N * C), *pr_d = mem.alloc<double>(N * C), *obj_d = mem.alloc<double>(N);
  unsigned char *fr_d = mem.alloc<unsigned char>(N), *cv_d = mem.alloc<unsigned char>(N);
  int* rd_d = mem.alloc<int>(N);
  if (mem.rc != CA_OK) return mem.rc;
  HIPCK(h, hipMemsetAsync(B_d, 0, (size_t)N * CA_LL_DMAX * sizeof(double), h->stream));   // (the padding factors)
  HIPCK(h, hipMemsetAsync(fr_d, 0, (size_t)N, h->stream));
  for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
    CACK(sweep_sums_batch(h, op, dev, part, lgpart, A_d, B_d, D, n_lo, n_cnt));
    ca_pm_ops m;
    m.Ut = dev.Ut; m.Vt = dev.Vt; m.Ez = dev.Ez; m.frozen = fr_d; m.zpart = zpart; m.mpart = mpart; m.n_lo = n_lo; m.n_cnt = n_cnt; m.K = K; m.NC = NZ; m.ngrp = ngz; m.nzc = nzc;
    ca_ps_ops s;
    s.zpart = zpart; s.mpart = mpart; s.A = A_d; s.B = B_d; s.lp = lp_d; s.Ut = dev.Ut; s.frozen = fr_d; s.conv = cv_d; s.rounds = rd_d; s.ll = ll_d; s.probs = pr_d; s.obj = obj_d;
    s.n_lo = n_lo; s.n_cnt = n_cnt; s.K = K; s.nzc = nzc; s.nmt = nmt; s.final = 0; s.tol = tol; s.max_step = max_step;
    bool all_frozen = false;
    for (int t = 0; K > 0 && t < max_iter && !all_frozen; ++t) {
      s.round = t;
      CACK(launch_proj_mom(h, m));
      CACK(launch_proj_step(h, s));
      if ((t + 1) % poll == 0 && t + 1 < max_iter) {
        HIPCK(h, hipMemcpyAsync(fr.data(), fr_d + n_lo, (size_t)n_cnt, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        all_frozen = std::find(fr.begin(), fr.begin() + n_cnt, (unsigned char)0) == fr.begin() + n_cnt;
      }
    }
    if (!all_frozen) {   // the cells that never froze (all of them when K = 0 or max_iter = 0): ll and the posterior at the psi they hold
      s.round = K > 0 ? max_iter : 0; s.final = 1;
      CACK(launch_proj_mom(h, m));
      CACK(launch_proj_step(h, s));
    }
  }
  HIPCK(h, hipMemcpyAsync(o_ll.p, ll_d, (size_t)N * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipMemcpyAsync(o_pr.p, pr_d, (size_t)N * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipMemcpyAsync(o_u.data(), dev.Ut, o_u.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipMemcpyAsync(objective, obj_d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipMemcpyAsync(o_rd.data(), rd_d, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipMemcpyAsync(converged, cv_d, (size_t)N, hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipStreamSynchronize(h->stream));
  o_ll.finish(); o_pr.finish();
  for (int64_t n = 0; n < N; ++n) {
    rounds[n] = o_rd[(size_t)n];
    for (int k = 0; k < K; ++k) psi[hidx(h->layout, n, k, N, K)] = o_u[(size_t)n * CA_LL_DMAX + k];
  }
  return CA_OK;
}

// The clone evidence with psi integrated out, per resident cell and clone (include/clonealign_hip.h has the algorithm and the rules; ca_k_evidence.hip.h the
// kernels).  ONE sweep over the matrix, ca_project_cells' (k_clone_ll against [log E | V], k_proj_sums: A, B and the constant); then per batch of cells Newton
// rounds of two launches (k_ev_mom with all moments, k_ev_step) that never read it, queued back to back with the host looking at the pairs' states every few
// rounds -- freezing is per (cell, clone), so WHEN the host looks changes no result -- and the quadrature: k_ev_nodes, ONE k_ev_mom over the (clone, node) slots
// (Z0 only), k_ev_reduce.  K = 0 is ca_clone_loglik itself.
int ca_clone_evidence(ca_handle h, const double* E, const double* V, int32_t K, int32_t P, const double* X, const double* psi_start, int32_t with_const,
                      int32_t n_nodes, const double* nodes, const double* weights, int32_t max_iter, double tol, double max_step, double* evidence, double* laplace,
                      double* psi_mode, double* psi_prec, int32_t* rounds, uint8_t* converged) {
  if (!h || !E || !evidence || !laplace || !rounds || !converged || (K > 0 && (!psi_mode || !psi_prec))) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  const int D = K + P, Q = n_nodes;
  auto refuse = [&](const std::string& why) { h->err = "ca_clone_evidence: " + why; return CA_ERR_INVALID; };
  { const std::string why = newton_args_refusal(K, P, V, X, max_iter, tol, max_step); if (!why.empty()) return refuse(why); }
  if (Q < 1 || Q > CA_EV_QMAX) return refuse("n_nodes = " + std::to_string(Q) + " is outside [1, " + std::to_string(CA_EV_QMAX) + "]");
  if (!nodes && K > 0) return refuse("nodes is NULL (n_nodes x K)");
  if (!weights) return refuse("weights is NULL (n_nodes)");
  {
    double wsum = 0.0;
    for (int q = 0; q < Q; ++q) {
      for (int k = 0; k < K; ++k)
        if (!std::isfinite(nodes[(size_t)q * K + k])) return refuse("node " + std::to_string(q) + " has a non-finite coordinate (factor " + std::to_string(k) + ")");
      if (!std::isfinite(weights[q]) || !(weights[q] > 0.0)) return refuse("weight " + std::to_string(q) + " is " + std::to_string(weights[q]) + ": not positive and finite");
      wsum += weights[q];
    }
    if (!(std::fabs(wsum - 1.0) <= 1e-12)) return refuse("the weights sum to " + std::to_string(wsum) + ": off 1 by more than 1e-12");
  }
  const int poll_set = (with_const >> 8) & 0xFF, poll = poll_set ? poll_set : 4;   // rounds between two looks at the pairs' states (255: practically never)
  const bool lgc = (with_const & 1) != 0;
  const int64_t N = h->N; const int G = h->G, C = h->C, nseg = h->nseg;
  if (K == 0) {   // nothing to integrate: ca_clone_loglik's value, bit for bit (its launches, its collective)
    std::vector<double> ll((size_t)N * C + 1);
    const int rc = clone_ll_impl(h, "ca_clone_evidence", E, X, V, P, lgc ? 1 : 0, 0, N, ll.data(), nullptr);
    if (rc != CA_OK) return rc;
    for (int64_t n = 0; n < N; ++n)
      for (int c = 0; c < C; ++c) {
        const size_t i = hidx(h->layout, n, c, N, C);
        evidence[i] = laplace[i] = ll[i];
        rounds[i] = 0;
        converged[i] = ll[i] > -HUGE_VAL ? 1 : 0;
      }
    return CA_OK;
  }
  HIPCK(h, hipSetDevice(h->device));
  const int NM = 1 + K + K * (K + 1) / 2, NH = K * (K + 1) / 2, nzc = cdiv(G, CA_LL_ZCHUNK), CQ = C * Q;
  ca_ll_operands op;   // U = [start | x]
  ll_operands(h, ca_ll_req{E, V, D, {{psi_start, K, "psi_start", "factor"}, {X, P, "X", "covariate"}}, 0, N, lgc, true, 0, true}, op);
  CACK(agree_on_verdict(h, op.bad));
  if (!op.bad.empty()) return refuse(op.bad);
  if (N == 0) return CA_OK;
  std::vector<double> nd(nodes, nodes + (size_t)Q * K), wt(weights, weights + Q);
  // cells in batches, so that the partial slabs stay below a quarter of a gigabyte
  const int zcols = std::max(C * NM, CQ), mcols = CQ;   // (one pair of slabs serves the rounds and the quadrature pass)
  const int64_t per_cell = ((int64_t)nseg * (op.nct + 1) + (int64_t)nzc * (zcols + mcols) + (int64_t)CQ * K + (int64_t)C * (K + NH + 5)) * (int64_t)sizeof(double);
  const int64_t NB = cells_per_batch(N, per_cell, CA_LL_BUDGET);
  std::vector<double> b_ev((size_t)NB * C), b_lap((size_t)NB * C), b_ps((size_t)NB * C * K), b_H((size_t)NB * C * NH);
  std::vector<int> b_rd((size_t)NB * C);
  std::vector<unsigned char> b_cv((size_t)NB * C), fr((size_t)NB * C);
  ca_call_mem mem(h);
  const ca_ll_dev dev = upload_operands(mem, op);
  const double *nd_d = mem.upload(nd), *wt_d = mem.upload(wt);
  double* part = mem.alloc<double>((int64_t)nseg * NB * op.nct);
  double* lgpart = lgc ? mem.alloc<double>((int64_t)nseg * NB) : nullptr;
  double *zpart = mem.alloc<double>((int64_t)nzc * NB * zcols), *mpart = mem.alloc<double>((int64_t)nzc * NB * mcols);
  double *A_d = mem.alloc<double>(N * C), *B_d = mem.alloc<double>(N * CA_LL_DMAX);
  double *ps_d = mem.alloc<double>(NB * C * K), *pq_d = mem.alloc<double>(NB * CQ * K), *fs_d = mem.alloc<double>(NB * C), *H_d = mem.alloc<double>(NB * C * NH);
  double *lap_d = mem.alloc<double>(NB * C), *ev_d = mem.alloc<double>(NB * C);
  unsigned char *fz_d = mem.alloc<unsigned char>(NB * C), *cv_d = mem.alloc<unsigned char>(NB * C);
  int* rd_d = mem.alloc<int>(NB * C);
  if (mem.rc != CA_OK) return mem.rc;
  HIPCK(h, hipMemsetAsync(B_d, 0, (size_t)N * CA_LL_DMAX * sizeof(double), h->stream));   // (the padding factors)
  for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
    CACK(sweep_sums_batch(h, op, dev, part, lgpart, A_d, B_d, D, n_lo, n_cnt));
    ca_evm_ops m;
    m.Ut = dev.Ut; m.Vt = dev.Vt; m.Ec = dev.Ec; m.ps = ps_d; m.fz = fz_d; m.zpart = zpart; m.mpart = mpart; m.n_lo = n_lo; m.n_cnt = n_cnt; m.K = K; m.Q = 1; m.nslot = C; m.nzc = nzc;
    m.full = true;
    ca_evs_ops s;
    s.zpart = zpart; s.mpart = mpart; s.A = A_d; s.B = B_d; s.Ut = dev.Ut; s.nodes = nd_d; s.wts = wt_d; s.ps = ps_d; s.pq = pq_d; s.fz = fz_d; s.conv = cv_d; s.rounds = rd_d;
    s.fstar = fs_d; s.Hm = H_d; s.lap = lap_d; s.ev = ev_d; s.n_lo = n_lo; s.n_cnt = n_cnt; s.K = K; s.Q = Q; s.nzc = nzc; s.round = 0; s.final = 0; s.tol = tol; s.max_step = max_step;
    CACK(launch_ev_fin(h, s, CA_EV_INIT));
    bool all_frozen = false;
    for (int t = 0; t < max_iter && !all_frozen; ++t) {
      s.round = t;
      CACK(launch_ev_mom(h, m));
      CACK(launch_ev_fin(h, s, CA_EV_STEP));
      if ((t + 1) % poll == 0 && t + 1 < max_iter) {
        HIPCK(h, hipMemcpyAsync(fr.data(), fz_d, (size_t)n_cnt * C, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        all_frozen = std::find(fr.begin(), fr.begin() + n_cnt * C, (unsigned char)CA_EV_LIVE) == fr.begin() + n_cnt * C;
      }
    }
    if (!all_frozen) {   // the pairs that never froze (all of them when max_iter = 0): f and H at the psi they hold
      s.round = max_iter; s.final = 1;
      CACK(launch_ev_mom(h, m));
      CACK(launch_ev_fin(h, s, CA_EV_STEP));
    }
    // the quadrature: the nodes' psi, Z0 of every (clone, node) slot in one launch, the reduction over the nodes
    CACK(launch_ev_fin(h, s, CA_EV_NODES));
    m.ps = pq_d; m.Q = Q; m.nslot = CQ; m.full = false;
    CACK(launch_ev_mom(h, m));
    CACK(launch_ev_fin(h, s, CA_EV_REDUCE));
    const size_t nc = (size_t)n_cnt * C;
    HIPCK(h, hipMemcpyAsync(b_ev.data(), ev_d, nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(b_lap.data(), lap_d, nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(b_ps.data(), ps_d, nc * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(b_H.data(), H_d, nc * NH * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(b_rd.data(), rd_d, nc * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(b_cv.data(), cv_d, nc, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    for (int64_t li = 0; li < n_cnt; ++li) {   // the batch's slabs are [column][cell]
      const int64_t n = n_lo + li;
      for (int c = 0; c < C; ++c) {
        const size_t i = hidx(h->layout, n, c, N, C), j = (size_t)c * n_cnt + li;
        evidence[i] = b_ev[j]; laplace[i] = b_lap[j]; rounds[i] = b_rd[j]; converged[i] = b_cv[j];
        for (int k = 0; k < K; ++k) psi_mode[hidx(h->layout, n, c * K + k, N, C * K)] = b_ps[((size_t)c * K + k) * n_cnt + li];
        for (int k = 0; k < NH; ++k) psi_prec[hidx(h->layout, n, c * NH + k, N, C * NH)] = b_H[((size_t)c * NH + k) * n_cnt + li];
      }
    }
  }
  return CA_OK;
}

extern "C++" {
namespace {
thread_local double boot_kernel_ms = 0.0;
// the event pairs around the launch groups of one call; their times are added after the call's last synchronise
struct ca_event_pairs {
  std::vector<hipEvent_t> ev;
  ~ca_event_pairs() { for (hipEvent_t e : ev) hipEventDestroy(e); }
  hipError_t mark(hipStream_t s) {
    hipEvent_t e = nullptr;
    hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return rc;
    ev.push_back(e);
    return hipEventRecord(e, s);
  }
  hipError_t total(double* ms) const {
    *ms = 0.0;
    for (size_t i = 0; i + 1 < ev.size(); i += 2) {
      float t = 0.f;
      hipError_t rc = hipEventElapsedTime(&t, ev[i], ev[i + 1]);
      if (rc != hipSuccess) return rc;
      *ms += t;
    }
    return hipSuccess;
  }
};
}  // namespace
}  // extern "C++"

// the kernel time of the calling thread's last successful ca_clone_loglik_reweighted (its launches between event pairs; no copy)
int ca_reweighted_kernel_ms(double* ms) {
  if (!ms) return CA_ERR_INVALID;
  *ms = boot_kernel_ms;
  return CA_OK;
}

// The gene-reweighted log-likelihood of the resident cells [cell_lo, cell_lo + cell_cnt) for R sets of gene weights, reduced to votes and shares on the device
// (bootstrap support for clone calls; include/clonealign_hip.h has the formulas and the rules, ca_k_bootll.hip.h the kernels).  The operands, the verdict, the
// batch size and the outputs' layout are the scoring family's; the replicates go in chunks of CA_BOOT_RCHUNK: per chunk one k_boot_build, then per batch of
// cells the product against the resident rows, the product against exp(eta - m) (D > 0), the side pass over the genes with a zero of E, k_boot_finish and
// k_boot_reduce.  votes / prob_sum / prob_sq stay on the device from the first chunk to the last.
int ca_clone_loglik_reweighted(ca_handle h, const double* E, const double* U, const double* V, int32_t D, const double* w, int32_t R, const double* log_prior, int64_t c_lo,
                               int64_t c_cnt, double* ll, int32_t* votes, double* prob_sum, double* prob_sq, double* reads) {
  if (!h) return CA_ERR_INVALID;
  const std::string pre = "ca_clone_loglik_reweighted: ";
  {
    const char* null_arg = !E ? "E" : !w ? "w" : !votes ? "votes" : !prob_sum ? "prob_sum" : !prob_sq ? "prob_sq" : nullptr;
    if (null_arg) { h->err = pre + null_arg + " is NULL"; return CA_ERR_INVALID; }
  }
  CA_NOT_IN_RUN(h);
  boot_kernel_ms = 0.0;
  if (D < 0 || D > CA_LL_DMAX) { h->err = pre + "D = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]"; return CA_ERR_INVALID; }   // (the same on every rank: no collective)
  if (D > 0 && (!U || !V)) { h->err = pre + "D = " + std::to_string(D) + " needs both U (cells x D) and V (genes x D)"; return CA_ERR_INVALID; }
  if (R < 1) { h->err = pre + "R = " + std::to_string(R) + " replicates is below 1"; return CA_ERR_INVALID; }
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C;
  HIPCK(h, hipSetDevice(h->device));
  ca_ll_operands op;
  ll_operands(h, ca_ll_req{E, V, D, {{U, D, "U", "factor"}, {nullptr, 0, "", ""}}, c_lo, c_cnt, false, false, 0, true}, op);
  std::string& bad = op.bad;
  for (int r = 0; r < R && bad.empty(); ++r) {   // (the weights are the same on every rank)
    bool any = false;
    for (int g = 0; g < G; ++g) {
      const double v = w[(size_t)r * G + g];
      if (!std::isfinite(v) || v < 0.0) { bad = "the weights have a negative or non-finite entry (replicate " + std::to_string(r) + ", gene " + std::to_string(g) + ")"; break; }
      any = any || v > 0.0;
    }
    if (bad.empty() && !any) bad = "the weights of replicate " + std::to_string(r) + " are all zero (genes 0 .. " + std::to_string(G - 1) + ")";
  }
  std::vector<double> lp;
  if (log_prior && bad.empty()) {
    lp.resize((size_t)N * C);
    for (int64_t n = 0; n < N && bad.empty(); ++n)
      for (int c = 0; c < C; ++c) {
        const double v = log_prior[hidx(h->layout, n, c, N, C)];
        if (std::isnan(v) || v == HUGE_VAL) { bad = "log_prior has a NaN or +inf entry (cell " + std::to_string(n) + ", clone " + std::to_string(c) + "); -inf excludes a clone"; break; }
        lp[(size_t)n * C + c] = v;
      }
  }
  CACK(agree_on_verdict(h, bad));
  if (!bad.empty()) { h->err = pre + bad; return CA_ERR_INVALID; }
  if (c_cnt == 0) return CA_OK;
  // the genes where some clone has E = 0, with the mask of those clones in words of 32
  const int nw = cdiv(C, 32);
  std::vector<int> zg;
  std::vector<unsigned> zm;
  for (int g = 0; g < G; ++g) {
    bool any = false;
    for (int c = 0; c < C && !any; ++c) any = op.Ec[(size_t)g * C + c] == 0.0;
    if (!any) continue;
    zg.push_back(g);
    zm.resize(zm.size() + (size_t)nw, 0u);
    for (int c = 0; c < C; ++c)
      if (op.Ec[(size_t)g * C + c] == 0.0) zm[zm.size() - (size_t)nw + (size_t)(c >> 5)] |= 1u << (c & 31);
  }
  const int nz = (int)zg.size();
  // columns of a full chunk, padded to whole tiles of 16; the slabs of a batch under the byte budget
  const int RC = std::min<int>(R, CA_BOOT_RCHUNK), nzc = cdiv(G, CA_LL_ZCHUNK);
  auto cols16 = [](int n) { return (n + 15) / 16 * 16; };
  const int nc1max = cols16(RC * (C + 1)), nc2max = cols16(RC * C);
  const int64_t per_cell = ((int64_t)nzc * (nc1max + (D > 0 ? nc2max + 1 : 0)) + (int64_t)RC * (C + 1) + 2 * (int64_t)C) * (int64_t)sizeof(double) +
                           ((int64_t)RC * nw + C) * (int64_t)sizeof(int);
  const int64_t NB = cells_per_batch(c_cnt, per_cell, CA_LL_BUDGET);
  ca_rows_out o_ll(h, ll, c_cnt, (int64_t)R * C), o_ps(h, prob_sum, c_cnt, C), o_pq(h, prob_sq, c_cnt, C), o_rd(h, reads, c_cnt, R);
  std::vector<int> o_vt((size_t)c_cnt * C);
  std::vector<double> wv(w, w + (size_t)R * G);
  ca_event_pairs evs;
  ca_call_mem mem(h);
  const ca_ll_dev dev = upload_operands(mem, op);
  ca_boot_ops o;
  o.W = mem.upload(wv); o.Ec = dev.Ec; o.Ut = dev.Ut; o.Vt = dev.Vt;
  o.zg = nz > 0 ? mem.upload(zg) : nullptr; o.zm = nz > 0 ? mem.upload(zm) : nullptr;
  const double* lp_d = log_prior ? mem.upload(lp) : nullptr;
  o.B1 = mem.alloc<double>((int64_t)Gp * nc1max);
  o.B2 = D > 0 ? mem.alloc<double>((int64_t)Gp * nc2max) : nullptr;
  o.Z0 = D > 0 ? nullptr : mem.alloc<double>((int64_t)RC * C);
  o.part = mem.alloc<double>((int64_t)nzc * NB * nc1max);
  o.zpart = D > 0 ? mem.alloc<double>((int64_t)nzc * NB * nc2max) : nullptr;
  o.mpart = D > 0 ? mem.alloc<double>((int64_t)nzc * NB) : nullptr;
  o.llb = mem.alloc<double>(NB * RC * C);
  o.sb = mem.alloc<double>(NB * RC);
  o.flags = nz > 0 ? mem.alloc<unsigned>(NB * RC * nw) : nullptr;
  int* vt_d = mem.alloc<int>(c_cnt * C);
  double *ps_d = mem.alloc<double>(c_cnt * C), *pq_d = mem.alloc<double>(c_cnt * C);
  if (mem.rc != CA_OK) return mem.rc;
  o.rcp = RC; o.nw = nw; o.nz = nz; o.D = D; o.nzc = nzc;
  HIPCK(h, hipMemsetAsync(vt_d, 0, (size_t)c_cnt * C * sizeof(int), h->stream));
  HIPCK(h, hipMemsetAsync(ps_d, 0, (size_t)c_cnt * C * sizeof(double), h->stream));
  HIPCK(h, hipMemsetAsync(pq_d, 0, (size_t)c_cnt * C * sizeof(double), h->stream));
  for (int r0 = 0; r0 < R; r0 += CA_BOOT_RCHUNK) {
    o.r0 = r0; o.rc = std::min<int>(CA_BOOT_RCHUNK, R - r0);
    o.nc1 = cols16(o.rc * (C + 1)); o.nc2 = cols16(o.rc * C);
    HIPCK(h, evs.mark(h->stream));
    CACK(launch_boot_build(h, o));
    HIPCK(h, evs.mark(h->stream));
    for (int64_t n_lo = c_lo; n_lo < c_lo + c_cnt; n_lo += NB) {
      o.n_lo = n_lo; o.n_cnt = std::min<int64_t>(NB, c_lo + c_cnt - n_lo);
      const int64_t row = n_lo - c_lo;
      HIPCK(h, evs.mark(h->stream));
      CACK(launch_boot_prod(h, o, false));
      if (D > 0) CACK(launch_boot_prod(h, o, true));
      if (nz > 0) CACK(launch_boot_zero(h, o));
      CACK(launch_boot_finish(h, o, lp_d, vt_d + row * C, ps_d + row * C, pq_d + row * C));
      HIPCK(h, evs.mark(h->stream));
      // (the copies run in stream order: before the next launches overwrite the batch's buffers)
      if (ll) HIPCK(h, hipMemcpy2DAsync(o_ll.p + ((size_t)row * R + (size_t)r0) * C, (size_t)R * C * sizeof(double), o.llb, (size_t)o.rc * C * sizeof(double),
                                        (size_t)o.rc * C * sizeof(double), (size_t)o.n_cnt, hipMemcpyDeviceToHost, h->stream));
      if (reads) HIPCK(h, hipMemcpy2DAsync(o_rd.p + (size_t)row * R + (size_t)r0, (size_t)R * sizeof(double), o.sb, (size_t)o.rc * sizeof(double), (size_t)o.rc * sizeof(double),
                                           (size_t)o.n_cnt, hipMemcpyDeviceToHost, h->stream));
    }
  }
  HIPCK(h, hipMemcpyAsync(o_vt.data(), vt_d, o_vt.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipMemcpyAsync(o_ps.p, ps_d, (size_t)c_cnt * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipMemcpyAsync(o_pq.p, pq_d, (size_t)c_cnt * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipStreamSynchronize(h->stream));
  HIPCK(h, evs.total(&boot_kernel_ms));
  o_ll.finish(); o_ps.finish(); o_pq.finish(); o_rd.finish();
  for (int64_t n = 0; n < c_cnt; ++n)
    for (int c = 0; c < C; ++c) votes[hidx(h->layout, n, c, c_cnt, C)] = o_vt[(size_t)(n * C + c)];
  return CA_OK;
}
