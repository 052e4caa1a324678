// ca_eng_predmom.inc -- part of clonealign_hip.hip (textually included there, after ca_eng_predictive.inc; one translation unit; ca_gen_call, the call's scaffold, is defined in ca_eng_simulate.inc): C ABI without a handle: the mean and variance of the log-likelihood's linear part per cell and the mean, variance and third cumulant of the per-clone gene totals of ca_predictive_stats's replicates, in closed form (ca_predictive_moments; include/clonealign_hip.h states the outputs), the kernel time of the calling thread's last call.
namespace { thread_local double predmom_kernel_ms = 0.0; }

int ca_predictive_moments_kernel_ms(double* ms) { return gen_kernel_ms(ms, predmom_kernel_ms); }

// How a call with factors is cut under a budget of `budget` bytes per kind of device buffer (64 MB): NB cells per batch (a cell's U row, clone, total, m, Z,
// mean, variance and list entry: 8 D + 56 bytes), SL list entries per strip of the gene phase.  SL: at least 64; about 2048 blocks per launch (strips x tiles of
// 256 genes) where the batch is large enough; and few enough strips for genepart [strips][3][G] -- a clone's last strip is short, so up to C more than NB / SL.
// Both depend on (N, G, C, D) alone, never on the device: two calls agree bit for bit anywhere.  What does not give way: the five tables of C x G float64 (E,
// log E, the three running sums), which stay below 64 MB together up to 1.6 million (gene, clone) pairs.
extern "C++" {
namespace {
struct ca_pm_cut { int64_t NB, SL, strips; };
inline ca_pm_cut predmom_cut(int64_t N, int32_t G, int32_t C, int32_t D, int64_t budget) {
  ca_pm_cut k;
  k.NB = std::min<int64_t>(N, std::max<int64_t>(1, budget / ((int64_t)D * 8 + 56)));
  const int64_t target = std::max<int64_t>(1, 2048 / cdiv(G, CA_PM_TB)), room = std::max<int64_t>(1, budget / ((int64_t)24 * G) - C);
  k.SL = std::max<int64_t>(64, std::max<int64_t>(cdiv(k.NB, target), cdiv(k.NB, room)));
  k.strips = (int64_t)C + k.NB / k.SL + 1;
  return k;
}
}  // namespace
}  // extern "C++"

// Validates everything on the host before the first byte of an output is written (ca_simulate_counts's checks, then the outputs).  D = 0: p depends on the
// clone alone, so the host does the whole call from the per-clone quantities (Z_c, h_c, the variance and S_c = the clone's sum of totals) in O(G C + N).
// D > 0, per batch of cells: k_predmom_cell, then -- over the batch's cells with total > 0, listed by clone (a stable counting sort) and cut into strips --
// k_predmom_gene and k_predmom_finish, which adds the batch's strips onto the running tables; the batches go in order, so the sums have one fixed order.
int ca_predictive_moments(int64_t N, int32_t G, int32_t C, int32_t D, const double* E, const double* V, const double* U, const int32_t* clone, const int64_t* total,
                          int32_t device, double* cell_mean, double* cell_var, double* T_mean, double* T_var, double* T_cum3, char* err) {
  ca_gen_call call("ca_predictive_moments", err, predmom_kernel_ms);
  std::string bad = sim_check_shape(N, G, C, D, E, V, U, clone, total, false, "E, clone and total must not be NULL", 0);
  if (!bad.empty()) return call.refuse(bad);
  const std::pair<const char*, const double*> outs[5] = {{"cell_mean", cell_mean}, {"cell_var", cell_var}, {"T_mean", T_mean}, {"T_var", T_var}, {"T_cum3", T_cum3}};
  for (const auto& o : outs)
    if (!o.second) return call.refuse(std::string(o.first) + " must not be NULL");
  std::vector<double> Et, Vt;
  bad = sim_check_values(N, G, C, D, E, V, U, clone, total, Et, Vt);
  if (!bad.empty()) return call.refuse(bad);
  const size_t CG = (size_t)C * G;
  if (N == 0) {
    for (double* T : {T_mean, T_var, T_cum3}) std::fill(T, T + CG, 0.0);
    return CA_OK;
  }

  if (D == 0) {
    std::vector<double> S((size_t)C, 0.0), hc((size_t)C, 0.0), vc((size_t)C, 0.0);
    for (int64_t n = 0; n < N; ++n) S[(size_t)clone[n]] += (double)total[n];
    for (int c = 0; c < C; ++c) {
      const double* e = Et.data() + (size_t)c * G;
      int gmax = 0;   // the largest weight (the first such gene), the others' sum, Z and the lp of a gene with p > 1/2: the cell phase's rules
      for (int g = 1; g < G; ++g)
        if (e[g] > e[gmax]) gmax = g;
      double rest = 0.0;
      for (int g = 0; g < G; ++g)
        if (g != gmax) rest += e[g];
      const double Z = rest + e[gmax];
      double h = 0.0, v = 0.0;
      if (Z > 0.0) {
        const double log_z = std::log(Z);
        const int gtop = e[gmax] / Z > 0.5 ? gmax : -1;
        const double lp_top = std::log1p(-(rest / Z));
        for (int g = 0; g < G; ++g)
          if (e[g] > 0.0) h += (e[g] / Z) * (g == gtop ? lp_top : std::log(e[g]) - log_z);
        for (int g = 0; g < G; ++g)
          if (e[g] > 0.0) { const double d = (g == gtop ? lp_top : std::log(e[g]) - log_z) - h; v += (e[g] / Z) * (d * d); }
      }
      hc[(size_t)c] = h; vc[(size_t)c] = v;
      for (int g = 0; g < G; ++g) {
        const size_t o = (size_t)g * C + c;
        double a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (S[(size_t)c] > 0.0 && e[g] > 0.0) {   // (S > 0 implies Z > 0: the host refused a positive total on an all-zero clone)
          const double p = e[g] / Z, tp = S[(size_t)c] * p, tpq = tp * (1.0 - p);
          a1 = tp; a2 = tpq; a3 = tpq * (1.0 - 2.0 * p);
        }
        T_mean[o] = a1; T_var[o] = a2; T_cum3[o] = a3;
      }
    }
    for (int64_t n = 0; n < N; ++n) {
      const double t = (double)total[n];
      cell_mean[n] = total[n] > 0 ? t * hc[(size_t)clone[n]] : 0.0;
      cell_var[n] = total[n] > 0 ? t * vc[(size_t)clone[n]] : 0.0;
    }
    return CA_OK;
  }

  const int64_t budget = (int64_t)64 << 20;
  const ca_pm_cut cut = predmom_cut(N, G, C, D, budget);
  const int64_t NB = cut.NB;
  const bool w_lds = (size_t)G * 8 <= CA_PM_LDS;
  int n_cu = 0;
  if (!call.open(device) || !call.note(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device), "hipDeviceGetAttribute")) return call.failed();
  int64_t blocks = std::min<int64_t>(NB, 8 * (int64_t)std::max(n_cu, 1));
  if (!w_lds) blocks = std::min<int64_t>(blocks, std::max<int64_t>(1, budget / ((int64_t)G * 8)));
  call.model(Et, Vt, D, NB);
  ca_predmom_ops o;
  o.Et = call.Et; o.Vt = call.Vt; o.U = call.U; o.clone = call.clone; o.total = call.total; o.G = G; o.C = C; o.D = D; o.w_lds = w_lds;
  o.lEt = call.alloc<double>((int64_t)CG);
  o.acc = call.alloc<double>(3 * (int64_t)CG);
  o.m = call.alloc<double>(NB); o.z = call.alloc<double>(NB); o.mean = call.alloc<double>(NB); o.var = call.alloc<double>(NB);
  int32_t *list_d = call.alloc<int32_t>(NB), *first_d = call.alloc<int32_t>((int64_t)C + 1);
  ca_pm_strip* st_d = call.alloc<ca_pm_strip>(cut.strips);
  o.list = list_d; o.first = first_d; o.strips = st_d;
  o.genepart = call.alloc<double>(cut.strips * 3 * G);
  o.w_blk = w_lds ? nullptr : call.alloc<double>(blocks * G);
  if (o.acc) call.note(hipMemsetAsync(o.acc, 0, 3 * CG * sizeof(double), call.stream), "hipMemsetAsync of the tables");
  if (!call.timed([&]() { return launch_predmom_loge(call.stream, o); })) return call.failed();
  std::vector<int32_t> list, first((size_t)C + 1), fill((size_t)C);
  std::vector<ca_pm_strip> strips;
  for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
    // the batch's cells with counts, by clone, in their own order inside a clone; strips of up to SL entries, none across a clone boundary
    std::fill(fill.begin(), fill.end(), 0);
    for (int64_t i = 0; i < n_cnt; ++i)
      if (total[n_lo + i] > 0) ++fill[(size_t)clone[n_lo + i]];
    strips.clear();
    int32_t at = 0;
    for (int c = 0; c < C; ++c) {
      first[(size_t)c] = (int32_t)strips.size();
      const int32_t cnt = fill[(size_t)c];
      for (int32_t lo = 0; lo < cnt; lo += (int32_t)cut.SL) strips.push_back(ca_pm_strip{at + lo, (int32_t)std::min<int64_t>(cut.SL, cnt - lo), c});
      fill[(size_t)c] = at;
      at += cnt;
    }
    first[(size_t)C] = (int32_t)strips.size();
    list.resize((size_t)at);
    for (int64_t i = 0; i < n_cnt; ++i)
      if (total[n_lo + i] > 0) list[(size_t)fill[(size_t)clone[n_lo + i]]++] = (int32_t)i;
    if ((int64_t)strips.size() > cut.strips) return call.fail(CA_ERR_HIP, "internal: more strips than planned");
    if (at > 0) {
      call.note(hipMemcpyAsync(list_d, list.data(), (size_t)at * sizeof(int32_t), hipMemcpyHostToDevice, call.stream), "hipMemcpyAsync of the list");
      call.note(hipMemcpyAsync(st_d, strips.data(), strips.size() * sizeof(ca_pm_strip), hipMemcpyHostToDevice, call.stream), "hipMemcpyAsync of the strips");
      call.note(hipMemcpyAsync(first_d, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, call.stream), "hipMemcpyAsync of the strips' index");
    }
    o.n_cnt = n_cnt; o.blocks = (int)std::min<int64_t>(blocks, n_cnt); o.nstrips = (int)strips.size();
    if (!call.feed(U, clone, total, n_lo, n_cnt) || !call.timed([&]() { return launch_predmom_cell(call.stream, o); })) return call.failed();   // (feed's wait covers the lists)
    if (at > 0 && (!call.timed([&]() { return launch_predmom_gene(call.stream, o); }) || !call.timed([&]() { return launch_predmom_finish(call.stream, o); }))) return call.failed();
    if (!call.ok(hipMemcpy(cell_mean + n_lo, o.mean, (size_t)n_cnt * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy", (size_t)n_cnt * sizeof(double)) ||
        !call.ok(hipMemcpy(cell_var + n_lo, o.var, (size_t)n_cnt * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy", (size_t)n_cnt * sizeof(double)))
      return call.failed();
  }
  // [3][c][g] on the device -> the caller's three [g][c]
  double* const outT[3] = {T_mean, T_var, T_cum3};
  if (!call.gene_major(o.acc, 3, C, G, [&](int64_t k) { return outT[k]; })) return call.failed();
  return call.done();
}
