// ca_eng_cnprofile.inc -- part of clonealign_hip.hip (textually included there, after ca_eng_separability.inc; one translation unit; ca_gen_call, the call's scaffold, is defined in ca_eng_simulate.inc): C ABI without a handle: the expression side of the likelihood profile over one entry (per-gene mode) or one block of genes (block mode) of the copy-number matrix, per clone and candidate copy number (ca_copy_number_profile; include/clonealign_hip.h states the output), the kernel time of the calling thread's last call.
namespace { thread_local double cnp_kernel_ms = 0.0; }

int ca_copy_number_profile_kernel_ms(double* ms) { return gen_kernel_ms(ms, cnp_kernel_ms); }

// predmom_cut's plan for this call, under the same budget of `budget` bytes per kind of device buffer: NB cells per batch (a cell's U row, clone, total, m, Z and
// list entry within predmom_cut's 8 D + 56 bytes; in block mode its two shares per block, 16 B more), SL list entries per strip: at least 64; about 2048 blocks per
// launch (strips x tiles of 256 lanes over W genes, or over J x B (candidate, block) pairs) where the batch is large enough; and few enough strips for part
// [strips][J][W].  All of it depends on the sizes alone, never on the device: two calls agree bit for bit anywhere.
extern "C++" {
namespace {
inline ca_pm_cut cnp_cut(int64_t N, int32_t W, int32_t C, int32_t D, int32_t J, bool by_block, int64_t budget) {
  ca_pm_cut k;
  k.NB = std::min<int64_t>(N, std::max<int64_t>(1, budget / ((int64_t)D * 8 + 56 + (by_block ? (int64_t)16 * W : 0))));
  const int64_t tiles = cdiv(by_block ? (int64_t)J * W : (int64_t)W, CA_PM_TB);
  const int64_t target = std::max<int64_t>(1, 2048 / tiles), room = std::max<int64_t>(1, budget / ((int64_t)8 * J * W) - C);
  k.SL = std::max<int64_t>(64, std::max<int64_t>(cdiv(k.NB, target), cdiv(k.NB, room)));
  k.strips = (int64_t)C + k.NB / k.SL + 1;
  return k;
}
inline double cnp_mul(double a, double b) { volatile double p = a * b; return p; }   // the product rounded on its own, as __dmul_rn on the device: never fused into the subtraction after it
}  // namespace
}  // extern "C++"

// Validates everything on the host before the first byte of cost is written (ca_simulate_counts's checks, then mu, kappa, J, B, the labels and cost).  The host
// also makes the structural tables of block mode: the run list (the genes stably sorted by label), full[c][b] (the block holds every gene with E[g][c] > 0, and there
// is one) and same[c][j][b] (every gene of the block has mu_g kappa_j == E[g][c] bit for bit: the entry is 0 by rule).  D = 0: x depends on the clone alone, so the
// host does the whole call from Z_c and S_c = the clone's sum of totals in O(G C J + N).  D > 0, per batch of cells: k_cnp_cell, then -- over the batch's cells
// with total > 0, listed by clone (a stable counting sort) and cut into strips -- k_cnp_gene or k_cnp_block and k_cnp_finish, which adds the batch's strips onto
// the running table; the batches go in order, so the sums have one fixed order.
int ca_copy_number_profile(int64_t N, int32_t G, int32_t C, int32_t D, const double* E, const double* V, const double* U, const int32_t* clone, const int64_t* total,
                           const double* mu, int32_t J, const double* kappa, int32_t B, const int32_t* block_of_gene, int32_t device, double* cost, char* err) {
  ca_gen_call call("ca_copy_number_profile", err, cnp_kernel_ms);
  std::string bad = sim_check_shape(N, G, C, D, E, V, U, clone, total, false, "E, clone and total must not be NULL", 0);
  if (!bad.empty()) return call.refuse(bad);
  if (!mu || !kappa) return call.refuse("mu and kappa must not be NULL");
  if (!cost) return call.refuse("cost must not be NULL");
  if (J < 1 || J > 16) return call.refuse("J = " + std::to_string(J) + " is outside [1, 16]");
  const bool by_block = block_of_gene != nullptr;
  if (!by_block && B != G) return call.refuse("B = " + std::to_string(B) + " but block_of_gene is NULL (per-gene mode), where B must equal G = " + std::to_string(G));
  if (by_block && B < 1) return call.refuse("B = " + std::to_string(B) + ": B must be >= 1");
  if (by_block && B > 2048)
    return call.refuse("B = " + std::to_string(B) + " blocks; block mode takes at most 2048: for a block per gene pass block_of_gene = NULL (per-gene mode)");
  std::vector<double> Et, Vt;
  bad = sim_check_values(N, G, C, D, E, V, U, clone, total, Et, Vt);
  if (!bad.empty()) return call.refuse(bad);
  for (int g = 0; g < G; ++g)
    if (!std::isfinite(mu[g]) || mu[g] < 0.0) return call.refuse("mu has a negative or non-finite entry (gene " + std::to_string(g) + ")");
  for (int j = 0; j < J; ++j)
    if (!std::isfinite(kappa[j]) || kappa[j] < 0.0) return call.refuse("kappa has a negative or non-finite entry (candidate " + std::to_string(j) + ")");
  if (by_block)
    for (int g = 0; g < G; ++g)
      if (block_of_gene[g] < 0 || block_of_gene[g] >= B)
        return call.refuse("block_of_gene[" + std::to_string(g) + "] = " + std::to_string(block_of_gene[g]) + " is outside [0, " + std::to_string(B) + ")");
  const int W = by_block ? B : G;
  const size_t JW = (size_t)J * W, CJW = (size_t)C * JW;
  std::fill(cost, cost + CJW, 0.0);
  if (N == 0) return CA_OK;

  // block mode: the run list and the two structural tables
  std::vector<int32_t> run_gene, run_first;
  std::vector<unsigned char> full, same;
  if (by_block) {
    run_first.assign((size_t)B + 1, 0);
    for (int g = 0; g < G; ++g) ++run_first[(size_t)block_of_gene[g] + 1];
    for (int b = 0; b < B; ++b) run_first[(size_t)b + 1] += run_first[(size_t)b];
    run_gene.resize((size_t)G);
    std::vector<int32_t> at(run_first.begin(), run_first.end() - 1);
    for (int g = 0; g < G; ++g) run_gene[(size_t)at[(size_t)block_of_gene[g]]++] = g;
    full.assign((size_t)C * B, 0); same.assign(CJW, 1);
    std::vector<int32_t> npos((size_t)B);
    for (int c = 0; c < C; ++c) {
      const double* e = Et.data() + (size_t)c * G;
      std::fill(npos.begin(), npos.end(), 0);
      int all = 0;
      for (int g = 0; g < G; ++g)
        if (e[g] > 0.0) { ++npos[(size_t)block_of_gene[g]]; ++all; }
      for (int b = 0; b < B; ++b) full[(size_t)c * B + b] = all > 0 && npos[(size_t)b] == all;
      for (int j = 0; j < J; ++j)
        for (int g = 0; g < G; ++g)
          if (cnp_mul(mu[g], kappa[j]) != e[g]) same[((size_t)c * J + j) * B + block_of_gene[g]] = 0;
    }
  }
  // acc[c][j][w] -> the caller's cost[w][c][j]
  auto deliver = [&](const double* acc) {
    for (int c = 0; c < C; ++c)
      for (int j = 0; j < J; ++j) {
        const double* src = acc + ((size_t)c * J + j) * W;
        for (int w = 0; w < W; ++w) cost[((size_t)w * C + c) * J + j] = src[w];
      }
  };

  if (D == 0) {
    std::vector<double> S((size_t)C, 0.0), acc(CJW, 0.0), A((size_t)W), Sh((size_t)W);
    for (int64_t n = 0; n < N; ++n) S[(size_t)clone[n]] += (double)total[n];
    for (int c = 0; c < C; ++c) {
      if (!(S[(size_t)c] > 0.0)) continue;   // no cell with counts: exactly 0 (S > 0 implies Z > 0: the host refused a positive total on an all-zero clone)
      const double* e = Et.data() + (size_t)c * G;
      int gmax = 0;   // Z by the cell phase's rule: the largest weight (the first such gene) joins the others' sum last
      for (int g = 1; g < G; ++g)
        if (e[g] > e[gmax]) gmax = g;
      double rest = 0.0;
      for (int g = 0; g < G; ++g)
        if (g != gmax) rest += e[g];
      const double Z = rest + e[gmax];
      if (by_block)
        for (int b = 0; b < B; ++b) {   // the shares, the run's genes in ascending order
          double sa = 0.0, ss = 0.0;
          for (int i = run_first[(size_t)b]; i < run_first[(size_t)b + 1]; ++i) {
            const int g = run_gene[(size_t)i];
            sa += mu[g] * (1.0 / Z);
            if (e[g] > 0.0) ss += e[g] / Z;
          }
          A[(size_t)b] = sa; Sh[(size_t)b] = full[(size_t)c * B + b] ? 1.0 : std::fmin(ss, CA_CNP_SMAX);
        }
      for (int j = 0; j < J; ++j) {
        double* out = acc.data() + ((size_t)c * J + j) * W;
        for (int w = 0; w < W; ++w) {
          double a;
          if (by_block) {
            if (same[((size_t)c * J + j) * B + w]) continue;
            a = std::fmax(cnp_mul(kappa[j], A[(size_t)w]) - Sh[(size_t)w], -1.0);
          } else {
            const double dl = cnp_mul(mu[w], kappa[j]) - e[w];
            if (dl == 0.0) continue;
            a = e[w] > 0.0 ? (dl / e[w]) * (e[w] / Z) : dl * (1.0 / Z);
          }
          out[w] = S[(size_t)c] * std::log1p(a);
        }
      }
    }
    deliver(acc.data());
    return CA_OK;
  }

  const int64_t budget = (int64_t)64 << 20;
  const ca_pm_cut cut = cnp_cut(N, W, C, D, J, by_block, budget);
  const int64_t NB = cut.NB;
  const bool w_lds = (size_t)G * 8 <= CA_PM_LDS;
  int n_cu = 0;
  if (!call.open(device) || !call.note(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device), "hipDeviceGetAttribute")) return call.failed();
  int64_t blocks = std::min<int64_t>(NB, 8 * (int64_t)std::max(n_cu, 1));
  if (!w_lds) blocks = std::min<int64_t>(blocks, std::max<int64_t>(1, budget / ((int64_t)G * 8)));
  call.model(Et, Vt, D, NB);
  ca_cnp_ops o{};
  o.Et = call.Et; o.Vt = call.Vt; o.U = call.U; o.clone = call.clone; o.total = call.total; o.G = G; o.C = C; o.D = D; o.J = J; o.B = W; o.w_lds = w_lds; o.by_block = by_block;
  const std::vector<double> mu_h(mu, mu + G), kappa_h(kappa, kappa + J);
  std::vector<double> mk_h;
  o.mu = call.upload(mu_h);
  o.kappa = call.upload(kappa_h);
  if (!by_block) {   // mu_g kappa_j, each product rounded on its own
    mk_h.resize((size_t)J * G);
    for (int j = 0; j < J; ++j)
      for (int g = 0; g < G; ++g) mk_h[(size_t)j * G + g] = cnp_mul(mu[g], kappa[j]);
    o.mk = call.upload(mk_h);
  }
  double* acc_d = call.alloc<double>((int64_t)CJW);
  o.acc = acc_d;
  o.m = call.alloc<double>(NB); o.z = call.alloc<double>(NB);
  if (by_block) {
    o.run_gene = call.upload(run_gene); o.run_first = call.upload(run_first); o.full = call.upload(full); o.same = call.upload(same);
    o.share = call.alloc<double>(NB * 2 * B);
  }
  int32_t *list_d = call.alloc<int32_t>(NB), *first_d = call.alloc<int32_t>((int64_t)C + 1);
  ca_pm_strip* st_d = call.alloc<ca_pm_strip>(cut.strips);
  o.list = list_d; o.first = first_d; o.strips = st_d;
  o.part = call.alloc<double>(cut.strips * (int64_t)JW);
  o.w_blk = w_lds ? nullptr : call.alloc<double>(blocks * G);
  if (acc_d) call.note(hipMemsetAsync(acc_d, 0, CJW * sizeof(double), call.stream), "hipMemsetAsync of the table");
  if (!call.note(hipStreamSynchronize(call.stream), "hipStreamSynchronize")) return call.failed();   // (the uploads have read this function's temporaries)
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
    if (!call.feed(U, clone, total, n_lo, n_cnt)) return call.failed();   // (feed's wait covers the lists)
    if (at > 0 && (!call.timed([&]() { return launch_cnp_cell(call.stream, o); }) || !call.timed([&]() { return launch_cnp_sum(call.stream, o); }) ||
                   !call.timed([&]() { return launch_cnp_finish(call.stream, o); })))
      return call.failed();
  }
  std::vector<double> acc(CJW);
  if (!call.ok(hipMemcpy(acc.data(), acc_d, CJW * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy", CJW * sizeof(double))) return call.failed();
  const int rc = call.done();
  if (rc == CA_OK) deliver(acc.data());
  return rc;
}
