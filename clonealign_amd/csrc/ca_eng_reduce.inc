// ca_eng_reduce.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): the transports' all-reduce of a device vector (peer-to-peer launch with its riders, host callback, RCCL).
// does a transport reduce this engine's sums over the ranks?
inline bool is_sharded(const ca_engine* h) { return h->opt.world > 1 || h->comm || h->host_ar || (h->p2p && h->p2p->connected); }
// CA_VAR_GENE_RIDE: does a series pass take the merged way back (reduction + per-gene pass + column jobs in one launch, ca_polygene.hip.h)?  Not a cell-sharded
// fit: its collective sits between the reduction and the per-gene pass.  Not without the mapped host word the bounded wait reports to.
inline bool gene_ride_merges(const ca_engine* h) { return h->gene_ride && !is_sharded(h) && h->host_dev != nullptr; }
// work that rides in the peer-to-peer all-reduce's launch instead of getting launches of its own in front of it (ca_p2p_args)
struct ca_ar_ride {
  const float* gpart = nullptr; int nslice = 0; int64_t fold_lo = 0, fold_n = 0;
  const double* yw_part = nullptr; int n_yw = 0; int64_t yw_index = -1;
};
inline bool p2p_ride_ok(const ca_engine* h, int64_t n) { return h->p2p && h->p2p->connected && h->p2p_ride && n <= h->p2p->cap; }
int allreduce(ca_engine* h, double* buf, int64_t n, const ca_ar_ride* ride = nullptr) {
  if (h->opt.world <= 1 && !h->comm && !h->host_ar && !(h->p2p && h->p2p->connected)) return CA_OK;   // a 1-rank communicator still reduces (tests)
  if (h->p2p && h->p2p->connected) {
    ca_p2p* pp = h->p2p;
    for (int64_t o = 0; o < n; o += pp->cap) {   // (one launch for everything the loop reduces; longer vectors go in pieces)
      const int64_t m = std::min<int64_t>(pp->cap, n - o);
      const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(m, CA_TB), 64));
      ca_p2p_args a;
      memset(&a, 0, sizeof(a));
      a.peers = pp->peers_dev; a.rank = h->opt.rank; a.world = h->opt.world; a.cap = pp->cap;
      a.seq = ++pp->seq; a.err = pp->err_dev; a.err_local = pp->err_local; a.timeout_ticks = pp->timeout_ticks;
      a.yw_index = -1;
      if (ride) {   // (only ever with n <= cap: one piece, p2p_ride_ok)
        a.gpart = ride->gpart; a.nslice = ride->nslice; a.fold_lo = ride->fold_lo; a.fold_n = ride->fold_n;
        a.yw_part = ride->yw_part; a.n_yw = ride->n_yw; a.yw_index = ride->yw_index;
      }
      LAUNCH(h, CA_KERNEL_OTHER, hipLaunchKernelGGL(k_p2p_allreduce, dim3(nblk), dim3(CA_TB), 0, h->stream, buf + o, m, a));
    }
    return CA_OK;
  }
  if (h->host_ar) {
    if (n > h->host_ar_cap) {
      if (h->host_ar_buf) HIPCK(h, hipHostFree(h->host_ar_buf));
      HIPCK(h, hipHostMalloc((void**)&h->host_ar_buf, (size_t)n * sizeof(double)));
      h->host_ar_cap = n;
    }
    HIPCK(h, hipMemcpyAsync(h->host_ar_buf, buf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SYNC(h);
    if (h->host_ar(h->host_ar_user, h->host_ar_buf, n) != 0) { h->err = "host all-reduce callback failed"; return CA_ERR_COMM; }
    HIPCK(h, hipMemcpyAsync(buf, h->host_ar_buf, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return CA_OK;
  }
  if (!h->comm) { h->err = "world > 1 but neither ca_comm_init() nor ca_set_host_allreduce() was called"; return CA_ERR_STATE; }
  int rc = g_rccl.AllReduce(buf, buf, (size_t)n, kNcclFloat64, kNcclSum, h->comm, h->stream);
  if (rc != 0) {
    h->err = std::string("ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
    return CA_ERR_COMM;
  }
  return CA_OK;
}
