// ca_k_sparse.hip.h -- part of ca_kernels.hip.h (textually included there, in this order): device ingest of a compressed (CSR / CSC) count
// matrix (ca_create_sparse).  The result is exactly what the dense path (k_scan_y, k_convert_y / k_convert_y_u8ovf) makes of the same
// matrix: the same storage pick, the same resident [N][Gp] rows, the same overflow entries.
//
// Every kernel reads a CSR view: `ptr` (run r = entries ptr[r] .. ptr[r + 1] - 1), `idx` (gene of the entry), `val`; cell n of the problem is
// run rows[n] (rows == NULL: run n), gene g of the source is gene ginv[g] of the problem (ginv == NULL: identity; -1 = not selected).
// flags: bit0 non-integral, bit1 negative / NaN (as k_scan_y), bit2 ptr not canonical, bit3 index out of range, bit4 index repeated or
// decreasing within a run.

// Canonical form of the caller's arrays, one wave per run (so that each run's boundaries are the wave's): ptr[0] = 0, ptr never decreases,
// ptr[nrun] = nnz; every index in [0, ndim) and strictly increasing within its run.  Nothing else reads idx before this has passed.
template <typename IT>
__global__ void __launch_bounds__(CA_TB) k_sp_check(const IT* __restrict__ ptr, const IT* __restrict__ idx, int64_t nrun, int64_t ndim,
                                                    int64_t nnz, int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  int f = 0;
  if (w0 == 0 && lane == 0 && ((int64_t)ptr[0] != 0 || (int64_t)ptr[nrun] != nnz)) f |= 4;
  for (int64_t r = w0; r < nrun; r += nw) {
    const int64_t a = (int64_t)ptr[r], b = (int64_t)ptr[r + 1];
    if (a < 0 || b < a || b > nnz) { f |= 4; continue; }
    for (int64_t e = a + lane; e < b; e += 64) {
      const int64_t j = (int64_t)idx[e];
      if (j < 0 || j >= ndim) f |= 8;
      if (e > a && (int64_t)idx[e - 1] >= j) f |= 16;
    }
  }
  if (f) atomicOr(flags, f);
}

// inverse of a selection list: inv[index[i]] = i (inv pre-filled with -1)
template <typename XT>
__global__ void k_sp_inverse(const XT* __restrict__ index, int64_t n, int32_t* __restrict__ inv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) inv[(int64_t)index[i]] = (int32_t)i;
}

// max / integrality / > 255 scan over the SELECTED stored entries (implicit zeros change none of the four), one wave per selected cell
template <typename PT, typename IT, typename VT>
__global__ void __launch_bounds__(CA_TB) k_sp_scan(const PT* __restrict__ ptr, const IT* __restrict__ idx, const VT* __restrict__ val,
                                                   const int64_t* __restrict__ rows, const int32_t* __restrict__ ginv, int64_t N,
                                                   double* __restrict__ maxv, int* __restrict__ flags, unsigned long long* __restrict__ n_over255) {
  __shared__ double sm[CA_TB];
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  double m = 0.0;
  int f = 0;
  unsigned long long over = 0;
  for (int64_t n = w0; n < N; n += nw) {
    const int64_t r = rows ? rows[n] : n;
    const int64_t a = (int64_t)ptr[r], b = (int64_t)ptr[r + 1];
    for (int64_t e = a + lane; e < b; e += 64) {
      if (ginv && ginv[(int64_t)idx[e]] < 0) continue;
      const double v = (double)val[e];
      if (!(v >= 0.0)) f |= 2;
      if (v != floor(v)) f |= 1;
      if (v > 255.0) ++over;
      m = v > m ? v : m;
    }
  }
  if (f) atomicOr(flags, f);
  if (over) atomicAdd(n_over255, over);
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int s = CA_TB / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sm[threadIdx.x] = sm[threadIdx.x] > sm[threadIdx.x + s] ? sm[threadIdx.x] : sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long*>(maxv), (unsigned long long)__double_as_longlong(sm[0]));
}

// ---- CSC -> CSR over the selection: per-cell counts, an exclusive scan, a scatter (entry order within a row is arbitrary: the dense
// row does not depend on it, and the overflow list is sorted on the host afterwards).  One wave per source gene.
template <typename IT>
__global__ void __launch_bounds__(CA_TB) k_sp_csc_count(const IT* __restrict__ ptr, const IT* __restrict__ idx, int64_t nrun,
                                                        const int32_t* __restrict__ ginv, const int32_t* __restrict__ cinv,
                                                        unsigned long long* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = w0; r < nrun; r += nw) {
    if (ginv && ginv[r] < 0) continue;
    for (int64_t e = (int64_t)ptr[r] + lane; e < (int64_t)ptr[r + 1]; e += 64) {
      const int64_t c = cinv ? (int64_t)cinv[(int64_t)idx[e]] : (int64_t)idx[e];
      if (c >= 0) atomicAdd(&cnt[c], 1ull);
    }
  }
}
template <typename IT, typename VT>
__global__ void __launch_bounds__(CA_TB) k_sp_csc_scatter(const IT* __restrict__ ptr, const IT* __restrict__ idx, const VT* __restrict__ val,
                                                          int64_t nrun, const int32_t* __restrict__ ginv, const int32_t* __restrict__ cinv,
                                                          unsigned long long* __restrict__ fill, int32_t* __restrict__ col, VT* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = w0; r < nrun; r += nw) {
    const int32_t g = ginv ? ginv[r] : (int32_t)r;
    if (g < 0) continue;
    for (int64_t e = (int64_t)ptr[r] + lane; e < (int64_t)ptr[r + 1]; e += 64) {
      const int64_t c = cinv ? (int64_t)cinv[(int64_t)idx[e]] : (int64_t)idx[e];
      if (c < 0) continue;
      const unsigned long long q = atomicAdd(&fill[c], 1ull);
      col[q] = g;
      out[q] = val[e];
    }
  }
}
// in place: a[0 .. n) counts -> exclusive prefix sums, a[n] = the total.  One block: thread t sums a contiguous slice, the slice sums are scanned
// in LDS, each thread writes its slice's prefixes (N / 1024 serial steps per thread: ~1000 at a million cells).
__global__ void __launch_bounds__(1024) k_sp_exscan(int64_t* __restrict__ a, int64_t n) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n + 1023) / 1024, lo = min(n, (int64_t)t * per), hi = min(n, lo + per);
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += a[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int64_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t i = lo; i < hi; ++i) { const int64_t c = a[i]; a[i] = run; run += c; }
  if (t == 1023) a[n] = part[1023];
}

// ---- densify: one block per selected cell.  The block builds `seg` padded elements of the row in LDS (zeros, then its run's selected
// entries converted as k_convert_y / k_convert_y_u8ovf convert them) and writes them out with 16-byte stores; rows wider than the LDS
// budget take several segments (the run is read once per segment).  ybytes: 1 (u8), 2 (u16), 4 (f32).  counter != NULL: u8 with an
// overflow list -- a count above 255 stores 255 and appends (cell, gene, v - 255).
template <typename PT, typename IT, typename VT>
__global__ void __launch_bounds__(CA_TB) k_sp_densify(const PT* __restrict__ ptr, const IT* __restrict__ idx, const VT* __restrict__ val,
                                                      const int64_t* __restrict__ rows, const int32_t* __restrict__ ginv, int Gp, int ybytes,
                                                      int seg, uint8_t* __restrict__ Y, int* __restrict__ flags,
                                                      unsigned long long* __restrict__ counter, int* __restrict__ orow, int* __restrict__ ocol,
                                                      float* __restrict__ oval) {
  extern __shared__ uint4 ca_sp_row[];
  const int64_t n = blockIdx.x;
  const int64_t r = rows ? rows[n] : n;
  const int64_t a = (int64_t)ptr[r], b = (int64_t)ptr[r + 1];
  uint8_t* const lb = reinterpret_cast<uint8_t*>(ca_sp_row);
  int f = 0;
  for (int s0 = 0; s0 < Gp; s0 += seg) {
    const int se = min(seg, Gp - s0);
    const int nq = se * ybytes / 16;
    for (int q = threadIdx.x; q < nq; q += blockDim.x) ca_sp_row[q] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (int64_t e = a + threadIdx.x; e < b; e += blockDim.x) {
      const int64_t gs = (int64_t)idx[e];
      const int g = ginv ? ginv[gs] : (int)gs;
      if (g < s0 || g >= s0 + se) continue;   // (unselected genes: g = -1)
      const int o = g - s0;
      const double v = (double)val[e];
      if (ybytes == 1) {
        uint8_t out;
        if (counter && v > 255.0) {
          out = 255;
          const unsigned long long k = atomicAdd(counter, 1ull);
          orow[k] = (int)n; ocol[k] = g; oval[k] = (float)(v - 255.0);
        } else {
          out = (uint8_t)v;
          if (!counter && (double)out != v) f |= 1;
        }
        lb[o] = out;
      } else if (ybytes == 2) {
        const uint16_t out = (uint16_t)v;
        if ((double)out != v) f |= 1;
        reinterpret_cast<uint16_t*>(lb)[o] = out;
      } else {
        const float out = (float)v;
        if ((double)out != v) f |= 1;
        reinterpret_cast<float*>(lb)[o] = out;
      }
      if (!counter && !(v >= 0.0)) f |= 2;
    }
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(Y + (n * (int64_t)Gp + s0) * ybytes);
    for (int q = threadIdx.x; q < nq; q += blockDim.x) dst[q] = ca_sp_row[q];
    __syncthreads();
  }
  if (f) atomicOr(flags, f);
}
