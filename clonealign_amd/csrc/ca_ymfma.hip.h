// The count matrix's two products of the VI loop on the int8 matrix cores (gfx950), from ONE copy of the matrix:
//   YW[n]    = sum_g y_ng W_g        (row products:    psi's gradient and the psi.(YW) term of EE_p_y)
//   YtPsi[g] = sum_n y_ng psi_n      (column products: W's gradient)
// They are the `y * log p` part of tfd$Multinomial$log_prob (R/inference-tflow.R:294-296) that depends on Y and the
// parameters only.  k_ypass computes both on the VALU from the row-major copy: 3.5 vector
// instructions per count, which it takes from the forward sweep it runs beside.  Here (K = 1, 1-byte storage) the matrix is
// streamed once per parameter state in 64-cell x 64-gene pieces; a piece goes through the wave's LDS region and comes back
// row-wise as the A operand of the row products and, through gfx950's transposing LDS read, as the B operand of the column
// products (ca_ys_mfma_body).  The parameters are quantised to 32-bit fixed point in four signed base-256 digits, one
// operand column (row) per digit (k_ys_quant and its riding forms).  No vector arithmetic per count; integer accumulation
// is exact, so a result is sum_g y_ng * round(W_g 2^e) 2^-e to the last bit, in any summation order.
//
// Two images of the matrix, same walk, picked at create time:
//   Ys  1 byte per count: stored byte = y ^ 0x80, i.e. y - 128 as a signed byte; the bias is undone from the digit sums of the
//       parameter images the quantiser leaves per 64-step (k_bias_y)
//   Y4  4 bits per count (CA_VAR_Y4): nibbles of min(y, 15), no bias; every count >= 15 has one word in an escape list that
//       the stream adds exactly (k_pack_y4, k_esc_count / k_esc_scan / k_esc_fill)
// Counts above 255 keep 255 in either image and their excess in the overflow list, like the row-major copy.  The layouts are
// stated where each image is made and above ca_ys_mfma_body.
// (Round 2's first form streamed two tiled copies, one per product, K <= 4: measured slower, deleted -- DESIGN_HISTORY.md.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef int ca_i32x4 __attribute__((ext_vector_type(4)));

#define CA_YM_TB 256

// fixed point of a parameter block: x = rint(v * 2^e) with |x| <= 2^30, e from the block's largest magnitude
__device__ __forceinline__ int ca_fix_exp(float amax) { return amax > 0.f ? 29 - ilogbf(amax) : 0; }

// ---------------------------------------------------------------- parameter images
// amax[0] = max |W_gk|, amax[1] = max |psi_nk| as float bit patterns (non-negative floats order like unsigned ints, so
// atomicMax gives the same value in any order); zeroed before each use.
__global__ void __launch_bounds__(CA_YM_TB) k_ym_absmax(const float* __restrict__ V, int Dv, int64_t G, const float* __restrict__ F, int Df,
                                                        int64_t N, int K, unsigned* __restrict__ amax) {
  const int64_t i = (int64_t)blockIdx.x * CA_YM_TB + threadIdx.x;
  float mw = 0.f, mp = 0.f;
  if (i < G) for (int k = 0; k < K; ++k) mw = fmaxf(mw, fabsf(V[i * Dv + k]));
  if (i < N) for (int k = 0; k < K; ++k) mp = fmaxf(mp, fabsf(F[i * Df + k]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mw = fmaxf(mw, __shfl_xor(mw, o, 64)); mp = fmaxf(mp, __shfl_xor(mp, o, 64)); }
  if ((threadIdx.x & 63) == 0) {
    if (i < G + 64) atomicMax(amax, __float_as_uint(mw));      // NaN parameters: the bit pattern is larger than any finite one,
    if (i < N + 64) atomicMax(amax + 1, __float_as_uint(mp));  // ca_fix_exp() of NaN is what it is -- the ELBO is NaN by then anyway
  }
}
// digit p (0..3) of the signed base-256 expansion of x: x = sum_p d_p 256^p, d_p in [-128, 127]
__device__ __forceinline__ int ca_digit(int x, int p) {
  int d = 0;
#pragma unroll
  for (int i = 0; i <= 3; ++i) {
    d = (int)(signed char)(x & 0xFF);
    if (i == p) break;
    x = (x - d) >> 8;
  }
  return d;
}
// row-major u8 [N][Gp] -> biased copy in 4-KiB pieces of 64 cells x 64 genes, [N64/64][Gp/64][64 rows][64 B] (rows past N:
// count 0): a wave's load instruction then covers 1 KiB of consecutive addresses, like the row-major stream's, instead of
// sixteen 64-byte pieces in sixteen DRAM pages (3.4 TB/s measured with the row-major copy).  One thread per 16 bytes.
__global__ void __launch_bounds__(CA_YM_TB) k_bias_y(const uint8_t* __restrict__ Y, uint4* __restrict__ Ys, int64_t N, int64_t N64, int Gp) {
  const int64_t i = (int64_t)blockIdx.x * CA_YM_TB + threadIdx.x;     // index of the 16-byte chunk in the DESTINATION
  const int64_t per_piece = 256, nb = Gp / 64;
  if (i >= (N64 / 64) * nb * per_piece) return;
  const int c = (int)(i & 3), r = (int)((i >> 2) & 63);
  const int64_t piece = i >> 8;
  const int64_t cs = piece / nb, gb = piece - cs * nb;
  const int64_t n = cs * 64 + r;
  uint4 v = {0u, 0u, 0u, 0u};
  if (n < N) v = *reinterpret_cast<const uint4*>(Y + n * (int64_t)Gp + gb * 64 + 16 * c);
  v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
  Ys[i] = v;
}

// ---------------------------------------------------------------- the 4-bit loop image and its escape list (CA_VAR_Y4)
// Y4 [N64/64][Gp/64][2 loads][64 lanes][16 B], 2-KiB pieces in the walk of Ys: nibbles of min(y, 15), no bias (0..15 is a valid signed
// byte).  Lane l = (j = l & 15, q = l >> 4) of load i, dword d, byte b: low nibble = cell 64 cs + 32 i + j, high nibble = cell 64 cs + 32 i
// + 16 + j, gene 64 gb + 16 q + 4 d + b -- so v & 0x0F0F0F0F and (v >> 4) & 0x0F0F0F0F are the A operands of the row products for cell
// tiles 2i and 2i + 1 straight from the load.  One thread per 16 bytes of the image.
__device__ __forceinline__ unsigned ca_nib4(unsigned lo, unsigned hi) {
  unsigned r = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const unsigned x = (lo >> (8 * b)) & 0xFFu, y = (hi >> (8 * b)) & 0xFFu;
    r |= ((x < 15u ? x : 15u) | ((y < 15u ? y : 15u) << 4)) << (8 * b);
  }
  return r;
}
__global__ void __launch_bounds__(CA_YM_TB) k_pack_y4(const uint8_t* __restrict__ Y, uint4* __restrict__ Y4, int64_t N, int64_t N64, int Gp) {
  const int64_t i = (int64_t)blockIdx.x * CA_YM_TB + threadIdx.x;
  const int64_t nb = Gp / 64;
  if (i >= (N64 / 64) * nb * 128) return;
  const int l = (int)(i & 63), ld = (int)((i >> 6) & 1);
  const int64_t piece = i >> 7, cs = piece / nb, gb = piece - cs * nb;
  const int64_t n0 = cs * 64 + 32 * ld + (l & 15), n1 = n0 + 16;
  const uint8_t* base = Y + gb * 64 + 16 * (l >> 4);
  uint4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
  if (n0 < N) a = *reinterpret_cast<const uint4*>(base + n0 * (int64_t)Gp);
  if (n1 < N) b = *reinterpret_cast<const uint4*>(base + n1 * (int64_t)Gp);
  Y4[i] = (uint4){ca_nib4(a.x, b.x), ca_nib4(a.y, b.y), ca_nib4(a.z, b.z), ca_nib4(a.w, b.w)};
}
// Escape list: every stored count y >= 15 as ONE word, cell-in-strip (9 bits) | gene-in-segment (9 bits) << 9 | (y - 15) << 18 (y <= 255:
// counts above keep 255 here and their excess in the overflow list).  Ordered by the stream's units -- row group rg, segment seg, wave
// strip wv of RS cells -- then by cell, then by gene: key(n, seg) = ((rg nseg + seg) 4 + wv) RS + (n - strip start), esc_off[key] = first
// entry of cell n in segment seg, esc_off[nkeys] = the total.  Built on the device: count, scan, fill (one wave per cell and segment).
__device__ __forceinline__ int64_t ca_esc_key(int64_t n, int seg, int nseg, int RS) {
  const int64_t s = n / RS;
  return (((s >> 2) * nseg + seg) * 4 + (s & 3)) * RS + (n - s * RS);
}
__device__ __forceinline__ int ca_esc_count8(uint2 v) {
  int c = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) c += (((v.x >> (8 * b)) & 0xFFu) >= 15u) + (((v.y >> (8 * b)) & 0xFFu) >= 15u);
  return c;
}
// The 2-bit / 4-bit image's list (CA_VAR_Y2; pos8 non-null): a gene's field is its POSITION in the segment's private order (pos8: eight 16-bit positions per lane,
// [Gp] by gene index), and a gene whose position lies in the first n2 64-gene blocks escapes from 3 up with excess y - 3 (its block stores min(y, 3) in 2 bits).
__device__ __forceinline__ unsigned ca_esc_pos(const uint4& p8, int b) { return ((b < 2 ? p8.x : b < 4 ? p8.y : b < 6 ? p8.z : p8.w) >> (16 * (b & 1))) & 0xFFFFu; }
__device__ __forceinline__ int ca_esc_count8_y2(uint2 v, uint4 p8, int n2) {
  int c = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const unsigned y = ((b < 4 ? v.x : v.y) >> (8 * (b & 3))) & 0xFFu;
    c += y >= ((int)ca_esc_pos(p8, b) < 64 * n2 ? 3u : 15u);
  }
  return c;
}
__global__ void __launch_bounds__(CA_YM_TB) k_esc_count(const uint8_t* __restrict__ Y, int64_t N, int Gp, int nseg, int RS, int* __restrict__ off,
                                                        const uint4* __restrict__ pos8 = nullptr, int n2 = 0) {
  const int64_t w = ((int64_t)blockIdx.x * CA_YM_TB + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= N * nseg) return;
  const int64_t n = w / nseg;
  const int seg = (int)(w - n * nseg);
  const uint2 v = *reinterpret_cast<const uint2*>(Y + n * (int64_t)Gp + seg * 512 + 8 * lane);
  int c = pos8 ? ca_esc_count8_y2(v, pos8[seg * 64 + lane], n2) : ca_esc_count8(v);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) off[ca_esc_key(n, seg, nseg, RS)] = c;
}
// exclusive scan of off[0 .. n) in place, off[n] = the total (create time: one block)
__global__ void __launch_bounds__(1024) k_esc_scan(int* __restrict__ off, int64_t n) {
  __shared__ int64_t sm[1024];
  const int t = threadIdx.x;
  const int64_t chunk = (n + 1023) / 1024, a = t * chunk, b = (a + chunk < n) ? a + chunk : n;
  int64_t s = 0;
  for (int64_t i = a; i < b; ++i) s += off[i];
  sm[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int64_t v = t >= o ? sm[t - o] : 0;
    __syncthreads();
    sm[t] += v;
    __syncthreads();
  }
  int64_t run = sm[t] - s;
  for (int64_t i = a; i < b; ++i) { const int c = off[i]; off[i] = (int)run; run += c; }
  if (t == 1023) off[n] = (int)sm[1023];
}
__global__ void __launch_bounds__(CA_YM_TB) k_esc_fill(const uint8_t* __restrict__ Y, int64_t N, int Gp, int nseg, int RS, const int* __restrict__ off,
                                                       unsigned* __restrict__ esc, const uint4* __restrict__ pos8 = nullptr, int n2 = 0) {
  const int64_t w = ((int64_t)blockIdx.x * CA_YM_TB + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= N * nseg) return;
  const int64_t n = w / nseg;
  const int seg = (int)(w - n * nseg);
  const uint2 v = *reinterpret_cast<const uint2*>(Y + n * (int64_t)Gp + seg * 512 + 8 * lane);
  uint4 p8 = {0u, 0u, 0u, 0u};
  if (pos8) p8 = pos8[seg * 64 + lane];
  const int c = pos8 ? ca_esc_count8_y2(v, p8, n2) : ca_esc_count8(v);
  int x = c;   // inclusive prefix over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(x, o, 64); if (lane >= o) x += u; }
  int e = off[ca_esc_key(n, seg, nseg, RS)] + x - c;
  const unsigned cl = (unsigned)(n % RS);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const unsigned y = ((b < 4 ? v.x : v.y) >> (8 * (b & 3))) & 0xFFu;
    const unsigned pos = pos8 ? ca_esc_pos(p8, b) : (unsigned)(8 * lane + b);
    const unsigned thr = (pos8 && (int)pos < 64 * n2) ? 3u : 15u;
    if (y >= thr) esc[e++] = cl | (pos << 9) | ((y - thr) << 18);
  }
}
// ---------------------------------------------------------------- the 2-bit / 4-bit loop image (CA_VAR_Y2)
// A third loop image, for the series form's own stream launch only.  Within each 512-gene segment the genes are ordered by their number of stored counts >= 3
// (ascending, ties by gene index; the host sorts 512 keys per segment from k_y2_hist's counts); the first n2 64-gene blocks of every segment hold min(y, 3) in
// 2 bits (1-KiB pieces), the others keep the 4-bit image's 2-KiB nibble pieces.  No gene changes segment and no cell moves: the stream's sums are the same
// integers.  Layout [N64/64][nseg][n2 x 1 KiB | (8 - n2) x 2 KiB].  Narrow piece, lane l = (j = l & 15, q = l >> 4), dword d, byte b: bits 2t .. 2t+1 = cell
// 64 cs + 16 t + j, position 64 a + 16 q + 4 d + b -- so (v >> 2t) & 0x03030303 is cell tile t's A operand.  Wide piece: k_pack_y4's, by position.
// per-gene counts of stored y >= 3 (hist[g]) and y >= 15 (hist[Gp + g]); hist zeroed before.  Four genes per thread, 64 cells per block: integer sums, any order.
__global__ void __launch_bounds__(CA_YM_TB) k_y2_hist(const uint8_t* __restrict__ Y, int64_t N, int Gp, int* __restrict__ hist) {
  const int g = 4 * ((int)blockIdx.x * CA_YM_TB + threadIdx.x);
  if (g >= Gp) return;
  const int64_t n0 = (int64_t)blockIdx.y * 64, n1 = n0 + 64 < N ? n0 + 64 : N;
  unsigned c3 = 0u, c15 = 0u;   // four byte-wide counters each (at most 64)
  for (int64_t n = n0; n < n1; ++n) {
    const unsigned v = *reinterpret_cast<const unsigned*>(Y + n * (int64_t)Gp + g);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const unsigned y = (v >> (8 * b)) & 0xFFu;
      c3 += (unsigned)(y >= 3u) << (8 * b);
      c15 += (unsigned)(y >= 15u) << (8 * b);
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int a3 = (int)((c3 >> (8 * b)) & 0xFFu), a15 = (int)((c15 >> (8 * b)) & 0xFFu);
    if (a3) atomicAdd(hist + g + b, a3);
    if (a15) atomicAdd(hist + Gp + g + b, a15);
  }
}
// one thread per 16 bytes of the image; perm[seg * 512 + position] = the gene's index in its segment
__global__ void __launch_bounds__(CA_YM_TB) k_pack_y2(const uint8_t* __restrict__ Y, uint4* __restrict__ Y2, int64_t N, int64_t N64, int Gp, int n2,
                                                      const unsigned short* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * CA_YM_TB + threadIdx.x;
  const int nseg = Gp / 512, sb = n2 * 64 + (8 - n2) * 128;   // 16-byte units per (cell step, segment)
  if (i >= (N64 / 64) * nseg * sb) return;
  const int64_t unit = i / sb, cs = unit / nseg;
  const int seg = (int)(unit - cs * nseg), r = (int)(i - unit * sb);
  const bool nar = r < n2 * 64;
  const int rw = r - n2 * 64;
  const int a = nar ? r >> 6 : n2 + (rw >> 7), l = nar ? r & 63 : rw & 63, ld = nar ? 0 : (rw >> 6) & 1;
  const int j = l & 15, q = l >> 4;
  const unsigned short* pp = perm + seg * 512 + 64 * a + 16 * q;
  const uint8_t* base = Y + seg * 512;
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int gb = 0; gb < 16; ++gb) {
    const uint8_t* col = base + pp[gb];
    unsigned x = 0u;
    if (nar) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t n = cs * 64 + 16 * t + j;
        const unsigned y = n < N ? col[n * (int64_t)Gp] : 0u;
        x |= (y < 3u ? y : 3u) << (2 * t);
      }
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int64_t n = cs * 64 + 32 * ld + 16 * t + j;
        const unsigned y = n < N ? col[n * (int64_t)Gp] : 0u;
        x |= (y < 15u ? y : 15u) << (4 * t);
      }
    }
    w[gb >> 2] |= x << (8 * (gb & 3));
  }
  Y2[i] = (uint4){w[0], w[1], w[2], w[3]};
}

// ---------------------------------------------------------------- the stream
__device__ __forceinline__ ca_i32x4 ca_mfma_i8(uint4 a, uint4 b, ca_i32x4 c) {
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(ca_i32x4, a), __builtin_bit_cast(ca_i32x4, b), c, 0, 0, 0);
}

// =====================================================================================================================
// ONE copy, both products: the count matrix stays row-major (biased bytes, y ^ 0x80) and every 64-cell x 128-gene piece
// goes through the wave's own LDS region once.  Read back row-wise (ds_read_b128) it is the A operand of the row
// products; read back through gfx950's transposing LDS read (ds_read_b64_tr_b8: per 16-lane group a block of 8 rows x 16
// bytes comes back column-major, lane 2q+p supplies the address of row q / bytes 8p..8p+7 and lane i receives column i --
// measured, tools/trb8_lab.hip) it is the B operand of the column products.  K = 1.
//
//   Ys   [N64/64][Gp/64][64][64 B]  biased bytes in 4-KiB pieces (64 cells x 64 genes, row-major inside), Gp a multiple of 512,
//        rows past N and genes past G hold 0x80 (count 0)
//   Wr   [Gp/64][64 lanes][16 B]  byte (l, b) = digit (l & 3) of fix(W[64 s + 16 (l >> 4) + b])   (every column group the same)
//   Pr   [N64/64][64 lanes][16 B] byte (l, b) = digit (l & 3) of fix(psi[64 s + 16 (l >> 4) + b])
// The digits are replicated over the four groups of four operand columns (rows) so that FOUR tiles share one accumulator:
// tile t multiplies against the image masked down to group t, and its sums land in columns (rows) 4t .. 4t+3.
//   YWi  [nseg][N][4]   int32 digit sums of a gene segment (512 genes), bias undone
//   YTi  [nrg][Gp][4]   int32 digit sums of a row group (4 strips of RS cells), bias undone
constexpr int CA_YS_GW = 512;      // genes per segment (block = one segment x four strips); the switch in k_ys_mfma assumes 8 x 64
static_assert(CA_YS_GW == 512, "k_ys_mfma's accumulator switch has eight cases");
constexpr int CA_YS_PITCH = 80;    // LDS row pitch of the 64-byte rows: 16 lanes of a ds_read_b128 group fall on 16 different bank quads
// Round 19: a cell tile (16 rows) of a staging region starts 128 B past the end of the one before.  A transposed read is served in lane groups {0-31} and
// {32-63}, i.e. two cell tiles at a time, and one tile's sixteen lanes cover 32 of the 64 banks (8 rows, 20 banks apart, two halves); at the plain pitch the
// tiles lie 16 x 80 B = 320 banks = 0 (mod 64) apart and the pair met on the same 32 banks: every transposed read a two-way conflict.  352 banks = 32 (mod 64)
// puts odd tiles on the other half.  Addresses only: the bytes a lane writes and reads back are the same.
constexpr int CA_YS_TILE = 16 * CA_YS_PITCH + 128;   // bytes from one cell tile of a staging region to the next
constexpr int CA_YS_STAGE = 4 * CA_YS_TILE;          // a wave's staging region (64 rows)
static_assert((CA_YS_TILE / 4) % 64 == 32 && CA_YS_TILE % 16 == 0, "odd cell tiles sit 32 banks off the even ones, 16-byte aligned");

// The eight transposed reads of a 64-gene block (four gene tiles x two halves of the 16 cells) and their wait in ONE asm
// statement: the compiler treats an asm output as valid as soon as the statement ends, and would otherwise be free to copy a
// result register (to line up the four VGPRs of an MFMA operand) before the data has arrived.
__device__ __forceinline__ void ca_ds_read_tr_b8_x8(unsigned addr, uint2 (&lo)[4], uint2 (&hi)[4]) {
  asm volatile(
      "ds_read_b64_tr_b8 %0, %8\n\tds_read_b64_tr_b8 %4, %8 offset:640\n\t"
      "ds_read_b64_tr_b8 %1, %8 offset:16\n\tds_read_b64_tr_b8 %5, %8 offset:656\n\t"
      "ds_read_b64_tr_b8 %2, %8 offset:32\n\tds_read_b64_tr_b8 %6, %8 offset:672\n\t"
      "ds_read_b64_tr_b8 %3, %8 offset:48\n\tds_read_b64_tr_b8 %7, %8 offset:688\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(lo[0]), "=&v"(lo[1]), "=&v"(lo[2]), "=&v"(lo[3]), "=&v"(hi[0]), "=&v"(hi[1]), "=&v"(hi[2]), "=&v"(hi[3])
      : "v"(addr)
      : "memory");
}
// two gene tiles at a time (the riding form: eight result registers live instead of sixteen; addr + 32 for tiles 2 and 3)
__device__ __forceinline__ void ca_ds_read_tr_b8_x4(unsigned addr, uint2 (&lo)[2], uint2 (&hi)[2]) {
  asm volatile(
      "ds_read_b64_tr_b8 %0, %4\n\tds_read_b64_tr_b8 %2, %4 offset:640\n\t"
      "ds_read_b64_tr_b8 %1, %4 offset:16\n\tds_read_b64_tr_b8 %3, %4 offset:656\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(lo[0]), "=&v"(lo[1]), "=&v"(hi[0]), "=&v"(hi[1])
      : "v"(addr)
      : "memory");
}
static_assert(8 * CA_YS_PITCH == 640, "offsets in ca_ds_read_tr_b8_x8 / _x4 assume the 80-byte pitch inside a cell tile (rows 8 .. 15 of the tile the lane's address names)");
__device__ __forceinline__ uint4 ca_and4(uint4 a, unsigned m) { return (uint4){a.x & m, a.y & m, a.z & m, a.w & m}; }

// The bias (stored byte = y - 128) is undone by the finisher: 128 x the digit sums of the parameter images, which the
// quantiser leaves per 64-step (Wsum[Gp/64][4], Psum[N64/64][4]) -- no all-ones MFMA and no accumulator for it here.
// DEPTH pieces (4 KiB each: 64 cells x 64 genes) and their W digits are in flight per wave; the piece loop is unrolled by
// DEPTH only (fully unrolled, the scheduler hoists every piece's loads and spills).
#ifndef CA_YS_DEPTH
#define CA_YS_DEPTH 2   // measured at 100k x 5k: depth 2 / 3 waves 92 us, depth 4 / 2 waves 95, depth 1 / 4 waves 104 (5.5 TB/s stored)
#endif
#ifndef CA_YS_WAVES
#define CA_YS_WAVES 3   // waves per SIMD the register budget is set for
#endif
// What the stream needs besides the matrix: the parameter images, their per-step digit sums (the bias of the stored bytes), the two
// fixed-point exponents the quantiser used, and the float partial slabs it leaves for the finisher -- the SAME slabs, with the same
// meaning, as the vector stream's (k_ypass): YWpart [nseg][N] = the segment's share of (Y.W)_n, YTpart [nrg][Gp] = the row group's
// share of (Y^T psi)_g, so one finisher (k_yfinish) serves both.  Digits are combined in fp64 from exact integer sums.
struct ca_ys_io {
  const uint4* Wr; const uint4* Pr; const int* Wsum; const int* Psum; const int* exps;   // exps[0] for W, exps[1] for psi
  float* YWpart; float* YTpart;
  const int* esc_off; const unsigned* esc;   // the 4-bit image's escape list (k_esc_fill); null: the image is the 1-byte one (Ys)
  const unsigned short* perm;                // the 2-bit / 4-bit image (N2 > 0): [Gp] position in the segment -> gene index in the segment
};
#ifndef CA_YS4_DEPTH
#define CA_YS4_DEPTH 4   // pieces in flight per wave of the 4-bit image's own launch (2 KiB each); round 12, at four waves per SIMD: 2 is 2 us per iteration slower, 8 spills
#endif
#ifndef CA_YS4_WAVES
#define CA_YS4_WAVES 4   // waves per SIMD of the 4-bit image's own launch: 128 VGPRs, four blocks per CU -- the whole grid of cfg-3 in one round
#endif
// LDS of the 4-bit image's own launch (OWN): the staging regions, then the segment's W image (read by the row products and the escapes
// instead of a buffer load per piece), the row-escape sums, each wave's copy of psi's digits for the step, and -- past the 32-KB combine
// buffer and the tables, since it is read in the combine -- the block's column-escape sums [512 genes] int64.  37 KB: four blocks per CU (160 KB).
constexpr int CA_YS4_OFF_W = 4 * CA_YS_STAGE;
constexpr int CA_YS4_OFF_ROW = CA_YS4_OFF_W + (CA_YS_GW / 64) * 1024;
constexpr int CA_YS4_OFF_PSI = CA_YS4_OFF_ROW + 4 * 64 * 8;
constexpr int CA_YS4_COMB = 4 * (CA_YS_GW / 64) * 64 * 4 * 4;   // the combine buffer
constexpr int CA_YS4_OFF_COL = CA_YS4_OFF_PSI + 4 * 256 > CA_YS4_COMB ? CA_YS4_OFF_PSI + 4 * 256 : CA_YS4_COMB;
constexpr int CA_YS4_LDS_BYTES = CA_YS4_OFF_COL + CA_YS_GW * 8;
static_assert(CA_YS4_OFF_PSI + 4 * 256 <= CA_YS4_OFF_COL && CA_YS4_COMB <= CA_YS4_OFF_COL, "the 4-bit launch's tables and the combine buffer lie below its column-escape sums");
static_assert(4 * CA_YS4_LDS_BYTES <= 160 * 1024, "four blocks of the 4-bit launch per CU");
// Y4: the loop image is the 4-bit one (k_pack_y4) and its escape list is added exactly -- row side into the cell's 64-bit sum before it
// becomes a float, column side into the block's integer combine -- so YWpart / YTpart are the 1-byte image's to the last bit.
// OWN (with Y4: the series form's own launch, k_ys_mfma / k_ys_mfma_ovf; CA_YS4_LDS_BYTES of LDS): the escapes come off the critical
// path -- the strip's step offsets are read once, a step's first 128 entries are loaded when the step starts (their wait is a piece's),
// both sides of an entry are LDS operations (fix(W_g) from the block's W image, fix(psi_n) from the step's digits, row and column sums
// in LDS int64) -- and the register budget is the one of four waves per SIMD: W from LDS, psi masked per MFMA.  The riding forms keep OWN
// = false: the same sums, the layout of CA_YS_LDS_BYTES.
// N2 > 0 (OWN with Y4 only, CA_VAR_Y2): the image is the 2-bit / 4-bit one (k_pack_y2) -- the first N2 gene blocks of the segment arrive as 1-KiB pieces of 2-bit
// counts, the segment's W image in LDS is gathered into the image's private gene order at the block's head, the escape list's gene fields are positions in that
// order, and YTpart is written at the gene's own index through io.perm.  The same integers as N2 = 0, which compiles to the launch as it was.
template <int DEPTH = CA_YS_DEPTH, bool Y4 = false, bool OWN = false, int N2 = 0>
__device__ __forceinline__ void ca_ys_mfma_body(int blk, const uint8_t* __restrict__ Ys, const ca_ys_io& io, int64_t N, int Gp,
                                                int RS /* cells per strip, multiple of 64 */,
                                                unsigned char* ca_ys_lds /* 16-byte aligned, CA_YS_LDS_BYTES: [4 waves][4 cell tiles][CA_YS_TILE], reused for the combine */) {
  const uint4* __restrict__ Wr = io.Wr;
  const uint4* __restrict__ Pr = io.Pr;
  constexpr bool Y4L = Y4 && OWN;
  constexpr int NP = CA_YS_GW / 64;
  static_assert(NP % DEPTH == 0, "pieces per cell step must be a multiple of the pipeline depth");
  static_assert(N2 == 0 || (Y4 && OWN && N2 < NP), "the 2-bit blocks belong to the 4-bit image's own launch");
  constexpr int SB2 = N2 * 1024 + (NP - N2) * 2048;   // (N2 > 0) bytes of a (cell step, segment): N2 narrow pieces, then the wide ones
  const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  // the wave index as a SCALAR: strip bounds, piece addresses and the piece loop are then wave-uniform (scalar registers, scalar
  // branches, loads of the form global_load v, v_off, s[base]) instead of 64-bit vector arithmetic per lane -- the kernel that rides
  // on the forward sweep has 128 vector registers for everything
  // (& 3, & 255 below: a 512-thread launch runs TWO units per block, waves 0-3 and 4-7 each with their own LDS region -- k_fwd_bal_ys;
  //  in a 256-thread launch they change nothing)
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6) & 3);
  const int nseg = Gp / CA_YS_GW;
  const int rg = blk / nseg, seg = blk - rg * nseg;
  unsigned char* my = ca_ys_lds + (size_t)wv * CA_YS_STAGE;
  const int64_t c0 = ((int64_t)rg * 4 + wv) * RS;             // first cell of this wave's strip
  const int64_t c1 = (c0 + RS < N) ? c0 + RS : N;             // (rows up to the next multiple of 64 exist and hold zeros)
  const int g0 = seg * CA_YS_GW;
  const unsigned grp = (unsigned)(j >> 2);
  // psi's row-group masks, two forms of the same thing: msk[] is read only where !Y4L (prm[], once per cell step), gsel only where Y4L (per MFMA); each
  // instantiation uses one, the other is dead code the compiler drops
  unsigned msk[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) msk[t] = grp == (unsigned)t ? 0xFFFFFFFFu : 0u;
  const unsigned gsel = 0xFFu << (8u * grp);   // (Y4L) the same masks in one register: msk[t] = the sign-extended byte t
  ca_i32x4 acc_yt[NP];
#pragma unroll
  for (int a = 0; a < NP; ++a) acc_yt[a] = (ca_i32x4){0, 0, 0, 0};
  // staging: load instruction i of a piece covers rows 16 i .. 16 i + 15 (cell tile i), 64 bytes each; row 16 t + r of the region is at t * CA_YS_TILE + r * CA_YS_PITCH
  const int lrow = lane >> 2, lch = lane & 3;
  unsigned char* wr_dst = my + lrow * CA_YS_PITCH + 16 * lch;
  const unsigned char* rd_row = my + j * CA_YS_PITCH + 16 * q;
  const unsigned rd_tr = (unsigned)(size_t)my + (unsigned)(q * CA_YS_TILE + (j >> 1) * CA_YS_PITCH + 8 * (j & 1));   // (lane group q reads cell tile q)
  constexpr int PB = Y4 ? 2048 : 4096, NL = PB / 1024;                              // bytes of a piece, 1-KiB loads per piece
  const uint8_t* src = N2 > 0 ? Ys + ((c0 >> 6) * (int64_t)nseg + seg) * SB2        // (scalar) the strip's first (cell step, segment) of the 2-bit / 4-bit image
                              : Ys + ((c0 >> 6) * (int64_t)(Gp / 64) + (g0 >> 6)) * PB;     // (scalar) piece (cell step, gene block), 1 KiB per load
  const uint4* wsrc = Wr + (int64_t)(g0 >> 6) * 64;                                 // (scalar)
  const unsigned voff = 16u * (unsigned)lane;                                       // the lane's 16 bytes of a 1-KiB load
  uint4 R[DEPTH][NL], W[DEPTH];
  // pieces of the strip: cell step st (64 cells), gene block a (0 .. NP-1); DEPTH pieces in flight
  const int nsteps = c0 < c1 ? (int)((c1 - c0 + 63) / 64) : 0;
  // Buffer loads: a scalar base (the strip's first piece; the segment's W image; psi's image) in a resource descriptor, the piece's byte offset in a
  // scalar register, the lane's 16 bytes in ONE vector register -- no 64-bit vector address per stream, which the riding form's register budget
  // (128, the sweep's) has no room for.  Offsets are 32-bit: the host uses this stream only where RS * Gp and 16 N stay far below 2^31.
  typedef unsigned ca_v4u __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(src), 0, 0x7FFFFFFF, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(wsrc), 0, NP * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(Pr + (c0 >> 6) * 64), 0, 0x7FFFFFFF, 0x00020000);
  // Cache policy of the piece loads: the non-temporal hint, except in the 4-bit image's own launch (round 19).  That launch reads the same image once per
  // iteration and nothing as large in between.  Measured by alternation only (profiles/r19_stream_ab.txt: 97.4 - 98.3 us per iteration against 98.9 - 99.9 with the
  // hint, no region overlapping).  Supposed, not measured: that part of the image (160 MB at the headline shape) is still in the memory-side cache on the next
  // pass -- the launch's HBM read bytes were not counted.  The riding forms share the sweep's lines: hint kept.
  auto issue = [&](int slot, int st, int a, unsigned vo) {
    const int so = N2 > 0 ? st * nseg * SB2 + (a < N2 ? a * 1024 : N2 * 1024 + (a - N2) * 2048) : (st * (Gp / 64) + a) * PB;   // (scalar)
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      if (N2 > 0 && i > 0 && a < N2) continue;   // (a narrow piece is one load; `a` is a constant wherever this is called)
      const ca_v4u v = __builtin_amdgcn_raw_buffer_load_b128(ry, (int)(vo + 1024u * (unsigned)i), so, Y4L ? 0 : 2 /* nt: streamed once */);
      R[slot][i] = (uint4){v.x, v.y, v.z, v.w};
    }
    if (!Y4L) {
      const ca_v4u w = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)voff, a * 1024, 0);
      W[slot] = (uint4){w.x, w.y, w.z, w.w};
    }
  };
  // Y4L: the block's tables (the segment's W image, loaded before the first pieces so that its wait is not theirs; the column-escape
  // sums zeroed), and the strip's escape offsets at its cell steps, lane st = the first entry of step st (lane nsteps: the end)
  uint4* wl = reinterpret_cast<uint4*>(ca_ys_lds + CA_YS4_OFF_W);
  unsigned long long* colesc = reinterpret_cast<unsigned long long*>(ca_ys_lds + CA_YS4_OFF_COL);
  uint4 wimg[2], pidx[2][2];
  int eoff = 0;
  if (Y4L) {
    wimg[0] = wsrc[threadIdx.x];
    wimg[1] = wsrc[threadIdx.x + CA_YM_TB];
    if (N2 > 0) {   // the sixteen genes behind each of the thread's two 16-byte rows of the permuted image: positions 16 (x >> 4) .. + 15 of the segment, x = the row
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const uint4* pq = reinterpret_cast<const uint4*>(io.perm + g0 + 16 * (((int)threadIdx.x + h2 * CA_YM_TB) >> 4));
        pidx[h2][0] = pq[0]; pidx[h2][1] = pq[1];
      }
    }
    if (lane <= nsteps) eoff = io.esc_off[((int64_t)blk * 4 + wv) * RS + (64 * lane < RS ? 64 * lane : RS)];
  }
  uint4 pr_nx = {0u, 0u, 0u, 0u};
  if (nsteps > 0) {
    if (Y4L) {   // psi's digits of the first step, in front of its pieces
      const ca_v4u pv = __builtin_amdgcn_raw_buffer_load_b128(rp, (int)voff, 0, 0);
      pr_nx = (uint4){pv.x, pv.y, pv.z, pv.w};
    }
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_) issue(d_, 0, d_, voff);
  }
  if (Y4L) {
    static_assert(2 * CA_YM_TB == CA_YS_GW, "the block's threads hold the segment's W image and column sums in two halves");
    if (N2 > 0) {
      // gather the W image into the private order: the image as the quantiser left it goes through the staging regions (8 KiB of their 22, no piece is parked yet),
      // and row x = (block a, lane 16 q + j) takes byte (digit j & 3, gene) of each of its sixteen genes -- the address the escapes use
      uint4* tmp = reinterpret_cast<uint4*>(ca_ys_lds);
      tmp[threadIdx.x] = wimg[0];
      tmp[threadIdx.x + CA_YM_TB] = wimg[1];
      __syncthreads();
      const unsigned char* tb = reinterpret_cast<const unsigned char*>(tmp) + 16 * ((int)threadIdx.x & 3);
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        unsigned w4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          const uint4& pv = pidx[h2][b >> 3];
          const unsigned two = (b & 7) < 2 ? pv.x : (b & 7) < 4 ? pv.y : (b & 7) < 6 ? pv.z : pv.w;
          const int gi = (int)((two >> (16 * (b & 1))) & 511u);
          w4[b >> 2] |= (unsigned)tb[((gi >> 6) * 64 + 16 * ((gi >> 4) & 3)) * 16 + (gi & 15)] << (8 * (b & 3));
        }
        wimg[h2] = (uint4){w4[0], w4[1], w4[2], w4[3]};
      }
      // (the barrier below also orders these reads of the staging regions before any wave parks a piece there)
    }
    wl[threadIdx.x] = wimg[0];
    wl[threadIdx.x + CA_YM_TB] = wimg[1];
    colesc[threadIdx.x] = 0ull;
    colesc[threadIdx.x + CA_YM_TB] = 0ull;
    __syncthreads();
  }
  // Round 5: the gene blocks of a cell step are UNROLLED, so that every accumulator is a fixed register (the loop over pieces with a switch on the
  // block index moved the 32 accumulator registers through chains of copies: ~40 v_mov per piece), the column products chain straight onto their
  // accumulator, and the images are never masked per piece -- row products: one accumulator per cell tile against the UNMASKED W image (K = 1: its
  // four column groups repeat the digits, so every group holds the tile's sums and the flush picks its own); column products: psi's image masked to
  // one row group per gene tile once per cell step.  Vector instructions per 4-KiB piece: ~76 -> 2, and with the buffer loads above the merged forward kernel
  // no longer spills (128 VGPRs, 6 spilled -> 0).  Measured: the launch's time at cfg-3 does NOT change (within +-1 us; 25k cells -1 us) -- what the
  // riding stream costs the sweep is its wave slot, not its instructions (profiles/r05_stream_slot.txt).
  ca_i32x4 acc_yw[4];
  uint4 prm[4];
  // bias of the row products: 128 x (digit sums of the segment's W image) per digit -- wave-uniform addresses, so the sums live
  // in scalar registers for the whole strip and cost the piece loop no vector register; a lane picks digit p = j & 3 at the flush
  int wtot[4] = {0, 0, 0, 0};
  if (!Y4) {
    const int* ws = io.Wsum + (g0 >> 6) * 4;
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
      for (int p_ = 0; p_ < 4; ++p_) wtot[p_] += ws[a * 4 + p_];
  }
  const int e_w = io.exps[0];
  // Y4: the bucket of this wave (its strip of the block's segment) in the escape list, and 64 int64 slots of LDS past the four staging
  // regions where a cell step's row-side escapes are summed (slot = cell in the step)
  const int64_t kb = ((int64_t)blk * 4 + wv) * RS;
  unsigned long long* rowesc = reinterpret_cast<unsigned long long*>(ca_ys_lds + (Y4L ? CA_YS4_OFF_ROW : 4 * CA_YS_STAGE)) + wv * 64;
  unsigned char* psl = ca_ys_lds + CA_YS4_OFF_PSI + wv * 256;   // (Y4L) psi's digits of the step: [cell quarter][digit][16 cells]
  if (Y4) rowesc[lane] = 0ull;
  for (int st = 0; st < nsteps; ++st) {
    const int64_t cs = c0 + (int64_t)st * 64;
    const bool more = st + 1 < nsteps;   // (wave-uniform)
    uint4 pr;
    if (Y4L) {
      pr = pr_nx;   // (loaded in front of the step's first pieces: the piece loop, below)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc_yw[t] = (ca_i32x4){0, 0, 0, 0};
    } else {
      // (the wait for this load is also the wait for the step's first piece, which is needed next anyway; a stream wave has ~2000 cycles per piece)
      const ca_v4u pv = __builtin_amdgcn_raw_buffer_load_b128(rp, (int)voff, st * 1024, 0);
      pr = (uint4){pv.x, pv.y, pv.z, pv.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) { acc_yw[t] = (ca_i32x4){0, 0, 0, 0}; if (!Y4L) prm[t] = ca_and4(pr, msk[t]); }
    }
    // Y4L: the step's first 128 escape entries (two per lane), issued after the step's own pieces and before the next step's: waited for
    // at the end of the step, when only the younger pieces are still in flight
    int e_lo = 0, e_hi = 0;
    unsigned en0 = 0u, en1 = 0u;
    if (Y4L) {
      e_lo = __builtin_amdgcn_readlane(eoff, st);
      e_hi = __builtin_amdgcn_readlane(eoff, st + 1);
      if (e_hi > e_lo) {   // (uniform; past the last entry: the last one again, never used)
        en0 = io.esc[e_lo + lane < e_hi ? e_lo + lane : e_hi - 1];
        en1 = io.esc[e_lo + 64 + lane < e_hi ? e_lo + 64 + lane : e_hi - 1];
      }
    }
#pragma unroll
    for (int a = 0; a < NP; ++a) {
      const int slot = a % DEPTH;
      __builtin_amdgcn_sched_barrier(0);   // (pieces one after the other: hoisting the next piece's LDS reads over this one's costs registers the sweep's budget has not)
      // the piece is in R[slot]: park it in LDS, start the loads of the piece DEPTH further on, then feed the matrix core
      const uint4 wr = Y4L ? wl[a * 64 + lane] : W[slot];
      if (Y4) {
        // the four cell tiles' A operands are the nibbles of the two loads: row products from registers, the bytes parked in LDS (row
        // 16 t + j, bytes 16 q ..) only for the transposed reads of the column products
        // (one tile at a time: four registers of unpacked bytes live, not sixteen -- the riding form's budget is 128)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bool nar = N2 > 0 && a < N2;   // (compile time: the block loop is unrolled) a narrow piece holds the four tiles in one load, two bits each
          const uint4 v = R[slot][nar ? 0 : t >> 1];
          const int sh = nar ? 2 * t : 4 * (t & 1);
          const uint4 av = ca_and4((uint4){v.x >> sh, v.y >> sh, v.z >> sh, v.w >> sh}, nar ? 0x03030303u : 0x0F0F0F0Fu);
          *reinterpret_cast<uint4*>(const_cast<unsigned char*>(rd_row) + t * CA_YS_TILE) = av;
          acc_yw[t] = ca_mfma_i8(av, wr, acc_yw[t]);
        }
        if (a + DEPTH < NP) issue(slot, st, a + DEPTH, voff);
        else if (Y4L) {
          // (round 12) the next step's first pieces WITHOUT a branch: the counter pass then waits for this step's last pieces with a counted vmcnt, not
          // with the stricter wait of two paths.  Past the strip's last step the lanes' offsets lie beyond the resource's range: a buffer load out of range
          // moves nothing and returns zeros.  psi's digits of the next step go out in front of its first piece, so their wait is that piece's and the escapes
          // and the flush of this step run with DEPTH pieces in flight.
          const unsigned vo = more ? voff : 0x80000000u + voff;
          if (a + DEPTH == NP) {
            const ca_v4u pv = __builtin_amdgcn_raw_buffer_load_b128(rp, (int)vo, (st + 1) * 1024, 0);
            pr_nx = (uint4){pv.x, pv.y, pv.z, pv.w};
          }
          issue(slot, st + 1, a + DEPTH - NP, vo);
        } else if (more) issue(slot, st + 1, a + DEPTH - NP, voff);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(wr_dst + i * CA_YS_TILE) = R[slot][i];
        if (a + DEPTH < NP) issue(slot, st, a + DEPTH, voff);
        else if (more) issue(slot, st + 1, a + DEPTH - NP, voff);
        // row products: the four cell tiles against this 64-gene block
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const uint4 av = *reinterpret_cast<const uint4*>(rd_row + t * CA_YS_TILE);
          acc_yw[t] = ca_mfma_i8(av, wr, acc_yw[t]);
        }
      }
      // column products: the four gene tiles of the block against the 64 cells, one accumulator (tile t -> rows 4t .. 4t+3)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        uint2 lo[2], hi[2];
        ca_ds_read_tr_b8_x4(rd_tr + 32u * (unsigned)h2, lo, hi);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          uint4 pa;
          if (Y4L) {   // psi masked to row group 2 h2 + t here, not held four times over the step: four ANDs against the lane's mask (round 19; before, a compare and selects per MFMA)
            // The lane's mask for group 2 h2 + t is one signed byte field of gsel (0xFF in byte `grp`): a single vector instruction, no lane-mask SGPR and none
            // of its wait states.  asm volatile: the four masked images are not shared between the pieces -- sixteen registers the budget has not.
            // (the "n" offset is a constant because the h2 and t loops are fully unrolled: this builds with optimisation on only, like the rest of the file's asm)
            unsigned m_;
            asm volatile("v_bfe_i32 %0, %1, %2, 8" : "=v"(m_) : "v"(gsel), "n"(8 * (2 * h2 + t)));
            pa = ca_and4(pr, m_);
          } else {
            pa = prm[2 * h2 + t];
          }
          acc_yt[a] = ca_mfma_i8(pa, (uint4){lo[t].x, lo[t].y, hi[t].x, hi[t].y}, acc_yt[a]);
        }
      }
    }
    if (Y4L) {   // the step's escapes, one per lane, both sides from LDS: excess x fix(W_g) into the cell's row sum, excess x fix(psi_n) into the gene's
      if (j < 4) *reinterpret_cast<uint4*>(psl + (4 * q + j) * 16) = pr;   // lane (q, digit j) of column group 0: cells 16 q + b
      const unsigned char* wlb = reinterpret_cast<const unsigned char*>(wl);
      auto esc1 = [&](unsigned en) {
        const int c = (int)(en & 63u), gi = (int)((en >> 9) & 511u);
        const unsigned char* dw = wlb + ((gi >> 6) * 64 + 16 * ((gi >> 4) & 3)) * 16 + (gi & 15);
        const unsigned char* dp = psl + 64 * (c >> 4) + (c & 15);
        // x = sum_p d_p 256^p modulo 2^32 (|x| < 2^31: exact)
        unsigned fw = 0u, fp = 0u;
#pragma unroll
        for (int p_ = 0; p_ < 4; ++p_) {
          fw += (unsigned)(int)(signed char)dw[16 * p_] << (8 * p_);
          fp += (unsigned)(int)(signed char)dp[16 * p_] << (8 * p_);
        }
        const long long x = (long long)(en >> 18);
        atomicAdd(rowesc + c, (unsigned long long)(x * (long long)(int)fw));
        atomicAdd(colesc + gi, (unsigned long long)(x * (long long)(int)fp));
      };
      const int ne = e_hi - e_lo;
      if (lane < ne) esc1(en0);
      if (64 + lane < ne) esc1(en1);
      for (int e = e_lo + 128 + lane; e < e_hi; e += 64) esc1(io.esc[e]);
    } else if (Y4) {   // the step's escapes, one per lane: excess x fix(W_g), the full fixed-point value reassembled from the digits the MFMAs took
      const int64_t sc = (int64_t)st * 64;
      const int e1 = io.esc_off[kb + ((sc + 64 < RS) ? sc + 64 : RS)];
      const signed char* wd = reinterpret_cast<const signed char*>(Wr);
      for (int e = io.esc_off[kb + sc] + lane; e < e1; e += 64) {
        const unsigned en = io.esc[e];
        const int g = g0 + (int)((en >> 9) & 511u);
        const signed char* d = wd + ((int64_t)(g >> 6) * 64 + 16 * ((g >> 4) & 3)) * 16 + (g & 15);
        const long long x = (long long)d[0] + (long long)d[16] * 256ll + (long long)d[32] * 65536ll + (long long)d[48] * 16777216ll;
        atomicAdd(rowesc + ((en & 511u) & 63u), (unsigned long long)((long long)(en >> 18) * x));
      }
    }
    {   // the cell step is complete: lane (column 4t + p, q) holds cells 16 t + 4 q + r, digit p
      const int t = j >> 2, p = j & 3;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = cs + 16 * t + 4 * q + r;
        const int wb = p == 0 ? wtot[0] : p == 1 ? wtot[1] : p == 2 ? wtot[2] : wtot[3];
        const int ar = t == 0 ? acc_yw[0][r] : t == 1 ? acc_yw[1][r] : t == 2 ? acc_yw[2][r] : acc_yw[3][r];
        long long v = ((long long)ar + 128ll * (long long)wb) << (8 * p);   // digit p of the quad's four (lanes j & 3): exact in 64 bits
        if (Y4 && p == 0) v += (long long)rowesc[16 * t + 4 * q + r];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        if (p == 0 && n < N) io.YWpart[(int64_t)seg * N + n] = (float)ldexp((double)v, -e_w);
      }
      if (Y4) rowesc[lane] = 0ull;   // (after every lane's reads: a wave's LDS operations complete in order)
    }
  }
  // column products of the strip: lane (gene n = j, q), accumulator a: gene tile 4 a + q, digits r = 0..3; combine the four
  // strips of the block in LDS (integer sums: any order), one row of YTi per block
  __syncthreads();
  int* comb = reinterpret_cast<int*>(ca_ys_lds);   // [4 waves][8 acc][64 lanes][4]: 32 KB > the 22 KB of tiles: the launch asks for 32 KB
#pragma unroll
  for (int a = 0; a < NP; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) comb[((wv * NP + a) * 64 + lane) * 4 + r] = acc_yt[a][r];
  __syncthreads();
  if (Y4 && !OWN) {   // the strip's escapes, four lanes per entry (lane & 3 = digit r of fix(psi_n)): excess x digit into the combine
    const signed char* pd = reinterpret_cast<const signed char*>(Pr);
    const int r = lane & 3;
    const int e1 = io.esc_off[kb + RS];
    for (int e = io.esc_off[kb] + (lane >> 2); e < e1; e += 16) {
      const unsigned en = io.esc[e];
      const int64_t n = c0 + (int64_t)(en & 511u);
      const int gi = (int)((en >> 9) & 511u);
      const int d = pd[((n >> 6) * 64 + 16 * ((n >> 4) & 3) + r) * 16 + (n & 15)];
      atomicAdd(comb + ((wv * NP + (gi >> 6)) * 64 + (gi & 63)) * 4 + r, (int)(en >> 18) * d);
    }
    __syncthreads();
  }
  // bias of the column products: 128 x (digit sums of psi's image over the block's cell steps); scale 2^-e_psi
  long long pb[4] = {0, 0, 0, 0};
  if (!Y4) {
    const int64_t s0_ = ((int64_t)rg * 4 * RS) >> 6;
    const int64_t s1_ = (((int64_t)rg * 4 + 4) * RS < ((N + 63) / 64) * 64 ? ((int64_t)rg * 4 + 4) * RS : ((N + 63) / 64) * 64) >> 6;
    for (int64_t st = s0_; st < s1_; ++st) {
      const int4 d4 = *reinterpret_cast<const int4*>(io.Psum + st * 4);
      pb[0] += d4.x; pb[1] += d4.y; pb[2] += d4.z; pb[3] += d4.w;
    }
  }
  const double inv_p = ldexp(1.0, -io.exps[1]);
  for (int i = (int)threadIdx.x & (CA_YM_TB - 1); i < NP * 64; i += CA_YM_TB) {
    const int l = i & 63, a = i >> 6;
    double v = 0.0;
#pragma unroll
    for (int r = 3; r >= 0; --r) {
      const int o = i * 4 + r;
      const int sr = (comb[o] + comb[o + NP * 256]) + (comb[o + 2 * NP * 256] + comb[o + 3 * NP * 256]);
      v = v * 256.0 + (double)((long long)sr + 128 * pb[r]);
    }
    const int gl = 16 * (4 * a + (l >> 4)) + (l & 15), gene = g0 + (N2 > 0 ? (int)io.perm[g0 + gl] : gl);   // (N2 > 0: gl is a position, the gene's own index through the map)
    if (Y4L) v += (double)(long long)colesc[gl];   // (integers below 2^53 throughout: the same total as the escapes added digit by digit)
    io.YTpart[(int64_t)rg * Gp + gene] = (float)(v * inv_p);
  }
}
template <bool Y4, int N2 = 0>
__global__ void __launch_bounds__(CA_YM_TB, Y4 ? CA_YS4_WAVES : CA_YS_WAVES) k_ys_mfma(const uint8_t* __restrict__ Ys, ca_ys_io io, int64_t N, int Gp, int RS) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ca_ys_dyn[];   // Y4: CA_YS4_LDS_BYTES, else CA_YS_LDS_BYTES
  ca_ys_mfma_body<Y4 ? CA_YS4_DEPTH : CA_YS_DEPTH, Y4, true, N2>((int)blockIdx.x, Ys, io, N, Gp, RS, ca_ys_dyn);
}
// (the riding forms -- k_fwd_cell_mix_ys, k_fwd_bal_ys -- are instantiated per format: the 1-byte ones are round 6's code; the 4-bit ones exist
//  only for the series form's rank-one shapes (D = 1, no c16 / s2), whose sweeps run only in the passes the series form hands over)
constexpr int CA_YS_LDS_BYTES = 4 * (CA_YS_GW / 64) * 64 * 4 * 4;   // the combine buffer (32 KB) >= 4 x CA_YS_STAGE (+ 4 x 64 x 8 B of the 4-bit image's row escapes)
static_assert(4 * CA_YS_STAGE + 4 * 64 * 8 <= CA_YS_LDS_BYTES, "staging + row escapes fit the combine buffer");

// Parameter images of the one-copy stream for one parameter state.  The fixed-point exponents need the largest magnitudes of W
// and psi: lag = 0 takes them from amax_in as exact maxima (k_ym_absmax ran before: ONE pair); in the loop amax_in holds the PREVIOUS
// state's maxima as per-block pairs (what this body left last time) and `slack` bounds what the Adam steps since can add to any
// magnitude (TF1 Adam: |step| <= lr_t (1 - b1) / sqrt((1 - b2)(1 - b1^2 / b2)), Cauchy-Schwarz on the two moving averages), so
// 2^e (max + slack) < 2^30 holds without a second pass.  Every block reduces the n_in pairs itself (a few KB from L2) and leaves
// its own pair in amax_out -- no atomics: the first form of this kernel raised one atomicMax per wave on two addresses and spent
// 20 of its 25 us queueing there (rocprofv3, profiles/r03_ab_ystream.txt).  Block 0 writes the exponents used to exps[2] for
// the stream.  Digit sums per 64-step go to Wsum / Psum (the bias of the stored bytes).  K = 1.
// In the loop the body runs as EXTRA BLOCKS of the per-cell Adam kernel (k_adam_cell), which is where W and psi become final.
struct ca_ysq_args {
  int nblk;                       // blocks of the quantiser (0 = none riding)
  const float* V; int Dv; int64_t G; int GS; const float* F; int Df; int64_t N; int64_t NS;
  const float* amax_in; int n_in; float slack_w, slack_p;
  float* amax_out;                // [nblk][2]
  int* exps; uint4* Wr; uint4* Pr; int* Wsum; int* Psum;
};
// One wave's 64-step of an image from entries that are in registers: vals[b] = entry 16 (l >> 4) + b of the step, own = entry l.
// Block-level: every thread of the block calls it (two barriers); `out` = this block's pair in amax_out.
__device__ __forceinline__ void ca_ys_quant_core(const ca_ysq_args& a, bool live, bool isw, int64_t step, const float (&vals)[16], float own,
                                                 int out, bool write_exps, float* sm /* >= 2 * (CA_YM_TB / 64) floats */) {
  const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
  // largest magnitudes of the state amax_in describes
  float mw = 0.f, mp = 0.f;
  for (int i = tid; i < a.n_in; i += CA_YM_TB) { mw = fmaxf(mw, a.amax_in[2 * i]); mp = fmaxf(mp, a.amax_in[2 * i + 1]); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mw = fmaxf(mw, __shfl_xor(mw, o, 64)); mp = fmaxf(mp, __shfl_xor(mp, o, 64)); }
  if (l == 0) { sm[2 * wv] = mw; sm[2 * wv + 1] = mp; }
  __syncthreads();
  mw = fmaxf(fmaxf(sm[0], sm[2]), fmaxf(sm[4], sm[6]));
  mp = fmaxf(fmaxf(sm[1], sm[3]), fmaxf(sm[5], sm[7]));
  __syncthreads();
  const int ew = ca_fix_exp(mw + a.slack_w), ep = ca_fix_exp(mp + a.slack_p);
  if (write_exps && tid == 0) { a.exps[0] = ew; a.exps[1] = ep; }
  float m = 0.f;
  if (live) {
    const float sc = ldexpf(1.f, isw ? ew : ep);
    // byte (l, b) of the step's image = digit p = l & 3 of fix(entry 16 (l >> 4) + b), from the entries already in registers
    const int p = l & 3;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int x = (int)rintf(fminf(fmaxf(vals[b] * sc, -2147483000.f), 2147483000.f));
      w[b >> 2] |= ((unsigned)ca_digit(x, p) & 0xFFu) << (8 * (b & 3));
    }
    const uint4 v = {w[0], w[1], w[2], w[3]};
    (isw ? a.Wr : a.Pr)[step * 64 + l] = v;
    int sd = 0;   // digit sums of the step (lanes with column p = l & 3 in the first group hold digit p for the 16 entries of group q)
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int b = 0; b < 4; ++b) sd += (int)(signed char)((w[d] >> (8 * b)) & 0xFFu);
    sd += __shfl_xor(sd, 16, 64);
    sd += __shfl_xor(sd, 32, 64);
    if (l < 4) (isw ? a.Wsum : a.Psum)[step * 4 + l] = sd;
    // exact maximum of this step's 64 entries, one per lane
    m = fabsf(own);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  }
  if (l == 0) { sm[2 * wv] = isw ? m : 0.f; sm[2 * wv + 1] = isw ? 0.f : m; }
  __syncthreads();
  if (tid == 0) {
    a.amax_out[2 * out] = fmaxf(fmaxf(sm[0], sm[2]), fmaxf(sm[4], sm[6]));
    a.amax_out[2 * out + 1] = fmaxf(fmaxf(sm[1], sm[3]), fmaxf(sm[5], sm[7]));
  }
}
__device__ __forceinline__ void ca_ys_quant_body(int blk, const ca_ysq_args& a, float* sm /* >= 2 * (CA_YM_TB / 64) floats */) {
  const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
  // this wave's 64-step of an image: its sixteen entries per lane (and the lane's own entry, for the step's exact maximum) are
  // loaded FIRST -- their addresses do not depend on the exponents, so the round trip runs beside the reduction in the core
  const int64_t st = (int64_t)blk * (CA_YM_TB / 64) + wv;      // one wave per 64-step of an image
  const bool live = st < a.GS + a.NS;
  const bool isw = !live || st < a.GS;
  const float* src = isw ? a.V : a.F;
  const int ld = isw ? a.Dv : a.Df;
  const int64_t rows = isw ? a.G : a.N, step = live ? (isw ? st : st - a.GS) : 0;
  float vals[16], own = 0.f;
  {
    const int64_t r0 = step * 64 + 16 * (l >> 4);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int64_t r = r0 + b;
      vals[b] = (live && r < rows) ? src[r * ld] : 0.f;
    }
    const int64_t r = step * 64 + l;
    if (live && r < rows) own = src[r * ld];
  }
  ca_ys_quant_core(a, live, isw, step, vals, own, blk, blk == 0, sm);
}
// Wave-level form of ca_ys_quant_core for ONE 64-step whose entries are in registers (round 4, the gene blocks of k_update_merged): no
// block-level operation; returns the step's exact maximum (wave-uniform).  The exponents come from the same maxima (a maximum does not
// depend on the order it is taken in), everything else is the core's arithmetic.
__device__ __forceinline__ float ca_ys_quant_wave(const ca_ysq_args& a, bool live, bool isw, int64_t step, float own, bool write_exps) {
  const int l = threadIdx.x & 63;
  float vals[16];
#pragma unroll
  for (int b = 0; b < 16; ++b) vals[b] = __shfl(own, 16 * (l >> 4) + b, 64);
  float mw = 0.f, mp = 0.f;
  for (int i = l; i < a.n_in; i += 64) { mw = fmaxf(mw, a.amax_in[2 * i]); mp = fmaxf(mp, a.amax_in[2 * i + 1]); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mw = fmaxf(mw, __shfl_xor(mw, o, 64)); mp = fmaxf(mp, __shfl_xor(mp, o, 64)); }
  const int ew = ca_fix_exp(mw + a.slack_w), ep = ca_fix_exp(mp + a.slack_p);
  if (write_exps && l == 0) { a.exps[0] = ew; a.exps[1] = ep; }
  float m = 0.f;
  if (live) {
    const float sc = ldexpf(1.f, isw ? ew : ep);
    const int p = l & 3;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int x = (int)rintf(fminf(fmaxf(vals[b] * sc, -2147483000.f), 2147483000.f));
      w[b >> 2] |= ((unsigned)ca_digit(x, p) & 0xFFu) << (8 * (b & 3));
    }
    const uint4 v = {w[0], w[1], w[2], w[3]};
    (isw ? a.Wr : a.Pr)[step * 64 + l] = v;
    int sd = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int b = 0; b < 4; ++b) sd += (int)(signed char)((w[d] >> (8 * b)) & 0xFFu);
    sd += __shfl_xor(sd, 16, 64);
    sd += __shfl_xor(sd, 32, 64);
    if (l < 4) (isw ? a.Wsum : a.Psum)[step * 4 + l] = sd;
    m = fabsf(own);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  }
  return m;
}
// The same images made where the entries are BORN (round 4, k_update_merged): a block of 256 genes (cells) has just stepped W_g0 (psi_n0),
// one entry per lane = four 64-steps of the W (psi) image; the sixteen entries a lane packs come from its wave-mates by shuffle.
// `own` = this lane's entry (0 past the last row).  Same arithmetic on the same floats as ca_ys_quant_body reading them back.
__device__ __forceinline__ void ca_ys_quant_inreg(const ca_ysq_args& a, bool isw, int blk, float own, int out, bool write_exps, float* sm) {
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t step = (int64_t)blk * (CA_YM_TB / 64) + wv;
  const bool live = step < (isw ? (int64_t)a.GS : a.NS);
  float vals[16];
#pragma unroll
  for (int b = 0; b < 16; ++b) vals[b] = __shfl(own, 16 * (l >> 4) + b, 64);
  ca_ys_quant_core(a, live, isw, live ? step : 0, vals, own, out, write_exps, sm);
}
__global__ void __launch_bounds__(CA_YM_TB) k_ys_quant(ca_ysq_args a) {
  __shared__ float sm[2 * (CA_YM_TB / 64)];
  ca_ys_quant_body((int)blockIdx.x, a, sm);
}
