// What does ds_read_b64_tr_b4 return?  (gfx950; the sibling of tools/trb8_lab.hip for the 4-bit form.)  Every lane supplies an 8-byte-aligned
// LDS address; a nibble can name only 4 bits of where it came from, so the probe runs four passes, pass k filling every nibble of the LDS
// with bits 4k .. 4k+3 of its own nibble index (nibble 2a = low half of byte a, 2a + 1 = high half), and puts the four answers together:
// the output shows which (row, nibble column) every nibble of every lane's 64-bit result came from.  Not product code.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/trb4_lab.bin tools/trb4_lab.hip && tools/trb4_lab.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)
constexpr int LDS_BYTES = 4096;   // 8192 nibbles: 13 bits of index, four passes of 4 bits
__global__ void probe(const int* addr, unsigned long long* out, int pass) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
  for (int i = threadIdx.x; i < LDS_BYTES; i += 64) {
    const unsigned lo = ((2u * i) >> (4 * pass)) & 15u, hi = ((2u * i + 1u) >> (4 * pass)) & 15u;
    lds[i] = (unsigned char)(lo | (hi << 4));
  }
  __syncthreads();
  const unsigned a = (unsigned)(size_t)lds + (unsigned)addr[threadIdx.x];
  unsigned long long v;
  asm volatile("ds_read_b64_tr_b4 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
  out[threadIdx.x] = v;
}
int main() {
  int h_addr[64]; int* d_addr; unsigned long long *d_out, res[4][64];
  CK(hipMalloc(&d_addr, 256)); CK(hipMalloc(&d_out, 512));
  // rows of ROWB bytes inside a 16-lane group's region of 1024 bytes
  for (int scheme = 0; scheme < 3; ++scheme) {
    const int ROWB = scheme == 2 ? 32 : 64;
    for (int l = 0; l < 64; ++l) {
      const int g = l >> 4, i = l & 15;
      if (scheme == 0) h_addr[l] = 1024 * g + ROWB * i;                            // lane i: row i, bytes 0..7 (nibbles 0..15)
      else if (scheme == 1) h_addr[l] = 1024 * g + ROWB * (i >> 1) + 8 * (i & 1);   // lane 2q+p: row q, bytes 8p..8p+7 (the b8 form's addressing)
      else h_addr[l] = 1024 * g + ROWB * i;                                        // as scheme 0 with 32-byte rows (64 nibbles = one piece row)
    }
    CK(hipMemcpy(d_addr, h_addr, 256, hipMemcpyHostToDevice));
    for (int pass = 0; pass < 4; ++pass) {
      hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d_addr, d_out, pass);
      CK(hipMemcpy(res[pass], d_out, 512, hipMemcpyDeviceToHost));
    }
    printf("scheme %d (rows of %d bytes in the group's 1024-byte region; result nibble e of a lane came from [group, row, nibble column])\n", scheme, ROWB);
    for (int l = 0; l < 64; ++l) {
      if ((l & 15) == 0) printf(" group %d\n", l >> 4);
      printf("  lane %2d (gave r%2d n%3d):", l, (h_addr[l] % 1024) / ROWB, 2 * (h_addr[l] % ROWB));
      for (int e = 0; e < 16; ++e) {
        int n = 0;
        for (int pass = 0; pass < 4; ++pass) n |= (int)((res[pass][l] >> (4 * e)) & 15) << (4 * pass);
        const int byte = n >> 1;
        printf(" [g%d r%2d n%3d]", byte / 1024, (byte % 1024) / ROWB, 2 * (byte % ROWB) + (n & 1));
      }
      printf("\n");
      if (l == 15) break;   // the groups behave alike: one is printed in full, the others' first lane below
    }
    for (int l = 16; l < 64; l += 16) {
      int n = 0;
      for (int pass = 0; pass < 4; ++pass) n |= (int)(res[pass][l] & 15) << (4 * pass);
      printf("  lane %2d nibble 0 <- byte %d of the LDS (group region %d)\n", l, n >> 1, (n >> 1) / 1024);
    }
  }
  return 0;
}
