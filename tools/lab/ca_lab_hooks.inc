// Timing-lab hook bodies for clonealign_amd/csrc/ca_kernels.hip.h -- included ONLY under -DCA_LAB (`make -C clonealign_amd/csrc lab`).
// Every hook only reads the clock and writes a stamp; none changes a result.  Readers: tools/stamps.py (merged forward launch),
// tools/stamps_small.py (update kernels), ca_lab_read_stamps*() in tools/lab/ca_lab_host.inc.
#pragma once
// {start, end, kind, 1} of every block of the update kernels of the last iteration
__device__ unsigned long long ca_lab_stamps2[4096 * 4];
struct ca_lab_stamp {
  unsigned long long t0; int slot, kind;
  __device__ ca_lab_stamp(int slot_, int kind_) : t0(__builtin_amdgcn_s_memrealtime()), slot(slot_), kind(kind_) {}
  __device__ ~ca_lab_stamp() {
    if (threadIdx.x == 0 && slot < 4096) {
      unsigned long long* st = ca_lab_stamps2 + 4 * (size_t)slot;
      st[0] = t0; st[1] = __builtin_amdgcn_s_memrealtime(); st[2] = (unsigned long long)kind; st[3] = 1;
    }
  }
};
#define CA_LAB_STAMP(slot, kind) ca_lab_stamp ca_lab_stamp_((slot), (kind))
// checkpoints inside a block (thread 0): slot 3072 + 8 * block + i
#define CA_LAB_CP(blk, i) do { if (threadIdx.x == 0 && (blk) < 64) { __builtin_amdgcn_s_waitcnt(0); ca_lab_stamps2[4 * (3072 + 8 * (blk) + (i))] = __builtin_amdgcn_s_memrealtime(); ca_lab_stamps2[4 * (3072 + 8 * (blk) + (i)) + 3] = 2; } } while (0)
// phases inside a forward sweep block (wave 0): slot = sweep block index, i = 0 entry, 1 head done, 2 k-loop done, 3 past the combine barrier
__device__ unsigned long long ca_lab_stamps3[2048 * 4];
#define CA_LAB_PH(blk, i) do { if (threadIdx.x == 0 && (blk) < 2048) ca_lab_stamps3[4 * (blk) + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define CA_LAB_PH_AFTER(value, blk, i) do { asm volatile("" ::"v"(value)); CA_LAB_PH(blk, i); } while (0)
// phases inside a pass of the series form's cell launch (k_poly_cell, wave 0 of the first 64 blocks, their first 8 passes), shader clock cycles:
// i = 0 top of the pass, 1 bins done, 2 powers stored (the epilogue starts), 3 epilogue and d/dF done, 4 past the first barrier, 5 gather done, 6 past the second
// (CA_VAR_CELL_MFMA: 4 moments done -- the wave's own MFMA gather, no barrier to wait at -- and the pass ends there)
__device__ unsigned long long ca_lab_stamps4[64 * 8 * 8];
#define CA_LAB_CELL_PH(blk, pass, i) do { if (threadIdx.x == 0 && (blk) < 64 && (pass) < 8) ca_lab_stamps4[((blk) * 8 + (pass)) * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
#define CA_LAB_CELL_PH_AFTER(value, blk, pass, i) do { asm volatile("" ::"v"(value)); CA_LAB_CELL_PH(blk, pass, i); } while (0)
// block-level stamps of EVERY block of the series form's cell launch (tools/cell_edges.py), the 100 MHz clock all compute units share: word i of block blk --
// cell blocks (kind 1): 0 block start, 1 first pass begins (head done), 2 last pass ends, 3 block returns; finisher blocks (kind 2 row jobs, 3 column jobs): 0 start,
// 3 return -- and the kind in word 4.  One clock read and one store by thread 0 each.
__device__ unsigned long long ca_lab_stamps5[4096 * 8];
#define CA_LAB_CELL_EDGE(blk, i, kind) do { if (threadIdx.x == 0 && (blk) < 4096) { ca_lab_stamps5[(blk) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); if ((i) == 0) ca_lab_stamps5[(blk) * 8 + 4] = (kind); } } while (0)
// (the return stamp behind a block barrier: the block's last wave, not thread 0's)
#define CA_LAB_CELL_EDGE_END(blk) do { __syncthreads(); CA_LAB_CELL_EDGE(blk, 3, 0); } while (0)
// every block of the merged forward launch leaves {start, end, kind << 32 | index, HW_ID | XCC_ID << 32}
__device__ unsigned long long ca_lab_stamps[8192 * 4];
#define CA_LAB_BLOCK_T0() const unsigned long long st0_ = __builtin_amdgcn_s_memrealtime()
#define CA_LAB_BLOCK_END(kind, idx)                                                                                                     \
  do {                                                                                                                                  \
    __syncthreads();                                                                                                                    \
    if (threadIdx.x == 0 && blockIdx.x < 8192) {                                                                                        \
      unsigned long long* st = ca_lab_stamps + 4 * (size_t)blockIdx.x;                                                                  \
      st[0] = st0_; st[1] = __builtin_amdgcn_s_memrealtime();                                                                           \
      st[2] = ((unsigned long long)(kind) << 32) | (unsigned)(idx);                                                                     \
      st[3] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32); \
    }                                                                                                                                   \
  } while (0)
#define CA_LAB_LEAVE(label) goto label
#define CA_LAB_LABEL(label) label: (void)0
