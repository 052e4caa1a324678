"""numpy restatement of the host's share of the 2-bit / 4-bit loop image (CA_VAR_Y2; ca_y2_plan_impl in clonealign_amd/csrc/ca_eng_create.inc): per 512-gene
segment the genes sorted by their stored counts >= 3, ascending, ties by gene index; the escape list of N2 narrow blocks; the rule that picks N2."""
import numpy as np

SEG = 512
CANDIDATES = (6, 5)


def stored_u8(Y):
    """The resident 1-byte matrix: counts above 255 keep 255 (their excess is the overflow list's)."""
    return np.minimum(np.asarray(Y), 255).astype(np.uint8)


def gene_counts(u8):
    """(cnt3, cnt15) padded with zeros to the engine's gene count for 1-byte storage, a multiple of 1024."""
    G = u8.shape[1]
    Gp = (G + 1023) // 1024 * 1024
    c3 = np.zeros(Gp, np.int32)
    c15 = np.zeros(Gp, np.int32)
    c3[:G] = (u8 >= 3).sum(0)
    c15[:G] = (u8 >= 15).sum(0)
    return c3, c15


def plan_counts(c3, c15, counts, force_n2=0):
    """(N2, list length, perm [Gp]: position -> gene in the segment, pos [Gp]: gene -> position) from the per-gene counts."""
    Gp = c3.size
    perm = np.empty(Gp, np.uint16)
    pos = np.empty(Gp, np.uint16)
    for s in range(0, Gp, SEG):
        order = np.lexsort((np.arange(SEG), c3[s:s + SEG]))      # by count, then by index
        perm[s:s + SEG] = order
        pos[s + order] = np.arange(SEG)

    def length(n2):
        narrow = pos < 64 * n2
        return int(c3[narrow].astype(np.int64).sum() + c15[~narrow].astype(np.int64).sum())

    if force_n2 > 0:
        n2 = force_n2
    else:
        n2 = next((k for k in CANDIDATES if length(k) * 256 <= counts), 0)
    return n2, length(n2), perm, pos


def plan_np(u8, force_n2=0):
    c3, c15 = gene_counts(u8)
    return plan_counts(c3, c15, u8.shape[0] * u8.shape[1], force_n2)
