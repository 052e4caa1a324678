"""Inputs and float64 / int64 references for the device-side fit helpers (ca_init_psi_pca, the loc0 = NULL mu guess of ca_create,
ca_clone_gene_sums, ca_preprocess) on every count storage.  numpy only: tests/test_device_helper_cases_host.py checks the inputs' own
conditions without a device, tests/test_gpu_device_helpers.py holds the engine to the references."""
import functools

import numpy as np

SEED = 5   # the first seed of this generator at which every shape and variant meets the conditions below (test_device_helper_cases_host.py asserts them)
SHAPES = [(333, 95), (700, 300), (257, 1030), (37, 1100), (1100, 40)]   # ragged both ways, one gene segment or several, fewer cells than a strip
VARIANTS = ("u8", "u8ovf", "u16", "f32int", "f32frac")
STORAGE = {"u8": "u8", "u8ovf": "u8", "u16": "u16", "f32int": "f32", "f32frac": "f32"}
LARGE = ("u16", "f32int", "u8ovf")
LARGE_SHAPE = (1100, 70, 4)
GAP_MIN, SD_MIN = 1.5, 0.1


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planted(N, G, seed=SEED):
    """Counts with two planted latent factors (int64 [N, G]): f ~ N(0, 1) * (1, 0.5), loadings N(0, 0.8) on a random half of the genes,
    base ~ lognormal(0.5, 1), Y = Poisson(base * exp(f w^T)); no empty cell, no empty gene."""
    rng = np.random.default_rng(seed)
    f = rng.normal(size=(N, 2)) * np.array([1.0, 0.5])
    w = rng.normal(0.0, 0.8, size=(G, 2))
    w[rng.permutation(G)[G // 2:]] = 0.0
    base = rng.lognormal(0.5, 1.0, size=G)
    Y = rng.poisson(base[None, :] * np.exp(f @ w.T)).astype(np.int64)
    Y[:, 0] += 1
    Y[0, :] += 1
    return _frozen(Y)


@functools.lru_cache(maxsize=None)
def variant(kind, N, G, seed=SEED):
    """float64 [N, G] counts of one storage variant, derived from planted(N, G, seed)."""
    rng = np.random.default_rng([seed, VARIANTS.index(kind), N, G])
    Y = planted(N, G, seed).copy()
    if kind in ("u8", "u8ovf"):
        Y = np.minimum(Y, 255)
        if kind == "u8ovf":
            flat = rng.choice(Y.size, Y.size // 200, replace=False)
            Y.flat[flat] = rng.integers(256, 5000, size=flat.size)
    elif kind in ("u16", "f32int"):
        mult, top = (150, 65535) if kind == "u16" else (3000, (1 << 24) - 1)
        genes = rng.choice(G, max(G // 8, 1), replace=False)
        Y[:, genes] = np.minimum(Y[:, genes] * mult + rng.integers(0, mult, size=(N, genes.size)), top)
    Y = Y.astype(np.float64)
    if kind == "f32frac":
        flat = rng.choice(Y.size, Y.size // 50, replace=False)
        Y.flat[flat] += 0.5
    return _frozen(Y)


def auto_storage(Y):
    """(storage the engine's scan picks for Y, entries of its u8 overflow list): the rule of pick_ystore."""
    Y = np.asarray(Y)
    over = int((Y > 255).sum())
    if np.any(Y != np.floor(Y)):
        return "f32", 0
    if Y.max() < (1 << 24) and over * 64 <= Y.size:
        return "u8", over
    return ("u16" if Y.max() <= 65535 else "f32"), 0


def storage_arg(kind, Y):
    """y_storage for the constructor: "auto" wherever the scan itself picks the variant's storage, else the forced one."""
    return "auto" if auto_storage(Y)[0] == STORAGE[kind] else STORAGE[kind]


def copy_numbers(G, C, seed=SEED):
    L = np.random.default_rng([seed, G, C, 77]).integers(1, 5, size=(G, C)).astype(np.float64)
    L[:, 0] = 1.0 + (np.arange(G) % 3)     # (no gene with one copy number in every clone by accident of a small G)
    L[:, C - 1] = 4.0 - (np.arange(G) % 3)
    return L


# ------------------------------------------------------------------ PCA
def pca_parts(Y, K):
    """The float64 pieces of prcomp(log2(Y + 1), center, scale) that the conditions and the rounding model need."""
    N = Y.shape[0]
    X = np.log2(np.asarray(Y, dtype=np.float64) + 1.0)
    mean = X.mean(0)
    Xc = X - mean
    sd = np.sqrt((Xc ** 2).sum(0) / (N - 1))
    Xs = Xc / sd
    _, sv, Vt = np.linalg.svd(Xs, full_matrices=False)
    V = Vt[:K].T
    V = V * np.where(V[np.abs(V).argmax(0), np.arange(K)] < 0, -1.0, 1.0)[None, :]
    return dict(X=X, mean=mean, sd=sd, Xs=Xs, lam=sv ** 2, V=V)


def pca_conditions(Y, K=2):
    """(smallest lambda_k / lambda_{k+1} over k = 1 .. K -- the ratios among the first K + 1 eigenvalues, which separate each of the K
    components from its neighbours --, smallest column sd) of the standardised log2(Y + 1)."""
    p = pca_parts(Y, K)
    lam = p["lam"]
    return float(min(lam[k] / lam[k + 1] for k in range(K))), float(p["sd"].min())


def r_scale(x):
    xc = x - x.mean(0, keepdims=True)
    return xc / np.sqrt((xc ** 2).sum(0, keepdims=True) / (x.shape[0] - 1))


def pca_model_error(Y, K):
    """Error of a float32 model of the device's final projection against the float64 scores, per column: x = float32(log2(y + 1)),
    weights float32(v / sd), products and their sum over the genes in float32 (numpy's pairwise order); the centring constant sum_g mean_g
    v_g / sd_g, the Rayleigh-Ritz step and scale() stay in float64, as on the device.  Computed from the float64 SVD alone."""
    p = pca_parts(Y, K)
    ref = r_scale(p["Xs"] @ p["V"])
    W = p["V"] / p["sd"][:, None]
    x32, w32 = p["X"].astype(np.float32), W.astype(np.float32)
    sc = np.stack([(x32 * w32[None, :, k]).sum(1, dtype=np.float32) for k in range(K)], 1).astype(np.float64) - (p["mean"] @ W)[None, :]
    return np.abs(r_scale(sc) - ref).max(0)


def sign_error(dev, ref):
    """Per column: max |dev -+ ref|, whichever sign fits."""
    return np.minimum(np.abs(dev - ref).max(0), np.abs(dev + ref).max(0))


# ------------------------------------------------------------------ per-clone sums
def clone_labels(N, C, seed=SEED, skew=False):
    """Clone labels uniform in -1 .. C - 1; ``skew``: four cells in five of clone 0 instead, the rest uniform -- so that a clone has more
    than 256 cells among the 512 of one strip block, which is what it takes for u16 counts (220 cells x 65535 stay below 2^24)."""
    rng = np.random.default_rng([seed, N, C, 6 if skew else 5])
    idx = rng.integers(-1, C, size=N)
    if skew:
        idx[rng.random(N) < 0.8] = 0
    return _frozen(idx)


LABELS = ("uniform", "skew")


def clone_sums_ref(Y, idx, C):
    """(T [G, C], Syy [G]) in float64 from int64 sums where the counts are integers (exact below 2^53), else float64 sums."""
    Y = np.asarray(Y)
    if np.all(Y == np.floor(Y)):
        Yi = Y.astype(np.int64)
        T = np.stack([Yi[idx == c].sum(0) for c in range(C)], 1)
        return T.astype(np.float64), (Yi[idx >= 0].astype(object) ** 2).sum(0).astype(np.float64)
    Yd = Y.astype(np.float64)
    return np.stack([Yd[idx == c].sum(0) for c in range(C)], 1), (Yd[idx >= 0] ** 2).sum(0)


@functools.lru_cache(maxsize=None)
def large_counts(kind, seed=SEED):
    """The large-count inputs of T and Syy: float64 [1100, 70] integer counts whose float32 partial sums pass 2^24."""
    N, G, _ = LARGE_SHAPE
    rng = np.random.default_rng([seed, 99, LARGE.index(kind)])
    if kind == "u16":
        Y = rng.integers(40000, 65536, size=(N, G))
    elif kind == "f32int":
        Y = rng.integers(100000, 1 << 24, size=(N, G))
    else:
        Y = rng.poisson(1.0, size=(N, G))
        Y[:, 0] += 1
        Y[:, 33] = rng.integers(70000, 130001, size=N)
    return _frozen(Y.astype(np.float64))


def large_tune(kind):
    return dict(tr=128) if kind == "u16" else None


def host_correlations(Y, L, idx):
    """compute_correlations (the host formula of R/clonealign.R:318-334) for integer clone labels, -1 = unassigned."""
    from clonealign_amd.api import compute_correlations
    names = [f"c{c}" for c in range(L.shape[1])]
    clones = np.array([names[c] if c >= 0 else "unassigned" for c in idx], dtype=object)
    return compute_correlations(Y, L, clones, names)


# ------------------------------------------------------------------ read-back, preprocessing
def one_cell_labels(N, cells):
    """Labels that put cell cells[c] alone in clone c: T[:, c] is then that cell's row of the resident matrix."""
    idx = np.full(N, -1, dtype=np.int64)
    idx[np.asarray(cells)] = np.arange(len(cells))
    return idx


def readback_cells(Y, C, strip=128):
    """2 C cells to read back, in two label sets of C: first, last, both sides of the strip boundaries, the cells holding the largest counts."""
    N = Y.shape[0]
    want = [0, N - 1] + [c for b in (strip, 2 * strip, 4 * strip) for c in (b - 1, b)] + list(np.argsort(-np.asarray(Y).max(1), kind="stable")[:C])
    cells = []
    for c in want + list(range(N)):
        if 0 <= c < N and c not in cells:
            cells.append(int(c))
        if len(cells) == 2 * C:
            break
    return cells[:C], cells[C:]        # (fewer than 2 C cells in all: shorter lists, the second may be empty)


def preprocess_case(N=2500, G=420, C=4, seed=SEED):
    """Integer counts on which every filter of preprocess_for_clonealign bites, with f32int-sized entries (below 2^24)."""
    rng = np.random.default_rng([seed, 12, N])
    mu = rng.lognormal(-1.0, 1.2, G)
    mu[:3] *= 300.0
    Y = rng.poisson(mu[None, :] * rng.lognormal(0, 0.6, N)[:, None]).astype(np.int64)
    genes = rng.choice(np.arange(60, G), G // 8, replace=False)
    Y[:, genes] = np.minimum(Y[:, genes] * 3000 + rng.integers(0, 3000, size=(N, genes.size)), (1 << 24) - 1)
    Y[:, genes[:8]] = rng.integers(100000, 1 << 24, size=(N, 8))      # (a cell's sum passes 2^24 too)
    Y[:40] = 0
    Y[:40, 5] = 1
    Y[:, 50:60] = 0
    L = rng.integers(1, 5, size=(G, C)).astype(np.float64)
    L[10:20] = 2.0
    L[30:34, 1] = 9.0
    return Y, L
