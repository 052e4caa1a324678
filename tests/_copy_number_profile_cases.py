"""What tests/test_copy_number_profile_host.py and tests/test_gpu_copy_number_profile.py share: the float64 numpy restatement of ca_copy_number_profile on whole
arrays with its scale (``numpy_cost``), the planted-recovery recipe (``planted``, ``check_planted``), the cases of values that are exact by rule
(``exact_cases``, ``check_exact``) and the case for the rules of delta_ll (``rules_case``, ``check_rules``).  Same seeds on both sides, by construction."""
import functools

import numpy as np

from clonealign_amd import api

NAMES4 = ["clone_a", "clone_b", "clone_c", "clone_d"]
S_MAX = 1.0 - 2.0 ** -53       # the largest share S of a block that does not hold every expressed gene of the cell's clone (include/clonealign_hip.h)


def numpy_cost(E, V, U, clone, total, mu, kappa, blocks=None):
    """(cost, scale), each [G or B, C, J]: the restatement of include/clonealign_hip.h on whole arrays; ``scale`` = sum_n s_n (|log1p(a)| + |a| / (1 + a)), the
    conditioning of log1p (inf where some cell has 1 + a == 0: there ``cost`` is -inf)."""
    E, mu, kappa = np.asarray(E, dtype=np.float64), np.asarray(mu, dtype=np.float64), np.asarray(kappa, dtype=np.float64)
    clone, t = np.asarray(clone), np.asarray(total, dtype=np.float64)
    (G, C), J = E.shape, kappa.shape[0]
    live = t > 0
    e = E[:, clone].T
    pos = e > 0
    eta = np.zeros(e.shape) if U is None else np.asarray(U) @ np.asarray(V).T
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = np.where(pos, eta, -np.inf).max(1, keepdims=True)
        ex = np.exp(np.where(live[:, None], eta - m, 0.0))
        w = np.where(pos, e * ex, 0.0)
        is_top = np.arange(G)[None, :] == w.argmax(1)[:, None]       # the largest w joins the sum last
        Z = np.where(is_top, 0.0, w).sum(1, keepdims=True) + w.max(1, keepdims=True)
        Z = np.where(live[:, None], Z, 1.0)
        p, x = w / Z, ex / Z
        delta = (mu[:, None] * kappa[None, :])[:, None, :] - E[:, :, None]                     # [G, C, J]
        if blocks is None:
            W = G
            cf = np.where(E[:, :, None] > 0, delta / np.where(E > 0, E, 1.0)[:, :, None], delta)
            cfn = cf[:, clone, :].transpose(1, 0, 2)                                            # [N, G, J]
            a = np.where(cfn == 0, 0.0, cfn * np.where(pos, p, x)[:, :, None])
        else:
            blocks = np.asarray(blocks)
            W = int(blocks.max()) + 1
            onehot = np.zeros((G, W))
            onehot[np.arange(G), blocks] = 1.0
            npos = onehot.T @ (E > 0)                                                           # [W, C]
            full = ((npos == npos.sum(0, keepdims=True)) & (npos.sum(0, keepdims=True) > 0))[:, clone].T    # [N, W]
            same = ((onehot.T @ (delta != 0).reshape(G, C * J).astype(np.float64)).reshape(W, C, J) == 0)[:, clone, :].transpose(1, 0, 2)
            A, S = (mu[None, :] * x) @ onehot, np.where(full, 1.0, np.minimum(p @ onehot, S_MAX))
            a = np.where(same, 0.0, np.maximum(kappa[None, None, :] * A[:, :, None] - S[:, :, None], -1.0))
        a = np.where(live[:, None, None], a, 0.0)
        term = t[:, None, None] * np.log1p(a)
        sc_n = t[:, None, None] * (np.abs(np.log1p(a)) + np.abs(a) / (1.0 + a))
        term, sc_n = np.where(live[:, None, None], term, 0.0), np.where(live[:, None, None], sc_n, 0.0)
    cost, scale = np.zeros((C, W, J)), np.zeros((C, W, J))
    np.add.at(cost, clone, term)
    np.add.at(scale, clone, sc_n)
    return cost.transpose(1, 0, 2), scale.transpose(1, 0, 2)


def hand_fit(mu, W, psi, z, names):
    ml = {"mu": mu}
    if W is not None:
        ml.update({"W": W, "psi": psi})
    return {"ml_params": ml, "clone_names": list(names), "clone": np.asarray(names, dtype=object)[z]}


def total_ll(Y, mu, L, W, psi, z):
    """(sum over the cells of the log-likelihood at the called clone, the sum of the terms' magnitudes), from scratch."""
    ll = api._clone_loglik_host(Y, mu[:, None] * L, psi, W, const=True)[np.arange(Y.shape[0]), z]
    return ll.sum(), np.abs(ll).sum()


@functools.lru_cache(maxsize=None)
def planted():
    """The recipe: default_rng(5); N, G, C, B = 240, 300, 3, 12; mu ~ lognormal(0, 1); segment labels sorted integers(0, B, G); segment copy numbers
    integers(1, 5); W ~ 0.5 N(0, 1), psi ~ N(0, 1); clones uniform; 2000 reads per cell from the true L.  The L handed over has four (segment, clone) entries
    replaced by true % 4 + 1.  Returns (fit, Y, L_given, L_true, segments, corrupted pairs, clones)."""
    rng = np.random.default_rng(5)
    N, G, C, B = 240, 300, 3, 12
    mu = rng.lognormal(0.0, 1.0, G)
    seg = np.sort(rng.integers(0, B, G))
    cn = rng.integers(1, 5, (B, C)).astype(np.float64)
    W, psi = 0.5 * rng.normal(size=(G, 1)), rng.normal(size=(N, 1))
    z = rng.integers(0, C, N)
    L_true = cn[seg]
    w = (mu[:, None] * L_true)[:, z].T * np.exp(psi @ W.T)
    Y = np.stack([rng.multinomial(2000, w[n] / w[n].sum()) for n in range(N)]).astype(np.int32)
    present = np.unique(seg)
    bad = [(int(present[k // C]), k % C) for k in rng.choice(present.size * C, 4, replace=False)]
    cn_given = cn.copy()
    for b, c in bad:
        cn_given[b, c] = cn[b, c] % 4 + 1
    L_given = cn_given[seg]
    for a in (Y, L_given, L_true, seg):
        a.setflags(write=False)
    return hand_fit(mu, W, psi, z, NAMES4[:C]), Y, L_given, L_true, seg, sorted(bad), z


def check_planted(fit, Y, L_given, L_true, seg, bad, **kw):
    """The planted case's assertions on api.copy_number_profile (host or device): block mode recovers every entry, lists exactly the four and repairs the
    matrix; per gene at least 0.90 of the corrupted entries are recovered and 0.90 of the clean ones kept.  Returns the two profiles."""
    names = list(dict.fromkeys(seg.tolist()))
    cand = np.arange(1, 7)
    blk = api.copy_number_profile(fit, Y, L_given, candidates=cand, blocks=seg, **kw)
    first = np.array([np.flatnonzero(seg == b)[0] for b in names])
    assert blk["block_names"] == names and np.array_equal(blk["map_cn"], L_true[first])
    assert np.array_equal(blk["input_cn"], np.asarray(L_given)[first])
    sus = api.suspect_copy_numbers(blk)
    assert sorted((s["block"], s["clone"]) for s in sus) == bad
    assert all(s["log_bf"] > 10.0 and s["map_cn"] == L_true[first[s["index"]], s["clone"]] and s["runner_up_delta_ll"] < s["log_bf"] for s in sus)
    assert [s["log_bf"] for s in sus] == sorted((s["log_bf"] for s in sus), reverse=True)
    clean = np.ones(blk["log_bf"].shape, dtype=bool)
    for s in sus:
        clean[s["index"], s["clone"]] = False
    assert (blk["log_bf"][clean] == 0.0).all()                       # the matrix as given is the best candidate: delta_ll = 0 exactly
    assert np.array_equal(api.apply_copy_number_calls(blk, L_given), L_true)
    assert np.array_equal(api.apply_copy_number_calls(blk, L_given, blocks=seg), L_true)
    gene = api.copy_number_profile(fit, Y, L_given, candidates=cand, **kw)
    wrong = np.asarray(L_given) != L_true
    recovered = float((gene["map_cn"][wrong] == L_true[wrong]).mean())
    kept = float((gene["map_cn"][~wrong] == L_true[~wrong]).mean())
    print(f"block mode: log_bf of the corrupted entries {min(s['log_bf'] for s in sus):.0f} .. {max(s['log_bf'] for s in sus):.0f}; "
          f"per gene: {wrong.sum()} corrupted entries, recovered {recovered:.3f}; {(~wrong).sum()} clean entries, kept {kept:.3f}")
    assert recovered >= 0.90 and kept >= 0.90
    return blk, gene


def exact_cases():
    """(name, (E, V, U, clone, total, mu, kappa), Lint) for the values of ``cost`` that are exact by rule, D = 0, 1, 3: E = mu * Lint with Lint in 0 .. 4 (a
    fifth of the entries 0), so that mu kappa_j == E bit for bit where kappa_j == Lint; clone 2 expresses gene 5 alone; clone 3 has no cells; cell 1 has
    total 0.  kappa = (0, 1, 2, 3, 4)."""
    rng = np.random.default_rng(11)
    N, G, C = 40, 70, 4
    mu = rng.lognormal(0.0, 1.0, G)
    Lint = rng.integers(1, 5, (G, C)).astype(np.float64)
    Lint[rng.random((G, C)) < 0.2] = 0.0
    Lint[:, 2] = 0.0
    Lint[5, 2] = 3.0
    clone = rng.integers(0, 3, N).astype(np.int32)
    clone[:4] = (2, 0, 2, 1)
    total = rng.integers(1, 500, N).astype(np.int64)
    total[1] = 0
    out = []
    for D in (0, 1, 3):
        V, U = (rng.normal(size=(G, D)) * 0.5, rng.normal(size=(N, D))) if D else (None, None)
        out.append((f"D = {D}", (mu[:, None] * Lint, V, U, clone, total, mu, np.arange(5.0)), Lint))
    return out


def check_exact(call, what, args, Lint):
    """``call(E, V, U, clone, total, mu, kappa, blocks)`` -> cost, on one of ``exact_cases``: per-gene mode and block mode (genes 0 .. 9 as one block, which
    holds clone 2's only expressed gene; then pairs of genes)."""
    E, V, U, clone, total, mu, kappa = args
    G, C = E.shape
    cost = call(*args, None)
    assert cost.shape == (G, C, 5) and not np.isnan(cost).any(), what
    assert (cost[:, 3, :] == 0.0).all(), what                                                   # an absent clone
    same = kappa[None, None, :] == Lint[:, :, None]
    assert (cost[same] == 0.0).all() and (cost[:, :3][~same[:, :3]] != 0.0).all(), what          # delta = 0 exactly; nothing else is 0
    assert cost[5, 2, 0] == -np.inf and np.isfinite(cost[5, 2, 1:]).all(), what                  # kappa = 0 on the only expressed gene of cells with reads
    assert np.isneginf(cost).sum() == 1, what
    assert (cost[:, :3, 1:][(Lint[:, :3] == 0)] > 0.0).all(), what                               # a gene switched on takes share from the others
    blocks = np.r_[np.zeros(10, dtype=np.int32), 1 + np.arange(G - 10, dtype=np.int32) // 2]
    cb = call(*args, blocks)
    B = int(blocks.max()) + 1
    assert cb.shape == (B, C, 5) and not np.isnan(cb).any() and (cb[:, 3, :] == 0.0).all(), what
    assert cb[0, 2, 0] == -np.inf and np.isfinite(cb[0, 2, 1:]).all() and np.isneginf(cb).sum() == 1, what
    uniform = np.stack([(Lint[blocks == b] == Lint[blocks == b][0]).all(0) for b in range(B)])  # [B, C]: the block's genes agree
    first = np.array([np.flatnonzero(blocks == b)[0] for b in range(B)])
    zero = uniform[:, :, None] & (kappa[None, None, :] == Lint[first][:, :, None])
    assert zero[:, :3].any() and (cb[zero] == 0.0).all(), what
    # cells without counts join no sum; no cell with counts: zeros
    assert (call(E, V, U, clone, np.zeros_like(total), mu, kappa, None) == 0.0).all() and (call(E, V, U, clone, np.zeros_like(total), mu, kappa, blocks) == 0.0).all(), what
    keep = total > 0
    sub = (E, V, None if U is None else U[keep], clone[keep], total[keep], mu, kappa)
    assert np.array_equal(call(*sub, None), cost) and np.array_equal(call(*sub, blocks), cb), what


@functools.lru_cache(maxsize=None)
def rules_case():
    """A fit, counts and L for the rules of delta_ll: 40 x 70 x 4, K = 1; L in 0 .. 4 with a fifth of the entries 0; clone_c expresses gene 5 alone;
    clone_d has no cells; cell 1 has no reads; cells 6 and 9 are "unassigned"; the counts are drawn from the model, then cell 3 (clone_b) gets one read on a
    gene where clone_b has copy number 0.  Returns (fit, Y, L, z, (planted gene, its clone))."""
    rng = np.random.default_rng(12)
    N, G, C = 40, 70, 4
    mu = rng.lognormal(0.0, 1.0, G)
    L = rng.integers(1, 5, (G, C)).astype(np.float64)
    L[rng.random((G, C)) < 0.2] = 0.0
    L[:, 2] = 0.0
    L[5, 2] = 3.0
    z = rng.integers(0, 3, N)
    z[:4] = (2, 0, 2, 1)
    W, psi = 0.5 * rng.normal(size=(G, 1)), rng.normal(size=(N, 1))
    w = (mu[:, None] * L)[:, z].T * np.exp(psi @ W.T)
    Y = np.stack([rng.multinomial(300, w[n] / w[n].sum()) for n in range(N)]).astype(np.int32)
    Y[1] = 0
    g0 = int(np.flatnonzero(L[:, 1] == 0)[0])
    Y[3, g0] += 1
    fit = hand_fit(mu, W, psi, z, NAMES4)
    fit["clone"][[6, 9]] = "unassigned"
    Y.setflags(write=False)
    L.setflags(write=False)
    return fit, Y, L, z, (g0, 1)


def check_rules(prof, Y, L, z, planted_read, what):
    """The rules of delta_ll on ``rules_case``, per-gene mode, candidates 0 .. 6."""
    g0, c0 = planted_read
    d, T = prof["delta_ll"], prof["T_observed"]
    used = np.setdiff1d(np.arange(40), [6, 9])
    want_T = np.zeros(L.shape)
    np.add.at(want_T.T, z[used], np.asarray(Y)[used].astype(np.float64))
    assert np.array_equal(T, want_T) and np.array_equal(prof["clone_cells"], np.bincount(z[used], minlength=4)), what
    for k in ("delta_ll", "gain", "cost", "posterior", "log_bf", "map_cn"):
        assert not np.isnan(prof[k]).any(), (what, k)
    assert np.allclose(prof["posterior"].sum(2), 1.0) and (prof["posterior"] >= 0).all(), what
    zero_no_reads = (L == 0) & (T == 0)
    zero_no_reads[:, 3] = False
    assert zero_no_reads[:, :2].any()
    assert (d[zero_no_reads][:, 0] == 0.0).all() and (d[zero_no_reads][:, 1:] < 0.0).all() and np.isfinite(d[zero_no_reads]).all(), what   # copy number 0, no reads: 0 stays best
    assert (prof["map_cn"][zero_no_reads] == 0.0).all() and (prof["log_bf"][zero_no_reads] == 0.0).all(), what
    assert T[g0, c0] == 1.0 and d[g0, c0, 0] == 0.0 and (d[g0, c0, 1:] == np.inf).all(), what     # copy number 0 with a read: the matrix as given is impossible
    assert np.allclose(prof["posterior"][g0, c0], np.r_[0.0, np.full(6, 1 / 6)]), what
    reads = (L > 0) & (T > 0)
    assert (d[reads][:, 0] == -np.inf).all(), what                                              # candidate 0 where the clone has reads
    assert (d[:, 3, :] == 0.0).all() and np.allclose(prof["posterior"][:, 3, :], 1 / 7), what   # a clone without cells
    assert d[5, 2, 0] == -np.inf and prof["cost"][5, 2, 0] == -np.inf and d[5, 2, 3] == 0.0 and np.isfinite(d[5, 2, 1:]).all(), what   # one expressed gene
    hit = (np.arange(7.0)[None, None, :] == L[:, :, None])
    assert (d[hit] == 0.0).all() and np.array_equal(prof["input_cn"], L), what
    assert np.array_equal(prof["posterior_input"], (prof["posterior"] * hit).sum(2)), what
