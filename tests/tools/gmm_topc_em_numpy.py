"""float64 numpy restatement of top-C EM (include/sidekit_amd/gmm_topc_em.h, sidekit_amd/mixture.py em_split_topc_device), on top of the
diagonal-GMM restatement (mixture_numpy.py: split, M-step, dense EM step), the top-C scoring restatement (gmm_topc_numpy.py: the
direct-form log posterior, the exact lists) and the top-C statistics restatement (gmm_topc_stats_numpy.py: posteriors and statistics
over lists), which are pinned to the reference's fixture.  With ``top_c >= distrib_nb`` every level is mixture_numpy's dense EM step."""
import numpy

import gmm_topc_numpy as gtn
import gmm_topc_stats_numpy as gsn
import mixture_numpy as mxn

TOPC_MAX = 32   # SC_GMM_TOPC_MAX


def split_candidates(idx, c_old):
    """(N, K) lists over c_old parents -> (N, 2 K) int32 [idx, idx + c_old]; -1 stays -1 in both halves"""
    idx = numpy.asarray(idx).astype(numpy.int64)
    return numpy.concatenate((idx, numpy.where(idx < 0, idx, idx + c_old)), axis=1).astype(numpy.int32)


def select(m, X, cand, K):
    """-> idx (N, K) int32, gaps (N,): per frame the K best valid candidates, ascending, then -1, and the gap between its K-th and
    (K + 1)-th valid candidate (inf with at most K).  A candidate is valid when it lies in [0, C) and no earlier entry of its row holds
    the same value; the larger lp wins, at equal lp the lower index, a nan lp ranks as -inf."""
    C = m["mu"].shape[0]
    cand = numpy.asarray(cand).astype(numpy.int64)
    lp = gtn.log_posteriors(m, X)
    key = numpy.where(numpy.isnan(lp), -numpy.inf, lp)
    idx = numpy.full((X.shape[0], K), -1, dtype=numpy.int32)
    gaps = numpy.full(X.shape[0], numpy.inf)
    for n, row in enumerate(cand):
        seen, valid = set(), []
        for c in row:
            if 0 <= c < C and c not in seen:
                seen.add(c)
                valid.append(int(c))
        ranked = sorted(valid, key=lambda c: (-key[n, c], c))
        idx[n, :min(K, len(ranked))] = sorted(ranked[:K])
        if len(ranked) > K:
            a, b = key[n, ranked[K - 1]], key[n, ranked[K]]
            gaps[n] = 0.0 if a == b else a - b
    return idx, gaps


def refine(m, X, cand, K):
    """-> idx (N, K) int32, post (N, K), lse (N,), the smallest gap over the frames between the K-th and the (K + 1)-th valid candidate
    (inf when no frame has more than K): ``select``, then the posteriors over the lists (gmm_topc_stats_numpy.posteriors)"""
    idx, gaps = select(m, X, cand, K)
    post, lse = gsn.posteriors(m, X, idx)
    return idx, post, lse, float(gaps.min())


def em_step(m, X, idx, ceil_cov=10, floor_cov=1e-2):
    """One E-step over the lists and the reference's M-step -> (model, llk = sum lse / sum stat0)"""
    s0, s1, s2, llk, _, _ = gsn.stats(m, X, idx)
    return mxn.maximization(m, s0[0], s1[0], s2[0], ceil_cov, floor_cov), llk[0] / numpy.sum(s0[0])


def em_split_topc(X, distrib_nb, iterations, top_c, exact_lists_at=()):
    """-> (the list of (model, llk) after every iteration, the lists the last level ended with (None after a dense level), the smallest
    candidate gap over all refinements).  Dense levels (C <= top_c) are mixture_numpy.em_step; a selective level takes its candidates
    once after the split (the children of the previous level's lists, or at a C in exact_lists_at the min(2 top_c, 32, C) best of all
    components under the just-split model), refines before every E-step and once more after its last M-step."""
    m = mxn.init_single(X)
    trace, idx, parents, smallest = [], None, 1, numpy.inf
    for it in iterations[:int(numpy.log2(distrib_nb))]:
        m = mxn.split(m)
        C = m["mu"].shape[0]
        if C <= top_c:
            for _ in range(it):
                m, llk = mxn.em_step(m, X)
                trace.append((m, llk))
            idx, parents = None, C
            continue
        if C in exact_lists_at:
            cand = gtn.lists(m, X, min(2 * top_c, TOPC_MAX, C))
        else:
            cand = split_candidates(numpy.tile(numpy.arange(parents), (X.shape[0], 1)) if idx is None else idx, parents)
        for _ in range(it):
            idx, _, _, gap = refine(m, X, cand, top_c)
            smallest = min(smallest, gap)
            m, llk = em_step(m, X, idx)
            trace.append((m, llk))
        idx, _, _, gap = refine(m, X, cand, top_c)
        smallest, parents = min(smallest, gap), C
    return trace, idx, smallest
