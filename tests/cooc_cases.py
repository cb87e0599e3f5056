"""What rri_cooccurrence_counts must answer, restated in numpy on the dense 0/1 form of a corpus, the coherence measures as plain
loops over those counts, and the corpora the GPU test counts.  Shared by tests/test_cooc_cpu.py and tests/test_cooc_gpu.py."""
import math

import numpy as np
import scipy.sparse as sp


def dense_counts(B, words):
    """B: (n_rows, n_cols) array, non-zero = the word occurs; words (g, M) with -1 for an empty slot.
    (df (g, M) int64, codf (g, M, M) int64) by a matrix product per group."""
    B = (np.asarray(B) != 0).astype(np.int64)
    words = np.asarray(words, dtype=np.int64)
    g, M = words.shape
    df = np.zeros((g, M), dtype=np.int64)
    codf = np.zeros((g, M, M), dtype=np.int64)
    for q in range(g):
        P = np.zeros((B.shape[0], M), dtype=np.int64)
        for a in range(M):
            if words[q, a] >= 0:
                P[:, a] = B[:, words[q, a]]
        codf[q] = P.T.dot(P)
        df[q] = np.diag(codf[q])
    return df, codf


def measure_reference(measure, words, df, codf, N, eps):
    """(per_topic, pairs_undefined) by loops over the pairs of slots a < b, as the issue states the three measures"""
    per, undefined = [], []
    for q in range(len(words)):
        vals, undef = [], 0
        M = len(words[q])
        for a in range(M):
            for b in range(a + 1, M):
                if words[q][a] < 0 or words[q][b] < 0:
                    continue
                Da, Db, Dab = int(df[q][a]), int(df[q][b]), int(codf[q][a][b])
                if measure == 'umass':
                    if Da == 0:
                        undef += 1
                    else:
                        vals.append(math.log((Dab + eps) / Da) if Dab + eps > 0 else -math.inf)
                elif Da * Db == 0:
                    undef += 1
                elif measure == 'pmi':
                    vals.append(math.log((Dab + eps) * N / (Da * Db)) if Dab + eps > 0 else -math.inf)
                elif Dab == 0:
                    vals.append(-1.0)
                elif Dab == N:
                    vals.append(1.0)
                else:
                    vals.append(math.log((Dab / N) / ((Da / N) * (Db / N))) / -math.log(Dab / N))
        per.append(sum(vals) / len(vals) if vals else float('nan'))
        undefined.append(undef)
    return np.array(per), np.array(undefined)


def corpus_with_row_lengths(lengths, n_cols, seed):
    """a CSR 0/1 corpus whose row r holds lengths[r] distinct random columns"""
    rng = np.random.RandomState(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_cols, size=n, replace=False)) for n in lengths] + [np.zeros(0, dtype=np.int64)])
    return sp.csr_matrix((np.ones(indices.size), indices.astype(np.int32), indptr), shape=(len(lengths), n_cols))


def random_words(n_groups, group_size, n_cols, seed, empty=0.0):
    """distinct columns per group; a share `empty` of the slots is -1 (where n_cols < group_size the rest is -1 as well)"""
    rng = np.random.RandomState(seed)
    words = np.full((n_groups, group_size), -1, dtype=np.int32)
    for q in range(n_groups):
        take = min(group_size, n_cols)
        slots = np.sort(rng.choice(group_size, size=take, replace=False))
        words[q, slots] = rng.choice(n_cols, size=take, replace=False)
    words[rng.rand(n_groups, group_size) < empty] = -1
    return words
