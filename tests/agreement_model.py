"""Test infrastructure: the definitions of replica agreement (include/sbmbp.h, sbmbp_batch_agreement / sbmbp_agreement_groups) in
a few lines of numpy. psis is a list of n marginal tables [N, Q]."""
import itertools

import numpy as np

KINDS = {"soft": 0, "hard_soft": 1, "hard": 2}


def labels(psi):
    """the label of the largest entry of every row; np.argmax takes the lowest index among equal maxima"""
    return np.argmax(psi, axis=1)


def one_hot(psi):
    H = np.zeros(psi.shape)
    H[np.arange(psi.shape[0]), labels(psi)] = 1.0
    return H


def confusion(psis, kind):
    """C[x, y, a, b] for every ordered pair of the list: X_x^T @ Y_y in float64"""
    X = [p if kind == "soft" else one_hot(p) for p in psis]
    Y = [one_hot(p) if kind == "hard" else p for p in psis]
    n, Q = len(psis), psis[0].shape[1]
    C = np.zeros((n, n, Q, Q))
    for x in range(n):
        for y in range(n):
            C[x, y] = X[x].T @ Y[y]
    return C


def overlap_brute(C, N):
    """max over all permutations of the trace / N, and a maximising permutation (Q <= 8)"""
    Q = C.shape[0]
    assert Q <= 8
    best, arg = -np.inf, None
    for p in itertools.permutations(range(Q)):
        s = sum(C[a, p[a]] for a in range(Q)) / N
        if s > best:
            best, arg = s, p
    return best, arg


def groups(overlap, threshold):
    """x joins the group of the first earlier leader g with overlap[g, x] >= threshold, else it leads a new group"""
    overlap = np.asarray(overlap)
    leaders, group = [], []
    for x in range(overlap.shape[0]):
        for k, g in enumerate(leaders):
            if overlap[g, x] >= threshold:
                group.append(k)
                break
        else:
            leaders.append(x)
            group.append(len(leaders) - 1)
    return np.array(group, dtype=np.uint32), len(leaders)
