"""The rule of asd_lookup_propose (include/asd_hip.h, PROMPT LOOKUP) in plain numpy, and the image of the one-hot draft rows.

TEST INFRASTRUCTURE, like tests/ngram_ref.py: never importable from the package."""
import numpy as np


def propose(H, K, N, n0):
    """One row's history H (a sequence of ints) -> (the K proposals, matched)."""
    H = [int(t) for t in H]
    n = len(H)
    best = (0, 0)                                        # (m, e): the longest match, then the most recent
    for e in range(1, n):
        m = 0
        while m < min(e, N) and H[e - 1 - m] == H[n - 1 - m]:
            m += 1
        best = max(best, (m, e))
    m, e = best
    if m >= n0:
        return [H[e + i % (n - e)] for i in range(K)], m
    return [H[-1] if n else 0] * K, 0


def propose_rows(tokens, row_start, seq_len, K, N, n0):
    """tokens int [B, cap], row_start / seq_len int [B] -> (tok int32 [B, K], matched int32 [B])."""
    out = [propose(tokens[b, row_start[b]:seq_len[b]], K, N, n0) for b in range(len(tokens))]
    return np.array([t for t, _ in out], dtype=np.int32).reshape(len(tokens), K), np.array([m for _, m in out], dtype=np.int32)


def onehot_image(tok, V):
    """tok int [B, K] -> float32 [B, K, V]: 0 at every proposal inside [0, V), -inf elsewhere."""
    img = np.full(tok.shape + (V,), -np.inf, dtype=np.float32)
    for idx in np.ndindex(*tok.shape):
        if 0 <= tok[idx] < V:
            img[idx + (int(tok[idx]),)] = 0.0
    return img
