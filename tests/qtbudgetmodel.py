"""numpy model of the quadtree encode to a leaf budget, on the per-level collage SSE arrays of the
quadtree models ({B: [Rh, Rw]}, qtmodel.level_sse and its colour twins).

A block v of side B > B_min splits under the float32 threshold t iff (double) SSE_v > (double) t * B * B, i.e. iff
k(v) = SSE_v * (256 / B^2) > 256 t, an integer compared with one denominator for every level.  v is reached only when every
ancestor splits, so with e(v) = min(k(v), k(parent(v)), ..) the tree has N_top + 3 #{v : e(v) > 256 t} leaves.  For a budget
of M leaves, S = (M - N_top) // 3 blocks may split: K is the (S+1)-th largest e(v) (0 when there are S or fewer) and the
threshold the smallest float32 >= K / 256.  Test infrastructure only."""
import numpy as np

import qtmodel as qm

KEY_MAX = (1 << 32) - 1     # the device keeps keys in 32 bits and saturates (only the all-ones SSE mark at B = 8 gets there)


def keys(sse, B_max, B_min):
    """int64 [n]: e(v) of every block above B_min, the blocks of B_max in scanline order first, then those of B_max / 2."""
    out, parent = [], None
    for B in qm.levels(B_max, B_min)[:-1]:
        k = np.minimum(np.asarray(sse[B]).astype(np.int64) * (256 // (B * B)), KEY_MAX)
        if parent is not None:
            k = np.minimum(k, np.repeat(np.repeat(parent, 2, axis=0), 2, axis=1))
        out.append(k.reshape(-1))
        parent = k
    return np.concatenate(out)


def select(e, rank):
    """The key of rank `rank` in descending order (rank 0: the largest), 0 past the last one."""
    e = np.sort(np.asarray(e).astype(np.int64))[::-1]
    return int(e[rank]) if rank < e.size else 0


def key_threshold(K):
    """The smallest float32 >= K / 256: K rounded up to a float32, times 2^-8 (exact)."""
    f = np.float32(K)
    if int(f) < K:
        f = np.nextafter(f, np.float32(np.inf))
    return np.float32(f * np.float32(2.0 ** -8))


def leaves_at(sse, B_max, B_min, t):
    """Leaves of the tree under float32 threshold t, from the keys: N_top + 3 #{e(v) > 256 t}."""
    e = keys(sse, B_max, B_min)
    return int(np.asarray(sse[B_max]).size + 3 * (e.astype(np.float64) > 256.0 * float(np.float32(t))).sum())


def budget_threshold(sse, w, h, B_max, B_min, M):
    """(threshold float32, K): the smallest non-negative float32 whose tree has at most M leaves.  ValueError for M < N_top."""
    n_top = (w // B_max) * (h // B_max)
    if M < n_top:
        raise ValueError(f"max_leaves = {M} below the {n_top} blocks of side {B_max}")
    K = select(keys(sse, B_max, B_min), (M - n_top) // 3)
    return key_threshold(K), K


def tree_stats(sse, leaves, B_max):
    """uint64 [4] = {collage SSE summed over the leaves, leaves of side B_max, B_max / 2, B_max / 4} of a leaf table."""
    lv = np.asarray(leaves)
    total = sum(int(np.asarray(sse[int(B)])[int(y) // int(B), int(x) // int(B)]) for x, y, B in lv[:, :3])
    return np.array([total] + [int((lv[:, 2] == (B_max >> l)).sum()) for l in range(3)], np.uint64)
