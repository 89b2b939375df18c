"""numpy model of the quadtree encode by rate-distortion pruning, on the per-level collage SSE arrays
of the quadtree models ({B: [Rh, Rw]}, qtmodel.level_sse and its colour twins).  Exact integers (int64) throughout.

For an integer lam >= 0 the cost of a block v is J(v) = S_v + lam at side B_min, else min(S_v + lam, sum of J over the four
children); v wants to split iff that sum is < S_v + lam (a tie keeps it whole), and in the tree T(lam) a block is split iff
it and all its ancestors want to.  k(v) is the smallest lam >= 0 at which v does not want to split, found here from that
property alone (bisection on the rule itself), e(v) = min(k(v), k(parent(v))), G_v = S_v - sum of S over the children.  The
identities N(lam) = N_top + 3 #{e > lam} and D(lam) = sum S_top - sum_{e > lam} G are what the tests check; nothing in
cost / wants / tree_* uses them.  Test infrastructure only."""
import numpy as np

import qtmodel as qm

LAM_MAX = (1 << 32) - 1
GOAL_LAMBDA, GOAL_LEAVES, GOAL_SSE = 0, 1, 2


def _s(sse, B):
    return np.asarray(sse[B]).astype(np.int64)


def child_sum(a):
    """[Rh, Rw] sums of the 2 x 2 children of every block, from the children's [2 Rh, 2 Rw]."""
    return a.reshape(a.shape[0] // 2, 2, a.shape[1] // 2, 2).sum(axis=(1, 3))


def rep(a):
    """A per-block array handed down to the four children."""
    return np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)


def cost(sse, B, B_min, lam):
    """J of every block of side B; lam an int or an int64 array of the level's shape (a lam of its own per block)."""
    lam = np.broadcast_to(np.asarray(lam, np.int64), _s(sse, B).shape)
    own = _s(sse, B) + lam
    return own if B == B_min else np.minimum(own, child_sum(cost(sse, B // 2, B_min, rep(lam))))


def wants(sse, B, B_min, lam):
    """bool per block of side B > B_min: the children's cost is strictly below the block's own."""
    lam = np.broadcast_to(np.asarray(lam, np.int64), _s(sse, B).shape)
    return child_sum(cost(sse, B // 2, B_min, rep(lam))) < _s(sse, B) + lam


def tree(sse, w, h, B_max, B_min, lam):
    """Leaves (x, y, B) of T(lam) in stream order (qtmodel.split's order)."""
    want = {B: wants(sse, B, B_min, lam) for B in qm.levels(B_max, B_min)[:-1]}
    out = []

    def visit(x, y, B):
        if B > B_min and want[B][y // B, x // B]:
            hb = B // 2
            for dx, dy in ((0, 0), (hb, 0), (0, hb), (hb, hb)):
                visit(x + dx, y + dy, hb)
        else:
            out.append((x, y, B))

    for y in range(0, h, B_max):
        for x in range(0, w, B_max):
            visit(x, y, B_max)
    return out


def tree_nd(sse, B_max, B_min, lam):
    """(leaves, collage SSE of the leaves) of T(lam), bottom-up from the rule: a block that wants to split takes its children's
    values, and a value is only ever read through a chain of ancestors that all want to."""
    Bs = qm.levels(B_max, B_min)
    n, d = np.ones_like(_s(sse, B_min)), _s(sse, B_min)
    for B in Bs[::-1][1:]:
        wt = wants(sse, B, B_min, lam)
        n, d = np.where(wt, child_sum(n), 1), np.where(wt, child_sum(d), _s(sse, B))
    return int(n.sum()), int(d.sum())


def k_of(sse, B, B_min):
    """int64 per block of side B > B_min: the smallest lam >= 0 at which the block does not want to split.  wants() is
    monotone in lam (its difference has slope >= 3) and false at 2^31 > ceil(S / 3), so a bisection on the rule finds it."""
    lo, hi = np.full(_s(sse, B).shape, -1, np.int64), np.full(_s(sse, B).shape, 1 << 31, np.int64)    # wants at lo (or lo = -1), not at hi
    while True:
        open_ = hi - lo > 1
        if not open_.any():
            return hi
        mid = (lo + hi) >> 1                                    # >= 0 wherever the interval is still open
        wt = wants(sse, B, B_min, np.maximum(mid, 0))
        lo, hi = np.where(open_ & wt, mid, lo), np.where(open_ & ~wt, mid, hi)


def keys_gains(sse, B_max, B_min):
    """(e int64 [n], G int64 [n]) of every block above B_min, the blocks of B_max in scanline order first, then those of
    B_max / 2 (the order of qtbudgetmodel.keys)."""
    e, G, parent = [], [], None
    for B in qm.levels(B_max, B_min)[:-1]:
        k = k_of(sse, B, B_min)
        if parent is not None:
            k = np.minimum(k, rep(parent))
        e.append(k.reshape(-1))
        G.append((_s(sse, B) - child_sum(_s(sse, B // 2))).reshape(-1))
        parent = k
    return np.concatenate(e), np.concatenate(G)


def n_of(e, n_top, lam):
    return int(n_top + 3 * (e > lam).sum())


def d_of(e, G, s_top, lam):
    return int(s_top - G[e > lam].sum())


def lambda_for_leaves(e, n_top, max_leaves):
    """The smallest lam whose tree has at most max_leaves leaves: the (S+1)-th largest e, S = (max_leaves - n_top) // 3."""
    if max_leaves < n_top:
        raise ValueError(f"max_leaves = {max_leaves} below the {n_top} top-level blocks")
    d = np.sort(e)[::-1]
    S = (max_leaves - n_top) // 3
    return int(d[S]) if S < d.size else 0


def select_weighted(keys, gains, need):
    """(boundary, #{key > boundary}, sum of gain over key > boundary): with the distinct keys in descending order followed by
    0, the first boundary at which the sum reaches `need`; the last one (0) when none does."""
    keys, gains = np.asarray(keys).astype(np.int64), np.asarray(gains).astype(np.int64)
    bounds = sorted(set(keys.tolist()) | {0}, reverse=True)
    for b in bounds:
        above = keys > b
        if int(gains[above].sum()) >= need:
            break
    return b, int(above.sum()), int(gains[above].sum())


def select_weighted_fast(keys, gains, need):
    """select_weighted by one sort (for the large sets)."""
    keys, gains = np.asarray(keys).astype(np.int64), np.asarray(gains).astype(np.int64)
    order = np.argsort(-keys, kind="stable")
    ks, cum = keys[order], np.cumsum(gains[order])
    first = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]            # where each distinct key starts, descending
    bounds = ks[first].tolist() + ([0] if ks[-1] != 0 else [])
    sums = [0] + cum[first[1:] - 1].tolist() + ([int(cum[-1])] if ks[-1] != 0 else [])
    counts = [0] + first[1:].tolist() + ([ks.size] if ks[-1] != 0 else [])
    for b, c, s in zip(bounds, counts, sums):
        if s >= need:
            return int(b), int(c), int(s)
    return int(bounds[-1]), int(counts[-1]), int(sums[-1])


def lambda_for_sse(e, G, s_top, max_sse):
    """The smallest lam of the tree of fewest leaves among the T(lam) with D <= max_sse; 0 (the tree T(0)) when none has."""
    return select_weighted(e, G, s_top - max_sse)[0]


def choose(sse, w, h, B_max, B_min, goal, value):
    """lam as the RD entries choose it."""
    n_top = (w // B_max) * (h // B_max)
    if goal == GOAL_LAMBDA:
        return int(value)
    e, G = keys_gains(sse, B_max, B_min)
    if goal == GOAL_LEAVES:
        return lambda_for_leaves(e, n_top, value)
    return lambda_for_sse(e, G, int(_s(sse, B_max).sum()), value)


def adversarial(w, h, B_max, B_min, seed=0):
    """{name: {B: uint32 [Rh, Rw]}}: SSE arrays that no encode produces, at the ends of the 32-bit range and of the rule."""
    Bs = qm.levels(B_max, B_min)
    rng = np.random.default_rng(20261020 + seed)
    shape = {B: (h // B, w // B) for B in Bs}
    full = lambda v: {B: np.full(shape[B], v, np.uint32) for B in Bs}                                   # noqa: E731
    out = {"equal": full(1000), "zeros": full(0), "all-ones": full(LAM_MAX), "one": full(1)}
    out["children-worse"] = {B: np.full(shape[B], 1000 * (B_max // B) ** 2, np.uint32) for B in Bs}     # G < 0 at every block
    out["children-free"] = {B: np.full(shape[B], LAM_MAX if B == B_max else 0, np.uint32) for B in Bs}  # the largest keys
    huge = full(3)
    huge[B_max][-1, -1] = LAM_MAX
    if len(Bs) == 3:
        huge[Bs[1]][-1, -1] = LAM_MAX - 7
    out["one-huge-block"] = huge
    out["ties"] = {B: (rng.integers(0, 3, shape[B]) * 3).astype(np.uint32) for B in Bs}                 # many equal keys, zero gains
    out["random-32bit"] = {B: rng.integers(0, 1 << 32, shape[B], dtype=np.uint64).astype(np.uint32) for B in Bs}
    out["random-decaying"] = {B: rng.integers(0, 1 << (10 + 2 * Bs[::-1].index(B) * 3), shape[B], dtype=np.uint64).astype(np.uint32) for B in Bs}
    return out


def knapsack(sse, B_max, B_min):
    """int64 [m_max + 1]: the least collage SSE of any quadtree with N_top + 3 m leaves, m = 0 .. m_max, by dynamic programming
    over the top-level blocks.  A top block has 17 leaf counts 0 .. 16 to offer, of which 1, 4, 7, .. (m = 0 .. 5 splits inside
    it) exist: whole; or split, with the m - 1 children of largest gain split too."""
    Bs = qm.levels(B_max, B_min)
    top = _s(sse, B_max).reshape(-1)
    kids = child_sum(_s(sse, Bs[1])).reshape(-1)
    if len(Bs) == 2:
        opts = np.stack([top, kids], axis=1)
    else:
        g1 = _s(sse, Bs[1]) - child_sum(_s(sse, Bs[2]))
        Rh, Rw = _s(sse, B_max).shape
        g = np.sort(g1.reshape(Rh, 2, Rw, 2).transpose(0, 2, 1, 3).reshape(-1, 4), axis=1)[:, ::-1]      # per top block, descending
        opts = np.concatenate([top[:, None], kids[:, None] - np.concatenate([np.zeros((top.size, 1), np.int64), np.cumsum(g, axis=1)], axis=1)], axis=1)
    INF = np.int64(1) << 62
    per = opts.shape[1] - 1
    best = np.full(per * top.size + 1, INF, np.int64)
    best[0] = 0
    for i in range(top.size):
        new = np.full_like(best, INF)
        hi = per * i                                            # splits possible so far
        for m in range(per + 1):
            new[m:m + hi + 1] = np.minimum(new[m:m + hi + 1], best[:hi + 1] + opts[i, m])
        best = new
    return best
