"""Brute-force DBSCAN in numpy float64, written from the definition in the header
of fs2_cluster.hip (no sklearn, no cells, no shortcuts): the reference the GPU
clustering tests compare with.

    neighbour(p, q)  <=>  fl(fl(dx*dx) + fl(dy*dy)) <= fl(eps*eps)   (p itself counts)
    core(p)          <=>  |{q : neighbour(p, q)}| >= min_samples
    clusters          =   grown from the unlabelled core points in index order, so
                          they are numbered by their smallest core index and a
                          border point gets the first cluster that reaches it
    centre            =   sequential sum of the members in index order / count
"""
import numpy as np

ROWS = 512          # rows of the O(n^2) neighbour matrix built at a time


def neighbour_lists(points, eps):
    """Per point, the ascending indices of its neighbours (itself included)."""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    eps = float(eps)
    eps2 = np.float64(eps * eps)
    x, y = pts[:, 0].copy(), pts[:, 1].copy()
    out = []
    for r0 in range(0, len(pts), ROWS):
        dx = x[r0:r0 + ROWS, None] - x[None, :]
        dy = y[r0:r0 + ROWS, None] - y[None, :]
        dx *= dx                               # fl(dx*dx)
        dy *= dy                               # fl(dy*dy)
        dx += dy                               # fl(fl(dx*dx) + fl(dy*dy)): numpy never contracts
        rows, cols = np.nonzero(dx <= eps2)
        out.extend(np.split(cols, np.searchsorted(rows, np.arange(1, len(dx)))))
    return out


def dbscan(points, eps, min_samples):
    """(labels int32 [n], centres float64 [K][2])."""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(pts)
    nbrs = neighbour_lists(pts, eps)
    core = np.array([len(v) >= min_samples for v in nbrs], dtype=bool)
    labels = np.full(n, -1, dtype=np.int32)
    K = 0
    for i in range(n):
        if labels[i] != -1 or not core[i]:
            continue
        labels[i] = K
        stack = [i]
        while stack:
            j = stack.pop()
            if not core[j]:
                continue                       # a border point joins but does not spread
            new = nbrs[j][labels[nbrs[j]] == -1]
            labels[new] = K
            stack.extend(new.tolist())
        K += 1
    return labels, centres_of(pts, labels)


def centres_of(points, labels):
    """Index-order sequential mean of every cluster, [K][2]."""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    K = int(labels.max()) + 1 if len(labels) else 0
    cen = np.zeros((max(K, 0), 2))
    for k in range(K):
        sx = sy = 0.0
        m = pts[labels == k]
        for px, py in m.tolist():
            sx += px
            sy += py
        cen[k] = (sx / len(m), sy / len(m))
    return cen


def known_landmark_points(cnt, lm):
    """Every landmark (x, y) of every particle in (particle, slot) order, [total][2]."""
    cnt = np.asarray(cnt)
    rows = [np.asarray(lm[i, :cnt[i], :2], dtype=np.float64) for i in range(len(cnt))]
    return np.concatenate(rows).reshape(-1, 2) if rows else np.zeros((0, 2))


def min_samples_of(total, N, fraction):
    """min_samples of update_known_landmarks: Python's own int(total / N * fraction)."""
    return int(int(total) / int(N) * float(fraction))
