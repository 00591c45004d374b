"""Static community prior of the community-enhanced model (CEMultiDismantler).

The model's node input has a third column: a per-node, per-layer prior computed once per graph
from a community partition of each layer.  Only the binary *boundary* prior is supported
(``COMM_PRIOR_FEATURE = "boundary"``): 1.0 where a node has a neighbour in another community,
else 0.0.  Nodes absent from the partition count as community 0; isolated nodes get 0.

Prior caches use the reference's npz layout (keys ``n``, ``feat0``, ``feat1``, ``boundary``), so
existing ``cache/comm_prior_<id>_boundary.npz`` files load as they are.

The partition comes from python-louvain (``community.best_partition(G, random_state=0)``) when
it is installed; otherwise :func:`partition` warns once and returns None, and the prior is all
zeros -- the reference's own fallback.
"""
import os
import warnings

import numpy as np

FEATURE = "boundary"
_warned = []


def boundary_prior(n, edges, labels):
    """float32 [n]: 1.0 where a node has a neighbour with a different label.

    edges   [E, 2] undirected edges on nodes 0..n-1
    labels  a dict node -> community, or an array of n labels (negative: absent); absent
            nodes count as community 0
    """
    n = int(n)
    if isinstance(labels, dict):
        lab = np.zeros(n, dtype=np.int64)
        if labels:
            k = np.fromiter(labels.keys(), dtype=np.int64, count=len(labels))
            v = np.fromiter(labels.values(), dtype=np.int64, count=len(labels))
            ok = (k >= 0) & (k < n)
            lab[k[ok]] = v[ok]
    else:
        lab = np.asarray(labels, dtype=np.int64).reshape(-1).copy()
        if lab.size != n:
            raise ValueError(f"expected {n} labels, got {lab.size}")
        lab[lab < 0] = 0
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(n, dtype=np.float32)
    if e.size:
        cross = lab[e[:, 0]] != lab[e[:, 1]]
        out[e[cross, 0]] = 1.0
        out[e[cross, 1]] = 1.0
    return out


def partition(n, edges, seed=0):
    """Louvain partition of one layer (node -> community) with python-louvain, or None (with
    one warning) when it is not installed."""
    try:
        import community as community_louvain
        best = community_louvain.best_partition
    except Exception:
        if not _warned:
            _warned.append(True)
            warnings.warn("python-louvain is not installed: the community prior is all zeros "
                          "(the reference's fallback); supply a prior cache or graph.node_comm_feat")
        return None
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(int(n)))
    g.add_edges_from((int(u), int(v)) for u, v in np.asarray(edges).reshape(-1, 2))
    return best(g, random_state=seed)


def cache_path(cache_dir, cache_id):
    return os.path.join(cache_dir, f"comm_prior_{cache_id}_{FEATURE}.npz")


def load_cache(path, n):
    """(prior0, prior1) from a prior cache of a graph of n nodes, or None (missing file, other n)."""
    if not os.path.isfile(path):
        return None
    with np.load(path, allow_pickle=False) as z:
        if "n" not in z.files or int(z["n"]) != int(n):
            return None
        return [np.asarray(z["feat0"], dtype=np.float32), np.asarray(z["feat1"], dtype=np.float32)]


def save_cache(path, priors):
    p0, p1 = (np.asarray(p, dtype=np.float32) for p in priors)
    union = np.where((p0 > 0.5) | (p1 > 0.5))[0].astype(np.int64)
    np.savez_compressed(path, n=np.int64(p0.size), feat0=p0, feat1=p1, boundary=union)


def zero_prior(n):
    return [np.zeros(int(n), np.float32), np.zeros(int(n), np.float32)]


def graph_prior(g):
    """The (prior0, prior1) a graph carries as ``node_comm_feat``, zeros when it has none."""
    feat = getattr(g, "node_comm_feat", None)
    if feat is None or len(feat) < 2:
        return zero_prior(g.num_nodes)
    out = []
    for l in range(2):
        a = np.asarray(feat[l], dtype=np.float32).reshape(-1)
        out.append(a if a.size == g.num_nodes else np.zeros(g.num_nodes, np.float32))
    return out


def attach_prior(g, cache_dir=None, cache_id=None):
    """Set ``g.node_comm_feat`` / ``g.boundary_nodes``: the cache, else a partition of each layer,
    else zeros.  A freshly computed prior is written to the cache when one is named."""
    n = g.num_nodes
    path = cache_path(cache_dir, cache_id) if cache_dir and cache_id else None
    priors = load_cache(path, n) if path else None
    if priors is None:
        parts = [partition(n, g.edges[l]) for l in range(2)]
        if parts[0] is None or parts[1] is None:
            priors = zero_prior(n)
        else:
            priors = [boundary_prior(n, g.edges[l], parts[l]) for l in range(2)]
            if path:
                os.makedirs(os.path.dirname(path), exist_ok=True)
                save_cache(path, priors)
    g.node_comm_feat = priors
    g.boundary_nodes = set(np.where((priors[0] > 0.5) | (priors[1] > 0.5))[0].tolist())
    return priors
