"""Restatement of the betweenness / closeness baselines (baseline/HBA/hba_add.py, hba_2max.py
critical_number, baseline/HCA/hca_add.py, hca_2max.py) on ``oracle.refenv.RefEnv`` -- TEST
INFRASTRUCTURE.

The environment's ``g1`` / ``g2`` are the scripts' ``G1`` / ``G2`` (covered nodes removed, pruned
edges removed, isolated nodes kept), ``L = len(g1)``.  Scores are float64 in the summation order
the device defines, which Python floats reproduce operation for operation:

* closeness: ``((r - 1.0) / tot) * ((r - 1.0) / (L - 1))`` from the BFS reach and distance sum;
* betweenness: per source ``sigma`` pulled over the predecessors and ``delta`` over the successors
  in the row order of the loaded edge list (``RefGraph.adj``), the sources in blocks of
  ``SRC_BLOCK`` consecutive ids, each block summed ascending from 0.0, the block sums ascending
  from 0.0, one multiply by ``1 / ((L - 1) * (L - 2))`` when ``L > 2``.

The live node (layer-0 degree > 0) of largest combined score is removed, the smallest id among
exact equals, until ``env.terminal()``.
"""
from collections import deque

from oracle import refenv

SRC_BLOCK = 8  # CENT_SRC_BLOCK of mdcommunity_amd/csrc/md_cent.h
KINDS = ("betweenness", "closeness")
COMBINES = ("max", "add")
POLICIES = tuple((k, c) for k in KINDS for c in COMBINES)


def alive_rows(env, layer):
    """{node: alive neighbours in the row order of the loaded edge list} of one residual layer."""
    g = env.g1 if layer == 0 else env.g2
    adj = env.graph.adj[layer]
    return {v: [u for u in adj[v] if g.has_edge(v, u)] for v in g.nodes}


def _bfs(rows, s):
    dist = {s: 0}
    order = [s]
    q = deque([s])
    while q:
        v = q.popleft()
        for u in rows[v]:
            if u not in dist:
                dist[u] = dist[v] + 1
                order.append(u)
                q.append(u)
    return dist, order


def closeness_layer(rows):
    big_l = len(rows)
    out = {}
    for v in rows:
        c = 0.0
        if rows[v]:
            dist, _ = _bfs(rows, v)
            tot = sum(dist.values())
            r = len(dist)
            if tot != 0 and big_l > 1:
                c = ((r - 1.0) / tot) * ((r - 1.0) / (big_l - 1))
        out[v] = c
    return out


def _dependencies(rows, s):
    """Brandes' delta_s over the nodes s reaches (s excluded), in the defined order."""
    dist, order = _bfs(rows, s)
    sigma = {s: 1.0}
    for w in order[1:]:
        dw = dist[w] - 1
        acc = 0.0
        for u in rows[w]:
            if dist.get(u) == dw:
                acc = acc + sigma[u]
        assert acc < 2.0 ** 53, "sigma leaves the exact range"
        sigma[w] = acc
    delta = {}
    for v in reversed(order[1:]):
        dv = dist[v] + 1
        sv = sigma[v]
        acc = 0.0
        for w in rows[v]:
            if dist.get(w) == dv:
                coeff = (1.0 + delta[w]) / sigma[w]
                acc = acc + sv * coeff
        delta[v] = acc
    return delta


def betweenness_layer(rows, n):
    big_l = len(rows)
    total = dict.fromkeys(rows, 0.0)
    for b0 in range(0, n, SRC_BLOCK):
        part = {}
        for s in range(b0, min(n, b0 + SRC_BLOCK)):
            if s not in rows or not rows[s]:
                continue
            for v, d in _dependencies(rows, s).items():
                part[v] = part.get(v, 0.0) + d
        for v, x in part.items():
            total[v] = total[v] + x
    if big_l > 2:
        scale = 1.0 / ((big_l - 1) * (big_l - 2))
        for v in total:
            total[v] = total[v] * scale
    return total


def scores(env, kind):
    """({node: c_0}, {node: c_1}) over the uncovered nodes of env's current state."""
    out = []
    for layer in range(2):
        rows = alive_rows(env, layer)
        out.append(closeness_layer(rows) if kind == "closeness" else betweenness_layer(rows, env.graph.num_nodes))
    return out[0], out[1]


def dense_scores(env, kind):
    """The two layers' scores as lists over all node ids (covered nodes 0.0): the device's layout."""
    c0, c1 = scores(env, kind)
    n = env.graph.num_nodes
    return [c0.get(v, 0.0) for v in range(n)], [c1.get(v, 0.0) for v in range(n)]


def combined(c0, c1, combine):
    return {v: (max(c0[v], c1[v]) if combine == "max" else c0[v] + c1[v]) for v in c0}


def pick_from(env, comb):
    best, bs = None, None
    for v in sorted(env.g1.nodes):
        if env.g1.degree(v) == 0:
            continue
        if best is None or comb[v] > bs:
            best, bs = v, comb[v]
    return best, bs


def pick(env, kind, combine):
    """(node, score) of the policy's pick in env's current state; (None, None): no live node."""
    c0, c1 = scores(env, kind)
    return pick_from(env, combined(c0, c1, combine))


def rollout(graph, kind, combine, env=None, max_steps=None, on_state=None):
    """(sequence, LMCC trace, score of every pick, env) from env's state (default: after s0).
    on_state(env, c0, c1, pick) sees every state before its removal."""
    env = env if env is not None else refenv.RefEnv(graph)
    seq, ranks, picked = [], [], []
    while not env.terminal() and (max_steps is None or len(seq) < max_steps):
        c0, c1 = scores(env, kind)
        a, s = pick_from(env, combined(c0, c1, combine))
        assert a is not None, "alive edges but no live node"
        if on_state is not None:
            on_state(env, c0, c1, a)
        ranks.append(env.step(a))
        seq.append(a)
        picked.append(s)
    return seq, ranks, picked, env
