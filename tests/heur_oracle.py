"""Restatement of the baseline heuristics (baseline/HDA/hda_2max.py, baseline/CI/ci_max.py and
the deterministic version of the add scripts) on ``oracle.refenv.RefEnv`` -- TEST INFRASTRUCTURE.

The environment's ``g1`` / ``g2`` are the scripts' ``G1`` / ``G2``: covered nodes removed, pruned
edges removed, isolated nodes kept.  A node is scored from the two residual degrees, the live
node (layer-0 degree > 0) of largest score is removed, the smallest id among equals, until
``env.terminal()`` (the scripts' ``ND_temp == 1``).  Python ints: exact at any size.
"""
from oracle import refenv


def layer_score(g, v, kind):
    d = g.degree(v)
    if kind == "hda":
        return d
    if d == 0:
        return -1
    return (d - 1) * sum(g.degree(u) - 1 for u in g.neighbors(v))


def node_score(env, v, kind, combine):
    s0, s1 = layer_score(env.g1, v, kind), layer_score(env.g2, v, kind)
    return max(s0, s1) if combine == "max" else s0 + s1


def pick(env, kind, combine):
    """(node, score) of the policy's pick in the environment's current state; (None, None) when
    no node is live."""
    best, bs = None, None
    for v in sorted(env.g1.nodes):
        if env.g1.degree(v) == 0:
            continue
        s = node_score(env, v, kind, combine)
        if best is None or s > bs:
            best, bs = v, s
    return best, bs


def max_score(env, kind, combine):
    """The largest score over every remaining node, live or not (what the scripts' lists hold)."""
    return max(node_score(env, v, kind, combine) for v in env.g1.nodes)


def rollout(graph, kind, combine, env=None, max_steps=None):
    """(sequence, LMCC trace, score of every pick, env) from env's state (default: after s0)."""
    env = env if env is not None else refenv.RefEnv(graph)
    seq, ranks, scores = [], [], []
    while not env.terminal() and (max_steps is None or len(seq) < max_steps):
        a, s = pick(env, kind, combine)
        assert a is not None, "alive edges but no live node"
        ranks.append(env.step(a))
        seq.append(a)
        scores.append(s)
    return seq, ranks, scores, env
