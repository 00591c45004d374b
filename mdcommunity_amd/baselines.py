"""The reference's hand-written baselines as device rollouts (drop-in for the ``baseline/``
scripts of every variant directory: ``HDA/hda_2max.py``, ``HDA/hda_add.py``, ``CI/ci_max.py``,
``CI/ci_add.py``).

Each removal of those scripts reruns the networkx mutual-LMCC cascade ``MCC(G1, G2)``; here the
whole rollout runs on the GPU (``md_heuristic_rollout``): the pick is the live node of largest
integer score -- HDA: residual degree, CI (radius 1): ``(d - 1) * sum(d_u - 1)`` over the alive
neighbours, -1 for an isolated node -- combined over the two layers by ``max`` or ``+``, the
smallest node id among equals, until the LMCC is 1.  That is exactly what ``hda_2max.py`` and
``ci_max.py`` compute (their stable ``sorted(..., reverse=True)`` over nodes in id order keeps
the smallest id).  The ``add`` scripts draw among the maxima with ``random.choice`` and
``ci_add.py`` keeps removing nodes after the LMCC has reached 1; ``combine="add"`` here uses the
deterministic rule and stop of the ``max`` scripts, so its sequences are one valid outcome of
the scripts' rule, not their seeded draw.

HBA / HCA (betweenness, closeness) are in ``mdcommunity_amd.baselines_centrality``.  Out of scope:
the ``_protect`` and ``_syn`` script variants, and the degree-cost baselines
(``MultiDismantler_degree_cost/baseline`` scores differently).
"""
import os

import numpy as np

from . import _lib

METHODS = ("hda", "ci")
COMBINES = ("max", "add")
# directory names of the scripts' outputs (../../../results/<dir>/none_cost/)
RESULT_DIR = {"hda": "HDA", "ci": "CI"}

_engine = None


def _shared_engine():
    """One context for the baselines (they read neither the weights nor a prior)."""
    global _engine
    if _engine is None:
        _engine = _lib.Engine(np.zeros(_lib.MD_WEIGHT_FLOATS, np.float32))
    return _engine


def _triple(g):
    if hasattr(g, "edges") and hasattr(g, "num_nodes"):
        return int(g.num_nodes), g.edges[0], g.edges[1]
    n, e0, e1 = g
    return int(n), e0, e1


def _check(method, combine):
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}: one of {METHODS}")
    if combine not in COMBINES:
        raise ValueError(f"unknown combine {combine!r}: one of {COMBINES}")


def maxcc_list(ranks, m_ori):
    """The scripts' ``ND_mcc``: ``[1, r_1 / M_ori, r_2 / M_ori, ...]`` (an int, then float64)."""
    return [1] + [int(r) / int(m_ori) for r in ranks]


def audc_score(mccs, n):
    """The scripts' own expression ``(sum(MCCs) - 1) / N`` over the list above (Python's
    left-to-right sum; an accumulated ``r / (M_ori * N)`` differs in the last bit)."""
    return (sum(mccs) - 1) / n


def dismantle_batch(graphs, method="hda", combine="max", engine=None):
    """All graphs in one launch.  graphs: Graph_test objects or (n, edges0, edges1) triples.
    Returns [(solution, MaxCCList, score)] per graph, as ``critical_number`` + the scripts' score."""
    _check(method, combine)
    eng = engine if engine is not None else _shared_engine()
    tr = [_triple(g) for g in graphs]
    eng.load_graphs(tr)
    eng.reset_deferred()
    res = eng.heuristic_rollout(method, combine)
    m_ori = eng.max_rank()
    out = []
    for (n, _, _), (seq, ranks), m in zip(tr, res, m_ori):
        mccs = maxcc_list(ranks, int(m)) if len(seq) else [1]
        out.append(([int(a) for a in seq], mccs, audc_score(mccs, n)))
    return out


def dismantle(g, method="hda", combine="max", engine=None):
    """(solution, MaxCCList, score) of one two-layer graph."""
    return dismantle_batch([g], method, combine, engine)[0]


def write_result_files(out_dir, name, layers, n, m_ori, solution, mccs):
    """The two files the scripts write, in their formats (one run, ``n = 1`` there):
    ``remove_nodes<name>_<l1><l2>_1.txt`` (a node id per line) and
    ``MaxCCList_Strategy_<name>_<l1><l2>_1.txt`` (N lines ``%.8f``: the list, padded with
    ``1 / M_ori``; then the score's mean and standard deviation).  Returns (paths, score)."""
    os.makedirs(out_dir, exist_ok=True)
    f1 = os.path.join(out_dir, "remove_nodes" + name + "_%s%s_1.txt" % (layers[0], layers[1]))
    f2 = os.path.join(out_dir, "MaxCCList_Strategy_" + name + "_%s%s_1.txt" % (layers[0], layers[1]))
    avg = [0 + mccs[i] for i in range(min(n, len(mccs)))]
    score = audc_score(mccs, n)
    scores = [score]
    with open(f1, "w") as fo:
        for c in solution:
            fo.write(str(c) + "\n")
    with open(f2, "w") as fo:
        for k in range(n):
            if k < len(avg):
                fo.write("%.8f\n" % (float(avg[k] / 1)))
            else:
                fo.write("%.8f\n" % (1 / m_ori))
    with open(f2, "a") as fo:
        fo.write("%.8f\n" % np.mean(scores))
        fo.write("%.8f\n" % np.std(scores))
    return (f1, f2), score


def evaluate_real_data(name, num_nodes, layers, out_dir, method="hda", combine="max", data_root="../../data",
                       engine=None):
    """One dataset of the scripts' ``__main__`` loop: reads ``<data_root>/real/<name>.edges`` with
    the multiplex reader of the agents, runs the baseline on layers (l1, l2) and writes the two
    result files into out_dir.  Returns (solution, score)."""
    from .agent import MultiDismantler
    from .graph import Graph_test
    _check(method, combine)
    _, gl = MultiDismantler.read_multiplex(None, os.path.join(data_root, "real", name + ".edges"), num_nodes)
    g = Graph_test.from_edges(num_nodes, gl[layers[0] - 1], gl[layers[1] - 1])
    eng = engine if engine is not None else _shared_engine()
    eng.load_graphs([_triple(g)])
    eng.reset_deferred()
    seq, ranks = eng.heuristic_rollout(method, combine)[0]
    m_ori = int(eng.max_rank()[0])
    sol = [int(a) for a in seq]
    mccs = maxcc_list(ranks, m_ori) if sol else [1]
    _, score = write_result_files(out_dir, name, layers, num_nodes, m_ori, sol, mccs)
    print("%s score: %s std %s" % (RESULT_DIR[method], np.mean([score]), np.std([score])))
    return sol, score
