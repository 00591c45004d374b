"""The reference's betweenness / closeness baselines as device rollouts (drop-in for the
``baseline/`` scripts ``HBA/hba_add.py``, ``HBA/hba_2max.py``, ``HCA/hca_add.py``,
``HCA/hca_2max.py`` of every variant directory).

Each removal of those scripts recomputes ``nx.betweenness_centrality`` or
``nx.closeness_centrality`` on both layers (an all-pairs BFS in Python) and reruns the networkx
mutual-LMCC cascade; here both run on the GPU (``md_centrality_rollout``): per removal an
all-sources BFS (Brandes) over the alive edges of both layers, the layers combined by ``max`` or
``+``, the live node of largest score removed, the smallest id among exact equals, until the LMCC
is 1.  The scripts draw among the maxima with ``random.choice``; the deterministic rule is one
valid outcome of theirs.  Closeness is networkx's value bit for bit; betweenness is summed in a
fixed order that stays within a few ulp of networkx's.

``method``: ``"hba"`` (betweenness) or ``"hca"`` (closeness).  Out of scope: ``hba_2max.py``'s
``one_pass`` (a static ranking computed once, which also removes isolated nodes), the
``_protect`` and ``_syn`` script variants, and the degree-cost baselines.
"""
import os

import numpy as np

from .baselines import COMBINES, _shared_engine, _triple, maxcc_list

METHODS = ("hba", "hca")
KIND = {"hba": "betweenness", "hca": "closeness"}
# directory names of the scripts' outputs (../../../results/<dir>/none_cost/)
RESULT_DIR = {"hba": "HBA", "hca": "HCA"}


def _check(method, combine):
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}: one of {METHODS}")
    if combine not in COMBINES:
        raise ValueError(f"unknown combine {combine!r}: one of {COMBINES}")


def script_score(mccs, n, n_removed, m_ori):
    """The scripts' own expression ``(sum(MCCs) - 1) / N + (N - len(remove_nodes) - 1) / (M_ori * N)``
    (Python's left-to-right sum over the list ``maxcc_list`` builds)."""
    return (sum(mccs) - 1) / n + (n - n_removed - 1) / (m_ori * n)


def dismantle_batch(graphs, method="hba", combine="max", engine=None):
    """All graphs advance together, one removal per round of launches.  graphs: Graph_test objects
    or (n, edges0, edges1) triples.  Returns [(solution, MaxCCList, score)] per graph, as
    ``critical_number`` + the scripts' score."""
    _check(method, combine)
    eng = engine if engine is not None else _shared_engine()
    tr = [_triple(g) for g in graphs]
    eng.load_graphs(tr)
    eng.reset_deferred()
    res = eng.centrality_rollout(KIND[method], combine)
    m_ori = eng.max_rank()
    out = []
    for (n, _, _), (seq, ranks), m in zip(tr, res, m_ori):
        mccs = maxcc_list(ranks, int(m)) if len(seq) else [1]
        out.append(([int(a) for a in seq], mccs, script_score(mccs, n, len(seq), int(m))))
    return out


def dismantle(g, method="hba", combine="max", engine=None):
    """(solution, MaxCCList, score) of one two-layer graph."""
    return dismantle_batch([g], method, combine, engine)[0]


def write_result_files(out_dir, name, layers, n, m_ori, solution, mccs):
    """The two files the scripts write, in their formats: ``remove_nodes<name>_<l1><l2>_1.txt`` (a
    node id per line) and ``MaxCCList_Strategy_<name>_<l1><l2>_1.txt`` (N lines ``%.8f``: the
    list's first ``len(solution)`` values, then ``1 / M_ori``; then the score.  These scripts
    append no standard-deviation line).  The scripts' own tags are hand-edited per run; the
    ``_<l1><l2>_1`` tag of ``baselines.write_result_files`` is used.  Returns (paths, score)."""
    os.makedirs(out_dir, exist_ok=True)
    f1 = os.path.join(out_dir, "remove_nodes" + name + "_%s%s_1.txt" % (layers[0], layers[1]))
    f2 = os.path.join(out_dir, "MaxCCList_Strategy_" + name + "_%s%s_1.txt" % (layers[0], layers[1]))
    score = script_score(mccs, n, len(solution), m_ori)
    with open(f1, "w") as fo:
        for c in solution:
            fo.write(str(c) + "\n")
    with open(f2, "w") as fo:
        for j in range(n):
            if j < len(solution):
                fo.write("%.8f\n" % mccs[j])
            else:
                fo.write("%.8f\n" % (1 / m_ori))
    with open(f2, "a") as fo:
        fo.write("%.8f\n" % score)
    return (f1, f2), score


def evaluate_real_data(name, num_nodes, layers, out_dir, method="hba", combine="max", data_root="../../data",
                       engine=None):
    """One dataset as the scripts' ``__main__`` treats theirs: reads ``<data_root>/real/<name>.edges``
    with the multiplex reader of the agents, runs the baseline on layers (l1, l2) and writes the
    two result files into out_dir.  Returns (solution, score)."""
    from .agent import MultiDismantler
    from .graph import Graph_test
    _check(method, combine)
    _, gl = MultiDismantler.read_multiplex(None, os.path.join(data_root, "real", name + ".edges"), num_nodes)
    g = Graph_test.from_edges(num_nodes, gl[layers[0] - 1], gl[layers[1] - 1])
    eng = engine if engine is not None else _shared_engine()
    eng.load_graphs([_triple(g)])
    eng.reset_deferred()
    seq, ranks = eng.centrality_rollout(KIND[method], combine)[0]
    m_ori = int(eng.max_rank()[0])
    sol = [int(a) for a in seq]
    mccs = maxcc_list(ranks, m_ori) if sol else [1]
    _, score = write_result_files(out_dir, name, layers, num_nodes, m_ori, sol, mccs)
    print("%s score: %s" % (RESULT_DIR[method], np.float64(score)))
    return sol, score
