#!/usr/bin/env python
"""Generate the centrality-baseline goldens with the REFERENCE's HBA / HCA scripts' own functions.

Runs only where the reference checkout is present (read-only; ``MD_REFERENCE`` names its root); the
tests read what it wrote.  The
scripts (``MultiDismantler_unit_cost/baseline/HBA/hba_add.py``, ``hba_2max.py``,
``HCA/hca_add.py``, ``hca_2max.py``) are loaded by path; they ``os.chdir`` on import, so the
working directory is restored.  No reference program text is copied: only results are stored.

The scripts draw among the maxima with ``random.choice``, so their sequences are pinned along the
restatement's deterministic sequence (tests/cent_oracle.py) instead of by a seeded draw.  Per
case (tests/centrality_cases.py) one ``centrality_<case>.npz``, per policy ``<kind>_<combine>``:
  n, m_ori          nodes, the scripts' M_ori = MCC(G1, G2)
  _seq              the restatement's removal sequence
  _lmcc             the script module's MCC after each of those removals, on the script's graphs
  _mccs             its MCCs list ([1, m / M_ori, ...], float64)
  _score            (sum(MCCs) - 1) / N + (N - len(remove_nodes) - 1) / (M_ori * N)
  _ref_pick, _ref_max   per step, on the script's graphs before the removal: the script's score
                    (its max_cs expression over nx.betweenness_centrality / nx.closeness_centrality)
                    of the restatement's pick, and the maximum of its list
For TEXT_CASE the two result files of the max policies are kept as text,
``centrality_<HBA|HCA>_<file name>``, written with the scripts' format expressions.
"""
import importlib.util
import json
import os
import sys
import time

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

import baseline_cases  # noqa: E402
import cent_oracle  # noqa: E402
import centrality_cases  # noqa: E402
from oracle import refenv  # noqa: E402

BASE = os.path.join(os.environ.get("MD_REFERENCE", "/root/reference"), "code", "MultiDismantler_unit_cost", "baseline")
SCRIPTS = {("betweenness", "max"): "HBA/hba_2max.py", ("betweenness", "add"): "HBA/hba_add.py",
           ("closeness", "max"): "HCA/hca_2max.py", ("closeness", "add"): "HCA/hca_add.py"}
NX_FN = {"betweenness": nx.betweenness_centrality, "closeness": nx.closeness_centrality}


def load_script(rel):
    cwd = os.getcwd()
    try:
        spec = importlib.util.spec_from_file_location("ref_" + os.path.basename(rel)[:-3], os.path.join(BASE, rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.chdir(cwd)
    return mod


def nx_pair(n, e0, e1):
    out = []
    for e in (e0, e1):
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from((int(u), int(v)) for u, v in e)
        out.append(g)
    return out


def run_policy(mod, kind, comb, n, e0, e1):
    seq, ranks, _, _ = cent_oracle.rollout(refenv.RefGraph(n, e0, e1), kind, comb)
    g1, g2 = nx_pair(n, e0, e1)
    m_ori = mod.MCC(g1, g2)
    mccs, lmcc, ref_pick, ref_max = [1], [], [], []
    for a in seq:
        c1, c2 = NX_FN[kind](g1), NX_FN[kind](g2)
        cs = {v: (max(c1[v], c2[v]) if comb == "max" else c1[v] + c2[v]) for v in c1}
        ref_pick.append(cs[a])
        ref_max.append(max(cs.values()))
        g1.remove_node(a)
        g2.remove_node(a)
        m = mod.MCC(g1, g2)
        mccs.append(m / m_ori)
        lmcc.append(m)
    assert lmcc == ranks, "the restatement's LMCC trace differs from the script's MCC"
    score = (sum(mccs) - 1) / n + (n - len(seq) - 1) / (m_ori * n)
    return m_ori, seq, lmcc, mccs, score, ref_pick, ref_max


def write_texts(name, n, m_ori, seq, mccs, score, result_dir):
    with open(os.path.join(HERE, centrality_cases.text_name(result_dir, "remove_nodes")), "w") as f:
        for c in seq:
            f.write(str(c) + '\n')
    with open(os.path.join(HERE, centrality_cases.text_name(result_dir, "MaxCCList_Strategy_")), "w") as f:
        for j in range(n):
            if j < len(seq):
                f.write('%.8f\n' % mccs[j])
            else:
                f.write('%.8f\n' % (1 / m_ori))
        f.write('%.8f\n' % score)


def main():
    t0 = time.time()
    mods = {k: load_script(v) for k, v in SCRIPTS.items()}
    meta = {"reference": "MultiDismantler_unit_cost/baseline/{HBA/hba_2max,HBA/hba_add,HCA/hca_2max,HCA/hca_add}.py",
            "networkx": nx.__version__, "cases": {}}
    for case, (n, e0, e1) in centrality_cases.graphs().items():
        d = {"n": np.int32(n)}
        info = {"n": n, "E": [len(e0), len(e1)]}
        for kind, comb in centrality_cases.POLICIES:
            m_ori, seq, lmcc, mccs, score, rp, rm = run_policy(mods[(kind, comb)], kind, comb, n, e0, e1)
            k = f"{kind}_{comb}"
            d["m_ori"] = np.int32(m_ori)
            d[k + "_seq"] = np.asarray(seq, np.int32)
            d[k + "_lmcc"] = np.asarray(lmcc, np.int32)
            d[k + "_mccs"] = np.asarray(mccs, np.float64)
            d[k + "_score"] = np.float64(score)
            d[k + "_ref_pick"] = np.asarray(rp, np.float64)
            d[k + "_ref_max"] = np.asarray(rm, np.float64)
            info[k] = {"removals": len(seq), "score": score}
            if case == centrality_cases.TEXT_CASE and comb == "max":
                rdir = [r for _, kk, r in centrality_cases.TEXT_METHODS if kk == kind][0]
                write_texts(case, n, m_ori, seq, mccs, score, rdir)
        info["m_ori"] = int(d["m_ori"])
        np.savez_compressed(os.path.join(HERE, f"centrality_{case}.npz"), **d)
        meta["cases"][case] = info
        print(case, info, flush=True)
    meta["seconds"] = time.time() - t0
    with open(os.path.join(HERE, "meta_centrality.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
