#!/usr/bin/env python
"""Generate the baseline-heuristic goldens by running the REFERENCE's baseline scripts here.

Runs only where the reference checkout is present (``/root/reference``, read-only); the tests
read what it wrote.  The scripts (``MultiDismantler_unit_cost/baseline/HDA/hda_2max.py``,
``hda_add.py``, ``CI/ci_max.py``, ``ci_add.py``) are loaded by path; they ``os.chdir`` on import,
so the working directory is restored.  No reference program text is copied: only their functions'
results are stored.

Per case (tests/baseline_cases.py) one ``baselines_<case>.npz``:
  n, m_ori                         nodes, the scripts' M_ori = MCC(G1, G2)
  <hda|ci>_max_seq / _lmcc         critical_number's removal sequence and the value of every MCC
                                   call it made (the module's MCC is wrapped to record them)
  <hda|ci>_max_mccs / _score       its ND_mcc list (float64) and the scripts' (sum(MCCs) - 1) / N
  <hda|ci>_add_seq                 the deterministic add policy's sequence (tests/heur_oracle.py)
  <hda|ci>_add_cert                per step of that sequence: the maximum of the add script's own
                                   score list on the script's graphs (ci_add: get_ci_dict sums;
                                   hda_add: the degree sums its delnode builds)
  <hda|ci>_add_lmcc                the add module's MCC after each of those removals
The add scripts break ties with random.choice and ci_add runs past LMCC 1, so their sequences are
pinned by this certificate (the pick attains the script's maximum at every step, and the LMCC
trace is the script's MCC on that sequence), not by a seeded draw.

File layer: ``hda_2max.py`` and ``ci_max.py`` are also run as ``__main__`` (runpy) in a temporary
tree laid out as they expect (``data/<name>.edges`` three levels up, ``results/<HDA|CI>/none_cost``);
their dataset list is hard-coded, so the tree holds synthetic multiplex files under those names
(written here, seeded; two of them are committed under ``baseline_data/`` with the text files the
scripts wrote for them, ``baseline_<HDA|CI>_<file name>``).
"""
import importlib.util
import json
import os
import runpy
import shutil
import sys
import tempfile
import time

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

import baseline_cases  # noqa: E402
import heur_oracle  # noqa: E402
from oracle import refenv  # noqa: E402

BASE = "/root/reference/code/MultiDismantler_unit_cost/baseline"
SCRIPTS = {("hda", "max"): "HDA/hda_2max.py", ("hda", "add"): "HDA/hda_add.py",
           ("ci", "max"): "CI/ci_max.py", ("ci", "add"): "CI/ci_add.py"}
# the scripts' hard-coded dataset list (name, node counts of its three layer pairs)
SCRIPT_DATA = (("us_air_transportation_american_delta_multiplex", 73, 4.0),
               ("drosophila_melanogaster_multiplex", 557, 3.0),
               ("netsci_co-authorship_multiplex", 40, 3.0))


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


def run_max(mod, n, e0, e1):
    g1, g2 = nx_pair(n, e0, e1)
    own = mod.MCC
    m_ori = own(g1, g2)
    rec = []

    def recording(a, b):
        r = own(a, b)
        rec.append(r)
        return r

    mod.MCC = recording
    try:
        out = mod.critical_number(g1.copy(), g2.copy(), n, m_ori)
    finally:
        mod.MCC = own
    mccs, sol = out[0], out[1]
    return m_ori, [int(a) for a in sol], rec, [float(x) for x in mccs], (sum(mccs) - 1) / n


def run_add(mod, kind, n, e0, e1):
    seq, ranks, scores, _ = heur_oracle.rollout(refenv.RefGraph(n, e0, e1), kind, "add")
    g1, g2 = nx_pair(n, e0, e1)
    mod.MCC(g1, g2)
    cert, lmcc = [], []
    for a in seq:
        if kind == "ci":
            c1, c2 = mod.get_ci_dict(g1), mod.get_ci_dict(g2)
            cert.append(max(c1[v] + c2[v] for v in c1))
        else:
            cert.append(max(g1.degree(v) + g2.degree(v) for v in g1.nodes))
        g1.remove_node(a)
        g2.remove_node(a)
        lmcc.append(mod.MCC(g1, g2))
    return seq, cert, lmcc


def write_script_data(folder):
    """Six-layer ``layer u v`` files under the scripts' dataset names (ids within every N of their list)."""
    os.makedirs(folder, exist_ok=True)
    for k, (name, n, mean_deg) in enumerate(SCRIPT_DATA):
        rs = np.random.RandomState(100 + k)
        with open(os.path.join(folder, name + ".edges"), "w") as f:
            for lid in range(1, 7):
                m = int(mean_deg * n / 2)
                for u, v in zip(rs.randint(0, n, m), rs.randint(0, n, m)):
                    f.write("%d %d %d\n" % (lid, u + 1, v + 1))


def run_script_mains():
    """hda_2max.py and ci_max.py as __main__ in the tree they expect; returns {file name: text}."""
    tmp = tempfile.mkdtemp(prefix="baseline_main_")
    out = {}
    try:
        work = os.path.join(tmp, "V", "baseline", "X")
        os.makedirs(work)
        write_script_data(os.path.join(tmp, "data"))
        for d in ("HDA", "CI"):
            os.makedirs(os.path.join(tmp, "results", d, "none_cost"))
        cwd, path0 = os.getcwd(), list(sys.path)
        for d, rel in (("HDA", SCRIPTS[("hda", "max")]), ("CI", SCRIPTS[("ci", "max")])):
            sys.path.insert(0, work)  # the scripts chdir to sys.path[0]
            try:
                runpy.run_path(os.path.join(BASE, rel), run_name="__main__")
            finally:
                os.chdir(cwd)
                sys.path[:] = path0
            res = os.path.join(tmp, "results", d, "none_cost")
            for fn in sorted(os.listdir(res)):
                out["baseline_%s_%s" % (d, fn)] = open(os.path.join(res, fn)).read()
        for name, _, _ in SCRIPT_DATA[:2]:
            os.makedirs(baseline_cases.DATA, exist_ok=True)
            shutil.copy(os.path.join(tmp, "data", name + ".edges"), os.path.join(baseline_cases.DATA, name + ".edges"))
    finally:
        shutil.rmtree(tmp)
    return out


def main():
    t0 = time.time()
    texts = run_script_mains()
    kept = []
    for _, stem, _, layers in baseline_cases.FILE_CASES[1:]:
        for d in ("HDA", "CI"):
            for pre in ("remove_nodes", "MaxCCList_Strategy_"):
                fn = "baseline_%s_%s%s_%s%s_1.txt" % (d, pre, stem, layers[0], layers[1])
                with open(os.path.join(HERE, fn), "w") as f:
                    f.write(texts[fn])
                kept.append(fn)
    mods = {k: load_script(v) for k, v in SCRIPTS.items()}
    meta = {"reference": "MultiDismantler_unit_cost/baseline/{HDA/hda_2max,HDA/hda_add,CI/ci_max,CI/ci_add}.py",
            "file_layer": "hda_2max.py and ci_max.py run as __main__ (runpy); texts kept: " + ", ".join(kept),
            "cases": {}}
    for case, (n, e0, e1) in baseline_cases.graphs().items():
        d = {"n": np.int32(n)}
        info = {"n": n, "E": [len(e0), len(e1)]}
        for kind in ("hda", "ci"):
            m_ori, sol, lmcc, mccs, score = run_max(mods[(kind, "max")], n, e0, e1)
            d["m_ori"] = np.int32(m_ori)
            d[f"{kind}_max_seq"] = np.asarray(sol, np.int32)
            d[f"{kind}_max_lmcc"] = np.asarray(lmcc, np.int32)
            d[f"{kind}_max_mccs"] = np.asarray(mccs, np.float64)
            d[f"{kind}_max_score"] = np.float64(score)
            seq, cert, lm = run_add(mods[(kind, "add")], kind, n, e0, e1)
            d[f"{kind}_add_seq"] = np.asarray(seq, np.int32)
            d[f"{kind}_add_cert"] = np.asarray(cert, np.int64)
            d[f"{kind}_add_lmcc"] = np.asarray(lm, np.int32)
            info[kind] = {"max_removals": len(sol), "add_removals": len(seq), "max_score": score}
        info["m_ori"] = int(d["m_ori"])
        np.savez_compressed(os.path.join(HERE, f"baselines_{case}.npz"), **d)
        meta["cases"][case] = info
        print(case, info, flush=True)
    meta["seconds"] = time.time() - t0
    with open(os.path.join(HERE, "meta_baselines.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
