#!/usr/bin/env python
"""Cost of the betweenness / closeness rollouts (md_centrality_rollout) against what a user of
the engine pays without them: a host loop of md_get_state, networkx centrality of both residual
layers, and md_step.  Writes profiles/centrality_bench.json.

The two kinds (combine max) alternate in one process:
  single   gmm1000_s0 (the golden graph), one graph per call
  batch    64 GMM graphs N = 1000 (seeds 0..63), one call
  large    N = 18 000 real-like multiplex (mdcommunity_amd.synth): first the cost of its first
           removals (md_centrality_scores, the pick on the host, md_step), then the whole rollout
           when the estimate fits --large-seconds; otherwise it is reported as not run
  host     gmm200_s7: the networkx host loop against the device rollout of the same graph
           (networkx at N = 1000 takes minutes per removal)
Reported: kernel ms (md_last_timing) and wall ms per rollout and per removal, medians.

    python scripts/cent_bench.py [--reps 3] [--batch-graphs 64] [--large-n 18000] [--large-seconds 240]
"""
import argparse
import json
import os
import statistics
import sys
import time

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mdcommunity_amd import _lib, synth  # noqa: E402

KINDS = ("betweenness", "closeness")
NX_FN = {"betweenness": nx.betweenness_centrality, "closeness": nx.closeness_centrality}


def golden_graph(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"rollout_{name}.npz")) as z:
        return int(z["n_nodes"]), z["edges0"].astype(np.int32), z["edges1"].astype(np.int32)


def device_call(eng, graphs, kind, load=True):
    if load:
        eng.load_graphs(graphs)
    t0 = time.perf_counter()
    eng.reset_deferred()
    res = eng.centrality_rollout(kind, "max")
    wall = (time.perf_counter() - t0) * 1e3
    ms, nl = eng.last_timing()
    return [s.tolist() for s, _ in res], dict(wall_ms=wall, kernel_ms=ms, launches=nl)


def summarize(runs, removals, graphs, rounds):
    out = {k: statistics.median(r[k] for r in runs) for k in ("wall_ms", "kernel_ms", "launches")}
    out["reps"] = len(runs)
    out["wall_ms_all"] = [round(r["wall_ms"], 3) for r in runs]
    out["wall_ms_per_rollout"] = out["wall_ms"] / graphs
    out["kernel_ms_per_rollout"] = out["kernel_ms"] / graphs
    out["wall_us_per_removal"] = 1e3 * out["wall_ms"] / max(1, removals)
    out["kernel_us_per_removal"] = 1e3 * out["kernel_ms"] / max(1, removals)
    # a batch advances together: one round of launches serves a removal of every running graph
    out["wall_us_per_round"] = 1e3 * out["wall_ms"] / max(1, rounds)
    return out


def device_rows(eng, graphs, reps):
    runs = {k: [] for k in KINDS}
    seqs = {}
    for k in KINDS:
        device_call(eng, graphs, k)  # warm-up
    for _ in range(reps):
        for k in KINDS:  # alternating
            seqs[k], t = device_call(eng, graphs, k)
            runs[k].append(t)
    out = {}
    for k in KINDS:
        rem = sum(len(s) for s in seqs[k])
        out[k] = dict(graphs=len(graphs), removals=rem, device=summarize(runs[k], rem, len(graphs), max(map(len, seqs[k]))))
        print(len(graphs), "graphs", k, json.dumps(out[k]), flush=True)
    return out, seqs


def networkx_loop(eng, g, kind):
    """md_get_state -> networkx centrality of both residual layers -> md_step, until terminal."""
    n = g[0]
    edges = [np.asarray(g[1 + l], np.int64).reshape(-1, 2) for l in range(2)]
    eng.load_graphs([g])
    t0 = time.perf_counter()
    eng.reset()
    seq = []
    while True:
        cov, r0, r1, _ = eng.get_state(0)
        cov = np.asarray(cov, bool)
        layers = []
        for e, rem in ((edges[0], r0), (edges[1], r1)):
            alive = ~np.asarray(rem, bool) & ~cov[e[:, 0]] & ~cov[e[:, 1]]
            gr = nx.Graph()
            gr.add_nodes_from(int(v) for v in np.flatnonzero(~cov))
            gr.add_edges_from((int(u), int(v)) for u, v in e[alive])
            layers.append(gr)
        if layers[0].number_of_edges() == 0 or layers[1].number_of_edges() == 0:
            break
        c0, c1 = NX_FN[kind](layers[0]), NX_FN[kind](layers[1])
        best, bs = -1, -1.0
        for v in range(n):
            if v in c0 and layers[0].degree(v) > 0 and max(c0[v], c1[v]) > bs:
                best, bs = v, max(c0[v], c1[v])
        eng.step([best])
        seq.append(best)
    return seq, (time.perf_counter() - t0) * 1e3


def first_removals(eng, g, kind, k):
    """Per-removal cost on a graph whose whole rollout may not fit the time: k removals by
    md_centrality_scores (the centrality launches of one removal), the pick on the host, md_step."""
    eng.load_graphs([g])
    eng.reset()
    rows = []
    for _ in range(k):
        t0 = time.perf_counter()
        c0, c1 = eng.centrality_scores(kind)[0]
        ms, _ = eng.last_timing()
        deg = np.zeros(g[0], bool)
        cov, r0, _, _ = eng.get_state(0)
        e = np.asarray(g[1], np.int64).reshape(-1, 2)
        alive = ~np.asarray(r0, bool) & ~np.asarray(cov, bool)[e[:, 0]] & ~np.asarray(cov, bool)[e[:, 1]]
        deg[e[alive].ravel()] = True
        if not deg.any():
            break
        a = int(np.argmax(np.where(deg, np.maximum(c0, c1), -1.0)))
        eng.step([a])
        ms2, _ = eng.last_timing()
        rows.append(dict(centrality_kernel_ms=ms, step_kernel_ms=ms2, wall_ms=(time.perf_counter() - t0) * 1e3))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-graphs", type=int, default=64)
    ap.add_argument("--large-n", type=int, default=18000)
    ap.add_argument("--large-seconds", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centrality_bench.json"))
    a = ap.parse_args()
    eng = _lib.Engine(np.zeros(_lib.MD_WEIGHT_FLOATS, np.float32))
    res = {"library": _lib.load_library().md_version().decode(), "networkx": nx.__version__,
           "device": "md_reset_deferred + md_centrality_rollout (combine max), the two kinds alternating",
           "host_loop": "md_reset, then per removal md_get_state, networkx centrality of both layers, md_step"}

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)

    res["single_gmm1000_s0"], _ = device_rows(eng, [golden_graph("gmm1000_s0")], a.reps)
    save()
    # what a user pays today, on the size networkx can still take
    small = golden_graph("gmm200_s7")
    dev, seqs = device_rows(eng, [small], a.reps)
    host = {}
    for k in KINDS:
        seq, wall = networkx_loop(eng, small, k)
        if k == "closeness":
            assert seq == seqs[k][0], "the networkx loop and the device rollout differ"
        host[k] = dict(removals=len(seq), wall_ms=wall, wall_us_per_removal=1e3 * wall / max(1, len(seq)),
                       same_sequence=seq == seqs[k][0],
                       wall_ratio_per_removal=(wall / max(1, len(seq))) / (dev[k]["device"]["wall_us_per_removal"] / 1e3))
        print("networkx loop", k, json.dumps(host[k]), flush=True)
    res["gmm200_s7"] = dict(device=dev, networkx_host_loop=host)
    save()
    if a.batch_graphs > 0:
        from mdcommunity_amd import gmm_gpu
        pairs = gmm_gpu.gmm_pairs(1000, list(range(a.batch_graphs)), exact=True, device=0)
        res[f"batch_{a.batch_graphs}_gmm1000"], _ = device_rows(eng, [(1000, e0, e1) for e0, e1 in pairs], max(1, a.reps - 1))
        save()
    if a.large_n > 0:
        lay = synth.real_like_layers(n=a.large_n, seed=0)
        es = [np.array(sorted({(min(u, v), max(u, v)) for u, v in l if u != v}), np.int32) for l in lay]
        g = (a.large_n, es[0], es[1])
        eng.load_graphs([g])
        eng.reset_deferred()
        est_removals = len(eng.heuristic_rollout("hda", "max")[0][0])  # a proxy for the rollout's length
        big = {"edges": [len(es[0]), len(es[1])], "hda_max_removals": est_removals}
        for k in KINDS:
            rows = first_removals(eng, g, k, 4)
            per = statistics.median(r["wall_ms"] for r in rows[1:]) if len(rows) > 1 else rows[0]["wall_ms"]
            big[k] = dict(first_removals=rows, wall_ms_per_removal=per, estimated_rollout_s=per * est_removals / 1e3)
            print("large first removals", k, json.dumps(big[k]), flush=True)
            res[f"large_real_like_{a.large_n}"] = big
            save()
        left = a.large_seconds
        for k in KINDS:
            est = big[k]["estimated_rollout_s"]
            if 1.5 * est > left:
                big[k]["rollout"] = "not run: the estimate (%.0f s) does not fit the %.0f s left of the time limit" % (est, left)
                continue
            seq, t = device_call(eng, [g], k)
            left -= t["wall_ms"] / 1e3
            big[k]["rollout"] = dict(removals=len(seq[0]), **summarize([t], len(seq[0]), 1, len(seq[0])))
            print("large rollout", k, json.dumps(big[k]["rollout"]), flush=True)
            save()
    eng.close()
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
