#!/usr/bin/env python
"""Cost of the baseline-heuristic rollouts (md_heuristic_rollout) against what the engine offered
before them: a host loop of md_step with the pick computed in numpy from the state md_get_state
returns.  Writes profiles/heuristic_bench.json.

Per policy (hda / ci x max / add), alternating the two in the same process:
  single   gmm1000_s0 (the golden graph), one graph per call
  batch    256 GMM graphs N = 1000 (seeds 0..255, the bench's batch object), one call
  hbm      N = 18 000 real-like multiplex (mdcommunity_amd.synth), the HBM path: new call only
and the oracle restatement's (networkx) wall time of `single` on this host.
Reported: kernel ms (md_last_timing) and wall ms per rollout, and both per removal.

    python scripts/heur_bench.py [--reps 5] [--batch-graphs 256] [--out profiles/heuristic_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mdcommunity_amd import _lib, synth  # noqa: E402

POLICIES = (("hda", "max"), ("hda", "add"), ("ci", "max"), ("ci", "add"))


def numpy_pick(n, e, cov, rem, kind, comb):
    """The policy's pick from a graph's state as md_get_state returns it; -1 when terminal."""
    deg, ns = [], []
    for l in range(2):
        u, v = e[l][:, 0], e[l][:, 1]
        alive = ~rem[l] & ~cov[u] & ~cov[v]
        u, v = u[alive], v[alive]
        d = np.bincount(u, minlength=n) + np.bincount(v, minlength=n)
        deg.append(d.astype(np.int64))
        if kind == "ci":
            ns.append((np.bincount(u, weights=d[v] - 1, minlength=n)
                       + np.bincount(v, weights=d[u] - 1, minlength=n)).astype(np.int64))
    if not deg[0].any() or not deg[1].any():
        return -1
    if kind == "hda":
        s = deg
    else:
        s = [np.where(deg[l] == 0, -1, (deg[l] - 1) * ns[l]) for l in range(2)]
    sc = np.maximum(s[0], s[1]) if comb == "max" else s[0] + s[1]
    sc = np.where(deg[0] > 0, sc, np.iinfo(np.int64).min)
    return int(np.argmax(sc))  # the first maximum: the smallest id


def host_loop(eng, graphs, kind, comb):
    """The parent's way: md_get_state -> numpy pick -> md_step, every graph of the batch per step."""
    eng.load_graphs(graphs)
    t0 = time.perf_counter()
    eng.reset()
    edges = [[np.asarray(g[1 + l], np.int64).reshape(-1, 2) for l in range(2)] for g in graphs]
    seqs = [[] for _ in graphs]
    kernel_ms, launches = 0.0, 0
    active = list(range(len(graphs)))
    while active:
        acts = np.full(len(graphs), -1, np.int32)
        nxt = []
        for g in active:
            cov, r0, r1, _ = eng.get_state(g)
            a = numpy_pick(graphs[g][0], edges[g], cov, (r0, r1), kind, comb)
            if a >= 0:
                acts[g] = a
                seqs[g].append(a)
                nxt.append(g)
        if not nxt:
            break
        eng.step(acts)
        ms, nl = eng.last_timing()
        kernel_ms += ms
        launches += nl
        active = nxt
    wall = (time.perf_counter() - t0) * 1e3
    return seqs, dict(wall_ms=wall, kernel_ms=kernel_ms, launches=launches)


def device_call(eng, graphs, kind, comb, load=True):
    if load:
        eng.load_graphs(graphs)
    t0 = time.perf_counter()
    eng.reset_deferred()
    res = eng.heuristic_rollout(kind, comb)
    wall = (time.perf_counter() - t0) * 1e3
    ms, nl = eng.last_timing()
    return [s.tolist() for s, _ in res], dict(wall_ms=wall, kernel_ms=ms, launches=nl)


def summarize(runs, removals, graphs):
    out = {k: statistics.median(r[k] for r in runs) for k in ("wall_ms", "kernel_ms", "launches")}
    out["reps"] = len(runs)
    out["wall_ms_all"] = [round(r["wall_ms"], 4) for r in runs]
    out["wall_ms_per_rollout"] = out["wall_ms"] / graphs
    out["kernel_ms_per_rollout"] = out["kernel_ms"] / graphs
    out["wall_us_per_removal"] = 1e3 * out["wall_ms"] / max(1, removals)
    out["kernel_us_per_removal"] = 1e3 * out["kernel_ms"] / max(1, removals)
    return out


def compare(eng, graphs, reps, host_reps):
    out = {}
    for kind, comb in POLICIES:
        dev, host = [], []
        seq_d = seq_h = None
        device_call(eng, graphs, kind, comb)  # warm-up
        for r in range(reps):
            if r < host_reps:
                seq_h, t = host_loop(eng, graphs, kind, comb)
                host.append(t)
            seq_d, t = device_call(eng, graphs, kind, comb)
            dev.append(t)
        rem = sum(len(s) for s in seq_d)
        row = dict(graphs=len(graphs), removals=rem, device=summarize(dev, rem, len(graphs)))
        if host:
            assert seq_h == seq_d, "host loop and device rollout differ"
            row["host_loop"] = summarize(host, rem, len(graphs))
            row["wall_speedup"] = row["host_loop"]["wall_ms"] / row["device"]["wall_ms"]
            row["kernel_speedup"] = row["host_loop"]["kernel_ms"] / row["device"]["kernel_ms"]
        out[f"{kind}_{comb}"] = row
        print(kind, comb, json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-graphs", type=int, default=256)
    ap.add_argument("--batch-host-reps", type=int, default=1)
    ap.add_argument("--hbm-n", type=int, default=18000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heuristic_bench.json"))
    a = ap.parse_args()
    eng = _lib.Engine(np.zeros(_lib.MD_WEIGHT_FLOATS, np.float32))
    res = {"library": _lib.load_library().md_version().decode(),
           "host_loop": "md_reset, then per removal md_get_state of every running graph, the pick in numpy, one md_step",
           "device": "md_reset_deferred + md_heuristic_rollout"}
    with np.load(os.path.join(ROOT, "tests", "golden", "rollout_gmm1000_s0.npz")) as z:
        single = (int(z["n_nodes"]), z["edges0"].astype(np.int32), z["edges1"].astype(np.int32))
    res["single_gmm1000_s0"] = compare(eng, [single], a.reps, a.reps)
    # the oracle restatement (networkx) on the same host
    import heur_oracle
    from oracle import refenv
    orc = {}
    for kind, comb in POLICIES:
        t0 = time.perf_counter()
        seq = heur_oracle.rollout(refenv.RefGraph(*single), kind, comb)[0]
        orc[f"{kind}_{comb}"] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, removals=len(seq))
    res["oracle_restatement_gmm1000_s0"] = orc
    print("oracle", json.dumps(orc), flush=True)
    if a.batch_graphs > 0:
        from mdcommunity_amd import gmm_gpu
        pairs = gmm_gpu.gmm_pairs(1000, list(range(a.batch_graphs)), exact=True, device=0)
        batch = [(1000, e0, e1) for e0, e1 in pairs]
        res[f"batch_{a.batch_graphs}_gmm1000"] = compare(eng, batch, max(2, a.reps // 2), a.batch_host_reps)
    if a.hbm_n > 0:
        lay = synth.real_like_layers(n=a.hbm_n, seed=0)
        es = [np.array(sorted({(min(u, v), max(u, v)) for u, v in l if u != v}), np.int32) for l in lay]
        g = (a.hbm_n, es[0], es[1])
        assert not _lib.heuristic_fits_lds(a.hbm_n, len(es[0]) + len(es[1]))
        res[f"hbm_real_like_{a.hbm_n}"] = compare(eng, [g], 2, 0)
    eng.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
