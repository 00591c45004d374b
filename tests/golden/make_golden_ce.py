#!/usr/bin/env python3
"""Golden fixtures of the community-enhanced model, by running the REFERENCE's CE code here.

Runs only in the build container.  ``code/CEMultiDismantler`` ("CE/") is imported unmodified
with the three shims of ``make_golden.py`` (torch_sparse stand-in, ``Tensor.cuda`` no-op,
``np.mat``) plus one more:

4. ``agent._attach_static_comm_prior`` is replaced by an assignment of a prior computed by this
   script.  ``python-louvain`` is not installed (CE/dataset.py then raises, and the agent falls
   back to an all-zero prior), so the partition of each layer comes from
   ``networkx.community.louvain_communities(g, seed=0)``; the prior itself is the reference's
   own ``dataset.participation_and_boundary`` on that partition (its boundary flags:
   ``COMM_PRIOR_FEATURE = "boundary"``, CE/MultiDismantler_torch.py:45).

Inference is not pruned (``ACTION_PRUNING_TEST = False``), so GetSol / GetSolution are the base
loop.  Records, per fixture, what ``make_golden.py`` records (sequence, ranks, score, maxcc and
every masked Q row, ``q_all``) plus the two prior arrays and the partition labels.

Usage: ``python tests/golden/make_golden_ce.py``.
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import MASK, edges_of, er_pair, gmm_pair, install_shims, pack_rows  # noqa: E402

CE_DIR = "/root/reference/code/CEMultiDismantler"
CE_CKPT = "./models/g0-1_10w_TORCH-Model_GMM_30_50/nrange_30_50_iter_30000.ckpt"  # CE/testReal.py main()
WEIGHTS_NPZ = "ce_g0-1_10w_iter30000.npz"


def load_ce_reference():
    install_shims()
    sys.path.insert(0, CE_DIR)
    import MultiDismantler_torch as M  # noqa: E402  (chdirs to CE_DIR)
    import graph as G  # noqa: E402
    import GMM  # noqa: E402
    import dataset  # noqa: E402
    return M, G, GMM, dataset


class Recorder:
    """Every prediction's masked Q row (CE's PredictWithCurrentQNet takes apply_pruning=)."""

    def __init__(self, agent):
        self.q_rows = []
        orig = agent.PredictWithCurrentQNet

        def pred(g_list, covered, remove_edges, **kw):
            out = orig(g_list, covered, remove_edges, **kw)
            self.q_rows.append(np.asarray(out[0], dtype=np.float64).copy())
            return out

        agent.PredictWithCurrentQNet = pred

    def reset(self):
        self.q_rows = []


def louvain_labels(g_nx, n):
    import networkx as nx
    comms = nx.community.louvain_communities(g_nx, seed=0)
    lab = np.full(n, -1, dtype=np.int32)
    for i, c in enumerate(comms):
        for v in c:
            lab[int(v)] = i
    return lab


def boundary_from_labels(dataset, g_nx, lab, n):
    """The reference's boundary flags (CE/dataset.py participation_and_boundary) of a partition
    given as labels (-1: the node is absent from the partition dict)."""
    part = {int(v): int(c) for v, c in enumerate(lab) if c >= 0}
    _, boundary = dataset.participation_and_boundary(g_nx, part, n)
    return np.asarray(boundary, dtype=np.float32)


def top2_gaps(q_rows):
    gaps = []
    for q in q_rows:
        lq = np.sort(q[q != MASK])[::-1]
        gaps.append(float(lq[0] - lq[1]) if lq.size > 1 else float("inf"))
    return gaps


def fixture(g, g1, g2, sol, score, env, rec, prior, labels, dt):
    ranks = [int(round(x * g.max_rank)) for x in env.MaxCCList[1:]]
    return dict(
        n_nodes=np.int32(g.num_nodes), edges0=edges_of(g1), edges1=edges_of(g2), max_rank=np.int32(g.max_rank),
        seq=np.asarray([int(a) for a in sol], dtype=np.int32), ranks=np.asarray(ranks, dtype=np.int32),
        score=np.float64(score), maxcc=np.asarray(env.MaxCCList, dtype=np.float64),
        q_all=pack_rows(rec.q_rows).reshape(len(rec.q_rows), g.num_nodes),
        step_gap=np.asarray(top2_gaps(rec.q_rows), dtype=np.float64),
        prior0=np.asarray(prior[0], dtype=np.float32), prior1=np.asarray(prior[1], dtype=np.float32),
        labels0=labels[0], labels1=labels[1], ref_seconds=np.float64(dt))


def meta_of(out):
    gaps = np.sort(out["step_gap"])
    return dict(removals=int(len(out["seq"])), audc=float(out["score"]), max_rank=int(out["max_rank"]),
                exact_ties=int(np.sum(gaps == 0.0)), smallest_gaps=[float(x) for x in gaps[:6]])


def main():
    import networkx as nx
    import torch
    M, G, GMM, dataset = load_ce_reference()
    assert M.ACTION_PRUNING_TEST is False and M.COMM_PRIOR_FEATURE == "boundary"
    agent = M.MultiDismantler()
    agent.LoadModel(CE_CKPT)
    sd = torch.load(os.path.join(CE_DIR, CE_CKPT), weights_only=True, map_location="cpu")
    arrays = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in sd.items()}
    assert arrays["w_n2l"].shape == (3, 64)
    np.savez_compressed(os.path.join(HERE, WEIGHTS_NPZ), **arrays)
    rec = Recorder(agent)
    pending = {}

    def attach(g, cache_id=None, **kw):  # shim 4
        g.node_comm_feat = [np.asarray(pending["prior"][l], dtype=np.float32) for l in range(2)]
        g.boundary_nodes = set(np.where((g.node_comm_feat[0] + g.node_comm_feat[1]) > 0.5)[0].tolist())

    agent._attach_static_comm_prior = attach
    meta = {"torch": torch.__version__, "numpy": np.__version__, "networkx": nx.__version__,
            "ckpt": "CE/" + CE_CKPT[2:], "partition": "networkx.community.louvain_communities(seed=0)", "graphs": {}}

    graphs = {"er40": (er_pair(40, 3, 4), ("zero", "boundary")),
              "er100": (er_pair(100, 1, 2), ("zero", "boundary")),
              "gmm200_s7": (gmm_pair(GMM, 200, 7), ("boundary",))}
    prior_cases = {}
    for name, ((a1, a2), kinds) in graphs.items():
        g1, g2 = nx.from_numpy_array(a1), nx.from_numpy_array(a2)
        n = a1.shape[0]
        labels = [louvain_labels(g1, n), louvain_labels(g2, n)]
        bnd = [boundary_from_labels(dataset, g1, labels[0], n), boundary_from_labels(dataset, g2, labels[1], n)]
        for kind in kinds:
            prior = bnd if kind == "boundary" else [np.zeros(n, np.float32), np.zeros(n, np.float32)]
            pending["prior"] = prior
            g = G.Graph_test(g1, g2)
            agent._attach_static_comm_prior(g)
            agent.InsertGraph(g, is_test=True)
            rec.reset()
            t0 = time.time()
            score, sol, _ = agent.GetSol(0)
            out = fixture(g, g1, g2, sol, score, agent.test_env, rec, prior, labels, time.time() - t0)
            agent.ClearTestGraphs()
            key = f"ce_{name}_{kind}"
            np.savez_compressed(os.path.join(HERE, f"rollout_{key}.npz"), **out)
            meta["graphs"][key] = meta_of(out)
            print(key, meta["graphs"][key], flush=True)

    # boundary flags on a partition that omits nodes, of a graph with isolated nodes (the
    # reference counts absent nodes as community 0)
    rng = np.random.default_rng(20261019)
    gi = nx.erdos_renyi_graph(50, 0.05, seed=9)
    gi.remove_edges_from(list(gi.edges(0)) + list(gi.edges(17)) + list(gi.edges(49)))
    lab = louvain_labels(gi, 50)
    lab[rng.choice(50, size=12, replace=False)] = -1
    prior_cases.update(partial_n=np.int32(50), partial_edges=edges_of(gi), partial_labels=lab,
                       partial_boundary=boundary_from_labels(dataset, gi, lab, 50))
    np.savez_compressed(os.path.join(HERE, "ce_prior_cases.npz"), **prior_cases)

    # testReal end-to-end on the committed multiplex file, layers (1, 2)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "r")
        real_dir = os.path.join(root, "data", "real")
        os.makedirs(real_dir)
        with open(os.path.join(HERE, "synth_multiplex.edges")) as f:
            txt = f.read()
        with open(os.path.join(real_dir, "synth_multiplex.edges"), "w") as f:
            f.write(txt)
        work = os.path.join(root, "a", "b")
        os.makedirs(work)
        save = os.path.join(tmp, "out")
        os.makedirs(save)
        here = os.getcwd()
        os.chdir(work)
        _, layers = agent.read_multiplex("../../data/real/synth_multiplex.edges", 60)
        g1, g2 = layers[0], layers[1]
        labels = [louvain_labels(g1, 60), louvain_labels(g2, 60)]
        prior = [boundary_from_labels(dataset, g1, labels[0], 60), boundary_from_labels(dataset, g2, labels[1], 60)]
        pending["prior"] = prior
        rec.reset()
        t0 = time.time()
        sol, _, score = agent.EvaluateRealData(None, "synth_multiplex.edges", save, 0, 60, (1, 2))
        dt = time.time() - t0
        env = agent.test_env
        g = G.Graph_test(g1, g2)
        out = fixture(g, g1, g2, sol, score, env, rec, prior, labels, dt)
        os.chdir(here)
        np.savez_compressed(os.path.join(HERE, "rollout_ce_synth60_boundary.npz"), **out)
        meta["graphs"]["ce_synth60_boundary"] = dict(meta_of(out), layers=[1, 2], N=60)
        print("ce_synth60_boundary", meta["graphs"]["ce_synth60_boundary"], flush=True)
        sub = os.path.join(save, "StepRatio_0.0000")
        for fn in sorted(os.listdir(sub)):
            with open(os.path.join(sub, fn)) as f:
                txt = f.read()
            with open(os.path.join(HERE, "ce_testreal_" + fn), "w") as f:
                f.write(txt)
        # the prior cache in the reference's format (CE/MultiDismantler_torch.py:224-231)
        union = sorted(set(np.where(prior[0] > 0.5)[0].tolist()) | set(np.where(prior[1] > 0.5)[0].tolist()))
        np.savez_compressed(os.path.join(HERE, "comm_prior_synth_multiplex.edges_layers12_boundary.npz"),
                            n=np.int64(60), feat0=prior[0], feat1=prior[1], boundary=np.asarray(union, dtype=np.int64))

    with open(os.path.join(HERE, "meta_ce.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
