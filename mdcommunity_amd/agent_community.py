"""The community-enhanced agent, inference path (drop-in for ``CEMultiDismantler/MultiDismantler_torch.py``).

The reference's CE model is the unit-cost network with a third node-input column, a static
per-node, per-layer community prior (``CE/MultiDismantler_net_graphsage.py:255-285``,
``CE/PrepareBatchGraph.py:140-148``); its inference loop is the base one
(``ACTION_PRUNING_TEST = False``).  This agent is :class:`mdcommunity_amd.agent.MultiDismantler`
on a community engine (``md_create_model(..., MD_MODEL_COMMUNITY)``): ``Evaluate`` and
``EvaluateRealData`` attach the prior the way the reference does (``_attach_static_comm_prior``:
the cache, then a Louvain partition, then zeros; ``cache_id = "<file>_layers<l0><l1>"``), and a
graph handed to ``InsertGraph`` keeps the ``node_comm_feat`` it carries.  Only the binary
boundary prior is supported.  No checkpoint is shipped: ``LoadModel`` needs an existing
CE ``.ckpt`` or converted ``.npz``.
"""
import os
import sys
import time

import numpy as np

from . import _lib, agent as _agent, community as _community, graph as _graph

CACHE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cache")


class MultiDismantler(_agent.MultiDismantler):
    cost_mode = _lib.MD_COST_UNIT
    model = _lib.MD_MODEL_COMMUNITY

    def __init__(self, device=0, cache_dir=None):
        super().__init__(device)
        self.cache_dir = cache_dir if cache_dir is not None else CACHE_DIR
        print("COMM_PRIOR_FEATURE: %s" % _community.FEATURE)  # CE/MultiDismantler_torch.py:136

    def _attach_static_comm_prior(self, g, cache_id=None):
        _community.attach_prior(g, self.cache_dir if cache_id else None, cache_id)

    def InsertGraph(self, g, is_test):  # noqa: N802
        if getattr(g, "node_comm_feat", None) is None:
            g.node_comm_feat = _community.zero_prior(g.num_nodes)
        super().InsertGraph(g, is_test)

    def _set_prior(self, eng, graphs):
        eng.set_node_prior([_community.graph_prior(g) for g in graphs])

    def PredictWithCurrentQNet(self, g_list, covered, remove_edges, apply_pruning=False):  # noqa: N802
        if apply_pruning:
            raise NotImplementedError("action pruning is training only (ACTION_PRUNING_TEST = False)")
        return super().PredictWithCurrentQNet(g_list, covered, remove_edges)

    def Evaluate(self, data_test, data_test_name, data_type, model_file=None, data_root="../../data"):  # noqa: N802
        """testSynthetic harness (CE/MultiDismantler_torch.py:719-757): the prior of each graph
        from a partition (no cache id), zeros without python-louvain."""
        print("The best model is :%s" % model_file)
        sys.stdout.flush()
        self.LoadModel(model_file)
        n_test = 2 if os.getenv("SMOKE_TEST", "0").strip().lower() in ("1", "true", "yes") else 20
        scores, times, costs = [], [], []
        for i in range(n_test):
            base = os.path.join(data_root, "synthetic", data_type, "syn_%s" % data_test_name)
            a1 = np.load(os.path.join(base, "adj1_%s.npy" % i))
            a2 = np.load(os.path.join(base, "adj2_%s.npy" % i))
            g = _graph.Graph_test.from_edges(a1.shape[0], np.argwhere(np.triu(a1) > 0), np.argwhere(np.triu(a2) > 0))
            self._attach_static_comm_prior(g)
            self.InsertGraph(g, is_test=True)
            t1 = time.time()
            val, sol, cost = self.GetSol(i)
            t2 = time.time()
            scores.append(val)
            times.append(t2 - t1)
            costs.append(cost)
        self.ClearTestGraphs()
        return np.mean(scores), np.std(scores), np.mean(times), np.std(times), np.mean(costs)

    def _real_graph(self, test_name, num_nodes, layers, data_root):
        _, gl = self.read_multiplex(os.path.join(data_root, "real", test_name), num_nodes)
        g = _graph.Graph_test.from_edges(num_nodes, gl[layers[0] - 1], gl[layers[1] - 1])
        self._attach_static_comm_prior(g, cache_id="%s_layers%s%s" % (test_name, layers[0], layers[1]))
        return g
