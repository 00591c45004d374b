"""The graphs of the centrality-baseline goldens (tests/golden/centrality_*.npz), shared by their
generator (tests/golden/make_golden_centrality.py) and the tests.  Pure numpy: no GPU, no
reference import."""
import os

import numpy as np

import baseline_cases

GOLDEN = baseline_cases.GOLDEN
# every case has n <= 130: the restatement and networkx run an all-pairs BFS per state
CASES = ("er100", "synth_multiplex", "file_usair_12", "edge_k2", "edge_path_triangle", "edge_shared_hub_star",
         "edge_isolated_nodes", "edge_wave_63", "edge_wave_65", "edge_tree_vs_dense", "edge_layer1_empty")
POLICIES = (("betweenness", "max"), ("betweenness", "add"), ("closeness", "max"), ("closeness", "add"))
# the multiplex file whose two result files are kept as text (baseline_cases.FILE_CASES[1])
TEXT_CASE = "file_usair_12"
TEXT_METHODS = (("hba", "betweenness", "HBA"), ("hca", "closeness", "HCA"))


def graphs():
    """{case: (n, edges0, edges1)} in CASES order."""
    got = baseline_cases.graphs(set(CASES))
    return {c: got[c] for c in CASES}


def load_golden(case):
    with np.load(os.path.join(GOLDEN, f"centrality_{case}.npz")) as z:
        return {k: z[k] for k in z.files}


def text_name(result_dir, prefix):
    _, stem, _, layers = baseline_cases.FILE_CASES[1]
    return "centrality_%s_%s%s_%s%s_1.txt" % (result_dir, prefix, stem, layers[0], layers[1])
