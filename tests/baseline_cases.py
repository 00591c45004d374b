"""The graphs of the baseline-heuristic goldens (tests/golden/baselines_*.npz), shared by their
generator (tests/golden/make_golden_baselines.py) and the tests.  Pure numpy: no GPU, no
reference import."""
import os

import numpy as np

from edge_graphs import cases as edge_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATA = os.path.join(GOLDEN, "baseline_data")
ROLLOUT_CASES = ("er100", "gmm200_s7", "gmm1000_s0")
# (case, file stem, N, layers): the multiplex files read with the agents' reader.  The last two
# carry dataset names of the reference scripts' own lists, so the scripts' __main__ can run on them.
FILE_CASES = (("synth_multiplex", "synth_multiplex", 60, (1, 3)),
              ("file_usair_12", "us_air_transportation_american_delta_multiplex", 84, (1, 2)),
              ("file_droso_34", "drosophila_melanogaster_multiplex", 625, (3, 4)))
POLICIES = (("hda", "max"), ("ci", "max"), ("hda", "add"), ("ci", "add"))


def file_path(stem):
    p = os.path.join(GOLDEN, stem + ".edges")
    return p if os.path.exists(p) else os.path.join(DATA, stem + ".edges")


def read_layers(path, n, layers):
    from mdcommunity_amd.agent import MultiDismantler
    _, gl = MultiDismantler.read_multiplex(None, path, n)
    return gl[layers[0] - 1], gl[layers[1] - 1]


def graphs(names=None):
    """{case: (n, edges0, edges1)} in a fixed order."""
    out = {}
    for name in ROLLOUT_CASES:
        if names is not None and name not in names:
            continue
        with np.load(os.path.join(GOLDEN, f"rollout_{name}.npz")) as z:
            out[name] = (int(z["n_nodes"]), z["edges0"].astype(np.int32), z["edges1"].astype(np.int32))
    for name, stem, n, layers in FILE_CASES:
        if names is not None and name not in names:
            continue
        e0, e1 = read_layers(file_path(stem), n, layers)
        out[name] = (n, e0, e1)
    for name, n, e0, e1 in edge_cases():
        if names is not None and "edge_" + name not in names:
            continue
        out["edge_" + name] = (n, e0, e1)
    return out


def load_golden(case):
    with np.load(os.path.join(GOLDEN, f"baselines_{case}.npz")) as z:
        return {k: z[k] for k in z.files}
