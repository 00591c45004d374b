"""The community-model checker (tests/ce_oracle.py) against the reference's own CE rollouts
(tests/golden/make_golden_ce.py), as tests/test_oracle.py pins the base oracle."""
import os

import numpy as np
import pytest
import torch

import ce_oracle
from conftest import GOLDEN, load_golden
from oracle import refenv, refmodel

MASK = refenv.MASK
FIXTURES = ["ce_er40_zero", "ce_er40_boundary", "ce_er100_zero", "ce_er100_boundary", "ce_gmm200_s7_boundary",
            "ce_synth60_boundary"]


@pytest.fixture(scope="module")
def weights():
    torch.set_num_threads(16)
    return refmodel.RefWeights.load(os.path.join(GOLDEN, "ce_g0-1_10w_iter30000.npz"))


@pytest.mark.parametrize("name", FIXTURES)
def test_ce_oracle_matches_reference(weights, name):
    """Teacher-forced along the reference's sequence: every masked Q row bit-identical on the
    build host (1e-6 elsewhere), LMCC trace, AUDC and maxcc equal; the free-running rollout
    equal where the reference has no exact tie."""
    z = load_golden(name)
    n = int(z["n_nodes"])
    g = refenv.RefGraph(n, z["edges0"], z["edges1"])
    assert g.max_rank == int(z["max_rank"])
    prior = [z["prior0"], z["prior1"]]
    rows = {}
    score, seq, ranks, maxcc = ce_oracle.rollout(weights, g, prior, forced=z["seq"].tolist(),
                                                 on_predict=lambda t, q, env: rows.__setitem__(t, q))
    assert seq == z["seq"].tolist() and ranks == z["ranks"].tolist()
    assert score == float(z["score"])  # AUDC, bit-exact float64
    assert np.array_equal(np.asarray(maxcc), z["maxcc"])
    assert len(rows) == len(z["q_rows"])
    for t, ref in enumerate(z["q_rows"]):
        assert np.array_equal(rows[t] == MASK, ref == MASK), t
        assert np.max(np.abs(rows[t] - ref)) <= 1e-6, t
    if not np.any(z["step_gap"] == 0.0):
        _, seq2, ranks2, _ = ce_oracle.rollout(weights, g, prior)
        assert seq2 == z["seq"].tolist() and ranks2 == z["ranks"].tolist()


def test_zero_prior_is_the_base_forward(weights):
    """With c = 0 the third row of w_n2l adds nothing: the forward equals the base oracle's on
    the same weights without that row."""
    z = load_golden("ce_er100_zero")
    g = refenv.RefGraph(int(z["n_nodes"]), z["edges0"], z["edges1"])
    base = refmodel.RefWeights.load(os.path.join(GOLDEN, "ce_g0-1_10w_iter30000.npz"))
    base.w_n2l = torch.nn.Parameter(base.w_n2l.detach()[:2].clone())
    zero = [np.zeros(g.num_nodes, np.float32)] * 2
    q_ce = ce_oracle.predict(weights, g, set(), refenv.RefEnv(g).removed, zero)
    q_b = refenv.predict(base, g, set(), refenv.RefEnv(g).removed)
    assert np.array_equal(q_ce == MASK, q_b == MASK)
    assert np.max(np.abs(q_ce - q_b)) <= 1e-6
