"""Host side of the community-enhanced model: the boundary prior, its cache, the weight blob,
the model checks and the CLI variant (no GPU)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from mdcommunity_amd import _lib, cli, community, engine

CE_WEIGHTS = os.path.join(GOLDEN, "ce_g0-1_10w_iter30000.npz")
FIXTURES = ["ce_er40_zero", "ce_er40_boundary", "ce_er100_zero", "ce_er100_boundary", "ce_gmm200_s7_boundary",
            "ce_synth60_boundary"]


@pytest.mark.parametrize("name", FIXTURES)
def test_boundary_prior_matches_reference(name):
    """boundary_prior on the recorded partition = the reference's boundary flags
    (CE/dataset.py participation_and_boundary; the zero-prior fixtures record the partition too)."""
    z = load_golden(name)
    n = int(z["n_nodes"])
    for l in range(2):
        got = community.boundary_prior(n, z[f"edges{l}"], z[f"labels{l}"])
        assert got.dtype == np.float32 and set(np.unique(got)) <= {0.0, 1.0}
        if name.endswith("_boundary"):
            assert np.array_equal(got, z[f"prior{l}"])
        else:
            assert not z[f"prior{l}"].any()
            assert np.array_equal(got, load_golden(name.replace("_zero", "_boundary"))[f"prior{l}"])


def test_boundary_prior_partial_partition_and_isolated_nodes():
    """Nodes absent from the partition count as community 0; isolated nodes get 0."""
    with np.load(os.path.join(GOLDEN, "ce_prior_cases.npz")) as z:
        n, edges, lab, ref = int(z["partial_n"]), z["partial_edges"], z["partial_labels"], z["partial_boundary"]
    assert (lab < 0).sum() == 12
    deg = np.bincount(edges.reshape(-1), minlength=n)
    assert (deg == 0).sum() >= 3
    got = community.boundary_prior(n, edges, lab)
    assert np.array_equal(got, ref)
    assert not got[deg == 0].any()
    as_dict = {int(v): int(c) for v, c in enumerate(lab) if c >= 0}
    assert np.array_equal(community.boundary_prior(n, edges, as_dict), ref)
    assert ref.any() and not ref.all()


def test_cache_round_trip_reference_layout(tmp_path):
    z = load_golden("ce_synth60_boundary")
    priors = [z["prior0"], z["prior1"]]
    path = community.cache_path(str(tmp_path), "synth_multiplex.edges_layers12")
    assert os.path.basename(path) == "comm_prior_synth_multiplex.edges_layers12_boundary.npz"
    community.save_cache(path, priors)
    ref_path = os.path.join(GOLDEN, os.path.basename(path))  # written in the reference's format
    with np.load(path) as a, np.load(ref_path) as b:
        assert sorted(a.files) == sorted(b.files) == ["boundary", "feat0", "feat1", "n"]
        for k in a.files:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    got = community.load_cache(ref_path, 60)
    assert np.array_equal(got[0], priors[0]) and np.array_equal(got[1], priors[1])
    assert community.load_cache(ref_path, 61) is None
    assert community.load_cache(str(tmp_path / "missing.npz"), 60) is None


def test_attach_prior_order_cache_then_partition_then_zeros(tmp_path):
    from mdcommunity_amd import graph
    z = load_golden("ce_synth60_boundary")
    g = graph.Graph_test.from_edges(60, z["edges0"], z["edges1"])
    pr = community.attach_prior(g, GOLDEN, "synth_multiplex.edges_layers12")
    assert np.array_equal(pr[0], z["prior0"]) and np.array_equal(g.node_comm_feat[1], z["prior1"])
    assert g.boundary_nodes == set(np.where((z["prior0"] + z["prior1"]) > 0.5)[0].tolist())
    try:
        import community as louvain  # python-louvain
        has_louvain = hasattr(louvain, "best_partition")
    except Exception:
        has_louvain = False
    if not has_louvain:  # no partition: zeros, the reference's fallback, and no cache file
        g2 = graph.Graph_test.from_edges(60, z["edges0"], z["edges1"])
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (the one-time "python-louvain is not installed" warning)
            pr2 = community.attach_prior(g2, str(tmp_path), "other_layers12")
        assert not pr2[0].any() and not pr2[1].any() and not os.listdir(tmp_path)


def test_participation_prior_rejected_before_any_device_call():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"device call {name}")

    eng = object.__new__(_lib.Engine)
    eng.lib, eng.h, eng.model = NoDevice(), None, _lib.MD_MODEL_COMMUNITY
    eng.n_nodes = np.asarray([4], np.int32)
    with pytest.raises(ValueError, match="participation"):
        eng.set_node_prior([(np.asarray([0, 1, 0.5, 0], np.float32), np.zeros(4, np.float32))])
    with pytest.raises(ValueError, match="prior values"):
        eng.set_node_prior([(np.zeros(3, np.float32), np.zeros(4, np.float32))])
    eng.model = _lib.MD_MODEL_BASE
    with pytest.raises(_lib.MDError, match="MD_ESTATE"):
        eng.set_node_prior([(np.zeros(4, np.float32), np.zeros(4, np.float32))])


def test_pack_weights_community_and_base():
    sd = engine.load_state(CE_WEIGHTS)
    assert sd["w_n2l"].shape == (3, 64) and sd["h2_weight" if "h2_weight" in sd else "last_w"].size == 36
    w = _lib.pack_weights(sd)
    assert w.size == _lib.MD_WEIGHT_FLOATS_COMMUNITY == 31269 and w.dtype == np.float32
    assert np.array_equal(w[:192].reshape(3, 64), sd["w_n2l"])
    assert np.array_equal(w[192:192 + 4096].reshape(64, 64), sd["p_node_conv"])
    for f in (engine.DEFAULT_UNIT, engine.DEFAULT_UNIT_REAL, engine.DEFAULT_DEGREE):
        assert engine.load_weights(f).size == _lib.MD_WEIGHT_FLOATS == 31205
    bad = dict(sd, h2_weight=np.zeros((37, 1), np.float32), last_w=np.zeros((37, 1), np.float32))
    with pytest.raises(ValueError, match="unsupported"):
        _lib.pack_weights(bad)


def test_resolve_model_refuses_the_other_model():
    with pytest.raises(ValueError, match="community-enhanced checkpoint"):
        engine.resolve_model(CE_WEIGHTS, _lib.MD_COST_UNIT, _lib.MD_MODEL_BASE)
    with pytest.raises(ValueError, match="base-model checkpoint"):
        engine.resolve_model(engine.DEFAULT_UNIT, _lib.MD_COST_UNIT, _lib.MD_MODEL_COMMUNITY)
    assert engine.resolve_model(CE_WEIGHTS, _lib.MD_COST_UNIT, _lib.MD_MODEL_COMMUNITY) == CE_WEIGHTS
    assert engine.resolve_model(engine.DEFAULT_UNIT, _lib.MD_COST_UNIT, _lib.MD_MODEL_BASE) == engine.DEFAULT_UNIT
    with pytest.raises(FileNotFoundError, match="no community-enhanced checkpoint is shipped"):
        engine.resolve_model(None, _lib.MD_COST_UNIT, _lib.MD_MODEL_COMMUNITY)
    assert engine.load_weights(CE_WEIGHTS, model=_lib.MD_MODEL_COMMUNITY).size == 31269


def test_cli_community_variant(capsys):
    assert cli.main(["community", "train", "-o", "x"]) == 2
    assert cli.main(["community", "drawLmcc", "-o", "x"]) == 2
    assert cli.main(["unit", "train", "-o", "x"]) == 2
    capsys.readouterr()
    if not os.path.exists(cli.COMMUNITY_MODEL):  # no shipped checkpoint: --model is required
        with pytest.raises(SystemExit) as ex:
            cli.main(["community", "testReal", "-o", "x"])
        assert ex.value.code == 2
        assert "--model is required" in capsys.readouterr().err
    assert cli.COMMUNITY_REAL == [("fao_trade_multiplex", 214, (3, 24)), ("celegans_connectome_multiplex", 279, (2, 3)),
                                  ("fb-tw", 1043, (1, 2))]


def test_meta_ce_matches_fixtures():
    with open(os.path.join(GOLDEN, "meta_ce.json")) as f:
        meta = json.load(f)["graphs"]
    assert sorted(meta) == sorted(FIXTURES)
    for name in FIXTURES:
        z = load_golden(name)
        assert meta[name]["removals"] == len(z["seq"]) and meta[name]["audc"] == float(z["score"])
    assert meta["ce_er100_zero"]["removals"] == 18 and meta["ce_er100_boundary"]["removals"] == 24
