"""GPU tests of the community-enhanced model (md_create_model(MD_MODEL_COMMUNITY),
md_set_node_prior) against the reference's own CE rollouts (tests/golden/make_golden_ce.py)
and the CPU checker tests/ce_oracle.py.  Bars: Q within 1e-5 of the reference at every
prediction; sequences equal to the reference's up to the first step where the reference is
ambiguous (exact tie or top-2 gap <= CERT_MARGIN) and certified beyond it, LMCC and AUDC exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ce_oracle
import edge_graphs
from conftest import GOLDEN, load_golden
from test_certificates import CERT_MARGIN
from mdcommunity_amd import _lib, engine
from oracle import refenv, refmodel

pytestmark = pytest.mark.gpu

Q_TOL = 1e-5
MASK = refenv.MASK
CE_WEIGHTS = os.path.join(GOLDEN, "ce_g0-1_10w_iter30000.npz")
COMM = _lib.MD_MODEL_COMMUNITY


@pytest.fixture(scope="module")
def blob():
    return engine.load_weights(CE_WEIGHTS, model=COMM)


@pytest.fixture(scope="module")
def ref_weights():
    torch.set_num_threads(16)
    return refmodel.RefWeights.load(CE_WEIGHTS)


@pytest.fixture(scope="module")
def eng(blob):
    e = _lib.Engine(blob)
    assert e.model == COMM
    yield e
    e.close()


def audc(ranks, max_rank, n):
    s = 0.0
    for r in ranks:
        s += -1 * (-float(r) / (max_rank * float(n)))  # U/mvc_env.py:86,133-137
    return s


def fixture(name):
    z = load_golden(name)
    return z, (int(z["n_nodes"]), z["edges0"], z["edges1"]), [z["prior0"], z["prior1"]]


def run(e, g, prior, step=1):
    e.load_graphs([g])
    e.set_node_prior([prior])
    mr = int(e.reset()[0])
    seq, ranks = e.rollout(step=step)[0]
    return mr, seq.tolist(), ranks.tolist()


def certify(ref_weights, g, prior, mr, seq, ranks, step=1):
    """The project's rule past an ambiguous step: ce_oracle teacher-forced along the GPU's
    sequence; the i-th pick of every prediction within CERT_MARGIN of the oracle's i-th best Q,
    LMCC trace and AUDC equal to the oracle's along that sequence."""
    rg = refenv.RefGraph(*g)
    assert rg.max_rank == mr
    rows = []
    score, seq_o, ranks_o, _ = ce_oracle.rollout(ref_weights, rg, prior, step=step, forced=seq,
                                                 on_predict=lambda t, q, env: rows.append(q))
    assert seq_o == seq and ranks_o == ranks
    assert audc(ranks, mr, g[0]) == score
    for t, q in enumerate(rows):
        best = np.sort(q)[::-1]
        for i, a in enumerate(seq[t * step:(t + 1) * step]):
            assert q[a] != MASK and q[a] >= best[i] - CERT_MARGIN, (t, i, a, q[a], best[i])


def check_against(ref_weights, g, prior, mr, seq, ranks, ref_seq, ref_ranks, ref_score, ref_max_rank, gaps, step=1):
    """Identical to the reference up to its first ambiguous prediction (gaps[t] <= CERT_MARGIN:
    an exact tie or a near-tie of the picks); identical throughout when there is none."""
    assert mr == ref_max_rank
    amb = next((t for t, x in enumerate(gaps) if x <= CERT_MARGIN), None)
    if amb is None:
        assert seq == ref_seq and ranks == ref_ranks
        assert audc(ranks, mr, g[0]) == ref_score  # bit-exact float64
        return
    assert seq[:amb * step] == ref_seq[:amb * step] and ranks[:amb * step] == ref_ranks[:amb * step]
    certify(ref_weights, g, prior, mr, seq, ranks, step)


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ce_er40_zero", "ce_er40_boundary", "ce_er100_zero", "ce_er100_boundary",
                                  "ce_gmm200_s7_boundary"])
def test_q_rows_within_tolerance(eng, name):
    """Teacher-forced along the reference's sequence, Q within 1e-5 at every prediction."""
    z, g, prior = fixture(name)
    eng.load_graphs([g])
    eng.set_node_prior([prior])
    assert int(eng.reset()[0]) == int(z["max_rank"])
    worst = 0.0
    for t, ref in enumerate(z["q_rows"]):
        q, _, _, _ = eng.predict()
        live = ref != MASK
        assert np.array_equal(np.isfinite(q), live), t
        worst = max(worst, float(np.max(np.abs(q[live].astype(np.float64) - ref[live]))))
        lm, _ = eng.step(np.array([z["seq"][t]], np.int32))
        assert int(lm[0]) == int(z["ranks"][t])
    print(name, "max |dQ|", worst)
    assert worst < Q_TOL, worst


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ce_er40_zero", "ce_er40_boundary"])
def test_rollout_identical_er40(eng, name):
    """Smallest top-2 gap 1.9e-4 / 7.6e-4 (19x the Q bound): no certificate needed."""
    z, g, prior = fixture(name)
    assert float(np.min(z["step_gap"])) > 19 * Q_TOL
    mr, seq, ranks = run(eng, g, prior)
    assert mr == int(z["max_rank"])
    assert seq == z["seq"].tolist() and ranks == z["ranks"].tolist()
    assert audc(ranks, mr, g[0]) == float(z["score"])


@pytest.mark.parametrize("name", ["ce_er100_zero", "ce_er100_boundary", "ce_gmm200_s7_boundary", "ce_synth60_boundary"])
def test_rollout_certified(eng, ref_weights, name):
    z, g, prior = fixture(name)
    mr, seq, ranks = run(eng, g, prior)
    check_against(ref_weights, g, prior, mr, seq, ranks, z["seq"].tolist(), z["ranks"].tolist(), float(z["score"]),
                  int(z["max_rank"]), z["step_gap"].tolist())


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ce_er100_zero", "ce_gmm200_s7_boundary"])
def test_zero_prior_equals_base_model(eng, blob, name):
    """A community context with an all-zero prior computes what a base context holding the same
    blob without w_n2l's third row computes: equal Q rows (==) along the rollout, same rollout."""
    _, g, _ = fixture(name)
    zero = [np.zeros(g[0], np.float32)] * 2
    base = _lib.Engine(np.concatenate([blob[:128], blob[192:]]))
    try:
        assert base.model == _lib.MD_MODEL_BASE
        base.load_graphs([g])
        out_c = run(eng, g, zero)
        assert (int(base.reset()[0]),) + tuple(x.tolist() for x in base.rollout()[0]) == out_c
        eng.reset()
        base.reset()
        for a in out_c[1]:
            qc, qb = eng.predict()[0], base.predict()[0]
            assert np.array_equal(qc, qb)
            act = np.array([a], np.int32)
            assert eng.step(act)[0].tolist() == base.step(act)[0].tolist()
    finally:
        base.close()


# 4 ---------------------------------------------------------------------------------------------
def test_prior_matters(eng):
    zz, g, zero = fixture("ce_er40_zero")
    zb, _, bnd = fixture("ce_er40_boundary")
    assert zz["seq"].tolist() != zb["seq"].tolist()
    s_zero, s_bnd = run(eng, g, zero)[1], run(eng, g, bnd)[1]
    assert s_zero == zz["seq"].tolist() and s_bnd == zb["seq"].tolist() and s_zero != s_bnd
    # md_set_node_prior between two predictions: no state touched, the next Q changes
    eng.set_node_prior([zero])
    eng.reset()
    q0 = eng.predict()[0]
    state0 = eng.get_state(0)
    eng.set_node_prior([bnd])
    state1 = eng.get_state(0)
    assert all(np.array_equal(a, b) for a, b in zip(state0, state1))
    q1 = eng.predict()[0]
    assert np.array_equal(np.isfinite(q0), np.isfinite(q1)) and not np.array_equal(q0, q1)
    eng.set_node_prior([zero])
    assert np.array_equal(eng.predict()[0], q0)


# 5 ---------------------------------------------------------------------------------------------
def _batch():
    rng = np.random.default_rng(515)
    graphs, priors = [], []
    for i in range(20):
        n = int(rng.integers(40, 65))
        graphs.append((n, edge_graphs.er_edges(rng, range(n), 4.0 / n), edge_graphs.er_edges(rng, range(n), 5.0 / n)))
        priors.append([rng.integers(0, 2, n).astype(np.float32), rng.integers(0, 2, n).astype(np.float32)])
    priors[7] = [np.ones(graphs[7][0], np.float32)] * 2
    return graphs, priors


def test_batch_equals_single(eng, blob, monkeypatch):
    """20 graphs (> 16: the wave-item and queue kernels) in one launch, each equal to its own
    single-graph rollout; also with workgroup items (MD_WQ=0) and in lock-step shared mode."""
    graphs, priors = _batch()
    single = []
    for g, pr in zip(graphs, priors):
        mr, seq, ranks = run(eng, g, pr)
        single.append((seq, ranks))
    assert sum(len(s) for s, _ in single) > 20

    def batch(e):
        e.load_graphs(graphs)
        e.set_node_prior(priors)
        e.reset()
        return [(s.tolist(), r.tolist()) for s, r in e.rollout()]

    assert batch(eng) == single
    for key, val in (("MD_WQ", "0"), ("MD_VARIANT", "32")):
        monkeypatch.setenv(key, val)
        e = _lib.Engine(blob)
        try:
            assert batch(e) == single, key
        finally:
            e.close()
        monkeypatch.delenv(key)


# 6 ---------------------------------------------------------------------------------------------
def test_fallback_tables(eng, blob, monkeypatch):
    """MD_H0G=0 (the per-graph 2 n-row tables rebuilt in phase A) gives the default rollouts, on
    er100 and on a graph whose hub reaches every other node in both layers: dmax = n - 1, and
    the hub's prior 1 reads the last of the 2 n rows."""
    _, g100, p100 = fixture("ce_er100_boundary")
    _, n, e0, e1 = next(c for c in edge_graphs.cases() if c[0] == "shared_hub_star")
    assert np.bincount(e0.reshape(-1))[0] == n - 1 and np.bincount(e1.reshape(-1))[0] == n - 1
    rng = np.random.default_rng(66)
    ph = [rng.integers(0, 2, n).astype(np.float32), rng.integers(0, 2, n).astype(np.float32)]
    ph[0][0] = ph[1][0] = 1.0
    cases = [(g100, p100), ((n, e0, e1), ph)]
    default = [run(eng, g, p) for g, p in cases]
    q_def = []
    for g, p in cases:
        eng.load_graphs([g])
        eng.set_node_prior([p])
        eng.reset()
        q_def.append(eng.predict()[0])
    monkeypatch.setenv("MD_H0G", "0")
    e = _lib.Engine(blob)
    try:
        for (g, p), d, q in zip(cases, default, q_def):
            assert run(e, g, p) == d
            e.reset()
            assert np.array_equal(e.predict()[0], q)
    finally:
        e.close()


# 7 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"MD_VARIANT": "64", "MD_ENV_MODE": "0"}, {"MD_VARIANT": "66", "MD_ENV_MODE": "0"},
                                 {"MD_DF": "0"}, {"MD_SPEC": "0"}, {"MD_VARIANT": "1"}],
                         ids=["grid_wide_env", "one_wg_env", "df0", "spec0", "no_prebuild"])
def test_execution_modes_same_rollout(eng, blob, monkeypatch, env):
    _, g, prior = fixture("ce_er100_boundary")
    default = run(eng, g, prior)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = _lib.Engine(blob)
    try:
        assert run(e, g, prior) == default
    finally:
        e.close()


# 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 63, 64, 65])
def test_k2_states_no_endgame_shortcut(eng, ref_weights, n):
    """A perfect matching shared by both layers (every state is a K2 state) with mixed priors:
    live nodes with different priors have different Q, so the end-game shortcut stays off (one
    forward pass per removal, the only host requests are exact ties), and the rollout is
    ce_oracle's."""
    rng = np.random.default_rng(800 + n)
    perm = rng.permutation(n)
    pairs = np.asarray([(perm[2 * i], perm[2 * i + 1]) for i in range(n // 2)], np.int32)
    g = (n, pairs, pairs[::-1].copy())
    prior = [rng.integers(0, 2, n).astype(np.float32), rng.integers(0, 2, n).astype(np.float32)]
    assert 0 < prior[0].sum() < n
    mr, seq, ranks = run(eng, g, prior)
    tr = eng.trace(0)
    assert len(tr["n_live"]) == len(seq) > 0          # a prediction per removal: no end-game answer
    assert eng.host_requests() == int(np.sum(tr["n_tie"] > 1))
    rows = []
    rg = refenv.RefGraph(*g)
    score, seq_o, ranks_o, _ = ce_oracle.rollout(ref_weights, rg, prior, on_predict=lambda t, q, env: rows.append(q))
    # numpy's argsort decides the exact ties from the whole row: the oracle's own sequence is
    # the GPU's when every pair of distinct live Q is further apart than twice the Q bound
    separated = all(np.min(np.diff(np.unique(q[q != MASK])), initial=1.0) > 2 * Q_TOL for q in rows)
    if separated:
        assert seq == seq_o and ranks == ranks_o and audc(ranks, mr, n) == score
    certify(ref_weights, g, prior, mr, seq, ranks)


# 9 ---------------------------------------------------------------------------------------------
def test_step_ratio(eng, ref_weights):
    _, g, prior = fixture("ce_er100_boundary")
    step = 3
    rows = []
    rg = refenv.RefGraph(*g)
    score, seq_o, ranks_o, _ = ce_oracle.rollout(ref_weights, rg, prior, step=step,
                                                 on_predict=lambda t, q, env: rows.append(q))
    gaps = []
    for q in rows:  # a prediction is ambiguous when any of its picks is within the margin of the next Q
        top = np.sort(q[q != MASK])[::-1][:step + 1]
        gaps.append(float(np.min(-np.diff(top))) if top.size > 1 else np.inf)
    mr, seq, ranks = run(eng, g, prior, step=step)
    check_against(ref_weights, g, prior, mr, seq, ranks, seq_o, ranks_o, score, rg.max_rank, gaps, step=step)


# 10 --------------------------------------------------------------------------------------------
def test_abi_cases(eng, blob):
    lib = _lib.load_library()
    f32p = ctypes.POINTER(ctypes.c_float)

    def create(w, cost, model):
        h = ctypes.c_void_p()
        st = lib.md_create_model(0, w.ctypes.data_as(f32p), w.size, cost, model, ctypes.byref(h))
        if h:
            lib.md_destroy(h)
        return st

    base_blob = np.ascontiguousarray(np.concatenate([blob[:128], blob[192:]]))
    assert create(base_blob, _lib.MD_COST_UNIT, COMM) == _lib.MD_EINVAL      # n_floats of the other model
    assert create(blob, _lib.MD_COST_UNIT, _lib.MD_MODEL_BASE) == _lib.MD_EINVAL
    assert create(blob, _lib.MD_COST_DEGREE, COMM) == _lib.MD_EINVAL         # no such variant
    assert create(blob, _lib.MD_COST_UNIT, 2) == _lib.MD_EINVAL
    assert create(blob, _lib.MD_COST_UNIT, COMM) == _lib.MD_OK
    assert create(base_blob, _lib.MD_COST_UNIT, _lib.MD_MODEL_BASE) == _lib.MD_OK
    with pytest.raises(_lib.MDError, match="MD_EINVAL"):
        eng.set_weights(base_blob)                                           # checked against the context's model

    _, g, bnd = fixture("ce_er40_boundary")
    n = g[0]
    eng.load_graphs([g])
    eng.reset()
    q_zero = eng.predict()[0]
    bad = np.zeros(2 * n, np.float32)
    bad[n + 3] = 0.5
    assert lib.md_set_node_prior(eng.h, bad.ctypes.data_as(f32p)) == _lib.MD_EINVAL
    assert b"participation-valued priors are not supported" in lib.md_last_error(eng.h)
    assert np.array_equal(eng.predict()[0], q_zero)                          # a refused prior changes nothing
    eng.set_node_prior([bnd])
    assert not np.array_equal(eng.predict()[0], q_zero)
    eng.load_graphs([g])                                                     # resets the prior to zeros
    eng.reset()
    assert np.array_equal(eng.predict()[0], q_zero)

    b = _lib.Engine(base_blob)
    try:
        b.load_graphs([g])
        ok = np.zeros(2 * n, np.float32)
        assert lib.md_set_node_prior(b.h, ok.ctypes.data_as(f32p)) == _lib.MD_ESTATE
        with pytest.raises(_lib.MDError, match="MD_ESTATE"):
            b.set_node_prior([bnd])
    finally:
        b.close()
    fresh = _lib.Engine(blob)
    try:
        ok = np.zeros(2 * n, np.float32)
        assert lib.md_set_node_prior(fresh.h, ok.ctypes.data_as(f32p)) == _lib.MD_ESTATE  # no graphs loaded
    finally:
        fresh.close()


# 11 --------------------------------------------------------------------------------------------
def test_dropin_evaluate_real_data(tmp_path):
    """agent_community's EvaluateRealData on the synthetic multiplex file, layers (1, 2), with
    the fixture prior cache: Soluion_* and NormalizedLMCC_* byte-identical to the reference's
    (its one exact tie goes through numpy's routine)."""
    from mdcommunity_amd import agent_community
    real = tmp_path / "data" / "real"
    real.mkdir(parents=True)
    (real / "synth_multiplex.edges").write_text(open(os.path.join(GOLDEN, "synth_multiplex.edges")).read())
    cache = tmp_path / "cache"
    cache.mkdir()
    name = "comm_prior_synth_multiplex.edges_layers12_boundary.npz"
    (cache / name).write_bytes(open(os.path.join(GOLDEN, name), "rb").read())
    out = tmp_path / "out"
    out.mkdir()
    agent = agent_community.MultiDismantler(cache_dir=str(cache))
    try:
        agent.LoadModel(CE_WEIGHTS)
        sol, _, score = agent.EvaluateRealData(None, "synth_multiplex.edges", str(out), 0, 60, (1, 2),
                                               data_root=str(tmp_path / "data"))
    finally:
        if agent._engine is not None:
            agent._engine.close()
    z = load_golden("ce_synth60_boundary")
    assert sol == z["seq"].tolist() and score == float(z["score"])
    sub = out / "StepRatio_0.0000"
    for fn in ("Soluion_synth_multiplex_12.txt", "NormalizedLMCC_synth_multiplex_12.txt"):
        assert (sub / fn).read_text() == open(os.path.join(GOLDEN, "ce_testreal_" + fn)).read(), fn
