"""Device rollouts of the betweenness / closeness baselines (md_centrality_rollout,
md_centrality_scores) on the GPU.

The device is compared with the restatement (tests/cent_oracle.py) bit for bit: float64 scores
with ``==``, sequences and LMCC traces as lists.  The restatement is held to networkx on the CPU
(tests/test_centrality.py); the goldens carry the reference scripts' own MCC trace, MCCs list and
float64 score along its sequences.  Shapes are the smallest at which the kernels can go wrong;
identities cover the batch, the HBM-scratch variant of the search arrays, launch rounds, repeats
and start states; then the state the rollout leaves, the errors and the CLI."""
import os

import numpy as np
import pytest

import baseline_cases
import cent_oracle
import centrality_cases
from mdcommunity_amd import _lib, baselines_centrality
from oracle import refenv

pytestmark = pytest.mark.gpu

POLICIES = list(centrality_cases.POLICIES)
KINDS = list(cent_oracle.KINDS)
METHOD = {"betweenness": "hba", "closeness": "hca"}
ZERO_W = np.zeros(_lib.MD_WEIGHT_FLOATS, np.float32)


def _rand_edges(rng, lo, hi, m):
    e = set()
    while len(e) < m:
        u, v = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        if u != v:
            e.add((min(u, v), max(u, v)))
    e = sorted(e)
    rng.shuffle(e)
    return np.array(e, np.int32).reshape(-1, 2)


def shape_graphs():
    """The smallest shapes at which the kernels can go wrong."""
    rng = np.random.default_rng(11)
    k2 = np.array([[0, 1]], np.int32)
    out = {"k2": (2, k2, k2),
           "path_triangle": (3, np.array([[0, 1], [1, 2]], np.int32), np.array([[0, 1], [1, 2], [0, 2]], np.int32))}
    for n in (63, 64, 65):  # a wavefront edge
        out[f"n{n}"] = (n, _rand_edges(rng, 0, n, 2 * n), _rand_edges(rng, 0, n, 2 * n))
    for n in (511, 513):  # the workgroup's node chunking and a source-block boundary; sparse
        out[f"n{n}"] = (n, _rand_edges(rng, 0, n, n + n // 4), _rand_edges(rng, 0, n, n + n // 4))
    ring = np.array([(v, (v + 1) % 48) for v in range(48)], np.int32)
    out["ring"] = (48, ring, np.roll(ring, 5, axis=0).copy())  # every score equal, a deep search
    path = np.array([(v, v + 1) for v in range(299)], np.int32)
    out["path300"] = (300, path, path[::-1].copy())  # 299 levels
    lat = np.array([(16 * r + c, 16 * r + c + 1) for r in range(16) for c in range(15)] +
                   [(16 * r + c, 16 * (r + 1) + c) for r in range(15) for c in range(16)], np.int32)
    out["lattice"] = (256, lat, rng.permutation(lat).astype(np.int32))  # sigma up to ~1.5e8, many equal paths
    star = np.array([(0, v) for v in range(1, 100)], np.int32)
    out["shared_hub"] = (100, star, star[::-1].copy())  # dmax 99, every leaf 0
    c1 = np.concatenate([_rand_edges(rng, 0, 40, 70), _rand_edges(rng, 40, 90, 90)])
    c2 = np.concatenate([_rand_edges(rng, 0, 40, 65), _rand_edges(rng, 40, 90, 95)])
    out["two_clusters"] = (90, c1, c2)  # r < L
    out["isolated_low"] = (70, _rand_edges(rng, 10, 70, 150), _rand_edges(rng, 10, 70, 140))  # 0-9 count in L, score 0
    out["layer1_empty"] = (30, _rand_edges(rng, 0, 30, 60), np.zeros((0, 2), np.int32))
    return out


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(ZERO_W)
    yield e
    e.close()


@pytest.fixture(scope="module")
def shapes():
    return shape_graphs()


@pytest.fixture(scope="module")
def golden_graphs():
    return centrality_cases.graphs()


@pytest.fixture(scope="module")
def shape_scores(shapes):
    """The restatement's scores of every shape at s0 and after three removals (its own first
    betweenness-max picks, fewer when the graph is terminal before), computed once:
    {name: (actions, {(kind, state): (layer0, layer1)})}."""
    out = {}
    for name, g in shapes.items():
        env = refenv.RefEnv(refenv.RefGraph(*g))
        sc = {(k, 0): cent_oracle.dense_scores(env, k) for k in KINDS}
        acts = []
        while len(acts) < 3 and not env.terminal():
            a, _ = cent_oracle.pick_from(env, cent_oracle.combined(*cent_oracle.scores(env, "betweenness"), "max"))
            env.step(a)
            acts.append(a)
        sc.update({(k, 1): cent_oracle.dense_scores(env, k) for k in KINDS})
        out[name] = (acts, sc)
    return out


def _scores(e, kind):
    return [(a.tolist(), b.tolist()) for a, b in e.centrality_scores(kind)]


def _step_each(e, actions, k):
    """Removal k of every graph's own action list (-1: none left)."""
    e.step([a[k] if k < len(a) else -1 for a in actions])


def _check_scores(e, names, shape_scores, state):
    for kind in KINDS:
        got = _scores(e, kind)
        for s, (c0, c1) in zip(names, got):
            want = shape_scores[s][1][(kind, state)]
            assert c0 == want[0], (s, kind, state, 0)
            assert c1 == want[1], (s, kind, state, 1)


def _shape_score_run(e, shapes, shape_scores):
    names = list(shapes)
    e.load_graphs([shapes[s] for s in names])
    e.reset()
    _check_scores(e, names, shape_scores, 0)
    acts = [shape_scores[s][0] for s in names]
    for k in range(3):
        _step_each(e, acts, k)
    _check_scores(e, names, shape_scores, 1)
    return dict(zip(names, _scores(e, "betweenness")))


def test_scores_match_the_restatement(eng, shapes, shape_scores):
    got = _shape_score_run(eng, shapes, shape_scores)
    # (the state after three removals)
    assert all(x == 0.0 for x in got["isolated_low"][0][:10])
    assert got["layer1_empty"] == ([0.0] * 30, [0.0] * 30)
    eng.load_graphs([shapes["ring"], shapes["shared_hub"]])
    eng.reset()
    (r0, r1), (h0, _) = _scores(eng, "betweenness")
    assert len(set(r0)) == 1 and r0 == r1 and r0[0] > 0.0
    assert h0[0] > 0.0 and h0[1:] == [0.0] * 99
    (r0, _), _ = _scores(eng, "closeness")
    assert len(set(r0)) == 1 and r0[0] > 0.0


@pytest.mark.parametrize("env_name,value", [("MD_CENT_SCRATCH", "1"), ("MD_CENT_ROUND_BLOCKS", "3")])
def test_scores_of_the_scratch_variant_and_of_short_rounds(env_name, value, shapes, shape_scores, monkeypatch):
    """The search arrays in HBM scratch, and launch rounds of three source blocks (the running sum
    over rounds): the same bits."""
    monkeypatch.setenv(env_name, value)
    e = _lib.Engine(ZERO_W)
    try:
        _shape_score_run(e, shapes, shape_scores)
    finally:
        e.close()


def run(e, graphs, kind, comb, deferred=True):
    e.load_graphs(graphs)
    if deferred:
        e.reset_deferred()
    else:
        e.reset()
    return [(s.tolist(), r.tolist()) for s, r in e.centrality_rollout(kind, comb)]


@pytest.mark.parametrize("kind,comb", POLICIES)
def test_rollouts_reproduce_the_goldens(kind, comb, eng, golden_graphs):
    """Sequence and LMCC trace of the restatement (the scripts' MCC along it), MaxCCList and score
    equal to the scripts' float64 values, every golden case in one call."""
    names = list(golden_graphs)
    gs = [golden_graphs[c] for c in names]
    res = run(eng, gs, kind, comb)
    full = baselines_centrality.dismantle_batch(gs, METHOD[kind], comb, engine=eng)
    k = f"{kind}_{comb}"
    for c, (seq, lmcc), (sol, mccs, score) in zip(names, res, full):
        g = centrality_cases.load_golden(c)
        assert seq == g[k + "_seq"].tolist(), c
        assert lmcc == g[k + "_lmcc"].tolist(), c
        assert sol == seq
        assert [float(x) for x in mccs] == g[k + "_mccs"].tolist(), c
        assert score == float(g[k + "_score"]), c  # float64, exact
    got = dict(zip(names, res))
    # end-games where every score is 0: the smallest live id goes
    assert got["edge_k2"] == ([0], [1])
    if (kind, comb) == ("closeness", "max"):
        assert got["edge_path_triangle"] == ([0, 1], [2, 1])  # every closeness 1.0 in the triangle, then the K2 {1, 2}
    assert got["edge_layer1_empty"] == ([], [])


@pytest.fixture(scope="module")
def mixed(shapes, golden_graphs):
    rng = np.random.default_rng(5)
    extra = [(40, _rand_edges(rng, 0, 40, 80), _rand_edges(rng, 0, 40, 80)),
             (130, _rand_edges(rng, 0, 130, 200), _rand_edges(rng, 0, 130, 190))]
    out = list(shapes.values()) + list(golden_graphs.values()) + extra
    assert len(out) == 27
    return out


@pytest.fixture(scope="module")
def single(eng, mixed):
    """Every mixed graph alone, per policy, computed once."""
    return {p: [run(eng, [g], *p)[0] for g in mixed] for p in POLICIES}


@pytest.mark.parametrize("kind,comb", POLICIES)
def test_batch_repeat_and_reset_identities(kind, comb, eng, mixed, single):
    """27 graphs in one call equal each graph alone; a repeated call and md_reset in place of
    md_reset_deferred change nothing."""
    want = single[(kind, comb)]
    assert run(eng, mixed, kind, comb) == want
    assert run(eng, mixed, kind, comb, deferred=False) == want
    assert all(len(s) == len(r) and (not s or r[-1] == 1) for s, r in want)


@pytest.mark.parametrize("env_name,value", [("MD_CENT_SCRATCH", "1"), ("MD_CENT_ROUND_BLOCKS", "3")])
def test_scratch_variant_and_short_rounds_roll_out_the_same(env_name, value, mixed, single, monkeypatch):
    monkeypatch.setenv(env_name, value)
    e = _lib.Engine(ZERO_W)
    try:
        for p in POLICIES:
            assert run(e, mixed, *p) == single[p], p
    finally:
        e.close()


def test_graph_above_the_lds_budget_takes_scratch(eng, shapes):
    """n = 1150 is past the betweenness LDS budget (n <= 1108), so a launch that holds it keeps every
    graph's search arrays in HBM scratch by itself; closeness still fits LDS.  Its 300 connected
    nodes keep the restatement cheap."""
    rng = np.random.default_rng(13)
    big = (1150, _rand_edges(rng, 0, 300, 450), _rand_edges(rng, 0, 300, 450))
    small = [shapes["n65"], shapes["ring"]]
    alone = {p: [run(eng, [g], *p)[0] for g in small] for p in (("betweenness", "max"), ("closeness", "add"))}
    eng.load_graphs([big] + small)
    eng.reset()
    env = refenv.RefEnv(refenv.RefGraph(*big))
    for kind in KINDS:
        assert _scores(eng, kind)[0] == tuple(cent_oracle.dense_scores(env, kind)), kind
    for (kind, comb), want in alone.items():
        res = run(eng, [big] + small, kind, comb)
        assert res[1:] == want
        seq, lmcc, _, _ = cent_oracle.rollout(refenv.RefGraph(*big), kind, comb, max_steps=3)
        assert (res[0][0][:3], res[0][1][:3]) == (seq, lmcc)
        assert res[0][1][-1] == 1 and all(a < 300 for a in res[0][0])


def _state(e, g=0):
    cov, r0, r1, cnt = e.get_state(g)
    return cov.tolist(), r0.tolist(), r1.tolist(), cnt.tolist()


@pytest.mark.parametrize("kind,comb", [("betweenness", "add"), ("closeness", "max")])
def test_state_after_rollout_and_partial_start(kind, comb, golden_graphs):
    g = golden_graphs["er100"]
    gold = centrality_cases.load_golden("er100")
    a, b = _lib.Engine(ZERO_W), _lib.Engine(ZERO_W)
    try:
        seq, lmcc = run(a, [g], kind, comb)[0]
        assert seq == gold[f"{kind}_{comb}_seq"].tolist()
        env = refenv.RefEnv(refenv.RefGraph(*g))
        b.load_graphs([g])
        b.reset()
        for x, lm in zip(seq, lmcc):
            got, term = b.step([x])
            assert int(got[0]) == lm == env.step(x)
        assert bool(term[0]) and env.terminal()
        # the state left behind is the environment's after those removals
        assert _state(a) == _state(b)
        assert sorted(np.flatnonzero(np.array(_state(a)[0])).tolist()) == sorted(env.covered)
        assert a.max_rank().tolist() == b.max_rank().tolist() == [int(gold["m_ori"])]
        # a later md_step is a no-op; md_predict sees a terminal graph; every score is 0
        a.step([int(seq[0])])
        assert _state(a) == _state(b)
        assert a.predict()[1].tolist() == [-1]
        assert _scores(a, kind) == [([0.0] * g[0], [0.0] * g[0])]
        # from a partly dismantled state (three md_steps first): the restatement from that state
        env = refenv.RefEnv(refenv.RefGraph(*g))
        a.reset()
        for x in seq[:3][::-1]:  # (not the policy's own order)
            a.step([x])
            env.step(x)
        before = _state(a)
        assert _scores(a, kind) == [tuple(cent_oracle.dense_scores(env, kind))]
        assert _state(a) == before  # md_centrality_scores leaves the state as it is
        s2, l2 = (x.tolist() for x in a.centrality_rollout(kind, comb)[0])
        want = cent_oracle.rollout(None, kind, comb, env=env)
        assert s2[:3] == seq[:3][::-1]  # the outputs hold every removal since the reset
        assert (s2[3:], l2[3:]) == (want[0], want[1])
        ms, launches = a.last_timing()
        assert launches >= 2 * len(want[0]) and ms > 0.0
        # md_step and md_predict work on a state the rollout left: reset, a step, a prediction
        a.reset()
        got, term = a.step([int(seq[0])])
        assert int(got[0]) == lmcc[0] and not bool(term[0])
        assert a.predict()[0].shape == (g[0],)
    finally:
        a.close()
        b.close()


def test_errors_and_contexts(golden_graphs):
    g = golden_graphs["er100"]
    e = _lib.Engine(ZERO_W)
    try:
        with pytest.raises(_lib.MDError, match="MD_ESTATE"):
            e.centrality_rollout("betweenness", "max")
        with pytest.raises(_lib.MDError, match="MD_ESTATE"):
            e.centrality_scores("closeness")
        e.load_graphs([g])
        for k, c in ((2, 0), (0, 2), (-1, 0)):
            with pytest.raises(_lib.MDError, match="MD_EINVAL"):
                e.centrality_rollout(k, c)
        with pytest.raises(_lib.MDError, match="MD_EINVAL"):
            e.centrality_scores(2)
        with pytest.raises(ValueError):
            e.centrality_rollout("hda", "max")
        with pytest.raises(_lib.MDError, match="MD_EINVAL"):
            e.heuristic_rollout(2, 0)  # md_heuristic_rollout keeps its own two kinds
        want = run(e, [g], "betweenness", "max")
        e.reset()
        want_scores = _scores(e, "betweenness")
    finally:
        e.close()
    d = _lib.Engine(ZERO_W, cost_mode=_lib.MD_COST_DEGREE)
    try:
        d.load_graphs([g], node_w=np.ones(2 * g[0], np.float32))
        with pytest.raises(_lib.MDError, match="MD_EINVAL"):
            d.centrality_rollout("betweenness", "max")
        with pytest.raises(_lib.MDError, match="MD_EINVAL"):
            d.centrality_scores("betweenness")
    finally:
        d.close()
    c = _lib.Engine(np.zeros(_lib.MD_WEIGHT_FLOATS_COMMUNITY, np.float32))
    try:
        assert run(c, [g], "betweenness", "max") == want  # a community context: the prior is not read
        c.reset()
        assert _scores(c, "betweenness") == want_scores
    finally:
        c.close()


def test_cli_writes_the_golden_files(tmp_path):
    from mdcommunity_amd import cli
    real = tmp_path / "data" / "real"
    real.mkdir(parents=True)
    _, stem, n, layers = baseline_cases.FILE_CASES[1]
    (real / (stem + ".edges")).write_text(open(baseline_cases.file_path(stem)).read())
    for method, _, d in centrality_cases.TEXT_METHODS:
        out = tmp_path / d
        assert cli.main(["baseline", "testReal", "--method", method, "--combine", "max", "-o", str(out),
                         "--data-root", str(tmp_path / "data"), "--dataset", "%s:%d:%d,%d" % (stem, n, *layers)]) == 0
        for pre in ("remove_nodes", "MaxCCList_Strategy_"):
            fn = "%s%s_%s%s_1.txt" % (pre, stem, layers[0], layers[1])
            want = open(os.path.join(centrality_cases.GOLDEN, centrality_cases.text_name(d, pre))).read()
            assert (out / fn).read_text() == want
