"""Device rollouts of the HDA / CI baselines (md_heuristic_rollout) on the GPU.

MAX policies: the reference scripts' own removal sequences, LMCC traces and float64 AUDC
(goldens of tests/golden/make_golden_baselines.py), bit-exact.  ADD policies: the certificate --
along the device's sequence the pick's score equals the maximum of the add script's own score
list, and the LMCC trace is the script's MCC on that sequence.  The smallest shapes that can
break the kernel against the oracle restatement (tests/heur_oracle.py), batch / repeat / HBM-path
identities, and the state the rollout leaves."""
import numpy as np
import pytest

import baseline_cases
import heur_oracle
from test_certificates import load_cert
from mdcommunity_amd import _lib, baselines, engine, synth
from oracle import refenv

pytestmark = pytest.mark.gpu

POLICIES = list(baseline_cases.POLICIES)
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
    """The smallest shapes at which the kernel can go wrong."""
    rng = np.random.default_rng(7)
    k2 = np.array([[0, 1]], np.int32)
    out = {"k2": (2, k2, k2)}
    for n in (63, 64, 65):  # a wavefront edge
        out[f"n{n}"] = (n, _rand_edges(rng, 0, n, 2 * n), _rand_edges(rng, 0, n, 2 * n))
    for n in (511, 512, 513):  # the workgroup's node chunking; sparse
        out[f"n{n}"] = (n, _rand_edges(rng, 0, n, n + n // 4), _rand_edges(rng, 0, n, n + n // 4))
    out["layer1_empty"] = (30, _rand_edges(rng, 0, 30, 60), np.zeros((0, 2), np.int32))
    star = np.array([(7, v) for v in range(40) if v != 7], np.int32)
    out["shared_hub"] = (40, star, star[::-1].copy())  # every CI is 0: the smallest live id wins
    ring = np.array([(v, (v + 1) % 48) for v in range(48)], np.int32)
    out["ring"] = (48, ring, np.roll(ring, 5, axis=0).copy())  # every score equal at the first step
    out["isolated_low"] = (70, _rand_edges(rng, 10, 70, 150), _rand_edges(rng, 10, 70, 140))  # 0-9 never picked
    # two equal hubs whose ids (5, 200) fall to different waves
    two = np.array([(5, v) for v in range(10, 22)] + [(200, v) for v in range(210, 222)], np.int32)
    out["tie_across_waves"] = (256, two, two[::-1].copy())
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
def shape_oracle(shapes):
    """The oracle restatement's rollouts of the shape graphs, computed once."""
    return {(name, kind, comb): heur_oracle.rollout(refenv.RefGraph(*g), kind, comb)[:2]
            for name, g in shapes.items() for kind, comb in POLICIES}


@pytest.fixture(scope="module")
def golden_graphs():
    return baseline_cases.graphs()


def run(e, graphs, kind, comb, deferred=True):
    e.load_graphs(graphs)
    if deferred:
        e.reset_deferred()
    else:
        e.reset()
    res = e.heuristic_rollout(kind, comb)
    return [(s.tolist(), r.tolist()) for s, r in res]


@pytest.mark.parametrize("kind", ["hda", "ci"])
def test_max_policies_reproduce_the_reference(kind, golden_graphs):
    """seq, LMCC trace and AUDC of hda_2max.py / ci_max.py on every golden case (one launch)."""
    names = list(golden_graphs)
    res = baselines.dismantle_batch([golden_graphs[c] for c in names], kind, "max")
    for c, (sol, mccs, score) in zip(names, res):
        g = baseline_cases.load_golden(c)
        assert sol == g[f"{kind}_max_seq"].tolist(), c
        assert [float(x) for x in mccs] == g[f"{kind}_max_mccs"].tolist(), c
        assert score == float(g[f"{kind}_max_score"]), c  # float64, exact


@pytest.mark.parametrize("kind", ["hda", "ci"])
def test_add_policies_meet_the_certificate(kind, eng, golden_graphs):
    names = list(golden_graphs)
    res = run(eng, [golden_graphs[c] for c in names], kind, "add")
    for c, (seq, lmcc) in zip(names, res):
        g = baseline_cases.load_golden(c)
        # the certificate is stored along the deterministic add sequence: the device must take it
        assert seq == g[f"{kind}_add_seq"].tolist(), c
        assert lmcc == g[f"{kind}_add_lmcc"].tolist(), c  # the add script's own MCC on that sequence
        # the pick's score, teacher-forced along the device's sequence, is the script's maximum
        env = refenv.RefEnv(refenv.RefGraph(*golden_graphs[c]))
        for a, want, lm in zip(seq, g[f"{kind}_add_cert"].tolist(), lmcc):
            assert env.g1.degree(a) > 0
            assert heur_oracle.node_score(env, a, kind, "add") == want, (c, a)
            assert env.step(a) == lm
        assert env.terminal()


@pytest.mark.parametrize("kind,comb", POLICIES)
def test_smallest_shapes_match_the_oracle(kind, comb, eng, shapes, shape_oracle):
    names = list(shapes)
    res = run(eng, [shapes[s] for s in names], kind, comb)
    for s, got in zip(names, res):
        assert got == shape_oracle[(s, kind, comb)], s
    got = dict(zip(names, res))
    assert got["layer1_empty"] == ([], [])  # terminal after s0: zero removals
    # the hub has the largest degree; every CI of a star is 0, so the smallest live id goes first
    assert got["shared_hub"][0] == ([7] if kind == "hda" else list(range(8)))
    assert got["ring"][0][0] == 0
    assert all(a >= 10 for a in got["isolated_low"][0])
    assert got["tie_across_waves"][0][:2] == [5, 200]


@pytest.mark.parametrize("kind,comb", POLICIES)
def test_batch_equals_single_graph_launches(kind, comb, eng, shapes, golden_graphs, monkeypatch):
    """27 mixed graphs in one launch, the same 27 on a context of 8 workgroups (the persistent
    loop), and a repeated launch: all equal, graph by graph, to single-graph launches."""
    mixed = list(shapes.values()) + list(golden_graphs.values())
    assert len(mixed) == 27
    single = [run(eng, [g], kind, comb)[0] for g in mixed]
    assert run(eng, mixed, kind, comb) == single
    assert run(eng, mixed, kind, comb, deferred=False) == single  # repeated; s0 by md_reset
    monkeypatch.setenv("MD_MAX_CUS", "8")
    few = _lib.Engine(ZERO_W)
    try:
        assert run(few, mixed, kind, comb) == single
    finally:
        few.close()


def test_more_graphs_than_workgroups(eng):
    """300 small graphs in one launch (more than the chip has CUs) against single-graph launches."""
    rng = np.random.default_rng(3)
    gs = []
    for _ in range(300):
        n = int(rng.integers(8, 25))
        gs.append((n, _rand_edges(rng, 0, n, n + 4), _rand_edges(rng, 0, n, n + 4)))
    batch = run(eng, gs, "ci", "max")
    for i in range(300):
        assert run(eng, [gs[i]], "ci", "max")[0] == batch[i], i
    for g, (seq, lmcc) in list(zip(gs, batch))[::10]:
        assert heur_oracle.rollout(refenv.RefGraph(*g), "ci", "max")[:2] == (seq, lmcc)


@pytest.mark.parametrize("kind,comb", POLICIES)
def test_hbm_path_equals_lds_path(kind, comb, eng, golden_graphs, monkeypatch):
    """MD_VARIANT=64 keeps the state in HBM: pick kernel + environment-step launch per removal."""
    gs = [golden_graphs[c] for c in ("edge_wave_65", "gmm200_s7", "gmm1000_s0")]
    want = run(eng, gs, kind, comb)
    monkeypatch.setenv("MD_VARIANT", "64")
    hbm = _lib.Engine(ZERO_W)
    try:
        for g, w in zip(gs, want):  # one graph per launch: the grid-wide environment step
            assert run(hbm, [g], kind, comb)[0] == w
        assert run(hbm, gs, kind, comb, deferred=False) == want  # together: one workgroup per graph
        assert hbm.last_timing()[1] >= 2 * len(want[2][0])  # a pick and a step launch per removal
    finally:
        hbm.close()


@pytest.fixture(scope="module")
def above_lds():
    """A real-like graph just above the LDS fit predicate."""
    prev = None
    for n in range(2400, 4001, 100):
        lay = synth.real_like_layers(n=n, seed=3)
        es = [np.array(sorted({(min(u, v), max(u, v)) for u, v in l if u != v}), np.int32) for l in lay]
        if not _lib.heuristic_fits_lds(n, len(es[0]) + len(es[1])):
            assert prev is not None and _lib.heuristic_fits_lds(*prev)
            return n, es[0], es[1]
        prev = (n, len(es[0]) + len(es[1]))
    raise AssertionError("no size above the predicate found")


@pytest.mark.parametrize("kind,comb", [("hda", "max"), ("ci", "add")])
def test_graph_above_the_lds_predicate(kind, comb, eng, above_lds):
    seq, lmcc = run(eng, [above_lds], kind, comb)[0]
    assert len(seq) >= 10 and lmcc[-1] == 1
    env = refenv.RefEnv(refenv.RefGraph(*above_lds))
    for a, lm in zip(seq[:10], lmcc[:10]):  # teacher-forced along the device's sequence
        assert heur_oracle.pick(env, kind, comb)[0] == a
        assert env.step(a) == lm


def _state(e, g=0):
    cov, r0, r1, cnt = e.get_state(g)
    return cov.tolist(), r0.tolist(), r1.tolist(), cnt.tolist()


@pytest.mark.parametrize("variant", ["0", "64"])
def test_state_after_rollout_and_partial_start(variant, golden_graphs, monkeypatch):
    monkeypatch.setenv("MD_VARIANT", variant)
    g = golden_graphs["er100"]
    a, b = _lib.Engine(ZERO_W), _lib.Engine(ZERO_W)
    try:
        seq, lmcc = run(a, [g], "ci", "max")[0]
        b.load_graphs([g])
        b.reset()
        for x, lm in zip(seq, lmcc):
            got, term = b.step([x])
            assert int(got[0]) == lm
        assert bool(term[0])
        assert _state(a) == _state(b)
        assert a.max_rank().tolist() == b.max_rank().tolist()
        # a later md_step is a no-op on both; md_predict sees a terminal graph
        assert a.predict()[1].tolist() == [-1]
        # from a partly dismantled state: the oracle from that state
        env = refenv.RefEnv(refenv.RefGraph(*g))
        a.reset()
        for x in seq[:3][::-1]:  # (not the policy's own order)
            a.step([x])
            env.step(x)
        s2, l2 = (x.tolist() for x in a.heuristic_rollout("hda", "add")[0])
        want = heur_oracle.rollout(None, "hda", "add", env=env)
        assert s2[:3] == seq[:3][::-1]  # the outputs hold every removal since the reset
        assert (s2[3:], l2[3:]) == (want[0], want[1])
        ms, launches = a.last_timing()
        assert launches >= 1 and ms > 0.0
    finally:
        a.close()
        b.close()


def test_model_rollout_unchanged_after_heuristic_rollout(golden_graphs):
    """md_reset + md_rollout on a context that ran a heuristic rollout: the certified sequence
    (tests/test_certificates.py) and the reference's LMCC trace along it, unchanged."""
    cert = load_cert("gmm200_s7")
    e = _lib.Engine(engine.load_weights(engine.DEFAULT_UNIT))
    try:
        e.load_graphs([golden_graphs["gmm200_s7"]])
        e.reset()
        e.heuristic_rollout("ci", "add")
        e.reset()
        seq, ranks = e.rollout()[0]
        assert seq.tolist() == cert["gpu_seq"].tolist() and ranks.tolist() == cert["ref_ranks_along"].tolist()
    finally:
        e.close()


def test_errors_and_contexts(golden_graphs):
    g = golden_graphs["er100"]
    e = _lib.Engine(ZERO_W)
    try:
        with pytest.raises(_lib.MDError, match="MD_ESTATE"):
            e.heuristic_rollout("hda", "max")
        e.load_graphs([g])
        for k, c in ((2, 0), (0, 2), (-1, 0)):
            with pytest.raises(_lib.MDError, match="MD_EINVAL"):
                e.heuristic_rollout(k, c)
        want = run(e, [g], "hda", "max")
    finally:
        e.close()
    d = _lib.Engine(ZERO_W, cost_mode=_lib.MD_COST_DEGREE)
    try:
        d.load_graphs([g], node_w=np.ones(2 * g[0], np.float32))
        with pytest.raises(_lib.MDError, match="MD_EINVAL"):
            d.heuristic_rollout("hda", "max")
    finally:
        d.close()
    c = _lib.Engine(np.zeros(_lib.MD_WEIGHT_FLOATS_COMMUNITY, np.float32))
    try:
        assert run(c, [g], "hda", "max") == want  # a community context: the prior is not read
    finally:
        c.close()


def test_cli_baseline_writes_the_scripts_files(tmp_path):
    import os
    from conftest import GOLDEN
    from mdcommunity_amd import cli
    real = tmp_path / "data" / "real"
    real.mkdir(parents=True)
    _, stem, n, layers = baseline_cases.FILE_CASES[1]
    (real / (stem + ".edges")).write_text(open(baseline_cases.file_path(stem)).read())
    for method, d in (("hda", "HDA"), ("ci", "CI")):
        out = tmp_path / d
        assert cli.main(["baseline", "testReal", "--method", method, "--combine", "max", "-o", str(out),
                         "--data-root", str(tmp_path / "data"), "--dataset", "%s:%d:%d,%d" % (stem, n, *layers)]) == 0
        for pre in ("remove_nodes", "MaxCCList_Strategy_"):
            fn = "%s%s_%s%s_1.txt" % (pre, stem, layers[0], layers[1])
            assert (out / fn).read_text() == open(os.path.join(GOLDEN, "baseline_%s_%s" % (d, fn))).read()
