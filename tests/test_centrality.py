"""The betweenness / closeness baselines on the CPU: the restatement (tests/cent_oracle.py) against
networkx on every state of its rollouts, the goldens made with the reference scripts' own MCC
(tests/golden/make_golden_centrality.py), the result-file writer and the CLI arguments.

Closeness is compared with ``==``.  Betweenness is summed in the device's fixed order, which is
not networkx's, so it is held by a derived bound: all terms are non-negative, so relative errors
add; sigma is exact below 2^53 (asserted by the restatement); a delta at height h carries at most
(dmax + 3) u more than its successors and h <= n; the sum over sources and the scale add
(n + 1) u.  That is n (dmax + 4) u per side, and the factor 4 covers both sides and the
second-order terms: tol = 4 n (dmax + 4) 2^-53, relative.  A pick p is valid when networkx's
combined score of p is at least (1 - 2 tol) times networkx's maximum at that state.
"""
import os

import networkx as nx
import numpy as np
import pytest

import baseline_cases
import cent_oracle
import centrality_cases
from mdcommunity_amd import baselines, baselines_centrality, cli
from oracle import refenv

CASES = centrality_cases.CASES
POLICIES = centrality_cases.POLICIES
NX_FN = {"betweenness": nx.betweenness_centrality, "closeness": nx.closeness_centrality}


@pytest.fixture(scope="module")
def graphs():
    return centrality_cases.graphs()


def tolerance(n, e0, e1):
    deg = np.zeros((2, n), np.int64)
    for l, e in enumerate((e0, e1)):
        for u, v in np.asarray(e).reshape(-1, 2):
            deg[l, u] += 1
            deg[l, v] += 1
    return 4.0 * n * (int(deg.max()) + 4) * 2.0 ** -53


@pytest.mark.parametrize("case", CASES)
def test_restatement_against_networkx(case, graphs):
    n, e0, e1 = graphs[case]
    tol = tolerance(n, e0, e1)
    gold = centrality_cases.load_golden(case)
    states = 0
    for kind, comb in POLICIES:
        def check(env, c0, c1, a, kind=kind, comb=comb):
            r0, r1 = NX_FN[kind](env.g1), NX_FN[kind](env.g2)
            for got, ref in ((c0, r0), (c1, r1)):
                assert set(got) == set(ref)
                for v in ref:
                    if kind == "closeness":
                        assert got[v] == ref[v], (case, v)
                    else:
                        assert (got[v] == 0.0) == (ref[v] == 0.0), (case, v)
                        assert abs(got[v] - ref[v]) <= tol * ref[v], (case, v, got[v], ref[v])
            ref = cent_oracle.combined(r0, r1, comb)
            assert env.g1.degree(a) > 0
            top = max(ref.values())
            if kind == "closeness":
                assert ref[a] == top
            else:
                assert ref[a] >= (1.0 - 2.0 * tol) * top
            nonlocal states
            states += 1

        seq, ranks, _, env = cent_oracle.rollout(refenv.RefGraph(n, e0, e1), kind, comb, on_state=check)
        assert env.terminal()
        k = f"{kind}_{comb}"
        assert seq == gold[k + "_seq"].tolist()
        assert ranks == gold[k + "_lmcc"].tolist() == env.ranks  # the scripts' MCC along the sequence; RefEnv's
    assert states == sum(len(gold[f"{k}_{c}_seq"]) for k, c in POLICIES)


@pytest.mark.parametrize("case", CASES)
def test_golden_reference_scores_certify_the_picks(case, graphs):
    """The scripts' own score lists along the golden sequences: every pick attains their maximum
    (closeness exactly, betweenness within the bound), and the module's list and score
    expressions reproduce the scripts' float64 values."""
    n, e0, e1 = graphs[case]
    tol = tolerance(n, e0, e1)
    g = centrality_cases.load_golden(case)
    assert int(g["n"]) == n
    m_ori = int(g["m_ori"])
    for kind, comb in POLICIES:
        k = f"{kind}_{comb}"
        rp, rm = g[k + "_ref_pick"], g[k + "_ref_max"]
        if kind == "closeness":
            assert rp.tolist() == rm.tolist()
        else:
            assert np.all(rp >= (1.0 - 2.0 * tol) * rm)
        seq, lmcc = g[k + "_seq"].tolist(), g[k + "_lmcc"].tolist()
        mccs = baselines.maxcc_list(lmcc, m_ori) if seq else [1]
        assert [float(x) for x in mccs] == g[k + "_mccs"].tolist()
        assert baselines_centrality.script_score(mccs, n, len(seq), m_ori) == float(g[k + "_score"])
        assert (lmcc[-1] == 1) if seq else (m_ori == 1)


def test_known_scores_of_small_shapes():
    # a 48-ring on both layers: every score equal, the smallest id goes; a star: every leaf 0
    ring = np.array([(v, (v + 1) % 48) for v in range(48)], np.int32)
    env = refenv.RefEnv(refenv.RefGraph(48, ring, ring[::-1].copy()))
    for kind in cent_oracle.KINDS:
        c0, c1 = cent_oracle.scores(env, kind)
        assert len(set(c0.values())) == 1 and c0 == c1 and c0[0] > 0.0
        assert cent_oracle.pick(env, kind, "add")[0] == 0
    star = np.array([(0, v) for v in range(1, 100)], np.int32)
    env = refenv.RefEnv(refenv.RefGraph(100, star, star[::-1].copy()))
    c0, _ = cent_oracle.scores(env, "betweenness")
    # the hub: 99 sources of dependency 98.0 each, an exact integer sum, then the one multiply
    assert c0[0] == 9702.0 * (1.0 / (99 * 98)) and all(c0[v] == 0.0 for v in range(1, 100))
    # K2: L = 2, no scale, every score 0: the smallest live id
    k2 = np.array([[0, 1]], np.int32)
    env = refenv.RefEnv(refenv.RefGraph(2, k2, k2))
    assert cent_oracle.pick(env, "betweenness", "max") == (0, 0.0)
    assert cent_oracle.scores(env, "closeness")[0] == {0: 1.0, 1: 1.0}


def test_block_order_is_part_of_the_definition():
    """The sum over sources is blocked by consecutive ids, with the device's constant; on a lattice
    (many equal-length paths, sigma up to ~1.5e8) the blocked sum stays within the derived bound."""
    assert cent_oracle.SRC_BLOCK == 8
    lat = np.array([(16 * r + c, 16 * r + c + 1) for r in range(16) for c in range(15)] +
                   [(16 * r + c, 16 * (r + 1) + c) for r in range(15) for c in range(16)], np.int32)
    env = refenv.RefEnv(refenv.RefGraph(256, lat, lat[::-1].copy()))
    rows = cent_oracle.alive_rows(env, 0)
    a = cent_oracle.betweenness_layer(rows, 256)
    ref = nx.betweenness_centrality(env.g1)
    tol = 4.0 * 256 * (4 + 4) * 2.0 ** -53
    assert all(abs(a[v] - ref[v]) <= tol * ref[v] for v in ref)


@pytest.mark.parametrize("method,kind,rdir", centrality_cases.TEXT_METHODS)
def test_writer_reproduces_the_golden_files(method, kind, rdir, tmp_path):
    _, stem, n, layers = baseline_cases.FILE_CASES[1]
    g = centrality_cases.load_golden(centrality_cases.TEXT_CASE)
    seq, lmcc, m_ori = g[f"{kind}_max_seq"].tolist(), g[f"{kind}_max_lmcc"].tolist(), int(g["m_ori"])
    (f1, f2), score = baselines_centrality.write_result_files(str(tmp_path), stem, layers, n, m_ori, seq,
                                                              baselines.maxcc_list(lmcc, m_ori))
    assert score == float(g[f"{kind}_max_score"])
    for path, pre in ((f1, "remove_nodes"), (f2, "MaxCCList_Strategy_")):
        assert os.path.basename(path) == "%s%s_%s%s_1.txt" % (pre, stem, layers[0], layers[1])
        want = open(os.path.join(centrality_cases.GOLDEN, centrality_cases.text_name(rdir, pre))).read()
        assert open(path).read() == want
    lines = open(f2).read().split("\n")
    assert len(lines) == n + 2 and lines[-1] == ""  # N values, the score, no standard-deviation line


def test_methods_and_arguments():
    assert baselines.METHODS == ("hda", "ci")  # the degree heuristics' module keeps its own list
    assert baselines_centrality.METHODS == ("hba", "hca")
    assert baselines_centrality.RESULT_DIR == {"hba": "HBA", "hca": "HCA"}
    for bad in (("hda", "max"), ("hbx", "max"), ("hba", "sum")):
        with pytest.raises(ValueError):
            baselines_centrality.dismantle_batch([], *bad)
    with pytest.raises(ValueError):
        baselines_centrality.evaluate_real_data("x", 3, (1, 2), "/nonexistent", "hca", "mul")


def test_cli_dispatches_hba_and_hca(tmp_path, monkeypatch, capsys):
    calls = []
    monkeypatch.setattr(baselines_centrality, "evaluate_real_data",
                        lambda *a, **k: calls.append(("centrality", a, k)) or ([], 0.0))
    monkeypatch.setattr(baselines, "evaluate_real_data", lambda *a, **k: calls.append(("degree", a, k)) or ([], 0.0))
    for method in ("hba", "hca", "ci"):
        assert cli.main(["baseline", "testReal", "--method", method, "--combine", "add", "-o", str(tmp_path),
                         "--data-root", "D", "--dataset", "net:9:1,3"]) == 0
    assert [c[0] for c in calls] == ["centrality", "centrality", "degree"]
    assert calls[0][1] == ("net", 9, (1, 3), str(tmp_path), "hba", "add") and calls[0][2] == {"data_root": "D"}
    assert calls[1][1][4] == "hca"
    with pytest.raises(SystemExit):
        cli.main(["baseline", "testReal", "--method", "hbx", "-o", str(tmp_path), "--dataset", "net:9:1,3"])
    with pytest.raises(SystemExit):
        cli.main(["baseline", "testSynthetic", "--method", "hba", "-o", str(tmp_path), "--dataset", "net:9:1,3"])
    capsys.readouterr()
