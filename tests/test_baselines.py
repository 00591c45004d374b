"""Baseline heuristics, host side (no GPU): the policy restatement on the oracle environment
(tests/heur_oracle.py) reproduces the reference scripts' own removal sequences and LMCC traces
(goldens of tests/golden/make_golden_baselines.py), and the file writer and score expression of
mdcommunity_amd.baselines reproduce the scripts' text files and float64 score."""
import os

import numpy as np
import pytest

import baseline_cases
import heur_oracle
from conftest import GOLDEN
from mdcommunity_amd import baselines, cli
from oracle import refenv

CASES = list(baseline_cases.graphs().items())


@pytest.fixture(scope="module")
def oracle_runs():
    """Every case's rollouts on the oracle, computed once."""
    cache = {}

    def get(case, kind, combine):
        key = (case, kind, combine)
        if key not in cache:
            n, e0, e1 = dict(CASES)[case]
            cache[key] = heur_oracle.rollout(refenv.RefGraph(n, e0, e1), kind, combine)[:3]
        return cache[key]

    return get


@pytest.mark.parametrize("case", [c for c, _ in CASES])
@pytest.mark.parametrize("kind", ["hda", "ci"])
def test_oracle_restatement_reproduces_max_goldens(case, kind, oracle_runs):
    g = baseline_cases.load_golden(case)
    seq, ranks, _ = oracle_runs(case, kind, "max")
    assert seq == g[f"{kind}_max_seq"].tolist()
    assert ranks == g[f"{kind}_max_lmcc"].tolist()
    n = dict(CASES)[case][0]
    assert refenv.RefGraph(*dict(CASES)[case]).max_rank == int(g["m_ori"])
    mccs = baselines.maxcc_list(ranks, int(g["m_ori"])) if seq else [1]
    assert [float(x) for x in mccs] == g[f"{kind}_max_mccs"].tolist()
    assert baselines.audc_score(mccs, n) == float(g[f"{kind}_max_score"])  # exact, float64


@pytest.mark.parametrize("case", [c for c, _ in CASES])
@pytest.mark.parametrize("kind", ["hda", "ci"])
def test_oracle_add_sequences_meet_the_certificate(case, kind, oracle_runs):
    g = baseline_cases.load_golden(case)
    seq, ranks, scores = oracle_runs(case, kind, "add")
    assert seq == g[f"{kind}_add_seq"].tolist()
    assert [int(s) for s in scores] == g[f"{kind}_add_cert"].tolist()
    assert ranks == g[f"{kind}_add_lmcc"].tolist()


def test_score_is_the_scripts_expression_not_an_accumulated_sum():
    """(sum(MCCs) - 1) / N over [1, r / M_ori, ...]: on gmm1000_s0 the accumulated
    sum of r / (M_ori * N) differs from it in the last bits, and the golden holds the former."""
    g = baseline_cases.load_golden("gmm1000_s0")
    ranks, m, n = g["hda_max_lmcc"].tolist(), int(g["m_ori"]), int(g["n"])
    s = baselines.audc_score(baselines.maxcc_list(ranks, m), n)
    assert s == float(g["hda_max_score"])
    acc = 0.0
    for r in ranks:
        acc += r / (m * n)
    assert abs(acc - s) < 1e-12


@pytest.mark.parametrize("case,stem,n,layers", baseline_cases.FILE_CASES[1:])
@pytest.mark.parametrize("kind", ["hda", "ci"])
def test_file_writer_reproduces_script_output(tmp_path, case, stem, n, layers, kind):
    g = baseline_cases.load_golden(case)
    sol = g[f"{kind}_max_seq"].tolist()
    mccs = baselines.maxcc_list(g[f"{kind}_max_lmcc"].tolist(), int(g["m_ori"]))
    (f1, f2), score = baselines.write_result_files(str(tmp_path), stem, layers, n, int(g["m_ori"]), sol, mccs)
    assert score == float(g[f"{kind}_max_score"])
    d = baselines.RESULT_DIR[kind]
    for f in (f1, f2):
        want = open(os.path.join(GOLDEN, "baseline_%s_%s" % (d, os.path.basename(f)))).read()
        assert open(f).read() == want


def test_file_writer_pads_and_handles_no_removal(tmp_path):
    (f1, f2), score = baselines.write_result_files(str(tmp_path), "x", (1, 2), 4, 1, [], [1])
    assert open(f1).read() == "" and score == 0.0
    assert open(f2).read() == "1.00000000\n" * 4 + "0.00000000\n" * 2


def test_cli_baseline_arguments():
    with pytest.raises(SystemExit):
        cli.main(["baseline", "testReal", "-o", "/tmp/x"])  # no dataset list of its own
    with pytest.raises(SystemExit):
        cli.main(["baseline", "testSynthetic", "-o", "/tmp/x", "--dataset", "a:1:1,2"])
    with pytest.raises(ValueError):
        baselines.dismantle_batch([], method="hba")
