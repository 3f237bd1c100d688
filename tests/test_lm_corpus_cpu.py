"""The LM corpus of tests/lm_corpus.py certifies itself on the CPU: what tests/test_gpu_refine_lm.py compares the GPU with is what the labels describe.

  * the Python chain of oracle.solve_pnp_iterative calls (whose statistics give the labels) equals oracle.refine bit for bit on every problem;
  * conditions on the corpus, not measurements: at most a quarter of each (map, steps) group is unstable under the equivalent perturbations, every
    hard-path label except the forced accept occurs at least 8 times among the stable problems, and the forced accept at the lambda ceiling occurs in the
    third call of every fixed-point problem.
"""
import numpy as np

import lm_corpus


def test_python_chain_equals_refine_bit_for_bit(orc):
    for key, g in lm_corpus.corpus(orc).items():
        assert g["init"].shape == (64, 6)
        for b, (pose, done, stats) in enumerate(g["chains"]):
            assert done == g["sd"][b] == g["steps"] and len(stats) == g["steps"], (key, b)
            assert np.array_equal(pose, g["ref"][b]), (key, b)
    fp = lm_corpus.fixed_point(orc)
    for steps, r in fp["runs"].items():
        for b, (pose, done, stats) in enumerate(r["chains"]):
            assert done == r["sd"][b] == steps, (steps, b)
            assert np.array_equal(pose, r["ref"][b]), (steps, b)


def test_one_step_problems_are_the_first_call_of_the_eight_step_ones(orc):
    G = lm_corpus.corpus(orc)
    for name in lm_corpus.MAPS:
        for c1, c8 in zip(G[(name, 1)]["chains"], G[(name, 8)]["chains"]):
            assert c1[2][0] == c8[2][0]


def test_at_most_a_quarter_of_every_group_is_unstable(orc):
    for key, g in lm_corpus.corpus(orc).items():
        n = int((~g["stable"]).sum())
        print("group %s: %d of %d problems unstable under the equivalent perturbations" % (key, n, len(g["stable"])))
        assert n <= lm_corpus.MAX_UNSTABLE, (key, n)
        assert np.all(g["spread"][g["stable"]] <= lm_corpus.STABLE_TOL)


def test_every_hard_branch_occurs_among_the_stable_problems(orc):
    count = dict.fromkeys(lm_corpus.LABELS, 0)
    for g in lm_corpus.corpus(orc).values():
        for b in np.flatnonzero(g["stable"]):
            for l in g["labels"][b]:
                count[l] += 1
    print("stable problems per label:", count)
    for l in lm_corpus.LABELS:
        if l != "forced":
            assert count[l] >= 8, (l, count)


def test_fixed_point_third_call_is_a_forced_accept(orc):
    fp = lm_corpus.fixed_point(orc)
    for steps in (3, 4):
        for b, (pose, done, stats) in enumerate(fp["runs"][steps]["chains"]):
            st = stats[2]
            assert st["forced"] and st["max_lambda_lg10"] == 17 and st["rejected"] >= 19, (steps, b, st)
    # the fixed point is one: the forced trial moves the pose by rounding only
    r2, r3 = fp["runs"][2]["ref"], fp["runs"][3]["ref"]
    assert np.all(np.abs(r3 - r2).max(-1) / np.maximum(1.0, np.abs(r2).max(-1)) < 1e-9)


def test_lm_statistics_are_consistent(orc):
    """The statistics are bookkeeping: the solve returns the same bits with and without them, and they obey the state machine's own arithmetic
    (lambda starts at 1e-3 and rises by one decade per rejection; 17 means the ceiling was passed, which is the forced accept)."""
    g = lm_corpus.corpus(orc)[("clean", 1)]
    fr, cells = g["frame"], g["perm"][0, :lm_corpus.MAX_INL]
    for b in (0, 17, 34, 50):  # problems without a replica perturbation
        assert g["px"][b, 0] < 0
        pose, it, err, st = orc.solve_pnp_iterative(fr["xyz"][cells], fr["uv"][cells], fr["cam"], g["init"][b], stats=True)
        pose3, it3, err3 = orc.solve_pnp_iterative(fr["xyz"][cells], fr["uv"][cells], fr["cam"], g["init"][b])
        assert np.array_equal(pose, pose3) and it == it3 == st["iters"] and np.array_equal(err, err3)
        assert 1 <= st["iters"] <= 20 and st["rejected"] >= 0 and st["min_margin"] >= 0
        assert -3 <= st["max_lambda_lg10"] <= min(17, -3 + st["rejected"] + (1 if st["forced"] else 0))
        assert st["forced"] == (st["max_lambda_lg10"] == 17)
