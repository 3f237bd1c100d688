"""The corpus of tests/pose_corpus.py certifies itself on the CPU, with the oracle alone: what tests/test_gpu_tail_edges.py holds the kernels to is what
the classes say, and the bound of every case comes from the oracle's own conditioning.

  * dmath.h's rodrigues_m2v skips the SVD that OpenCV and the oracle run first: restated in numpy (the same branches) and put in front of orc.dLossMax
    it stays within every case's J6 bound, so skipping the SVD is inside the bound before any GPU is involved;
  * every case reaches the branch its class names, by the oracle's own numbers, and none sits on the discontinuity between the two branches;
  * unstable cases (bound above 1e-4) are at most 1/8 of any class and none in jp_pi and jp_zero;
  * the pose-gradient restatement the K4 test compares with equals orc.dScore's G6 where orc.dScore can be asked;
  * orc.refine on the identity scene is stable under one-ulp moves of the start.
"""
import numpy as np

import pose_corpus as pc


def kernel_m2v(R):
    """dm::rodrigues_m2v (dsac_amd/csrc/dmath.h) in numpy: no SVD, the same branches."""
    R = np.asarray(R, np.float64).reshape(9)
    if not np.all((R > -100.0) & (R < 100.0)):
        return np.zeros(3)
    r = np.array([R[7] - R[5], R[2] - R[6], R[3] - R[1]])
    s = np.sqrt((r * r).sum() * 0.25)
    c = min(1.0, max(-1.0, (R[0] + R[4] + R[8] - 1) * 0.5))
    theta = np.arccos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        rx = np.sqrt(max((R[0] + 1) * 0.5, 0.0))
        ry = np.sqrt(max((R[4] + 1) * 0.5, 0.0)) * (-1.0 if R[1] < 0 else 1.0)
        rz = np.sqrt(max((R[8] + 1) * 0.5, 0.0)) * (-1.0 if R[2] < 0 else 1.0)
        if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[5] > 0) != (ry * rz > 0):
            rz = -rz
        return np.array([rx, ry, rz]) * (theta / np.sqrt(rx * rx + ry * ry + rz * rz))
    return r * (theta / (2 * s))


def _jp_angle(orc, cv6):
    return float(np.linalg.norm(orc.cv_to_jp6(cv6)[:3]))


def test_class_sizes_unstable_cases_and_bounds(orc):
    cases = pc.loss_cases(orc)
    summ = pc.summary(cases)
    for cls, (n, unstable, largest) in summ.items():
        print("class %-12s %3d cases, %2d unstable, largest J6 bound among the stable ones %.3e" % (cls, n, unstable, largest))
        assert n >= 16, cls
        assert unstable <= pc.MAX_UNSTABLE_SHARE * n, (cls, unstable, n)
    assert summ["jp_pi"][1] == 0 and summ["jp_zero"][1] == 0
    for c in cases:
        assert c["bound"] == max(1e-8, 4 * c["sens"]) and c["stable"] == (c["bound"] <= 1e-4 and not c["on_exit"])
        if c["stable"]:
            assert np.isfinite(c["J6"]).all()
        assert not c["on_exit"] or c["cls"] == "zero"
    n = len(pc.padded_loss_cases(orc))
    assert n > 128 and n % 64 != 0
    # every magnitude the classes are made of is there
    tags = {(c["cls"], c["tag"]) for c in cases}
    for m in pc.JP_PI_M:
        assert ("jp_pi", "m=%g vs generic" % m) in tags and ("jp_pi", "m=%g vs identity scene" % m) in tags
    for d in pc.JP_ZERO_D:
        assert ("jp_zero", "d=%g vs generic" % d) in tags
    assert ("jp_zero", "cv rvec (pi, 0, 0) vs generic") in tags
    for a in (1e-5, 1e-3, 1.0, np.pi - 1e-3, np.pi - 1e-6, np.pi - 1e-9, np.pi):
        assert ("rot_err", "a=%.10g" % a) in tags
    for L in pc.GT_SINGULAR_LEN:
        assert ("gt_singular", "glen=%.10g" % L) in tags


def test_the_kernels_m2v_without_the_svd_stays_inside_every_bound(orc):
    worst = dict.fromkeys(pc.CLASSES, (0.0, 0.0))
    for c in pc.loss_cases(orc):
        J = pc.oracle_J6(orc, c["est"], c["gt"], m2v=kernel_m2v)
        if c["stable"]:
            d = float(np.abs(J - c["J6"]).max() / max(1.0, np.abs(c["J6"]).max()))
            assert d <= c["bound"], (c["cls"], c["tag"], d, c["bound"])
            w = worst[c["cls"]]
            worst[c["cls"]] = (max(w[0], d), max(w[1], d / c["bound"]))
        if c["robust_zero"]:
            assert not J.any(), (c["cls"], c["tag"], J)
    for cls, (d, ratio) in worst.items():
        print("class %-12s kernel m2v in front of orc.dLossMax: worst J6 difference %.3e, worst ratio to the case's bound %.3f" % (cls, d, ratio))


def test_every_case_reaches_the_branch_of_its_class(orc):
    cases = pc.loss_cases(orc)
    for c in cases:
        rot, tcm = c["rotErr"], c["tErr"] / 10
        if c["cls"] == "jp_pi":
            assert abs(_jp_angle(orc, c["est"]) - np.pi) <= 1e-4, c["tag"]
        if c["cls"] == "jp_zero":
            assert _jp_angle(orc, c["est"]) <= 1.1e-4, c["tag"]  # our2cv's matrix -> vector at cv angle pi keeps the small jp angle to about 1e-6
        if c["cls"] == "rot_err":
            assert rot > 10 * tcm, c["tag"]
        if c["cls"] == "t_err":
            assert tcm > 10 * rot, c["tag"]
        if c["cls"] == "zero":
            assert rot + tcm < 1e-5, c["tag"]
        if c["cls"] == "clamp":
            assert (c["loss"] == 1e7 and not c["J6"].any()) if c["tag"] == "beyond" else (9e6 < c["loss"] < 1e7 and c["J6"].any()), c["tag"]
        if c["cls"] == "nan_t":
            assert np.isnan(c["est"][3:]).any() and np.isfinite(c["loss"]) and np.isfinite(c["J6"]).all()
        if c["cls"] not in ("zero",):  # the branch is a discontinuity: a case on it tests nothing (the zero class sits on the zero-error exit instead)
            assert abs(rot - tcm) > 1e-6 * max(rot, tcm), (c["cls"], c["tag"], rot, tcm)
    sing = [c for c in cases if c["cls"] == "gt_singular"]
    lens = sorted({float(np.linalg.norm(c["gt"][:3])) for c in sing})
    assert lens[0] == 0.0 and any(0 < L <= 1e-5 for L in lens) and any(1e-5 < L < 1e-4 for L in lens) and any(abs(L - np.pi) < 1e-12 for L in lens)
    # rot_err goes up to the trace clamp at -1: at least one case whose rotation error is 180 degrees to rounding
    assert any(c["cls"] == "rot_err" and abs(c["rotErr"] - 180.0) < 1e-5 for c in cases)
    # the zero class reaches the zero-error exit in the oracle
    assert sum(c["cls"] == "zero" and c["robust_zero"] for c in cases) >= 16


def test_pose_gradient_restatement_equals_dscore(orc, frame40):
    fr = frame40
    N = 6
    poses, sets, ok, _ = orc.sample(N, 11, fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    rng = np.random.default_rng(3)
    d_err = rng.normal(size=(N, 1600))
    d_err[np.arange(N)[:, None], sets] = 0
    _, G6, _ = orc.dScore(sets, d_err, fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    got = pc.pose_gradients(orc, fr, poses, d_err)
    rel = float((np.abs(got - G6).max(1) / np.abs(G6).max(1)).max())
    print("pose-gradient restatement vs orc.dScore: max-rel %.3e" % rel)
    assert rel <= 1e-12


def test_identity_scene_and_its_refinement_in_the_oracle(orc, synth):
    perm = synth.fast_permutations(1600, 8)
    for noise in (1.0, 0.0):
        fr = pc.identity_scene(4201, noise)
        assert fr["xyz"].dtype == np.float32 and fr["xyz"].shape == (1600, 3) and np.array_equal(fr["gt_pose"], pc.IDENT_CV)
        e = orc.get_diff_maps(fr["gt_pose"], fr["xyz"], fr["uv"], 40, 40, fr["cam"])[0]
        assert e.max() < (3.0 if noise else 1e-2)  # no outliers
        init = pc.singular_starts(4202, 5.0)
        assert not init[0, :3].any() and not init[1, :3].any()  # rvec exactly 0 among the starts
        for steps in (1, 8):
            ref, sd = orc.refine(init, perm[:steps], fr["xyz"], fr["uv"], 40, 40, fr["cam"])
            assert np.all(sd == steps)
            worst = 0.0
            for away in (np.inf, -np.inf):
                r, s = orc.refine(np.nextafter(init, away), perm[:steps], fr["xyz"], fr["uv"], 40, 40, fr["cam"])
                assert np.array_equal(s, sd)
                worst = max(worst, float((np.abs(r - ref).max(-1) / np.maximum(1.0, np.abs(ref).max(-1))).max()))
            print("identity scene, noise %g mm, %d steps: refined poses under one-ulp moves of the start agree to %.3e" % (noise, steps, worst))
            # all eight steps: 1e-12.  One step is one LM call that ends on its FLT_EPSILON stop, so a neighbouring start may end it an iteration's worth
            # (up to ~1e-7 of the pose's scale) elsewhere: held to 1e-9 like tests/lm_corpus.py's STABLE_TOL, 100 times tighter than what the GPU is held to
            assert worst <= (1e-12 if steps == 8 else 1e-9)


def test_score_cases_are_what_they_say(orc):
    for N in pc.SCORE_N:
        cases = pc.score_cases(N)
        assert [c[0] for c in cases] == ["one -inf", "half -inf", "all equal", "beyond underflow", "subnormal weights", "NaN at index 0", "NaN elsewhere",
                                         "+inf", "all -inf"]
        for name, s, poses in cases:
            assert s.shape == (N,) and poses.shape == (N, 6) and 1000 < np.abs(poses[:, 3:]).max() < 4000
            w = orc.softMax(s)
            nan_expected = name in ("NaN at index 0", "NaN elsewhere", "+inf", "all -inf") or (N == 1 and name == "one -inf")
            assert np.isnan(w).all() if nan_expected else np.isfinite(w).all(), (N, name)
            if name == "subnormal weights" and N > 1:
                assert np.all(w[1:] < 2.3e-308) and np.any(w[1:] > 0)
            if name == "one -inf" and N > 1:
                assert w[N // 2] == 0 and abs(w.sum() - 1) < 1e-12
    w = orc.softMax([-np.inf, 0.0, 1.0])
    assert np.allclose(w, [0, 0.268941, 0.731059], atol=1e-6) and abs(orc.entropy(w) - 0.83994) < 1e-5
