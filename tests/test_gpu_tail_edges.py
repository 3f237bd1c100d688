"""The fp64 tail kernels (K3, K4's finish, K6, K7) at singular poses and on non-finite scores, against the CPU oracle.

Every other oracle comparison of these kernels runs at ordinary poses (rotations of 0-30 degrees about a random axis) and Gaussian scores.  This file owns
the hand-written special cases of dmath.h, loss_math.h and k_loss.hip that those never reach: rodrigues_m2v's s < 1e-5 branch at jp angle pi (a camera
aligned with the scene axes, cv rvec = 0, is a jp rotation by exactly pi about x) with its sign heuristics and its c > 0 exit to the zero vector, the
theta < DBL_EPSILON select of rodrigues_R / rodrigues_J and the 1 - cos cancellation just above it, k_pose_loss's zero-error exit, NaN-to-zero rule, trace
clamps, loss clamp and glen > 1e-5 branch -- and k_softmax on -inf, underflowing, subnormal, NaN and +inf scores.

The inputs come from tests/pose_corpus.py; the oracle alone labels them and gives every K7 case its J6 bound max(1e-8, 4 x the oracle's own one-ulp
sensitivity) (tests/test_pose_corpus_cpu.py holds the corpus to its conditions; nothing measured on the GPU enters either).  All other tolerances are the
ones the same quantities have at ordinary poses: test_loss_and_gradient (a7, a8), test_pose_gradients_of_the_last_call (a10), tests/test_gpu_refine.py
(a6), test_softmax_entropy_avg (a4, a5).

Three things the corpus decides rather than this file.  A K7 case whose bound exceeds 1e-4 is unstable and only its loss is compared.  So is a case
with est = gt at a generic rotation: J6 is 0 / 0 there and the zero-error exit hangs on the last bit of a trace of nine rounded products (the oracle
itself returns 0 for some such poses and 1e-6-sized residue for others; pose_corpus._on_the_zero_exit) -- the exit is tested where the trace is 3 in any
arithmetic, at jp rotations by pi about x and by 0.  And within 2e-6 of a rotation error of pi the reference's own factor 1 / sqrt(3 - tr^2 + 2 tr) is
1 / sqrt(0) whenever the trace rounds onto the clamp at -1: J6 is infinite in the reference itself there (the oracle returns inf on some of those
cases), so on them only the absence of NaN is asserted; on every other case J6 must be finite.
"""
import numpy as np
import pytest

import pose_corpus as pc
from conftest import margin

pytestmark = pytest.mark.gpu


# ---- K7 ---------------------------------------------------------------------------------------------------------------------------------------------
def _singles(engine, ests, gts):
    out4, J = np.zeros((len(ests), 4)), np.zeros((len(ests), 6))
    for i, (e, g) in enumerate(zip(ests, gts)):
        r = engine.maxLoss(e, g, want_grad=True)
        out4[i] = (r["loss"], r["rotErr"], r["tErr"], float(r["correct"]))
        J[i] = r["grad"]
    return out4, J


@pytest.fixture(scope="module")
def k7_corpus(engine, orc):
    cases = pc.padded_loss_cases(orc)
    ests, gts = np.stack([c["est"] for c in cases]), np.stack([c["gt"] for c in cases])
    out4, J = _singles(engine, ests, gts)
    return dict(cases=cases, n=len(pc.loss_cases(orc)), ests=ests, gts=gts, out4=out4, J=J)


def test_k7_against_the_oracle_on_the_corpus(k7_corpus):
    cases, out4, J = k7_corpus["cases"][:k7_corpus["n"]], k7_corpus["out4"], k7_corpus["J"]
    worst = {cls: dict(loss=0.0, err=0.0, ratio=0.0, bound=0.0, stable=0, unstable_err=0.0) for cls in pc.CLASSES}
    failed = []  # every case is looked at before the test fails: (index, class, tag, what, figures)
    for i, c in enumerate(cases):
        loss, rot, tr, correct = out4[i]
        w = worst[c["cls"]]

        def hold(ok, what, *fig):
            if not ok:
                failed.append((i, c["cls"], c["tag"], what) + fig)

        w["loss"] = max(w["loss"], abs(loss - c["loss"]) / (1e-5 + 1e-9 * loss))
        hold(abs(loss - c["loss"]) <= 1e-5 + 1e-9 * loss, "loss", loss, c["loss"])
        hold(abs(rot - c["rotErr"]) <= 1e-5, "rotErr", rot, c["rotErr"])
        hold(abs(tr - c["tErr"]) <= 1e-7 * max(1.0, c["tErr"]), "tErr", tr, c["tErr"])
        hold(bool(correct > 0.5) == c["correct"], "correct", correct, c["correct"])
        hold(not np.isnan(J[i]).any(), "NaN in J6", J[i])
        at_clamp = c["cls"] == "rot_err" and c["rotErr"] > np.rad2deg(pc.ROT_ERR_AT_CLAMP)
        if not at_clamp:
            hold(np.isfinite(J[i]).all(), "J6 not finite", J[i])
        if c["robust_zero"]:
            hold(not J[i].any(), "J6 not exactly zero", J[i])
        with np.errstate(invalid="ignore", over="ignore"):
            d = float(np.abs(J[i] - c["J6"]).max() / max(1.0, np.abs(c["J6"]).max())) if np.isfinite(c["J6"]).all() and np.isfinite(J[i]).all() else np.inf
        if c["stable"]:
            w["stable"] += 1
            w["err"], w["ratio"], w["bound"] = max(w["err"], d), max(w["ratio"], d / c["bound"]), max(w["bound"], c["bound"])
            hold(d <= c["bound"], "J6 beyond the case's bound", d, c["bound"])
        else:
            w["unstable_err"] = max(w["unstable_err"], d)
    for f in failed:
        print("FAILED CASE", f)
    assert not failed, "%d of %d cases, the first: %r" % (len(failed), len(cases), failed[0])
    for cls, w in worst.items():
        print("class %-12s %3d stable cases; unstable ones (not asserted) differ by up to %.3e" % (cls, w["stable"], w["unstable_err"]))
        margin("a7", "K7 maxLoss on singular poses, class %s: worst |loss - oracle| / (1e-5 + 1e-9 loss)" % cls, w["loss"], 1.0)
        margin("a8", "K7 dLossMax on singular poses, class %s: worst J6 max-rel among the stable cases (asserted: the class's largest case bound)" % cls, w["err"], w["bound"])
        margin("a8", "K7 dLossMax on singular poses, class %s: worst J6 max-rel / the case's bound max(1e-8, 4 x oracle sensitivity)" % cls, w["ratio"], 1.0)


def test_k7_batch_forms_equal_the_single_calls_bit_for_bit(engine, orc, k7_corpus):
    ests, gts, n = k7_corpus["ests"], k7_corpus["gts"], len(k7_corpus["cases"])
    assert n > 128 and n % 64 != 0  # more than two workgroups of 64 lanes and a ragged last one
    # every estimate with its own ground truth
    r = engine.maxLossFrames(ests, gts, want_grad=True)
    assert np.array_equal(r["out4"], k7_corpus["out4"], equal_nan=True) and np.array_equal(r["grad"], k7_corpus["J"], equal_nan=True)
    # the whole corpus against one ground truth
    gt = orc.cv_to_jp6(pc.GT_CV)
    out4_1, J_1 = _singles(engine, ests, [gt] * n)
    r = engine.maxLossBatch(ests, gt, want_grad=True)
    got4 = np.stack([r["loss"], r["rotErr"], r["tErr"], r["correct"].astype(np.float64)], -1)
    assert np.array_equal(got4, out4_1, equal_nan=True) and np.array_equal(r["grad"], J_1, equal_nan=True)
    # groups of 3 and of 7 estimates per ground truth
    from dsac_amd.capi import check, lib, ptr
    for per in (3, 7):
        F = n // per
        e = np.ascontiguousarray(ests[:F * per])
        g = np.ascontiguousarray(gts[np.arange(F) * per])  # frame f is judged by the ground truth of its first estimate
        out4_b, J_b = np.zeros((F * per, 4)), np.zeros((F * per, 6))
        check(engine._ctx, lib.dsac_loss_batch_frames(engine._ctx, F, per, ptr(e), ptr(g), ptr(out4_b), ptr(J_b)))
        out4_s, J_s = _singles(engine, e, np.repeat(g, per, axis=0))
        assert np.array_equal(out4_b, out4_s, equal_nan=True) and np.array_equal(J_b, J_s, equal_nan=True), per


# ---- K4 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(40, 40), (37, 41)])
def test_k4_pose_gradients_at_singular_poses(engine, orc, H, W):
    """The jp Jacobian behind dsac_last_pose_gradients (cv2our -> rodrigues_m2v -> rodrigues_v2m with the derivative) at jp angle pi: poses next to the
    identity scene's ground truth, a quarter of them with rvec exactly 0.  40 x 40 takes the matrix-core form's finish, 37 x 41 (1517 cells: no multiple
    of 4) the VALU form's.  The reference is the oracle's dProjectdHyp summed over the cells (pose_corpus.pose_gradients, equal to orc.dScore's G6 to
    1e-12 where that can be asked: tests/test_pose_corpus_cpu.py)."""
    N, P = 64, H * W
    fr = pc.identity_scene(4301, 1.0, H, W)
    rng = np.random.default_rng(4302)
    m = np.concatenate([np.zeros(N // 4), np.resize(np.asarray(pc.JP_PI_M[1:]), N - N // 4)])
    u = rng.normal(size=(N, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    poses = np.tile(pc.IDENT_CV, (N, 1))
    poses[:, :3] = m[:, None] * u
    poses[:, 3:] += rng.normal(size=(N, 3)) * 3.0
    assert (np.abs(poses[:, :3]).max(1) == 0).sum() == N // 4
    sets = np.stack([rng.choice(P, 4, replace=False) for _ in range(N)]).astype(np.int32)
    d_err = rng.normal(size=(N, P)).astype(np.float32)
    d_err[np.arange(N)[:, None], sets] = 0
    ref = pc.pose_gradients(orc, fr, poses, d_err)
    assert np.isfinite(ref).all()
    engine.set_frame(fr["xyz"], fr["uv"], H, W, fr["cam"])
    engine.dScore(poses, sets, d_err, dpnp=np.zeros((N, 6, 12)))  # the pose gradients are taken before dPNP
    got = engine.lastPoseGradients(N)
    assert np.isfinite(got).all()
    rel = np.abs(got - ref).max(1) / np.abs(ref).max(1)
    print("K4 %d x %d at jp angle pi: max-rel per hypothesis: median %.3e, max %.3e (rvec exactly 0: max %.3e)" % (H, W, np.median(rel), rel.max(), rel[:N // 4].max()))
    margin("a10", "K4 %d x %d, poses at jp angle pi: per-hypothesis pose gradients, median of max-rel error" % (H, W), np.median(rel), 1e-4)
    margin("a10", "K4 %d x %d, poses at jp angle pi: per-hypothesis pose gradients, max of max-rel error" % (H, W), rel.max(), 1e-3)


# ---- K6 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_mm", [1.0, 0.0])
@pytest.mark.parametrize("steps", [1, 8])
def test_k6_on_the_identity_scene(engine, orc, synth, noise_mm, steps):
    """Refinement towards cv rvec = 0: lm_pnp's Rodrigues derivative runs at and next to theta < DBL_EPSILON, and the refined rvec is 1e-3 (1 mm of noise) to
    1e-8 (none), which a plain allclose with atol = 1e-9 would not see -- the pose is compared as max |d| / max(1, |pose|) <= 1e-7 (row a6) and the rotation
    vector on its own scale below."""
    fr = pc.identity_scene(4201, noise_mm)
    perm = synth.fast_permutations(1600, 8)[:steps]
    init = pc.singular_starts(4202, 5.0)
    assert not init[0, :3].any()
    ref, sd_r = orc.refine(init, perm, fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    assert np.all(sd_r == steps)
    engine.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    res = {}
    try:
        for waves in (1, 4):
            engine.set_option("k6_waves", waves)
            res[waves] = engine.refineAll(init, perm, want_inlier_maps=True)
    finally:
        engine.set_option("k6_waves", 0)
    for a, b in zip(res[1], res[4]):
        assert np.array_equal(a, b)
    got, sd, maps = res[1]
    assert np.array_equal(sd, sd_r)
    for b in range(init.shape[0]):
        _, imap_r, _ = orc.refine(init[b], perm, fr["xyz"], fr["uv"], 40, 40, fr["cam"], want_inlier_map=True)
        assert np.array_equal(maps[b], imap_r), b
    rel = np.abs(got - ref).max(-1) / np.maximum(1.0, np.abs(ref).max(-1))
    print("K6 identity scene, noise %g mm, %d steps: refined |rvec| %.1e ... %.1e, max |d rvec| %.3e" %
          (noise_mm, steps, np.linalg.norm(ref[:, :3], axis=1).min(), np.linalg.norm(ref[:, :3], axis=1).max(), np.abs(got[:, :3] - ref[:, :3]).max()))
    margin("a6", "K6 on the identity scene (cv rvec -> 0; noise %g mm, %d steps): refined pose vs oracle, max |d| / max(1, |pose|)" % (noise_mm, steps), rel.max(), 1e-7)
    # the rotation vector in radians against the same 1e-7: 1e-7 rad moves a point at 2 m by 0.2 um, the scale of 1e-7 x the translation
    margin("a6", "K6 on the identity scene (cv rvec -> 0; noise %g mm, %d steps): refined rvec vs oracle, max |d| [rad]" % (noise_mm, steps),
           np.abs(got[:, :3] - ref[:, :3]).max(), 1e-7)


# ---- K3 ---------------------------------------------------------------------------------------------------------------------------------------------
def _k3_check(orc, name, scores, poses, w, ent, avg, what):
    wr = orc.softMax(scores)
    if np.isnan(wr).all():  # a NaN score, a +inf score, all -inf: the reference's weights are all NaN (its entropy of 0 there is an artefact of its > 0 test)
        assert np.isnan(w).all(), what
        return None
    assert np.isfinite(wr).all(), what
    return (float(np.abs(w - wr).max()), float(abs(ent - orc.entropy(wr))), float(np.abs(avg - orc.avg_pose(wr, poses)).max() / max(1.0, np.abs(poses).max())))


@pytest.mark.parametrize("N", pc.SCORE_N)
def test_k3_on_masked_underflowing_and_non_finite_scores(engine, orc, N):
    """A score model that masks a hypothesis hands K3 a -inf: weight 0, and the entry does not count in the entropy (orc.softMax([-inf, 0, 1]) =
    [0, 0.268941, 0.731059], 0.83994 bits).  k_softmax's entropy term e * x is 0 * -inf = NaN there unless the term is dropped when e == 0."""
    worst = np.zeros(3)
    for name, scores, poses in pc.score_cases(N):
        w, ent, avg = engine.softMax(scores, 1.0, poses)
        fig = _k3_check(orc, name, scores, poses, w, ent[0], avg, (N, name))
        if fig is not None:
            print("N = %4d %-18s |w - oracle| %.3e  |H - oracle| %.3e bits  avg6 %.3e" % ((N, name) + fig))
            assert fig[0] <= 1e-12 and fig[1] <= 1e-10 and fig[2] <= 1e-10, (N, name, fig)
            worst = np.maximum(worst, fig)
    margin("a4", "K3 softmax on -inf / underflowing / subnormal scores: max |w - oracle|", worst[0], 1e-12)
    margin("a4", "K3 entropy on -inf / underflowing / subnormal scores: |H - oracle| bits", worst[1], 1e-10)
    margin("a5", "K3 soft-argmax pose on -inf / underflowing / subnormal scores: max abs difference / max(1, |pose|max)", worst[2], 1e-10)


def test_k3_frames_next_to_a_nan_frame_are_untouched(engine, orc):
    N = 257
    cases = {name: (s, p) for name, s, p in pc.score_cases(N)}
    order = ("one -inf", "NaN elsewhere", "half -inf")
    scores = np.concatenate([cases[k][0] for k in order])
    poses = np.concatenate([cases[k][1] for k in order])
    w, ent, avg = engine.softMaxFrames(scores, N, 1.0, poses)
    assert np.isnan(w[N:2 * N]).all()
    for f in (0, 2):
        w1, e1, a1 = engine.softMax(cases[order[f]][0], 1.0, cases[order[f]][1])
        assert np.array_equal(w[f * N:(f + 1) * N], w1) and ent[f] == e1[0] and np.array_equal(avg[f], a1), f
        assert np.isfinite(w1).all() and np.isfinite(e1[0]) and np.isfinite(a1).all()
