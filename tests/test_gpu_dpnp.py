"""K5 (k_dpnp) against the CPU oracle off the one shape of test_dpnp_parity, and against exact P3P roots: the corpus of tests/dpnp_corpus.py
(tests/test_dpnp_corpus_cpu.py holds it to its conditions) and the fixture tests/golden/dpnp_exact.npz.

Per set the rule is the project's K5 rule: rel = max |J - J_oracle| / max(1, |J_oracle|max) <= bound = max(1e-6, 4 sens), sens the oracle's own change under
one-ulp moves of the set's float coordinates.  A set whose bound exceeds 1e-2 is unstable: its J is not compared, its finiteness is.  Where the oracle's J
is exactly zero and stays so under every one-ulp move -- P3P fails on both sides of every difference -- the engine's is exactly zero.
"""
import os

import numpy as np
import pytest

import dpnp_corpus as dc
from conftest import margin

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dpnp_exact.npz")


def _check(J, cs, what):
    """every set finite, the stable ones within their bound, exact zeros where the oracle's zero is robust; returns rel of the stable sets and rel / bound"""
    J = np.asarray(J)
    assert J.shape == (len(cs), 6, 12) and np.isfinite(J).all(), what
    rel, ratio = [], []
    for h, c in enumerate(cs):
        if not c["stable"]:
            continue
        r = dc.rel(J[h], c["J"])
        assert r <= c["bound"], (what, h, c["set"], r, c["bound"], c["sens"])
        if c["zero"]:
            assert not J[h].any(), (what, h, c["set"])
        rel.append(r)
        ratio.append(r / c["bound"])
    return np.array(rel), np.array(ratio)


@pytest.mark.parametrize("tag,kind,eps", dc.groups())
def test_corpus_against_the_oracle(engine, orc, tag, kind, eps):
    cs = dc.cases(orc, tag, kind, eps)
    dc.set_frame(engine, tag)
    J = engine.dPNP(np.stack([c["set"] for c in cs]), eps=eps)
    what = "frame %s %s eps %g" % (tag, kind, eps)
    rel, ratio = _check(J, cs, what)
    print("%s: %d sets, %d stable: rel median %.2e  max %.2e;  worst rel / bound %.2f" % (what, len(cs), len(rel), np.median(rel), rel.max(), ratio.max()))
    margin("a11", "K5 dPNP corpus vs oracle, %s: median relative error over the stable sets" % what, np.median(rel), 1e-6)
    margin("a11", "K5 dPNP corpus vs oracle, %s: worst error in units of the set's bound max(1e-6, 4 sens)" % what, ratio.max(), 1.0)


@pytest.mark.parametrize("tag", ("A", "B", "C"))
def test_zero_pose_on_both_sides_gives_exact_zeros(engine, orc, tag):
    dc.set_frame(engine, tag)
    J = np.asarray(engine.dPNP(np.array(dc.ZERO[tag], np.int32)))
    assert J.shape == (dc.N_ZERO, 6, 12)
    assert not J.any(), np.argwhere(J.reshape(dc.N_ZERO, -1).any(axis=1)).ravel()  # 0.0 in all 72 entries of every set


@pytest.mark.parametrize("tag", ("A", "C"))
def test_big_sets(engine, orc, tag):
    """|J| of 1e3 - 1e5: one side of the steepest column is safeSolvePnP's zero pose (the win < 0 lane), or the two sides pick different roots."""
    cs = dc.big_cases(orc, tag)
    dc.set_frame(engine, tag)
    J = np.asarray(engine.dPNP(np.stack([c["set"] for c in cs])))
    rel, ratio = _check(J, cs, "big " + tag)
    assert len(rel) == len(cs)
    for cls in ("one_sided", "switch"):
        sel = np.array([c["cls"] == cls for c in cs])
        assert sel.sum() >= 4
        margin("a11", "K5 dPNP big sets (|J|max > 1e3) vs oracle, frame %s class %s: worst error in units of the set's bound" % (tag, cls), ratio[sel].max(), 1.0)
        # the steep column itself: a kernel that misses the zero pose or the other root is off by the column's size, not by rounding
        for h in np.flatnonzero(sel):
            col = int(np.argmax(np.abs(cs[h]["J"]).max(axis=0)))
            assert np.abs(J[h][:, col]).max() > 0.5 * dc.BIG_ABOVE


def test_poisoned_map(engine, orc):
    """A NaN / +inf / -inf coordinate in the map: the hypotheses that read it give the oracle's answer, the others are untouched."""
    p = dc.poisoned(orc)
    fr = dc.frame("A")
    dc.set_frame(engine, "A", xyz=p["xyz"])
    n = len(p["sets"])
    J = np.asarray(engine.dPNP(np.concatenate([p["sets"], p["clean"]])))
    assert np.isfinite(J).all()
    for k in range(n):
        if not p["J"][k].any():
            assert not J[k].any(), (k, p["kinds"][k])
        else:  # the fourth point only chooses among the roots
            v = dc.verdict(orc, fr, p["sets"][k], xyz=p["xyz"])
            assert np.array_equal(v["J"], p["J"][k]) and v["stable"]
            r = dc.rel(J[k], v["J"])
            print("poisoned %s in the fourth point: rel %.2e, bound %.2e" % (p["kinds"][k], r, v["bound"]))
            assert J[k].any() and r <= v["bound"], (k, p["kinds"][k], r, v["bound"])
    alone = np.asarray(engine.dPNP(p["clean"]))
    assert np.array_equal(J[n:], alone)
    dc.set_frame(engine, "A")
    assert np.array_equal(np.asarray(engine.dPNP(p["clean"])), alone)  # ... and the pristine map gives them the same bits


def test_replay_of_the_float_perturbation(engine, orc):
    cs = dc.replay_cases(orc)
    dc.set_frame(engine, dc.REPLAY_TAG)
    J = np.asarray(engine.dPNP(np.stack([c["set"] for c in cs]), eps=dc.REPLAY_EPS))
    rel, ratio = _check(J, cs, "replay")
    assert len(rel) == len(cs)
    far = np.array([dc.rel(J[h], c["J_noreplay"]) for h, c in enumerate(cs)])
    lane = np.array([dc.rel(J[h], c["J_lane"]) for h, c in enumerate(cs)])
    print("replay: rel(J, oracle) median %.2e max %.2e;  rel(J, J_noreplay) min %.2e;  smallest rel(J, J_noreplay) / rel(J, oracle) %.1f;  nearer to the oracle "
          "than to J_lane on %d of %d" % (np.median(rel), rel.max(), far.min(), (far / np.maximum(rel, 1e-300)).min(), (rel < lane).sum(), len(cs)))
    margin("a11", "K5 dPNP replay list vs oracle: worst error in units of the set's bound", ratio.max(), 1.0)
    # the kernel is on the replayed side by an order of magnitude
    margin("a11", "K5 dPNP replay list: smallest rel(J, J_noreplay) / rel(J, oracle)", (far / np.maximum(rel, 1e-300)).min(), 10.0, at_least=True)
    # ... and on the side of the `cc < c` round trips: every set of the list has J_lane at least one one-ulp sensitivity (and 1e-7) away from the oracle, so
    # a kernel that replays is nearer to the oracle unless its own error exceeds half of that; one that does not sits at J_lane up to its rounding and is
    # nearer to J_lane on nearly every set.  3 in 4 leaves the first room for the rounding differences test_dpnp_parity measures (up to 0.6 sens)
    margin("a11", "K5 dPNP replay list: share of sets nearer to the oracle than to the oracle without the round trips in front of a column", (rel < lane).mean(), 0.75,
           at_least=True)


def test_out_of_range_and_repeated_indices(engine, orc):
    """load_set clamps an index into [0, H W - 1]: the clamped twin gives the same bits (so nothing outside the map is read), on a map with a table of
    positions and on the implicit grid.  A repeated cell gives the oracle's result -- which is not zero in general: the perturbation itself pulls the two
    copies 0.1 mm apart, so a cell repeated among the three points of the P3P is a needle triangle (|J| of 1e4, unstable by the verdict: finiteness only,
    except where every solve fails and J is exactly zero), and one repeated in the fourth point is a set like any other."""
    for tag in ("A", "B"):
        fr = dc.set_frame(engine, tag)
        P = fr["H"] * fr["W"]
        base = dc.accepted_sets(orc, tag)[:6]
        bad, twin = [], []
        for k, v in enumerate((-1, -1000, -2 ** 31, P, P + 7, 2 ** 31 - 1)):
            for pos in range(4):
                s = base[k].copy()
                s[pos] = v
                bad.append(s)
                t = base[k].copy()
                t[pos] = min(max(v, 0), P - 1)
                twin.append(t)
        Jb, Jt = np.asarray(engine.dPNP(np.array(bad, np.int32))), np.asarray(engine.dPNP(np.array(twin, np.int32)))
        assert np.isfinite(Jb).all() and np.array_equal(Jb, Jt), tag
        assert Jt.any()
        # the clamped twins against the oracle (an index clamped to a corner cell is a set like any other)
        cs = [dc.verdict(orc, fr, t) for t in twin[::4]]
        _check(Jt[::4], cs, "clamped " + tag)
        # the same cell twice
        rep = []
        for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3))):
            s = base[k].copy()
            s[j] = s[i]
            rep.append(s)
        cs = [dc.verdict(orc, fr, s) for s in rep]
        Jr = np.asarray(engine.dPNP(np.array(rep, np.int32)))
        rel, _ = _check(Jr, cs, "repeated " + tag)
        assert len(rel) >= 2 and sum(c["robust_zero"] for c in cs) >= 1  # the oracle alone: see the docstring
        print("frame %s: repeated cells: %d of 6 sets stable, %d exactly zero" % (tag, len(rel), sum(c["zero"] for c in cs)))


def test_launch_shapes(engine, orc):
    """N = 1, 3 and 1025 (one workgroup per hypothesis): every row is the row of the same set in the N = 64 call, with host arrays and with device tensors."""
    import torch
    dev = torch.device("cuda:0")
    sets = dc.accepted_sets(orc, "A")
    dc.set_frame(engine, "A")
    base = np.asarray(engine.dPNP(sets)).copy()
    _check(base, dc.cases(orc, "A", "accepted"), "N = 64")
    for N in (1, 3, 1025):
        idx = (np.arange(N) * 7 + 5) % len(sets)
        tiled = np.ascontiguousarray(sets[idx])
        J = np.asarray(engine.dPNP(tiled))
        assert J.shape == (N, 6, 12) and np.array_equal(J, base[idx]), N
        out = torch.full((N + 1, 6, 12), -7.0, dtype=torch.float64, device=dev)  # one row more: the launch writes N rows
        got = engine.dPNP(torch.from_numpy(tiled).to(dev), out=out)
        engine.synchronize()
        assert got is out
        o = out.cpu().numpy()
        assert np.array_equal(o[:N], base[idx]) and np.all(o[N] == -7.0), N


BATCH_CAMS = ((525.0, 525.0, 320.0, 240.0), dc.CAM_C, (480.0, 520.0, 330.0, 235.0))


def _batch(cams):
    """3 maps of 24 x 32 rendered under `cams`, each with its own table of positions (the stratified sub-sample plus a sub-pixel jitter)"""
    from dsac_amd import synth
    frames = []
    for f, cam in enumerate(cams):
        fr = synth.chess_like_frame(24, 32, seed=5200 + f, cam=cam)
        p = np.arange(24 * 32, dtype=np.float64)
        fr["uv"] = (fr["uv"].astype(np.float64) + 0.31 * np.stack([np.sin(1.3 * p + f), np.cos(2.9 * p - f)], -1)).astype(np.float32)
        frames.append(fr)
    return frames


@pytest.mark.parametrize("per_frame_cams", (False, True))
def test_frame_batch_against_the_oracle(engine, orc, per_frame_cams):
    """Every frame's slice of a batch call against orc.dPNP on that frame's map, table and camera (batch == single-frame calls is tested elsewhere): 40
    accepted sets per frame, under one camera for the batch (frame C's) and under one camera per frame (frame C's is the second)."""
    cams = list(BATCH_CAMS) if per_frame_cams else [dc.CAM_C] * 3
    frames = _batch(cams)
    n = 40
    per = []
    for f, fr in enumerate(frames):
        _, sets, ok, _ = orc.sample(n, 5300 + f, fr["xyz"], fr["uv"], 24, 32, cams[f])
        assert ok.all()
        per.append((fr, sets, [dc.verdict(orc, fr, s) for s in sets]))
    engine.set_frames(np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames])), np.ascontiguousarray(np.stack([fr["uv"] for fr in frames])), 24, 32,
                      np.array(cams, np.float32) if per_frame_cams else cams[0], uv_per_frame=True)
    assert engine.get_option("frame_cams") == (1 if per_frame_cams else 0)
    J = np.asarray(engine.dPNP(np.concatenate([sets for _, sets, _ in per])))
    for f, (view, sets, cs) in enumerate(per):
        rel, ratio = _check(J[f * n:(f + 1) * n], cs, "batch frame %d" % f)
        assert len(rel) >= 0.75 * n, (f, len(rel))
        margin("a11", "K5 dPNP frame batch (%s) vs oracle per frame: median relative error" % ("one camera per frame" if per_frame_cams else "shared camera"),
               np.median(rel), 1e-6)
        margin("a11", "K5 dPNP frame batch (%s) vs oracle per frame: worst error in units of the set's bound" % ("one camera per frame" if per_frame_cams else "shared camera"),
               ratio.max(), 1.0)
    dc.set_frame(engine, "A")  # leave a single frame behind


def test_against_exact_p3p_roots(engine, orc):
    """J against central differences of EXACT poses (tests/golden/make_dpnp_exact.py), the bound measured against the oracle's own error on the same set:
    rel(J_gpu, J_exact) <= max(1e-6, 4 rel(J_oracle, J_exact)) -- the factor and the floor of the K5 rule."""
    z = np.load(FIXTURE)
    assert [int(c) for c in z["frame_crc"]] == [dc.checksum(t) for t in ("A", "B", "C")]
    done = 0
    for tag, eps in sorted({(str(t), float(e)) for t, e in zip(z["tag"], z["eps"])}):
        sel = np.flatnonzero((z["tag"] == tag) & (z["eps"] == eps))
        dc.set_frame(engine, tag)
        J = np.asarray(engine.dPNP(np.ascontiguousarray(z["set"][sel]), eps=eps))
        rel = np.array([dc.rel(J[k], z["J_exact"][i]) for k, i in enumerate(sel)])
        ratio = rel / np.maximum(1e-6, 4 * z["oracle_rel"][sel])
        print("frame %s eps %g: K5 vs exact over %d sets: median %.2e  max %.2e;  oracle vs exact median %.2e;  worst rel / max(1e-6, 4 oracle's) %.2f" % (
            tag, eps, len(sel), np.median(rel), rel.max(), np.median(z["oracle_rel"][sel]), ratio.max()))
        margin("a11", "K5 dPNP vs exact P3P roots, frame %s eps %g: median relative error" % (tag, eps), np.median(rel), 1e-6)
        margin("a11", "K5 dPNP vs exact P3P roots, frame %s eps %g: worst error in units of max(1e-6, 4 x the oracle's own)" % (tag, eps), ratio.max(), 1.0)
        done += len(sel)
    assert done == len(z["tag"]) >= 300
