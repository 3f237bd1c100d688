"""K6's finite-difference stage (dk::refine_fd_plan / _run / _finish behind dsac_refine_fd and dsac_refine_fd_set / _sets) where one plan and one finish kernel
serve both replica lists -- soft-argmax (12 head replicas, dRefineHyp + dRefineObj) and the DSAC variant (18, dRefine): the one-workgroup plan on a ragged map,
and a `cap` below the number of selected cells in both plan forms.

Selected cells and n_obj are integers: exact.  Jacobians against the oracle at the tolerances of tests/test_gpu_refine.py (1e-4 of the largest entry) and
tests/test_gpu_dsac_variant.py (2e-3); a capped call against the uncapped one: the same replicas in the same slots, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 37 x 41: P = 1517 cells, two per segment of the one-workgroup scan and the last third of its 1024 threads without one; H != W: a row / column mix-up shows.
# 120 x 160: above 16384 cells, the tiled plan (two full 64-column tiles and a half one, 15 used row segments).
SIZES = {"one workgroup": (37, 41), "tiled": (120, 160)}
# The start pose's distance from the ground truth, in units of (0.003, -0.002, 0.001) rad and (2, -3, 4) mm.  dRefineHyp is zero to rounding wherever the twelve
# perturbed starts all walk into the same inlier sets, and of order one where a cell changes sides: at these distances the oracle's J_hyp is of order one (at
# 37 x 41 the distance 1 gives 1e-11, rounding noise that no relative tolerance can be asked of); the test asserts it from the oracle.
START = {(37, 41): 3.0, (120, 160): 1.0}
_cache = {}


def _setup(engine, orc, synth, H, W):
    """Frame, permutations, a start pose with the inlier map of its refinement, three sampled hypotheses with theirs (the engine is left on the frame)."""
    fr = synth.chess_like_frame(H, W, seed=5)
    engine.set_frame(fr["xyz"], fr["uv"], H, W, fr["cam"])
    if (H, W) not in _cache:
        perm = synth.fast_permutations(H * W, 8, seed=3)
        init = fr["gt_pose"] + START[(H, W)] * np.array([0.003, -0.002, 0.001, 2.0, -3.0, 4.0])
        _, sd, imap = engine.refine(init, perm, want_inlier_map=True)
        poses, sets, ok, _ = orc.sample(3, 4, fr["xyz"], fr["uv"], H, W, fr["cam"])
        _, sds, maps = engine.refineAll(poses, perm, sets=sets, want_inlier_maps=True)
        assert sd[0] == 8 and (sds == 8).all()
        for a in (imap, maps, sets, perm, init):
            a.setflags(write=False)
        _cache[(H, W)] = dict(fr=fr, perm=perm, init=init, imap=imap, sets=sets, maps=maps)
    return _cache[(H, W)]


def _selection(imap, H, W, skip):
    """the reference's walk: x outer / y inner, every skip-th inlier cell (core/cnn_softam.h:868-880, core/cnn.h:935-945)"""
    return [y * W + x for x in range(W) for y in range(H) if imap[y * W + x]][skip - 1::skip]


@pytest.mark.parametrize("sub,skip", [(1.0, 1), (0.3, 3), (0.049, 20)])
def test_one_workgroup_plan_on_a_ragged_map(engine, orc, synth, sub, skip):
    H, W = SIZES["one workgroup"]
    s = _setup(engine, orc, synth, H, W)
    fr, perm = s["fr"], s["perm"]
    geo = (fr["xyz"], fr["uv"], H, W, fr["cam"])
    # soft-argmax
    want = _selection(s["imap"], H, W, skip)
    assert len(want) >= 5
    Jh, px, Jo = engine.dRefine(s["init"], perm, s["imap"], sub_sample=sub)
    assert [int(p) for p in px] == want  # n_obj == len(want): dRefine returns the first n_obj entries
    Jh_r = orc.dRefineHyp(s["init"], perm, *geo)
    Jo_r = orc.dRefineObj(s["init"], perm, s["imap"], *geo, sub_sample=sub)
    assert np.abs(Jh_r).max() > 1e-3  # a Jacobian, not rounding noise (START)
    assert np.abs(Jh - Jh_r).max() <= 1e-4 * np.abs(Jh_r).max()
    dense = np.zeros((6, H * W * 3))
    for i, p in enumerate(px):
        dense[:, p * 3:p * 3 + 3] = Jo[i]
    assert np.abs(dense - Jo_r).max() <= 1e-4 * max(np.abs(Jo_r).max(), 1e-12)
    # DSAC variant: two hypotheses, each with its own map
    sets, maps = s["sets"][:2], s["maps"][:2]
    J_set, n_obj, pxs, J_obj = engine.dRefineSets(sets, perm, maps, sub_sample=sub)
    for m in range(2):
        want = _selection(maps[m], H, W, skip)
        assert len(want) >= 5
        assert n_obj[m] == len(want) and [int(p) for p in pxs[m][:n_obj[m]]] == want
        Jr = orc.dRefineDSAC(sets[m], perm, maps[m], *geo, sub_sample=sub)
        got = np.zeros_like(Jr)
        for pt in range(3):
            got[:, sets[m][pt] * 3:sets[m][pt] * 3 + 3] = J_set[m][:, pt * 3:pt * 3 + 3]
        for i in range(n_obj[m]):
            got[:, pxs[m][i] * 3:pxs[m][i] * 3 + 3] = J_obj[m][i]
        scale = max(np.abs(Jr).max(), 1e-12)
        assert np.abs(got - Jr).max() <= 2e-3 * scale, (m, np.abs(got - Jr).max(), scale)


@pytest.mark.parametrize("form", sorted(SIZES))
def test_cap_below_the_number_of_selected_cells(engine, orc, synth, form):
    H, W = SIZES[form]
    s = _setup(engine, orc, synth, H, W)
    perm, sub, skip, cap = s["perm"], 0.3, 3, 7
    # soft-argmax
    want = _selection(s["imap"], H, W, skip)
    assert len(want) > cap
    Jh, px, Jo = engine.dRefine(s["init"], perm, s["imap"], sub_sample=sub)
    assert len(px) == len(want)
    Jh_c, px_c, Jo_c = engine.dRefine(s["init"], perm, s["imap"], sub_sample=sub, cap=cap)
    assert [int(p) for p in px_c] == want[:cap]  # n_obj == cap
    assert np.array_equal(Jo_c, Jo[:cap]) and np.array_equal(Jh_c, Jh)
    Jh_0, px_0, Jo_0 = engine.dRefine(s["init"], perm, s["imap"], sub_sample=sub, cap=0)
    assert len(px_0) == 0 and np.array_equal(Jh_0, Jh)
    # DSAC variant
    sets, maps = s["sets"], s["maps"]
    wants = [_selection(maps[m], H, W, skip) for m in range(3)]
    assert min(len(w_) for w_ in wants) > cap
    J_set, n_obj, pxs, J_obj = engine.dRefineSets(sets, perm, maps, sub_sample=sub)
    assert [int(k) for k in n_obj] == [len(w_) for w_ in wants]
    J_set_c, n_c, pxs_c, J_obj_c = engine.dRefineSets(sets, perm, maps, sub_sample=sub, cap=cap)
    assert (n_c == cap).all() and np.array_equal(J_set_c, J_set)
    for m in range(3):
        assert [int(p) for p in pxs_c[m]] == wants[m][:cap]
        assert np.array_equal(J_obj_c[m], J_obj[m][:cap])
    J_set_0, n_0, _, _ = engine.dRefineSets(sets, perm, maps, sub_sample=sub, cap=0)
    assert not n_0.any() and np.array_equal(J_set_0, J_set)
