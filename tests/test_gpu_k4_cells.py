"""K4 (score backward: k_score_backward_mfma, k_score_backward and the finish kernels) per cell and per hypothesis against tests/k4_ref.py, on maps and
hypothesis counts off its tile grid.

The metric.  For every cell p:  max_c |grad[p, c] - ref[p, c]| <= 1e-3 * scale[p] + 1e-30,  scale[p] = sum_h |w[h, p]| * ||dProjectdObj[h, p]||, the
absolute sum behind the cell -- SURVEY.md 8(c)'s fp32-fast tolerance applied to each cell's own scale instead of the map's largest entry, so that a wrong
term in a cell of small weight counts.  Cells with scale == 0 hold exactly 0.0.  The pose sums (lastPoseGradients), per hypothesis relative to its largest
component: median <= 1e-4, max <= 1e-3 (the figures of tests/test_gpu_backward.py).  tests/test_k4_ref_cpu.py shows on the CPU that a correct fp32
evaluation of the kernel's formulas passes these bounds on every case here and that six wrong kernels do not.

Inputs (tests/k4_ref.py): synth.chess_like_frame with the default noise and outliers, poses = ground truth + N(0, 0.03 rad) / N(0, 40 mm), any 4 distinct
cells as sets, dpnp = 0 (K4's result is then the per-cell term alone).  Three inputs per case: (a) d_err = N(0, 1) * 1e-3, (b) d_err = N(0, 1) * 10^U(-4, 0)
with the exponent drawn per cell, both zero on mask_pairs, and the fused soft-inlier form (tau = 10, beta = 0.5, g ~ N(0, 1)), per cell on the cells
without a masked pair.

The corpus and the values of dk::backward_plan each case relies on (CH = chunks of 16 cells per wave, a pixel tile = 64 CH cells, PT tiles; HT = hypothesis
tile, NT tiles, nh = hypotheses of the last tile; G = workgroups per hypothesis tile):
  tiny                  2x2 sampled (P = 4), 3x4 implicit (P = 12); N = 1, 5; k4_variant -1, 1, 2.  PT = 1, HT = 16: one partial chunk, the d_err / uv
                        load clamp min(p0, P - 4) = 0, nh - 1 = 0 at N = 1.  -1 takes the small-map plan (form 1, HT 16).
  chunk tail            38x42 sampled (P = 1596, P % 16 = 12), N = 40 = 2 * 16 + 8; -1, 1 .. 7.  CH = 2, 4, 5, 6, 3, 2, 3 -> PT = 13, 7, 5, 5, 9, 13, 9: a
                        partial last chunk and a partial last tile in every CH, ragged last group (8 of 16 columns).  Also the accumulation check.
  implicit tail         36x44 implicit (P = 1584, W % 4 == 0), N = 17 = 16 + 1; -1, 1 .. 7: implicit-grid rows, a last group of one hypothesis.
  one tile + 4          4 x (16 CH + 1) sampled: P = 64 CH + 4, N = 16; form 1 .. 7 on the map of its own CH: PT = 2, the second tile has 4 valid cells.
  VALU forms            37x41 sampled (P % 4 = 1): the scalar VALU build; 38x42 implicit (W % 4 = 2): the vector VALU build, chosen by the plan; N = 33
                        (HT = 32: NT = 2, nh = 1); -1, 0.
  hypothesis edges      38x42 sampled, N = 1, 15, 16, 17, 257; -1, 2.  Form 2 at N = 257: HT = 256, NT = 2, nh = 1, not direct: the grad_part layers and
                        k_grad_reduce.  -1: the small-map plan, HT = 16 (N = 257: NT = 17).
  split tiles, direct   168x200 sampled (P = 33 600), N = 48; 101 (form 1, one workgroup per CU): PT = 263 > G = 256, HT = 48, NT = 1: 789 (tile, group)
                        items on 256 workgroups -- pixel tiles whose groups two workgroups add into grad_xyz.
  split tiles, layered  120x160 sampled (P = 19 200), N = 80; 111 (form 1, 64-hypothesis tiles, one workgroup per CU): HT = 64, NT = 2 (nh = 16),
                        G = 128 < PT = 150: layer 0 / layer 1 of grad_part.
  staged                38x42 sampled, N = 40; 1999, 1002: the k_backward_prep records instead of the fused set-up.
  transposed index      40x40 sampled, N = 24; -1, 0: flags bit 0, per cell.
  16-bit images         38x42 sampled, N = 40; -1, 1, 5 (forms 1, 1, 5): d_err (a) and (b) rounded to float16 / bfloat16 first, the reference gets the
                        rounded values.
  frame batch           3 frames of 38x42 sampled, one camera per frame (fx = fy: 525, 260, 610 px, three principal points), 3 x 48 hypotheses; -1:
                        HT = Nf = 48, one tile per frame; the per-frame cams row in the main pass and the finish; the reference per frame under its camera.
No case of the corpus names a form the entry point refuses for its input; a refusal raises and fails the case.

Measured (MI355X), worst over the corpus: per cell 4.1e-5 with d_err (flat and heavy-tailed alike), 6.7e-5 in the fused form; pose sums median 5.2e-6,
max 4.4e-5; every family's own figures are in the margin report (rows a9 / a10).  The asserted values are the stated tolerances, not these."""
import numpy as np
import pytest

import k4_ref as kr
from conftest import margin

pytestmark = pytest.mark.gpu

PARAMS = [(i, v) for i, c in enumerate(kr.CORPUS) for v in c["variants"]]
IDS = ["%s-v%d" % (kr.case_id(kr.CORPUS[i]), v) for i, v in PARAMS]


def _set_frames(engine, b):
    parts = b["parts"]
    implicit = b["case"]["implicit"]
    if b["frames"] == 1:
        fr = parts[0]["fr"]
        engine.set_frame(fr["xyz"], None if implicit else fr["uv"], b["H"], b["W"], fr["cam"])
    else:
        xyz = np.ascontiguousarray(np.stack([p["fr"]["xyz"] for p in parts]))
        uv = None if implicit else np.ascontiguousarray(np.stack([p["fr"]["uv"] for p in parts]))
        cams = np.array([p["fr"]["cam"] for p in parts], np.float32)
        engine.set_frames(xyz, uv, b["H"], b["W"], cams, uv_per_frame=uv is not None)


def run_case(engine, idx, variant):
    """One launch form on one case: per input the measured figures (nothing asserted here)."""
    b = kr.build_case(idx)
    parts, elem, tr = b["parts"], b["elem"], b["transpose"]
    FN = b["frames"] * b["N"]
    poses = np.concatenate([p["poses"] for p in parts])
    sets = np.concatenate([p["sets"] for p in parts])
    dpnp = np.zeros((FN, 6, 12))
    _set_frames(engine, b)
    engine.set_option("k4_variant", variant)
    out = []
    try:
        for name in ("flat", "heavy", "soft"):
            ref = b["refs"][name]
            if name == "soft":
                if elem != "f32":
                    continue  # the fused form reads no gradient images
                g = np.concatenate([p["g"] for p in parts])
                grad = engine.dSoftScore(poses, sets, g, tau=kr.TAU, beta=kr.BETA, dpnp=dpnp, quirk_transpose=tr)
                cells = b["clean_cells"]
            else:
                d = np.ascontiguousarray(np.concatenate([(p["d_err"] if elem == "f32" else p["bits"])[name] for p in parts]))
                grad = engine.dScore(poses, sets, d, dpnp=dpnp, quirk_transpose=tr, elem="bf16" if elem == "bf16" else None)
                cells = np.ones(ref["scale"].shape[0], bool)
            G6 = engine.lastPoseGradients(FN)
            pr = kr.pose_ratios(G6, ref["G6"])
            r = dict(name=name, finite=bool(np.isfinite(grad).all() and np.isfinite(G6).all()), cell=kr.cell_ratio(grad, ref, cells), pose_median=float(np.median(pr)),
                     pose_max=float(pr.max()), zeros=not grad[(ref["scale"] == 0) & cells].any(), twice=None)
            if name == "flat" and b["case"]["opt"].get("accumulate"):
                twice = engine.dScore(poses, sets, d, dpnp=dpnp, grad=grad.copy())
                r["twice"] = bool(np.allclose(twice, 2 * grad, rtol=1e-6, atol=1e-9 * np.abs(grad).max()))
            print("%s %s: per-cell %.3e, pose sums median %.3e max %.3e, zero cells %s" % (IDS[PARAMS.index((idx, variant))], name, r["cell"], r["pose_median"],
                                                                                        r["pose_max"], "exact" if r["zeros"] else "NOT ZERO"), flush=True)
            out.append(r)
    finally:
        engine.set_option("k4_variant", -1)
    return out


@pytest.mark.parametrize("idx,variant", PARAMS, ids=IDS)
def test_k4_per_cell(engine, orc, idx, variant):
    b = kr.build_case(idx)
    fam, elem = b["case"]["family"], b["elem"]
    for r in run_case(engine, idx, variant):
        assert r["finite"]
        what = "K4 per cell, %s%s, %s" % (fam, "" if elem == "f32" else " " + elem, r["name"])
        margin("a9", what + ": max over cells of max_c |g - ref| / (sum_h |w| ||dProjectdObj||)  (SURVEY 8(c) fp32-fast 1e-3, per cell)", r["cell"], kr.CELL_TOL)
        assert r["zeros"], "a cell without any weight is not exactly 0"
        margin("a10", what + ": pose sums, median over hypotheses of max-rel to the largest component", r["pose_median"], kr.POSE_MEDIAN)
        margin("a10", what + ": pose sums, max over hypotheses of max-rel to the largest component", r["pose_max"], kr.POSE_MAX)
        assert r["twice"] in (None, True), "a second call into the same gradient does not give twice the first"
